"""GPU: the device half of the image writer (csrc/image_out.hip) and the asynchronous writer on top of it.  Every
comparison is exact: gigs_pack_images against torch's x.mul(255).add_(bias).clamp_(0, 255).to(uint8) on the same device,
gigs_png_filter against the numpy restatement of the PNG filters (tests/png_ref.py), the files against both."""
import os

import numpy as np
import pytest
import torch

import png_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIZES = [(1, 1), (3, 5), (127, 130), (800, 800)]  # H x W


def _torch_u8(x, bias):
    """[C,H,W] float -> [H,W,3] uint8, torch's own arithmetic."""
    q = x.clone().mul(255).add_(bias).clamp_(0, 255).to(torch.uint8)
    if q.shape[0] == 1:
        q = q.expand(3, -1, -1)
    return q.permute(1, 2, 0).contiguous()


def _planes(C_, H, W, seed):
    """Seeded planes with values below 0, above 1, on the rounding boundaries k/255 - 0.5/255, and +-inf."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((C_, H, W), generator=g) * 1.4 - 0.2
    flat = x.view(-1)
    n = flat.numel()
    k = torch.arange(n) % 257
    sel = torch.arange(n) % 3 == 0
    flat[sel] = (k[sel].float() / 255.0 - 0.5 / 255.0)  # what save_image's rounding turns on
    if n > 8:
        flat[1], flat[2], flat[5], flat[7] = float("inf"), float("-inf"), 1.0, 0.0
    return x.to(DEV)


def _pack(descs):
    """gigs_pack_images over a list of dicts(src, dst, lohi, dst_x, dst_stride, bias)."""
    import gigs_lib
    tab = (gigs_lib.PackDesc * len(descs))()
    for d, e in zip(tab, descs):
        src = e["src"]
        d.src, d.dst, d.lohi = src.data_ptr(), e["dst"].data_ptr(), e["lohi"].data_ptr() if e.get("lohi") is not None else None
        d.channels, d.height, d.width = src.shape
        d.dst_x, d.dst_stride, d.bias = e.get("dst_x", 0), e["dst_stride"], e.get("bias", 0.5)
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    gigs_lib.check(gigs_lib.lib().gigs_pack_images(len(descs), dev_tab.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "pack_images")
    torch.cuda.synchronize()


def _filter(sheet, W):
    """gigs_png_filter on one sheet [H, stride] uint8 (3 W bytes used per row) -> the stream as numpy bytes."""
    import gigs_lib
    H, stride = sheet.shape
    out = torch.full((H * (1 + 3 * W) + 8,), 0xEE, dtype=torch.uint8, device=DEV)
    tab = (gigs_lib.FilterDesc * 1)()
    tab[0].sheet, tab[0].out, tab[0].height, tab[0].width, tab[0].stride = sheet.data_ptr(), out.data_ptr(), H, W, stride
    dev_tab = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    gigs_lib.check(gigs_lib.lib().gigs_png_filter(1, dev_tab.data_ptr(), torch.cuda.current_stream().cuda_stream), "png_filter")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[-8:] == 0xEE).all(), "gigs_png_filter wrote past the stream"
    return got[:-8]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("bias", [0.5, 0.0])
def test_pack_equals_torch(H, W, C_, bias):
    x = _planes(C_, H, W, seed=H * 7 + W + C_)
    sheet = torch.full((H, W, 3), 0xEE, dtype=torch.uint8, device=DEV)
    _pack([dict(src=x, dst=sheet, dst_stride=3 * W, bias=bias)])
    assert torch.equal(sheet, _torch_u8(x, bias))


def test_pack_nan_is_zero():
    x = _planes(3, 16, 16, seed=1)
    x[0, 3, 4] = float("nan")
    x[2, 0, 0] = float("nan")
    sheet = torch.empty((16, 16, 3), dtype=torch.uint8, device=DEV)
    _pack([dict(src=x, dst=sheet, dst_stride=48)])
    want = _torch_u8(torch.nan_to_num(x, nan=-1.0, posinf=float("inf"), neginf=float("-inf")), 0.5)
    assert int(sheet[3, 4, 0]) == 0 and int(sheet[0, 0, 2]) == 0
    assert torch.equal(sheet, want)


@pytest.mark.parametrize("H,W", [(3, 5), (127, 130), (64, 64)])
def test_pack_side_by_side_with_offsets(H, W):
    """render.py's brdf image: albedo | roughness | metallic in one sheet, three descriptors, one launch; a padded row
    stride; nothing outside the three windows is written."""
    a, r, m = _planes(3, H, W, 1), _planes(1, H, W, 2), _planes(1, H, W, 3)
    stride = (3 * 3 * W + 15) // 16 * 16 + 16
    sheet = torch.full((H, stride), 0xEE, dtype=torch.uint8, device=DEV)
    _pack([dict(src=a, dst=sheet, dst_stride=stride, dst_x=0), dict(src=r, dst=sheet, dst_stride=stride, dst_x=W, bias=0.0),
           dict(src=m, dst=sheet, dst_stride=stride, dst_x=2 * W)])
    want = torch.cat([_torch_u8(a, 0.5), _torch_u8(r, 0.0), _torch_u8(m, 0.5)], dim=1).reshape(H, 9 * W)
    assert torch.equal(sheet[:, :9 * W], want)
    assert bool((sheet[:, 9 * W:] == 0xEE).all())


@pytest.mark.parametrize("H,W", [(3, 5), (127, 130), (800, 800)])
def test_depth_mode_equals_torch(H, W):
    import gigs_lib
    g = torch.Generator().manual_seed(H + W)
    d = (torch.rand((1, H, W), generator=g) * 7.0 + 0.3).to(DEV)
    d[0, 0, 0] = 0.0  # background depth
    lohi = torch.empty(2, device=DEV)
    scratch = torch.empty(gigs_lib.MINMAX_SCRATCH_FLOATS, device=DEV)
    gigs_lib.check(gigs_lib.lib().gigs_plane_minmax(d.numel(), d.data_ptr(), scratch.data_ptr(), lohi.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "plane_minmax")
    assert float(lohi[0]) == float(d.min()) and float(lohi[1]) == float(d.max())
    sheet = torch.empty((H, W, 3), dtype=torch.uint8, device=DEV)
    _pack([dict(src=d, dst=sheet, dst_stride=3 * W, lohi=lohi)])
    assert torch.equal(sheet, _torch_u8((d - d.min()) / (d.max() - d.min()), 0.5))


@pytest.mark.parametrize("H,W", SIZES + [(128, 128), (5, 2000), (33, 341)])
def test_filter_equals_reference(H, W):
    img = png_ref.quantize(png_ref.test_image(H, W))
    want, types = png_ref.scanlines(img)
    for stride in (3 * W, (3 * W + 15) // 16 * 16 + 16):  # the byte path and, for an aligned stride, the dwordx4 path
        sheet = torch.zeros((H, stride), dtype=torch.uint8, device=DEV)
        sheet[:, :3 * W] = torch.from_numpy(img.reshape(H, 3 * W)).to(DEV)
        got = _filter(sheet, W)
        rows = got.reshape(H, 1 + 3 * W)
        assert np.array_equal(rows[:, 0], types), "filter types differ"
        assert got.tobytes() == want
    if (H, W) in ((127, 130), (128, 128)):
        assert (np.bincount(types, minlength=5) >= 2).all()


def test_filter_of_packed_sheets_through_encode():
    """image_writer.encode: pack + filter of several images of different sizes in one launch each."""
    from PIL import Image as PILImage

    import image_writer
    import io
    srcs = [_planes(3, 127, 130, 5), _planes(1, 64, 64, 6), torch.from_numpy(png_ref.test_image(128, 128)).to(DEV),
            _planes(3, 1, 1, 7)]
    streams, sheets = image_writer.encode([(None, s) for s in srcs] + [image_writer.Image(None, [srcs[1], srcs[1]], bias=0.0)],
                                          want_sheets=True)
    wants = [_torch_u8(s, 0.5) for s in srcs] + [torch.cat([_torch_u8(srcs[1], 0.0)] * 2, dim=1)]
    for st, sh, want in zip(streams, sheets, wants):
        assert torch.equal(sh, want)
        ref, _ = png_ref.scanlines(want.cpu().numpy())
        assert st.tobytes() == ref
        H, W, _ = want.shape
        im = PILImage.open(io.BytesIO(image_writer.png_bytes(st, W, H)))
        assert np.array_equal(np.asarray(im), want.cpu().numpy())


def test_image_writer_many_submissions(tmp_path):
    """40 views of 13 images through three slots; the source planes are overwritten right after each submit on the same
    stream, so a missing event or a slot reused too early shows as wrong bytes."""
    from PIL import Image as PILImage

    import image_writer
    H, W = 96, 112
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    planes = [torch.empty((3 if i % 3 else 1, H, W), device=DEV) for i in range(12)]
    depth = torch.empty((1, H, W), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    expected = {}
    with image_writer.ImageWriter(workers=12, slots=3) as wr:
        for v in range(40):
            for p in planes:
                p.copy_(torch.rand(p.shape, generator=g, device=DEV) * 1.2 - 0.1)
            depth.copy_(torch.rand(depth.shape, generator=g, device=DEV) * 5.0 + 1.0)
            items = []
            for i, p in enumerate(planes):
                path = str(tmp_path / ("v%02d_%02d.png" % (v, i)))
                bias = 0.0 if i == 4 else 0.5
                items.append((path, p, bias))
                expected[path] = _torch_u8(p, bias)
            path = str(tmp_path / ("v%02d_depth.png" % v))
            items.append(image_writer.Image(path, depth, normalize=True))
            expected[path] = _torch_u8((depth - depth.min()) / (depth.max() - depth.min()), 0.5)
            wr.submit(items)
            for p in planes + [depth]:
                p.fill_(0.25)  # the planes are free again as soon as submit returns
    assert wr.files == 40 * 13
    names = sorted(os.listdir(tmp_path))
    assert len(names) == 40 * 13 and not any(n.endswith(".tmp") for n in names)
    for path, want in expected.items():
        im = PILImage.open(path)
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), want.cpu().numpy()), path
    del planes, depth, items, p, expected, want
    torch.cuda.synchronize()
    assert abs(torch.cuda.memory_allocated() - m0) <= 1 << 20, (m0, torch.cuda.memory_allocated())


def test_image_writer_reports_worker_errors(tmp_path):
    import image_writer
    x = _planes(3, 16, 16, 0)
    wr = image_writer.ImageWriter(workers=2, slots=2)
    wr.submit([(str(tmp_path / "ok.png"), x), (str(tmp_path / "no_such_dir" / "a.png"), x)])
    with pytest.raises(OSError):
        wr.close()
    assert os.path.exists(tmp_path / "ok.png") and not any(n.endswith(".tmp") for n in os.listdir(tmp_path))
    with pytest.raises(RuntimeError):
        wr.submit([(str(tmp_path / "late.png"), x)])


# ---- end to end: render_scene / relight_scene ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A scene folder (synthetic_dataset, 128 x 128) and an output folder holding the teacher scene as chkpnt7.pth + cfg_args:
    what trainer.py leaves behind, without a training run."""
    import importlib
    from argparse import Namespace
    importlib.import_module("gi-gs_amd")
    import densify
    import optim
    import relight
    import scene_io
    import scenes
    import synthetic_dataset
    import train_iteration as ti
    src = synthetic_dataset.write_synthetic_dataset(str(tmp_path_factory.mktemp("scene")), size=128)
    out = str(tmp_path_factory.mktemp("run"))
    sc = scenes.surface_scene(P=4000, sh_degree=0, seed=3, scale_mu=0.05)
    raw = ti.raw_from_scene(sc, DEV)
    opt = optim.FusedAdam([{"params": [raw[k]], "lr": 0.0, "name": k} for k in raw], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, raw, densify.DensifyState(raw["xyz"].shape[0], DEV), opt, 1.0),
                             light.state_dict(), {}, 7)
    with open(os.path.join(out, "cfg_args"), "w") as f:
        f.write(str(Namespace(sh_degree=3, source_path=src, model_path=out, images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)))
    del raw, opt, light
    return src, out, ck


def _hand_setup(src, ck):
    import dataset_readers as dr
    import pbr
    import pipeline
    import scene_io
    sc = scene_io.load_scene(ck)
    ckpt = scene_io.load_checkpoint(ck)
    light = pbr.CubemapLight(base_res=256, device=DEV)
    light.load_state_dict({k: v.to(DEV) for k, v in ckpt["cubemap"].items()})
    light.eval()
    g = {k: torch.from_numpy(sc[k]).to(DEV) for k in pipeline.RASTER_KEYS}
    cams = [dr.camera_from_info(ci, -1, device=DEV) for ci in dr.readNerfSyntheticInfo(src, False, True)["test_cameras"]]
    return g, light, cams, int(ckpt["gaussians"][0])


def _png(path):
    from PIL import Image as PILImage
    im = PILImage.open(path)
    assert im.mode == "RGB", path
    return np.asarray(im)


def test_render_scene_end_to_end(trained):
    import json

    import evaluate
    import pipeline
    import render_scene
    import scenes
    src, out, ck = trained
    res = render_scene.render_scene(["-m", out, "--checkpoint", ck, "--pbr", "--metallic", "--indirect", "--skip_train"])
    g, light, cams, deg = _hand_setup(src, ck)
    names = [c["image_name"] for c in cams]
    assert len(cams) == 8 and list(res) == ["test"] and res["test"]["n_views"] == 8
    listed = render_scene.planned_paths(out, "test", 7, names)
    for path in listed:
        assert os.path.exists(path), path
    assert res["test"]["files"] == 3 + 13 * 8
    for root, _, files in os.walk(out):
        assert not any(f.endswith(".tmp") for f in files), root
    # the same views through an evaluator driven by hand (tests/test_gpu_trainer.py:68-83), with and without the opt-in planes
    gi = dict(scenes.GI_DEFAULTS)
    ev = evaluate.NovelViewEvaluator(light, gi, deg, metallic=True, extra_planes=True)
    ev0 = evaluate.NovelViewEvaluator(light, gi, deg, metallic=True)
    rays = pipeline.canonical_rays(cams[0], DEV)
    for idx, c in enumerate(cams):
        vd = pipeline.view_dirs_for(c, rays, DEV)
        p = {k: v.clone() for k, v in ev(c, g, vd, c["original_image"], c["gt_alpha_mask"]).items() if torch.is_tensor(v)}
        p0 = ev0(c, g, vd, c["original_image"], c["gt_alpha_mask"])
        assert set(evaluate.PLANES) <= set(p0) and not set(evaluate.EXTRA_PLANES) & set(p0)
        for k in evaluate.PLANES:  # the default evaluator is what it was; the opt-in changes none of its planes
            assert torch.equal(p0[k], p[k]), k
        if idx not in (0, 3, 7):
            continue
        paths = render_scene.view_paths(out, "test", 7, idx, c["image_name"])
        for suffix, plane in render_scene.PBR_PLANES.items():
            if isinstance(plane, tuple):
                want = torch.cat([_torch_u8(p[n], 0.5) for n in plane], dim=1)
            else:
                want = _torch_u8(p[plane], 0.0 if suffix == "_occlusion" else 0.5)
            assert np.array_equal(_png(paths[suffix]), want.cpu().numpy()), paths[suffix]
        for k in ("normal", "from_depth"):
            assert np.array_equal(_png(paths[k]), _torch_u8(p[k], 0.5).cpu().numpy()), k
        d = p["depth"]
        assert np.array_equal(_png(paths["depth"]), _torch_u8((d - d.min()) / (d.max() - d.min()), 0.5).cpu().numpy())
        assert float(p["diffuse"].max()) > 0 and float(p["specular"].max()) > 0 and float(d.max()) > 0
    want = ev.results()
    ev.close()
    ev0.close()
    with open(os.path.join(out, "test", "ours_7", "pbr", names[-1] + "_NVS.json")) as f:
        nvs = json.load(f)
    assert sorted(nvs) == ["psnr_avg", "ssim_avg"]
    assert nvs["psnr_avg"] == want["psnr_avg"] and nvs["ssim_avg"] == want["ssim_avg"]  # same kernels, same order
    assert res["test"]["psnr_avg"] == want["psnr_avg"]
    # the environment map: the .hdr reads back as the RGBE quantisation of what the light exports
    import image_writer
    env = light.export_envmap(return_img=True).detach()
    back = image_writer.read_hdr(os.path.join(out, "test", "envmap.hdr"))
    assert back.shape == tuple(env.shape)
    assert np.array_equal(back, image_writer._rgbe_to_float(image_writer.float_to_rgbe(env.clamp(min=0).cpu().numpy())))
    assert np.array_equal(_png(os.path.join(out, "test", "unscaled_envmap.png")), _torch_u8(env.permute(2, 0, 1), 0.5).cpu().numpy())
    assert np.array_equal(_png(os.path.join(out, "test", "envmap.png")),
                          _torch_u8(env.permute(2, 0, 1) / env.max(), 0.5).cpu().numpy())


def test_brdf_eval_writes_ratio_and_metrics(trained):
    """After the pbr run: ground-truth albedo files beside the frames (Synthetic4Relight's naming), then --brdf_eval."""
    import json

    from PIL import Image as PILImage

    import evaluate
    import pipeline
    import render_scene
    src, out, ck = trained
    pbr_dir = os.path.join(out, "test", "ours_7", "pbr")
    if not os.path.exists(os.path.join(pbr_dir, "test_0_albedo.png")):
        render_scene.render_scene(["-m", out, "--checkpoint", ck, "--pbr", "--metallic", "--skip_train"])
    os.makedirs(os.path.join(src, "test"), exist_ok=True)
    rng = np.random.RandomState(0)
    gts, preds, masks = [], [], []
    for i in range(8):
        pred = _png(os.path.join(pbr_dir, "test_%d_albedo.png" % i)).copy()
        alpha = np.asarray(PILImage.open(os.path.join(src, "test_%d.png" % i)))[..., 3]
        gt = np.clip(pred.astype(np.int32) * 3 // 4 + rng.randint(0, 8, pred.shape), 0, 255).astype(np.uint8)
        PILImage.fromarray(np.dstack([gt, alpha]), "RGBA").save(os.path.join(src, "test", "test_%d_albedo.png" % i))
        mask = alpha > 0
        gt, pred = gt.copy(), pred.copy()
        gt[~mask] = 0
        pred[~mask] = 0
        gts.append(pipeline.srgb_to_linear(torch.from_numpy(gt).to(DEV) / 255.0))
        preds.append(torch.from_numpy(pred).to(DEV) / 255.0)
        masks.append(torch.from_numpy(mask).to(DEV))
    res = render_scene.render_scene(["-m", out, "--checkpoint", ck, "--brdf_eval", "--skip_train"])
    with open(os.path.join(pbr_dir, "albedo_ratio.json")) as f:
        ratio = json.load(f)["three_channel_ratio"]
    want = evaluate.albedo_ratio(gts, preds, masks)
    assert ratio == want.cpu().tolist() and len(ratio) == 3
    with open(os.path.join(pbr_dir, "albedo_metrics.json")) as f:
        metrics = json.load(f)
    assert metrics == evaluate.albedo_metrics(gts, preds, masks, ratio=want)
    assert res["test"]["albedo_psnr"] == metrics["albedo_psnr"]
    for i in (0, 7):
        scaled = (preds[i] * want).permute(2, 0, 1)
        assert np.array_equal(_png(os.path.join(pbr_dir, "test_%d_albedo_val.png" % i)), _torch_u8(scaled, 0.5).cpu().numpy())
        assert np.array_equal(_png(os.path.join(pbr_dir, "test_%d_albedo_srgb.png" % i)),
                              _torch_u8(pipeline.linear_to_srgb(scaled), 0.5).cpu().numpy())
        assert np.array_equal(_png(os.path.join(pbr_dir, "test_%d_albedo_val_gt.png" % i)),
                              _torch_u8(gts[i].permute(2, 0, 1), 0.5).cpu().numpy())
    os.remove(os.path.join(pbr_dir, "albedo_ratio.json"))  # the relight test below runs without a ratio


def test_relight_scene_end_to_end(trained, tmp_path):
    import image_writer
    import pipeline
    import relight
    import relight_scene
    import scenes
    src, out, ck = trained
    maps = {}
    for name, seed in (("dawn", 1), ("noon", 2)):
        path = str(tmp_path / (name + ".hdr"))
        image_writer.write_hdr(path, scenes.synthetic_envmap(64, 128, seed=seed), rle=(name == "noon"))
        maps[name] = path
    res = relight_scene.relight_scene(["-m", out, "--checkpoint", ck, "--hdri", maps["dawn"], maps["noon"], "--metallic",
                                       "--skip_train"])
    g, _, cams, deg = _hand_setup(src, ck)
    names = [c["image_name"] for c in cams]
    listed = relight_scene.planned_paths(out, "test", 7, names, ["dawn", "noon"])
    for path in listed:
        assert os.path.exists(path), path
    assert res["test"]["files"] == len(listed) == 2 + 8 * 4 and res["test"]["albedo_ratio"] is None
    lights = [relight.make_light(torch.from_numpy(image_writer.read_hdr(maps[n])).to(DEV), res=256) for n in ("dawn", "noon")]
    mr = relight.MultiRelighter(lights, dict(scenes.GI_DEFAULTS), deg, metallic=True)
    rays = pipeline.canonical_rays(cams[0], DEV)
    for idx in (0, 5):
        c = cams[idx]
        o = mr(c, g, pipeline.view_dirs_for(c, rays, DEV), alpha_mask=c["gt_alpha_mask"])
        paths = relight_scene.view_paths(out, "test", 7, c["image_name"], ["dawn", "noon"])
        for k in range(2):
            assert np.array_equal(_png(paths[2 * k]), _torch_u8(o["render_rgb"][k], 0.5).cpu().numpy()), paths[2 * k]
            assert np.array_equal(_png(paths[2 * k + 1]), _torch_u8(o["occlusion"], 0.5).cpu().numpy())
        assert not np.array_equal(_png(paths[0]), _png(paths[2]))  # two lights, two images
    mr.close()
    for n, light in zip(("dawn", "noon"), lights):
        env = light.export_envmap(return_img=True).permute(2, 0, 1).clamp(0.0, 1.0)
        assert np.array_equal(_png(os.path.join(out, "test", "envmap_relight_%s.png" % n)), _torch_u8(env, 0.5).cpu().numpy())
    # one map alone writes the same files for that map, byte for byte
    noon = [p for p in listed if "noon" in os.path.basename(p)]
    before = {p: open(p, "rb").read() for p in noon}
    for p in noon:
        os.remove(p)
    relight_scene.relight_scene(["-m", out, "--checkpoint", ck, "--hdri", maps["noon"], "--metallic", "--skip_train"])
    for p in noon:
        assert open(p, "rb").read() == before[p], p
    # --gt_dir: relight_eval.py's metrics.  Ground truth = the written prediction plus 3 grey levels (clipped), so every
    # pixel is off by at most 3/255 and the PSNR is at least 20 log10(255 / 3) = 38.58 dB
    import json

    from PIL import Image as PILImage
    os.makedirs(str(tmp_path / "gt" / "noon"))
    for n in names:
        pred = _png(os.path.join(out, "test", "ours_7", "relight", "%s_noon.png" % n)).astype(np.int32)
        PILImage.fromarray(np.clip(pred + 3, 0, 255).astype(np.uint8), "RGB").save(str(tmp_path / "gt" / "noon" / (n + ".png")))
    res = relight_scene.relight_scene(["-m", out, "--checkpoint", ck, "--hdri", maps["noon"], "--metallic", "--skip_train",
                                       "--gt_dir", str(tmp_path / "gt")])
    with open(os.path.join(out, "test", "ours_7", "relight", "noon.json")) as f:
        m = json.load(f)
    assert sorted(m) == ["psnr_avg", "ssim_avg"] and m == res["test"]["metrics"]["noon"]
    assert 38.58 <= m["psnr_avg"] < 100.0 and 0.0 < m["ssim_avg"] <= 1.0
