"""Novel-view evaluation on the GPU (gi-gs_amd/evaluate.py): CubemapLight.export_envmap, the pad_normal G-buffer
post (gigs_gbuffer_post_pad), the per-view metrics (gigs_image_metrics, gigs_normal_angular_error) against float64
restatements, and NovelViewEvaluator against the CPU oracle composition of render.py's pbr branch."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scenes
from oracle import stage2_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = stage2_ref.KEYS


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cam_t(cam):
    return {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}


def view_dirs(cam):
    import pipeline
    return pipeline.view_dirs_for(cam_t(cam), pipeline.canonical_rays(cam, DEV), DEV)


def ssim64(a, b):
    """utils/loss_utils.py:55-98 in float64: window 11 (its fp32 Gaussian), zero padding, depthwise conv2d."""
    x, y = torch.as_tensor(a).double()[None], torch.as_tensor(b).double()[None]
    C = x.shape[1]
    g = torch.tensor([math.exp(-((i - 5) ** 2) / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    g = (g / g.sum()).double()
    w = (g[:, None] @ g[None, :]).expand(C, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 ** 2, conv(y * y) - mu2 ** 2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s11 + s22 + C2))
    return float(m.mean())


def psnr_mean64(a, b):
    return float(np.mean(stage2_ref.psnr(np.asarray(a, np.float64), np.asarray(b, np.float64))))


# ---- 1. export_envmap -------------------------------------------------------------------------------------------
def test_export_envmap():
    import relight
    from pbr import CubemapLight
    from pbr.texture import cube_texture
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=256)
    img = light.export_envmap(return_img=True)
    assert tuple(img.shape) == (512, 1024, 3)
    res = [512, 1024]
    gy, gx = torch.meshgrid(torch.linspace(0.0 + 1.0 / res[0], 1.0 - 1.0 / res[0], res[0], device=DEV),
                            torch.linspace(-1.0 + 1.0 / res[1], 1.0 - 1.0 / res[1], res[1], device=DEV), indexing="ij")
    st, ct, sp, cp = torch.sin(gy * np.pi), torch.cos(gy * np.pi), torch.sin(gx * np.pi), torch.cos(gx * np.pi)
    refl = torch.stack((st * sp, ct, -st * cp), dim=-1)
    assert torch.equal(img, cube_texture(light.base, refl))
    # render.py:143, as written
    assert tuple(light.export_envmap(return_img=True).permute(2, 0, 1).shape) == (3, 512, 1024)
    # lit on face 2 (+y) only: only the top of the panorama is lit
    top = CubemapLight(base_res=32, device=DEV)
    with torch.no_grad():
        top.base.zero_()
        top.base[2] = 1.0
    im = top.export_envmap(return_img=True, res=[64, 128])
    im_d = im.detach()
    assert float(im_d[:8].min()) > 0.9 and float(im_d[32:].abs().max()) == 0.0
    # differentiable w.r.t. base
    im.sum().backward()
    assert top.base.grad is not None and float(top.base.grad[2].sum()) > 0


# ---- 2. the pad_normal G-buffer post ----------------------------------------------------------------------------
def test_gbuffer_post_pad_matches_torch_path():
    import gigs_lib
    import pipeline
    lib = gigs_lib.lib()
    W, H = 176, 144
    sc = scenes.surface_scene(P=9000, sh_degree=2, seed=4, scale_mu=0.03)
    cam = scenes.orbit_camera(1, 8, W, H, radius=3.5)
    g = {k: tt(sc[k]) for k in KEYS}
    with torch.no_grad():
        (out, _, st) = pipeline.rasterize(cam_t(cam), g, 2, torch.zeros(3, device=DEV), scenes.GI_DEFAULTS, inference=True)
    (_, _, opac, _, nfd, nm, _, _, _, _, onv, _) = out
    opac = opac.clone()
    flat = opac.view(-1)
    vals = torch.tensor([0.003, 0.004, 0.996, 0.997], device=DEV)
    flat[torch.arange(400, 800, device=DEV)] = vals.repeat(100)
    vm = st.viewmatrix.contiguous().float()
    ref = pipeline.gbuffer_post(nfd, nm, onv, vm, opacity_map=opac, pad_normal=True)
    e = lambda *s: torch.empty(s, device=DEV)  # noqa: E731
    nv, onv_o, nfd_o, world, op_o, mf = e(3, H, W), e(3, H, W), e(3, H, W), e(3, H, W), e(1, H, W), e(1, H, W)
    mu = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    gigs_lib.check(lib.gigs_gbuffer_post_pad(H, W, nm.data_ptr(), nfd.data_ptr(), opac.data_ptr(), onv.data_ptr(),
                                             vm.data_ptr(), mu.data_ptr(), mf.data_ptr(), world.data_ptr(), nv.data_ptr(),
                                             onv_o.data_ptr(), nfd_o.data_ptr(), op_o.data_ptr(), None), "pad")
    torch.cuda.synchronize()
    r_nfd, _, r_nv, r_mask, r_onv, r_op = ref
    assert torch.equal(mu.bool()[None], r_mask) and torch.equal(mf.bool(), r_mask)
    assert int(r_mask.sum()) > 1000 and int((~r_mask).sum()) > 1000
    assert torch.equal(op_o, r_op)
    assert int((op_o == 0).sum()) >= 100 and int((op_o == 1).sum()) >= 100
    for a, b in ((nv, r_nv), (onv_o, r_onv), (nfd_o, r_nfd)):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert float((a.nan_to_num() - b.nan_to_num()).abs().max()) <= 1e-6
    R = vm[:3, :3]
    assert float((-(world.permute(1, 2, 0) @ R).permute(2, 0, 1) - nv).nan_to_num().abs().max()) <= 1e-6
    # gigs_gbuffer_post (pad_normal=False) keeps its results
    nv2, onv2 = e(3, H, W), e(3, H, W)
    gigs_lib.check(lib.gigs_gbuffer_post(H, W, nm.data_ptr(), onv.data_ptr(), vm.data_ptr(), nv2.data_ptr(), mu.data_ptr(),
                                         None, onv2.data_ptr(), None), "post")
    torch.cuda.synchronize()
    _, _, q_nv, q_mask, q_onv = pipeline.gbuffer_post(nfd, nm, onv, vm)
    assert torch.equal(mu.bool()[None], q_mask)
    assert float((nv2 - q_nv).nan_to_num().abs().max()) <= 1e-6 and float((onv2 - q_onv).nan_to_num().abs().max()) <= 1e-6


# ---- 3. per-view image metrics ----------------------------------------------------------------------------------
def _check_record(rec, a, b, mask=None):
    rec = rec.cpu().numpy()
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    mse = ((a64 - b64) ** 2).reshape(a.shape[0], -1).mean(1)
    np.testing.assert_allclose(rec[:3], mse, rtol=1e-6)
    assert abs(rec[3] - psnr_mean64(a, b)) <= 1e-4
    s = ssim64(a, b)
    assert abs(rec[4] - s) <= 1e-6 * abs(s), (rec[4], s)
    if mask is not None:
        m = np.asarray(mask, bool)
        want = ((a64 - b64) ** 2)[:, m].mean()
        assert abs(rec[5] - want) <= 1e-6 * want and rec[6] == 3 * m.sum()


def test_image_metrics_random_and_reproducible():
    import evaluate
    rng = np.random.default_rng(3)
    C, H, W = 3, 150, 203
    gt = rng.uniform(size=(C, H, W)).astype(np.float32)
    pred = np.clip(gt + 0.1 * rng.standard_normal((C, H, W)), 0, 1).astype(np.float32)
    mask = rng.uniform(size=(H, W)) > 0.4
    r1 = evaluate.image_metrics(tt(pred), tt(gt), mask=tt(mask))
    r2 = evaluate.image_metrics(tt(pred), tt(gt), mask=tt(mask))
    assert torch.equal(r1, r2)
    _check_record(r1, pred, gt, mask)
    # slot mode: six views into successive rows == six single calls
    preds = [np.clip(gt + s * rng.standard_normal((C, H, W)), 0, 1).astype(np.float32) for s in (0.01, 0.03, 0.05, 0.1, 0.2, 0.3)]
    out = torch.full((6, C + 4), -1.0, dtype=torch.float64, device=DEV)
    slot = torch.zeros(1, dtype=torch.int32, device=DEV)
    for p in preds:
        evaluate.image_metrics(tt(p), tt(gt), mask=tt(mask), slot=slot, out=out)
    assert int(slot) == 6
    for i, p in enumerate(preds):
        assert torch.equal(out[i], evaluate.image_metrics(tt(p), tt(gt), mask=tt(mask)))


# ---- 4. NovelViewEvaluator against the oracle composition -------------------------------------------------------
def _oracle_view(orc, sc, cam, gi, diffuse, spec, gt, alpha, metallic):
    """render.py:196-363 for one view from the CPU oracle pieces."""
    _f32 = np.float32
    H, W = cam["image_height"], cam["image_width"]
    fx, fy = stage2_ref.focal(cam)
    raw = stage2_ref.operator_forward(orc, sc, cam, gi, 2, inference=True)
    post = stage2_ref.gbuffer_post(orc, raw, cam["viewmatrix"], pad_normal=True)
    vd = stage2_ref.canonical_view_dirs(cam)
    direct = stage2_ref.shade_direct(orc, post, vd, post["albedo_map"], post["roughness_map"],
                                     post["metallic_map"] if metallic else None, post["occlusion_map"], diffuse, spec,
                                     stage2_ref.brdf_lut())
    if metallic:
        F0 = (_f32(0.0) + post["albedo_map"] * post["metallic_map"]).astype(_f32)
        metal = post["metallic_map"]
    else:
        F0 = np.full_like(post["albedo_map"], 0.04)
        metal = np.zeros_like(post["roughness_map"])
    a = (gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
    irr, _ = orc.ssr(W, H, fx, fy, *a, post["out_normal_view"], post["depth_pos"], stage2_ref.srgb_to_linear(direct),
                     post["albedo_map"], post["roughness_map"], metal, F0)
    irr2 = orc.median3x3(stage2_ref.linear_to_srgb(irr)).astype(_f32)
    mask = post["normal_mask"]
    pbr = np.where(mask, direct + irr2, _f32(0)).astype(_f32)
    comp = lambda x: np.clip(x * alpha, 0, 1).astype(_f32)  # noqa: E731
    gt_c = np.clip(gt * alpha, 0, 1).astype(_f32)
    occ = np.broadcast_to(comp(post["occlusion_map"]), (3, H, W))
    return dict(pbr=pbr, DIR=(pbr - irr2).astype(_f32), indirect=irr2, occlusion=occ, gt=gt_c)


@pytest.mark.parametrize("metallic", [False, True])
def test_evaluator_matches_oracle(orc, metallic):
    import evaluate
    import relight
    W, H, res = 176, 144, 64
    sc = scenes.surface_scene(P=9000, sh_degree=2, seed=4, scale_mu=0.03)
    cam = scenes.orbit_camera(1, 8, W, H, radius=3.5)
    gi = scenes.GI_DEFAULTS
    env = scenes.synthetic_envmap(128, 256, seed=5)
    rng = np.random.default_rng(1)
    alpha = (rng.uniform(size=(1, H, W)) > 0.1).astype(np.float32)
    gt = rng.uniform(size=(3, H, W)).astype(np.float32)
    light = relight.make_light(tt(env), res=res)
    diffuse, spec = stage2_ref.build_mips(orc, light.base.detach().cpu().numpy())
    ref = _oracle_view(orc, sc, cam, gi, diffuse, spec, gt, alpha, metallic)
    g = {k: tt(sc[k]) for k in KEYS}
    for fused in (False, True):
        ev = evaluate.NovelViewEvaluator(light, gi, 2, metallic=metallic, graphs=False, fused=fused)
        out = ev(cam_t(cam), g, view_dirs(cam), tt(gt), tt(alpha))
        for k in ("pbr", "DIR", "indirect", "occlusion"):
            a, b = out[k].cpu().numpy(), ref[k]
            assert a.shape == b.shape, (k, a.shape, b.shape)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (fused, k)
            d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
            assert d.mean() <= 1e-4, (fused, k, d.mean())
            if k == "pbr":
                assert stage2_ref.psnr(np.nan_to_num(a), np.nan_to_num(b)) >= 60.0
        for k in evaluate.PLANES:
            assert tuple(out[k].shape) == (3, H, W), k
        rec = ev.records()
        assert rec.shape == (1, 7)
        ref_pbr = np.nan_to_num(ref["pbr"])
        assert abs(rec[0, 3] - psnr_mean64(ref["gt"], ref_pbr)) <= 1e-3
        assert abs(rec[0, 4] - ssim64(ref["gt"], ref_pbr)) <= 1e-3
        # the metrics on rendered images: pbr against its direct part
        a, b = out["pbr"].nan_to_num(), out["DIR"].nan_to_num()
        _check_record(evaluate.image_metrics(a, b), a.cpu().numpy(), b.cpu().numpy())
    assert float(np.nan_to_num(ref["pbr"]).max()) > 0.2 and float(np.nan_to_num(ref["indirect"]).max()) > 0


# ---- 5. C3 size: graphed == fused == op-by-op, accumulated results ----------------------------------------------
def test_evaluator_c3_graphed_fused_unfused():
    import evaluate
    import relight
    W = H = 800
    sc = scenes.surface_scene(P=300_000, sh_degree=2, seed=0)
    gi = scenes.GI_DEFAULTS
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=256)
    g = {k: tt(sc[k]) for k in KEYS}
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - 400) ** 2 + (yy - 400) ** 2) < 380 ** 2).astype(np.float32)[None])
    rng = np.random.default_rng(2)
    gt = tt(rng.uniform(size=(3, H, W)).astype(np.float32))
    evs = {m: evaluate.NovelViewEvaluator(light, gi, 2, graphs=(m == "graphed"), fused=(m != "unfused"))
           for m in ("graphed", "fused", "unfused")}
    per_view = {m: [] for m in evs}
    for view in (11, 30, 11):
        cam = scenes.orbit_camera(view, 64, W, H, radius=3.5)
        vd = view_dirs(cam)
        outs = {m: {k: v.clone() for k, v in ev(cam_t(cam), g, vd, gt, alpha).items() if k in evaluate.PLANES}
                for m, ev in evs.items()}
        for m in ("graphed", "unfused"):
            for k in evaluate.PLANES:
                d = float((outs[m][k].nan_to_num() - outs["fused"][k].nan_to_num()).abs().max())
                assert d <= 2e-6, (m, k, d)
        gt_c = (gt * alpha).clamp(0, 1)
        for m in evs:
            pbr = outs[m]["pbr"]
            one = evaluate.image_metrics(pbr, gt_c).cpu()
            per_view[m].append((psnr_mean64(gt_c.cpu().numpy(), pbr.cpu().numpy()),
                                ssim64(gt_c.cpu().numpy(), pbr.cpu().numpy()), float(one[3]), float(one[4])))
    rec = evs["graphed"].records()
    np.testing.assert_allclose(rec[0].numpy(), rec[2].numpy(), rtol=1e-6)
    for m, ev in evs.items():
        r = ev.results()
        assert r["n_views"] == 3
        # the same per-view metric calls made independently on the returned planes: the same means
        assert abs(r["psnr_avg"] - np.mean([v[2] for v in per_view[m]])) <= 1e-12, m
        assert abs(r["ssim_avg"] - np.mean([v[3] for v in per_view[m]])) <= 1e-12, m
        # and float64 restatements (the ssim map itself is fp32 on the device, as in the training loss)
        assert abs(r["psnr_avg"] - np.mean([v[0] for v in per_view[m]])) <= 1e-4, m
        assert abs(r["ssim_avg"] - np.mean([v[1] for v in per_view[m]])) <= 1e-5 * abs(r["ssim_avg"]), m
    evs["graphed"].close()


# ---- 6. normal MAE ----------------------------------------------------------------------------------------------
def _mae_numpy(preds, gts):
    """normal_eval.py:11-18 and :35-58 on PNG-rounded planes (torchvision save_image arithmetic)."""
    gt_stack, gs_stack = [], []
    bg = np.array([0.0, 0.0, 1.0])
    for p, img in zip(preds, gts):
        u8 = torch.from_numpy(p).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
        n = img[..., :3] / 255
        n = (n - 0.5) * 2.0
        a = img[..., [-1]] / 255
        n = n * a + bg * (1.0 - a)
        gt_stack.append(n / np.linalg.norm(n, axis=-1, ord=2, keepdims=True))
        q = u8 / 255
        q = (q - 0.5) * 2.0
        q[(u8 == np.array([128, 128, 255], dtype=np.uint8)).all(-1)] = np.array([0.0, 0.0, 1.0])
        gs_stack.append(q / np.linalg.norm(q, axis=-1, ord=2, keepdims=True))
    g, s = np.stack(gt_stack), np.stack(gs_stack)
    return np.mean(np.arccos(np.clip(np.sum(g * s, axis=-1), -1, 1)) * 180 / np.pi).item()


def test_normal_mae_matches_normal_eval():
    import evaluate
    rng = np.random.default_rng(7)
    H, W = 120, 97
    preds, gts = [], []
    for i in range(3):
        v = rng.standard_normal((3, H, W))
        v /= np.linalg.norm(v, axis=0, keepdims=True)
        p = ((np.clip(v, 0, 1) + 1) / 2).astype(np.float32)
        p[:, :10, :10] = np.array([128, 128, 255], np.float32)[:, None, None] / 255  # the (128,128,255) substitution
        gt = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
        gt[..., 3] = np.where(rng.uniform(size=(H, W)) > 0.3, 255, rng.integers(0, 256, size=(H, W)))
        gt[:20, :20, :3] = p[:, :20, :20].transpose(1, 2, 0) * 255 + 0.5  # near-identical normals: acos near 1
        gt[:20, :20, 3] = 255
        preds.append(p)
        gts.append(gt)
    got = evaluate.normal_mae([tt(p) for p in preds], [tt(g) for g in gts])
    want = _mae_numpy(preds, gts)
    assert abs(got - want) <= 1e-6, (got, want)
