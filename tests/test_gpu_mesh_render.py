"""GPU: the mesh rasterizer (csrc/mesh_raster.hip through mesh_render.py) against its numpy restatement
(tests/mesh_raster_ref.py), the mesh relighters against relight.py's op sequence on the same planes, and render_mesh.py.

Coverage and visibility are integer decisions on the projected screen integers, so the raster + resolve tests run the
restatement on the GPU's own projected arrays and compare tri_id as integers, without an exemption; the float planes
are compared within 1e-5 (the mesh tests' bound for attributes in [-1, 1]: a handful of fp32 operations on such values).
The projection itself may differ from numpy in the last bit of u, which moves rint(256 u) by at most one unit: under the
library's contract (every operation rounded on its own, IEEE division) all integers should be equal."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_raster_ref as rr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PW, PH = rr.PW, rr.PH
ATTR = ("normals", "albedo", "roughness", "metallic")
FLOAT_PLANES = ("opacity", "depth", "pos", "normal", "albedo", "roughness", "metallic")


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cam_t(cam):
    return {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}


@functools.lru_cache(maxsize=None)
def _mesh():
    return rr.sphere_mesh()[0]


@functools.lru_cache(maxsize=None)
def _cams():
    return rr.sphere_cameras(seventh=True)


@functools.lru_cache(maxsize=None)
def _rast():
    import mesh_render
    return mesh_render.MeshRasterizer(_mesh(), device=DEV)


def _host(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def test_projection_matches_the_restatement():
    m, rast = _mesh(), _rast()
    for v, cam in enumerate(_cams()[:6]):
        view_pos, screen, flags = (t.cpu().numpy() for t in rast.project(cam_t(cam)))
        rp, rs, rf = rr.project(m["vertices"], cam)
        d = np.abs(screen.astype(np.int64) - rs)
        print("view %d: view_pos max error %.3g, screen integers equal at %d of %d" % (
            v, float(np.abs(view_pos - rp).max()), int((d == 0).all(1).sum()), len(d)))
        assert np.abs(view_pos - rp).max() <= 1e-5
        assert d.max() <= 1 and (d == 0).all(1).mean() >= 0.99
        assert np.array_equal(flags, rf) and not flags.any()


@functools.lru_cache(maxsize=None)
def _gpu_and_ref(view):
    """One view on the GPU, and the restatement on the GPU's projected arrays.  Read-only for the tests."""
    m, rast, cam = _mesh(), _rast(), _cams()[view]
    got = _host(rast(cam_t(cam)))
    view_pos, screen, flags = rast._view_pos.cpu().numpy(), rast._screen.cpu().numpy(), rast._flags.cpu().numpy()
    vis = rast._vis.cpu().numpy().view(np.uint64)
    ref_vis = rr.raster(m["faces"], view_pos, screen, flags, PW, PH)
    ref = rr.resolve(ref_vis, m["faces"], view_pos, screen, flags, m["normals"], m["albedo"], m["roughness"], m["metallic"],
                     cam["viewmatrix"])
    return got, vis, ref, ref_vis, screen


@pytest.mark.parametrize("view", range(7))
def test_raster_and_resolve_match_the_restatement(view):
    got, vis, ref, ref_vis, _ = _gpu_and_ref(view)
    assert np.array_equal(got["tri_id"], ref["tri_id"])
    covered = int((ref["tri_id"] >= 0).sum())
    assert covered == PW * PH if view == 6 else 300 < covered < PW * PH
    print("view %d: covered %d, key planes bit-equal: %s" % (view, covered, np.array_equal(vis, ref_vis)))
    for k in FLOAT_PLANES:
        assert np.abs(got[k] - ref[k]).max() <= 1e-5, k
    assert np.allclose(got["normal_view"], ref["normal_view"], rtol=0, atol=1e-5, equal_nan=True)
    assert np.array_equal(np.isnan(got["normal_view"]).any(0), ref["tri_id"] < 0)
    # the depth plane has the bits of the winning key
    hit = got["tri_id"] >= 0
    assert np.array_equal((vis[hit] >> np.uint64(32)).astype(np.uint32), got["depth"][0][hit].view(np.uint32))
    assert (vis[~hit] == rr.EMPTY).all()


def _box_pixels(screen, faces):
    s = screen.astype(np.int64)[faces]  # [F,3,2]
    lo, hi = -(-s.min(1) // rr.SUB), s.max(1) // rr.SUB
    lo = np.maximum(lo, 0)
    hi = np.minimum(hi, np.array([PW - 1, PH - 1]))
    return np.prod(np.maximum(hi - lo + 1, 0), axis=1)


@pytest.mark.parametrize("view", [0, 6])
def test_both_paths_and_every_small_max_give_the_same_bits(view):
    import gigs_lib
    rast, cam = _rast(), cam_t(_cams()[view])
    base = {k: v.clone() for k, v in rast(cam).items()}
    base_vis = rast._vis.clone()
    if view == 6:
        # real work on both sides of every threshold below.  The restatement's projection of this view has 1357 triangles
        # with a box in the image: 1194 of at most 8 pixels, 143 of 9..64, 20 of 65..81
        boxes = _box_pixels(rast._screen.cpu().numpy(), _mesh()["faces"])
        assert boxes.max() == 81 and (boxes > gigs_lib.MESH_SMALL_MAX).sum() >= 10
        assert ((boxes > 8) & (boxes <= gigs_lib.MESH_SMALL_MAX)).sum() >= 100 and ((boxes > 0) & (boxes <= 8)).sum() >= 1000
    for small_max in (0, 8, gigs_lib.MESH_SMALL_MAX, 2 ** 30):
        out = rast(cam, small_max=small_max)
        assert torch.equal(rast._vis, base_vis), small_max
        for k in base:
            a, b = out[k], base[k]
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num()), (small_max, k)


def test_owner_rule_on_edges_through_pixel_centres():
    import mesh_render
    screen, faces, interior, (W, H) = rr.owner_rule_case()
    V = len(screen)
    view_pos = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (V, 1))
    flags = np.zeros(V, np.uint8)
    ref_vis, cover = rr.raster(faces, view_pos, screen, flags, W, H, counts=True)
    assert cover.max() == 1 and (cover[interior] == 1).all()
    dummy = dict(vertices=view_pos, faces=faces, normals=view_pos, albedo=view_pos, roughness=view_pos[:, 0],
                 metallic=view_pos[:, 0])
    with mesh_render.MeshRasterizer(dummy, device=DEV) as rast:
        for small_max in (0, None, 2 ** 30):
            vis = rast.raster(W, H, view_pos=tt(view_pos), screen=tt(screen), flags=tt(flags),
                              small_max=small_max).cpu().numpy().view(np.uint64)
            owner = np.where(vis == rr.EMPTY, -1, (vis & np.uint64(0xFFFFFFFF)).astype(np.int64))
            ref_owner = np.where(ref_vis == rr.EMPTY, -1, (ref_vis & np.uint64(0xFFFFFFFF)).astype(np.int64))
            assert np.array_equal(owner, ref_owner), small_max  # one owner inside the union, none outside
            assert np.array_equal(owner >= 0, cover == 1)


def _view_space_cam(W=PW, H=PH, tanfovx=0.36):
    return dict(viewmatrix=np.eye(4, dtype=np.float32), tanfovx=tanfovx, tanfovy=tanfovx * H / W, image_width=W, image_height=H)


def _small_mesh(vertices, faces):
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    n = len(v)
    rng = np.random.default_rng(3)
    return dict(vertices=v, faces=np.asarray(faces, np.int32).reshape(-1, 3), normals=rng.normal(size=(n, 3)).astype(np.float32),
                albedo=rng.uniform(size=(n, 3)).astype(np.float32), roughness=rng.uniform(size=n).astype(np.float32),
                metallic=rng.uniform(size=n).astype(np.float32))


def _assert_background(o):
    assert bool((o["tri_id"] == -1).all()) and bool((o["opacity"] == 0).all()) and bool((o["depth"] == 0).all())
    assert bool((o["roughness"] == 1).all()) and bool(torch.isnan(o["normal_view"]).all())
    for k in ("pos", "normal", "albedo", "metallic"):
        assert bool((o[k] == 0).all()), k


def test_ties_drops_and_the_guard_band():
    import mesh_render
    cam = _view_space_cam()
    tri = [(-0.3, -0.3, 2.0), (0.4, -0.2, 2.0), (0.0, 0.5, 2.0)]
    with mesh_render.MeshRasterizer(_small_mesh(tri, [(0, 1, 2), (0, 1, 2)]), device=DEV) as rast:
        o = rast(cam)  # two identical triangles: the lower index wins
        ids = o["tri_id"]
        assert int((ids == 0).sum()) > 100 and bool(((ids == 0) | (ids == -1)).all())
        assert float((o["depth"][0][ids == 0] - 2.0).abs().max()) <= 1e-5
    near = tri[:2] + [(0.0, 0.05, 0.1)]
    for vertices, faces in ((tri, [(0, 1, 1)]), (tri, [(0, 1, 3)]), (tri, [(0, -1, 2)]), (near, [(0, 1, 2)]),
                            (tri, np.zeros((0, 3), np.int32)), (np.zeros((0, 3)), [(0, 1, 2)])):
        with mesh_render.MeshRasterizer(_small_mesh(vertices, faces), device=DEV) as rast:
            for small_max in (0, None):
                _assert_background(rast(cam, small_max=small_max))
            if vertices is near:
                assert rast._flags.cpu().tolist() == [0, 0, 1]
    big = [(-100.0, -100.0, 1.0), (100.0, -100.0, 1.0), (0.0, 150.0, 1.0)]  # thousands of pixels beyond every border
    with mesh_render.MeshRasterizer(_small_mesh(big, [(0, 1, 2)]), device=DEV) as rast:
        for small_max in (0, None, 2 ** 30):
            o = rast(cam, small_max=small_max)
            assert bool((o["tri_id"] == 0).all()) and bool((o["opacity"] == 1).all())
            assert float((o["depth"] - 1.0).abs().max()) <= 1e-5
        assert int(rast._screen.abs().max()) > 256 * 5000 and not bool(rast._flags.any())
    far = [(10.0 * x, 10.0 * y, z) for x, y, z in big]  # outside the guard band: no clipping, the triangle is dropped
    with mesh_render.MeshRasterizer(_small_mesh(far, [(0, 1, 2)]), device=DEV) as rast:
        _assert_background(rast(cam))
        assert bool(rast._flags.all()) and int(rast._screen.abs().max()) == 0


# ---- relighting ----------------------------------------------------------------------------------------------------------
RW, RH, RES = 176, 144, 64  # tests/test_gpu_relight.py's small case


@functools.lru_cache(maxsize=None)
def _relight_setup():
    import mesh_render
    import pipeline
    import relight
    import scenes
    m = dict(_mesh())
    m["normals"] = (m["vertices"] / np.linalg.norm(m["vertices"], axis=1, keepdims=True)).astype(np.float32)
    # a convex body alone reflects nothing of itself: a ground plane under the sphere (the stand-in scenes' z = -0.65) gives
    # the SSR march something to hit, and triangles of thousands of pixels for the wave path
    n = 7
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, n), np.linspace(-1.6, 1.6, n), indexing="xy")
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(n * n, -0.65)], axis=1).astype(np.float32)
    cell = np.array([(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, j * n + i, (j + 1) * n + i + 1, (j + 1) * n + i)
                     for j in range(n - 1) for i in range(n - 1)], np.int32).reshape(-1, 3)
    rng = np.random.default_rng(11)
    V0 = len(m["vertices"])
    m["vertices"] = np.concatenate([m["vertices"], ground])
    m["faces"] = np.concatenate([m["faces"], cell + V0])
    m["normals"] = np.concatenate([m["normals"], np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n * n, 1))])
    m["albedo"] = np.concatenate([m["albedo"], rng.uniform(0.2, 0.9, size=(n * n, 3)).astype(np.float32)])
    m["roughness"] = np.concatenate([m["roughness"], rng.uniform(0.1, 0.6, size=n * n).astype(np.float32)])
    m["metallic"] = np.concatenate([m["metallic"], rng.uniform(0.0, 1.0, size=n * n).astype(np.float32)])
    rast = mesh_render.MeshRasterizer(m, device=DEV)
    cam = scenes.orbit_camera(1, 8, RW, RH, radius=3.5)
    lights = [relight.make_light(tt(scenes.synthetic_envmap(128, 256, seed=5 + k)), res=RES) for k in range(3)]
    c = cam_t(cam)
    vd = pipeline.view_dirs_for(c, pipeline.canonical_rays(cam, DEV), DEV)
    return rast, c, vd, lights


@pytest.mark.parametrize("metallic", [False, True])
def test_mesh_relighter_equals_the_op_sequence_on_the_same_planes(metallic):
    """relight.Relighter._unfused's sequence, spelled with the drop-in operators on mesh_planes' output; the bound is
    tests/test_gpu_relight.py's for fused against unfused."""
    import mesh_render
    import pipeline
    import scenes
    from diff_gaussian_rasterization import Gaussian_SSR, filters
    from pbr import get_brdf_lut, pbr_shading
    rast, cam, vd, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    light = lights[0]
    rl = mesh_render.MeshRelighter(light, gi, metallic=metallic)
    ratio = (0.9, 1.1, 0.8) if metallic else None
    alpha = tt((np.random.default_rng(0).uniform(size=(1, RH, RW)) > 0.1).astype(np.float32))
    out = rl(cam, rast, vd, alpha_mask=alpha, albedo_ratio=ratio)
    assert int((out["tri_id"] >= 0).sum()) > 2000

    r = mesh_render.mesh_planes(rast, cam, gi)
    _, _, normals_view, normal_mask, onv = pipeline.gbuffer_post(r["normal_map_from_depth"], r["normal_map"],
                                                                 r["out_normal_view"], r["viewmatrix"])
    albedo_map, roughness_map, metallic_map = r["albedo_map"], r["roughness_map"], r["metallic_map"]
    rt = torch.ones(3, device=DEV) if ratio is None else torch.tensor(ratio, dtype=torch.float32, device=DEV)
    res = pbr_shading(light=light, normals=normals_view.permute(1, 2, 0), view_dirs=vd, mask=normal_mask.permute(1, 2, 0),
                      albedo=(albedo_map * rt[:, None, None]).permute(1, 2, 0), roughness=roughness_map.permute(1, 2, 0),
                      metallic=metallic_map.permute(1, 2, 0) if metallic else None, tone=False,
                      occlusion=r["occlusion_map"].permute(1, 2, 0), gamma=False, brdf_lut=get_brdf_lut().to(DEV))
    render_direct = torch.where(normal_mask, res["render_rgb"].permute(2, 0, 1), torch.zeros(3, device=DEV)[:, None, None])
    ssr = Gaussian_SSR(cam["tanfovx"], cam["tanfovy"], RW, RH, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"],
                       gi["start"])
    if metallic:  # relight.py:236-240, as written
        F0, metallic_in = torch.ones_like(albedo_map) * 0.04, torch.zeros_like(roughness_map)
    else:
        F0, metallic_in = (1.0 - float(metallic)) * 0.04 + albedo_map * metallic_map, metallic_map
    IRR, _ = ssr(onv, r["depth_pos"], pipeline.srgb_to_linear(render_direct), albedo_map, roughness_map, metallic_in, F0)
    render_rgb = (render_direct + filters.median_blur(pipeline.linear_to_srgb(IRR)[None, ...], (3, 3))[0]) * alpha
    want = dict(render_direct=render_direct, IRR=IRR, render_rgb=render_rgb)
    for k, w in want.items():
        d = float((out[k].nan_to_num() - w.nan_to_num()).abs().max())
        print("metallic %s, %s: max difference %.3g" % (metallic, k, d))
        assert d <= 2e-6, k
    assert torch.equal(out["occlusion"], r["occlusion_map"]) and torch.equal(out["depth_map"], r["depth_map"])
    assert float(out["render_rgb"].nan_to_num().max()) > 0.2 and float(out["IRR"].nan_to_num().max()) > 0
    assert float(out["render_rgb"][:, alpha[0] == 0].abs().max()) == 0.0
    assert out["radii"] is None and torch.equal(out["albedo_map"], albedo_map)


def test_multi_and_turntable_equal_the_single_light_relighter():
    import mesh_render
    import scenes
    rast, cam, vd, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    ratio = (0.9, 1.1, 0.8)
    single = []
    for light in lights:
        o = mesh_render.MeshRelighter(light, gi)(cam, rast, vd, albedo_ratio=ratio)
        single.append({k: o[k].clone() for k in ("render_rgb", "render_direct", "IRR")})
    multi = mesh_render.MeshMultiRelighter(lights, gi)(cam, rast, vd, albedo_ratio=ratio)
    with mesh_render.MeshTurntableRelighter(lights, gi) as tr:
        turn = tr(cam, rast, vd, albedo_ratio=ratio)
        assert tr.last_hits is not None and tr.last_hits > 0  # the recorded march, not the fallback
    for name, o in (("multi", multi), ("turntable", turn)):
        assert tuple(o["render_rgb"].shape) == (3, 3, RH, RW) and o["tri_id"].dtype == torch.int32
        for k, want in enumerate(single):
            for key, w in want.items():
                a = o[key][k]
                assert torch.equal(torch.isnan(a), torch.isnan(w)) and torch.equal(a.nan_to_num(), w.nan_to_num()), (name, k, key)


def test_graphs_are_refused():
    import mesh_render
    import scenes
    _, _, _, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    for make in (lambda: mesh_render.MeshRelighter(lights[0], gi, graphs=True),
                 lambda: mesh_render.MeshMultiRelighter(lights, gi, graphs=True),
                 lambda: mesh_render.MeshTurntableRelighter(lights, gi, graphs=True)):
        with pytest.raises(ValueError, match="graphs"):
            make()
    with pytest.raises(TypeError, match="MeshRasterizer"):
        mesh_render.MeshRelighter(lights[0], gi)(None, {"means3D": None}, None)


# ---- the command-line tool -------------------------------------------------------------------------------------------------
def test_render_mesh_tool(tmp_path):
    """extract_mesh.py then render_mesh.py --compare on a scene folder and an output folder as trainer.py leaves them
    (the helpers of tests/test_gpu_mesh.py's tool test).  No threshold on the PSNR: the files exist, the PNGs decode, the
    JSON is finite."""
    from argparse import Namespace

    from PIL import Image

    import densify
    import extract_mesh
    import optim
    import relight
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    import train_iteration as ti
    src = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=6, size=64)
    out = str(tmp_path / "run")
    os.makedirs(out)
    raw = ti.raw_from_scene(scenes.surface_scene(P=4000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [raw[k]], "lr": 0.0, "name": k} for k in raw], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, raw, densify.DensifyState(raw["xyz"].shape[0], DEV), opt, 1.0),
                             light.state_dict(), {}, 7)
    with open(os.path.join(out, "cfg_args"), "w") as f:
        f.write(str(Namespace(sh_degree=3, source_path=src, model_path=out, images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)))
    ex = extract_mesh.extract_mesh(["-m", out, "--checkpoint", ck, "--grid", "32", "--split", "test"])
    assert ex["faces"] > 0
    res = render_mesh.render_mesh(["-m", out, "--mesh", "mesh.ply", "--checkpoint", ck, "--compare", "--split", "train"])
    assert res["n_views"] == 2 and res["faces"] == ex["faces"] and res["lights"] == ["trained"]
    folder = os.path.join(out, "mesh_train")
    files = sorted(os.listdir(folder))
    assert len(files) == 2 * 7 and res["files"] == 14
    for name in files:
        img = np.array(Image.open(os.path.join(folder, name)))
        assert img.shape[:2] == (64, 64), name
    lit = [np.array(Image.open(os.path.join(folder, n))) for n in files if n.endswith("_trained.png")]
    assert len(lit) == 2 and all(int(a.max()) > 0 for a in lit)
    with open(os.path.join(out, "mesh_vs_splat.json")) as f:
        cmp = json.load(f)
    assert cmp["light"] == "trained" and len(cmp["views"]) == 2
    for v in cmp["views"] + [cmp["average"]]:
        for k in ("relit_psnr", "relit_ssim", "albedo_psnr", "albedo_ssim", "depth_abs_diff"):
            assert np.isfinite(v[k]), (k, v)
    assert all(v["pixels_both_cover"] > 0 for v in cmp["views"])
    print("mesh against splats:", json.dumps(cmp["average"]))
    # a map with rotations and no checkpoint: the cameras come from cfg_args alone
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    res2 = render_mesh.render_mesh(["-m", out, "--mesh", os.path.join(out, "mesh.ply"), "--hdri", hdr, "--rotations", "2",
                                    "--split", "train"])
    assert res2["lights"] == ["sky_rot000", "sky_rot001"] and "compare" not in res2
    assert sum(n.endswith("_sky_rot001.png") for n in os.listdir(folder)) == 2
