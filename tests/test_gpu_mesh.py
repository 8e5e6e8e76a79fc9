"""GPU: TSDF fusion and surface nets (csrc/mesh.hip through mesh.py) against their numpy restatement (tests/mesh_ref.py).

Integration: weights are compared exactly, tsdf and the attributes within 1e-5 absolute (a bound on eight sequential fp32
updates of values in [-1, 1]), over every sample that is not fragile: a sample is fragile if in some view u + 0.5 or
v + 0.5 lies within 1e-4 of an integer or sdf within 1e-4 trunc of -trunc or +trunc; at most 1 % may be fragile.
Extraction runs on load()-ed fields, so both sides read identical inputs: faces are compared as integers, vertices within
1e-4 h, the other attributes within 1e-5."""
import functools

import numpy as np
import pytest
import torch

import mesh_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
DIMS = (28, 20, 24)
PW, PH = 40, 56  # plane size: no multiple of the tile or of the wave
FOVX = 0.6911
KEYS = ("opacity", "depth", "normal", "albedo", "roughness", "metallic")


def _sphere_planes(cam, seed, radius=0.6):
    """Analytic z-depth and coverage of the sphere |x| = radius at the pixel centres ((2x + 1) / W - 1) tanfov, and seeded
    random attribute planes."""
    W, H = cam["image_width"], cam["image_height"]
    m = np.asarray(cam["viewmatrix"], np.float64).reshape(16)
    c = np.array([m[12], m[13], m[14]])
    dx = ((2.0 * np.arange(W) + 1.0) / W - 1.0) * cam["tanfovx"]
    dy = ((2.0 * np.arange(H) + 1.0) / H - 1.0) * cam["tanfovy"]
    d = np.stack(np.broadcast_arrays(dx[None, :], dy[:, None], np.ones((H, W))), axis=-1)
    a, b = (d * d).sum(-1), d @ c
    disc = b * b - a * (c @ c - radius * radius)
    hit = disc > 0
    depth = np.where(hit, (b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)
    rng = np.random.default_rng(seed)
    return dict(opacity=hit.astype(np.float32)[None], depth=depth.astype(np.float32)[None],
                normal=rng.normal(size=(3, H, W)).astype(np.float32), albedo=rng.uniform(size=(3, H, W)).astype(np.float32),
                roughness=rng.uniform(size=(1, H, W)).astype(np.float32), metallic=rng.uniform(size=(1, H, W)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _views():
    import scenes
    cams = [scenes.orbit_camera(i, 6, PW, PH, radius=3.0, fovx=FOVX, elevation=0.5 if i % 2 == 0 else -0.6) for i in range(6)]
    cams += [scenes.look_at_camera((0.05, 0.02, z), (0.0, 0.0, 0.0), PW, PH, FOVX, up=(0.0, 1.0, 0.0)) for z in (3.0, -3.0)]
    return cams, [_sphere_planes(c, 100 + i) for i, c in enumerate(cams)]


def _grid():
    lo, h = mesh_ref.sphere_grid(DIMS)
    return lo, h, np.float32(3.0) * h


@functools.lru_cache(maxsize=None)
def _reference(carve):
    """The restatement's volume after the eight views, and the union of the fragile masks.  Read-only for the tests."""
    cams, planes = _views()
    lo, h, trunc = _grid()
    ref = mesh_ref.Volume(lo, h, DIMS, trunc, carve=carve)
    fragile = np.zeros(ref.tsdf.shape, bool)
    for c, p in zip(cams, planes):
        fragile |= ref.integrate(c, p)["fragile"]
    return ref, fragile


def _to_dev(planes):
    return {k: torch.from_numpy(v).to(DEV) for k, v in planes.items()}


def _volume(carve=True, dims=DIMS, lo=None, h=None, trunc=None, **kw):
    import mesh
    glo, gh, gtrunc = _grid()
    return mesh.TSDFVolume(glo if lo is None else lo, gh if h is None else h, dims, gtrunc if trunc is None else trunc,
                           carve=carve, device=DEV, **kw)


def _fields(vol):
    return (vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(), vol.attr_weight.cpu().numpy(), vol.attributes().cpu().numpy())


def _compare_volume(vol, ref, fragile, what):
    share = float(fragile.mean())
    ok = ~fragile
    tsdf, weight, attr_weight, attr = _fields(vol)
    dt, da = float(np.abs(tsdf - ref.tsdf)[ok].max()), float(np.abs(attr - ref.attr)[ok].max())
    print("%s: fragile share %.4f, max |tsdf diff| %.3g, max |attr diff| %.3g, updated %.3f, with attributes %.3f" % (
        what, share, dt, da, float((ref.weight > 0).mean()), float((ref.attr_weight > 0).mean())))
    assert share <= 0.01
    assert np.array_equal(weight[ok], ref.weight[ok])
    assert np.array_equal(attr_weight[ok], ref.attr_weight[ok])
    assert dt <= 1e-5 and da <= 1e-5
    assert (ref.weight > 0).any() and (ref.attr_weight > 0).any() and (ref.attr_weight == 0).any()


@pytest.mark.parametrize("carve", [True, False])
def test_integration_matches_the_restatement(carve):
    cams, planes = _views()
    ref, fragile = _reference(carve)
    vol = _volume(carve)
    vol.integrate(cams, [_to_dev(p) for p in planes])
    assert vol.tsdf.shape == (DIMS[2], DIMS[1], DIMS[0]) and vol.attributes().shape == (DIMS[2], DIMS[1], DIMS[0], 8)
    _compare_volume(vol, ref, fragile, "sphere carve=%s" % carve)
    if not carve:
        assert float((ref.weight > 0).mean()) < float((_reference(True)[0].weight > 0).mean())


@pytest.mark.parametrize("n", [1, 3, 8, 11])
def test_batched_views_equal_single_view_calls_bit_for_bit(n):
    cams, planes = _views()
    cams, planes = (cams + cams[:3])[:n], [_to_dev(p) for p in (planes + planes[:3])[:n]]
    a, b = _volume(), _volume()
    a.integrate(cams, planes)
    for c, p in zip(cams, planes):
        b.integrate(c, p)
    for x, y in zip((a.tsdf, a.weight, a.attr_weight, a.attributes()), (b.tsdf, b.weight, b.attr_weight, b.attributes())):
        assert torch.equal(x, y)
    assert float(a.weight.max()) >= min(n, 2)


def test_skipped_samples_keep_their_state():
    """The volume contains the camera and the view sees part of it; the opacity plane sits just below, at and just above
    opacity_min."""
    import scenes
    dims, h = (24, 18, 20), np.float32(0.1)
    lo = np.array([-1.2, -0.9, -1.0], np.float32)
    cam = scenes.look_at_camera((0.13, 0.07, -0.21), (0.2, 0.1, 1.5), 33, 47, FOVX, up=(0.0, 1.0, 0.0))
    W, H = 33, 47
    rng = np.random.default_rng(7)
    below, above = np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))
    planes = dict(opacity=rng.choice(np.array([below, 0.5, above], np.float32), size=(1, H, W)),
                  depth=rng.uniform(0.5, 1.2, size=(1, H, W)).astype(np.float32),
                  normal=rng.normal(size=(3, H, W)).astype(np.float32), albedo=rng.uniform(size=(3, H, W)).astype(np.float32),
                  roughness=rng.uniform(size=(1, H, W)).astype(np.float32), metallic=rng.uniform(size=(1, H, W)).astype(np.float32))
    for carve in (True, False):
        ref = mesh_ref.Volume(lo, h, dims, np.float32(0.3), carve=carve)
        masks = ref.integrate(cam, planes)
        vol = _volume(carve, dims=dims, lo=lo, h=h, trunc=np.float32(0.3))
        vol.integrate(cam, _to_dev(planes))
        tsdf, weight, attr_weight, attr = _fields(vol)
        skipped = masks["behind"] | masks["outside"]
        assert masks["behind"].any() and masks["outside"].any() and (~skipped).any()
        assert (tsdf[skipped] == 1).all() and (weight[skipped] == 0).all() and (attr_weight[skipped] == 0).all()
        assert (attr[skipped] == 0).all()
        _compare_volume(vol, ref, masks["fragile"], "skips carve=%s" % carve)
        if not carve:  # pixels below opacity_min leave their samples alone, those at and above it do not
            assert 0 < (ref.weight > 0).sum() < (~skipped).sum()


def _compare_mesh(m, ref, h, what):
    V = len(ref["vertices"])
    faces = m.faces.cpu().numpy()
    assert m.vertices.shape == (V, 3) and m.faces.dtype == torch.int32 and faces.shape == ref["faces"].shape
    assert np.array_equal(faces, ref["faces"])
    assert faces.size == 0 or (faces.min() >= 0 and faces.max() < V)
    dv = float(np.abs(m.vertices.cpu().numpy() - ref["vertices"]).max()) if V else 0.0
    da = max([float(np.abs(getattr(m, k).cpu().numpy() - ref[k]).max()) for k in ("normals", "albedo", "roughness", "metallic")]
             if V else [0.0])
    print("%s: V %d, F %d, max vertex diff %.3g h, max attribute diff %.3g" % (what, V, len(faces), dv / float(h), da))
    assert dv <= 1e-4 * float(h) and da <= 1e-5


def _load_and_extract(lo, h, tsdf, weight, attr_weight, attr, min_weight):
    dims = tsdf.shape[::-1]
    vol = _volume(dims=dims, lo=lo, h=h, trunc=np.float32(3.0) * h)
    vol.load(tsdf, weight, attr_weight, attr)
    return vol.extract(min_weight), mesh_ref.surface_nets(tsdf, weight, attr_weight, attr, lo, h, min_weight)


def _analytic(dims, seed=5):
    lo, h, tsdf = mesh_ref.sphere_field(dims)
    rng = np.random.default_rng(seed)
    attr = rng.uniform(-1.0, 1.0, size=tsdf.shape + (8,)).astype(np.float32)
    attr_weight = rng.integers(0, 3, size=tsdf.shape).astype(np.float32)  # a third of the endpoints carry no attributes
    return lo, h, tsdf, np.ones_like(tsdf), attr_weight, attr


def test_extraction_matches_the_restatement_on_the_analytic_sphere():
    lo, h, tsdf, weight, attr_weight, attr = _analytic((21, 26, 23))
    m, ref = _load_and_extract(lo, h, tsdf, weight, attr_weight, attr, 1)
    _compare_mesh(m, ref, h, "analytic sphere")
    print(mesh_ref.check_closed_sphere(m.vertices.cpu().numpy(), m.faces.cpu().numpy(), h))
    n = torch.linalg.norm(m.normals, dim=1)
    assert bool(((n - 1).abs() < 1e-5).logical_or(n == 0).all())


@pytest.mark.parametrize("min_weight", [1, 2])
def test_extraction_matches_the_restatement_on_the_fused_volume(min_weight):
    ref_vol, _ = _reference(True)
    lo, h, _ = _grid()
    m, ref = _load_and_extract(lo, h, ref_vol.tsdf, ref_vol.weight, ref_vol.attr_weight, ref_vol.attr, min_weight)
    assert len(ref["vertices"]) > 100 and len(ref["faces"]) > 100
    _compare_mesh(m, ref, h, "fused volume, min_weight %d" % min_weight)


def test_holes_and_grid_borders():
    # a hole: no weight in one octant
    lo, h, tsdf, weight, attr_weight, attr = _analytic((21, 26, 23))
    weight[23 // 2:, 26 // 2:, 21 // 2:] = 0
    m, ref = _load_and_extract(lo, h, tsdf, weight, attr_weight, attr, 1)
    _compare_mesh(m, ref, h, "octant hole")
    _, counts = mesh_ref.edge_counts(m.faces.cpu().numpy())
    assert counts.max() <= 2 and (counts == 1).any() and mesh_ref.euler(len(ref["vertices"]), ref["faces"]) == 1
    # the sphere leaves this grid through its last y layer (the layer lies at y = 0.591 < 0.6)
    lo, h, tsdf, weight, attr_weight, attr = _analytic(DIMS)
    assert (tsdf[:, -1, :] < 0).any()
    m, ref = _load_and_extract(lo, h, tsdf, weight, attr_weight, attr, 1)
    _compare_mesh(m, ref, h, "surface leaves the grid")
    _, counts = mesh_ref.edge_counts(m.faces.cpu().numpy())
    assert (counts == 1).any()
    # one axis of length 2: a tilted plane between the two x layers
    dims = (2, 9, 11)
    Gx, Gy, Gz = dims
    h, lo = np.float32(0.1), np.array([0.0, -0.4, -0.5], np.float32)
    k, j, i = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    tsdf = ((i - 0.5) + 0.04 * (j - 4) - 0.03 * (k - 5)).astype(np.float32) / np.float32(3.0)
    rng = np.random.default_rng(11)
    attr = rng.uniform(size=tsdf.shape + (8,)).astype(np.float32)
    m, ref = _load_and_extract(lo, h, tsdf, np.ones_like(tsdf), np.ones_like(tsdf), attr, 1)
    assert len(ref["vertices"]) == (Gy - 1) * (Gz - 1) and len(ref["faces"]) == 2 * (Gy - 2) * (Gz - 2)
    _compare_mesh(m, ref, h, "axis of length 2")
    # nothing to extract: an all-positive volume, and a grid without cells
    m, ref = _load_and_extract(lo, h, np.ones_like(tsdf), np.ones_like(tsdf), np.ones_like(tsdf), attr, 1)
    assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3) and m.roughness.shape == (0,) and len(ref["faces"]) == 0
    flat = _volume(dims=(1, 9, 11))
    flat.load(-np.ones((11, 9, 1), np.float32), np.ones((11, 9, 1), np.float32), np.ones((11, 9, 1), np.float32),
              np.zeros((11, 9, 1, 8), np.float32))
    assert flat.extract().vertices.shape == (0, 3) and flat.extract().faces.shape == (0, 3)


def test_end_to_end_scene_to_ply(tmp_path):
    import mesh
    import scene_io
    import scenes
    sc = scenes.surface_scene(P=20_000)
    g = {k: torch.from_numpy(sc[k]).to(DEV) for k in ("means3D", "opacities", "normal", "albedo", "roughness", "metallic",
                                                      "shs", "scales", "rotations")}
    cams = [scenes.orbit_camera(i, 12, 96, 96, radius=3.5, elevation=0.5 if i % 2 == 0 else 0.9) for i in range(12)]
    lo, hi = mesh.auto_bounds(g)
    voxel, dims = mesh.grid_for_bounds(lo, hi, 48)
    assert max(dims) == 48
    trunc = 4.0 * voxel
    vol = mesh.TSDFVolume(lo, voxel, dims, trunc, device=DEV)
    planes = mesh.fuse_views(g, 2, cams, scenes.GI_DEFAULTS, vol, keep_planes=True)
    assert len(planes) == 12
    ref = mesh_ref.Volume(lo, voxel, dims, trunc)
    fragile = np.zeros(ref.tsdf.shape, bool)
    for c, p in zip(cams, planes):
        fragile |= ref.integrate(c, {k: v.cpu().numpy() for k, v in p.items()})["fragile"]
    _compare_volume(vol, ref, fragile, "surface scene")
    m = vol.extract(min_weight=2)
    V, F = m.vertices.shape[0], m.faces.shape[0]
    assert V > 0 and F > 0 and int(m.faces.min()) >= 0 and int(m.faces.max()) < V
    for t in (m.vertices, m.normals, m.albedo, m.roughness, m.metallic):
        assert bool(torch.isfinite(t).all())
    path = str(tmp_path / "mesh.ply")
    scene_io.save_mesh_ply(path, *m)
    r = scene_io.read_mesh_ply(path)
    assert np.array_equal(r["vertices"], m.vertices.cpu().numpy()) and np.array_equal(r["faces"], m.faces.cpu().numpy())
    assert np.array_equal(r["roughness"], m.roughness.cpu().numpy())
    assert np.abs(r["albedo"] - m.albedo.clamp(0, 1).cpu().numpy()).max() <= 1.0 / 255.0
    # not asserted (it depends on the rasterizer's depth): how far the vertices lie from the scene's spheres and plane
    v = m.vertices.cpu().numpy().astype(np.float64)
    centers = np.array([[0.0, 0.0, 0.0], [0.9, 0.5, -0.3], [-0.8, -0.6, -0.35], [0.1, -1.0, -0.45]])
    radii = np.array([0.6, 0.35, 0.3, 0.2])
    dist = np.abs(np.linalg.norm(v[:, None, :] - centers[None], axis=2) - radii[None]).min(axis=1)
    dist = np.minimum(dist, np.abs(v[:, 2] + 0.65))
    print("surface scene: V %d, F %d, median distance to the scene's surfaces %.3f h" % (V, F, float(np.median(dist)) / voxel))


def test_extract_mesh_tool(tmp_path):
    """The command-line tool on a scene folder and an output folder as trainer.py leaves them (without a training run)."""
    import os
    from argparse import Namespace

    import densify
    import extract_mesh
    import optim
    import relight
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
    a = extract_mesh.parse_args(["-m", out, "--checkpoint", ck])
    assert (a.grid, a.trunc_voxels, a.min_weight, a.opacity_min, a.no_carve, a.split, a.output, a.bounds) == (
        256, 4.0, 2.0, 0.5, False, "train", "mesh.ply", None)
    res = extract_mesh.extract_mesh(["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test", "-o", "test.ply"])
    assert res["path"] == os.path.join(out, "test.ply") and max(res["dims"]) == 40 and res["views"] == 6
    assert res["samples"] == res["dims"][0] * res["dims"][1] * res["dims"][2]
    r = scene_io.read_mesh_ply(res["path"])
    assert len(r["vertices"]) == res["vertices"] > 0 and len(r["faces"]) == res["faces"] > 0
    assert np.isfinite(r["vertices"]).all() and (r["vertices"] >= np.array(res["lo"]) - 1e-5).all()
    assert (r["vertices"] <= np.array(res["lo"]) + res["voxel"] * (np.array(res["dims"]) - 1) + 1e-5).all()
    box = ["--bounds", "-0.7", "-0.7", "-0.7", "0.7", "0.7", "0.7"]
    res2 = extract_mesh.extract_mesh(["-m", out, "--checkpoint", ck, "--grid", "24", "--split", "test", "--no_carve",
                                      "--min_weight", "1", "-o", str(tmp_path / "box.ply")] + box)
    assert res2["dims"] == [24, 24, 24] and res2["path"] == str(tmp_path / "box.ply") and os.path.exists(res2["path"])
