"""GPU: ray-traced light per point (csrc/mesh_gather.hip through mesh.gather_points / mesh.final_gather, mesh_render.RaytracedLight
/ RaytracedGBuffer, render_mesh.py --occlusion / --lighting raytraced, relight_scene.py --occluder) against its numpy restatement
(tests/mesh_gather_ref.py) and against the shipped bakes.  Hits and counters by array_equal, float outputs as bit patterns: the
arithmetic is float64 + - * / without contraction and the summation order is fixed, so there is no tolerance anywhere but for
the prepared points and normals of an image, which pass through torch's float64 sqrt and are held within one float32 ulp."""
import functools
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import helpers
import mesh_clean_ref as cr
import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raster_ref as raster_ref
import mesh_raycast_ref as rr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
R, K = 64, 4
OUTPUTS = ("occlusion", "irradiance", "indirect")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _rho(V, seed=3):
    import mesh_distance_ref as dr
    return dr.uniform(seed, np.arange(3 * V, dtype=np.uint64), 1).astype(np.float32).reshape(V, 3)


def _mesh(v, f, normals, rho=None):
    import mesh
    v = _dev(np.asarray(v, np.float32).reshape(-1, 3))
    f = _dev(np.asarray(f, np.int32).reshape(-1, 3))
    z1 = torch.zeros(v.shape[0], device=DEV)
    albedo = torch.zeros_like(v) if rho is None else _dev(np.asarray(rho, np.float32))
    return mesh.Mesh(v, f, _dev(np.asarray(normals, np.float32).reshape(-1, 3)), albedo, z1, z1.clone())


@functools.lru_cache(maxsize=None)
def _blob():
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    assert (int(m.vertices.shape[0]), int(m.faces.shape[0])) == (980, 1944)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, normals, arguments, every: the stride of the faces whose centroids are the points).  Read-only."""
    if name == "open_box":
        return lr.open_box() + ({}, 1)
    if name == "box":
        return rr.box_interior() + ({}, 1)
    if name == "crease":
        v, f, n, _ = rr.crease()
        return v, f, n, dict(bias=1e-3, seed=9), 1
    if name == "blob":
        return _blob() + (dict(seed=2), 8)
    if name == "plane":
        v, f = sr.plane_grid()
        return v, f, np.repeat([[0.0, 0.0, 1.0]], len(v), 0).astype(np.float32), {}, 1
    d = sr.shared_cases()[name][0]
    v, f = d["vertices"], d["faces"]
    return v, f, lr.vertex_normals(v, f), dict(seed=5), 1


@functools.lru_cache(maxsize=None)
def _points(name):
    """The face centroids of a case with unit face normals, every 5th masked, and three that get no rays: a NaN position, a
    zero normal and a normal of length 1.01.  -> (points, normals, mask uint8).  Read-only."""
    v, f, _, _, every = _case(name)
    p, n = gr.face_points(v, f, every)
    p, n = p.copy(), n.copy()
    mask = (np.arange(len(p)) % 5 != 0).astype(np.uint8)
    p[1, 0] = np.nan
    n[2] = 0.0
    n[3] = n[3] * np.float32(1.01)
    return p, n, mask


def _compare(what, light, report, want):
    got = dict(occlusion=light.occlusion, irradiance=light.irradiance, indirect=light.indirect)
    hits = light.hits.cpu().numpy()
    differ = {k: int((_bits(got[k]) != _bits(want[k])).sum()) for k in OUTPUTS if want[k] is not None}
    print("%s: %d points, hits differ at %d, bit patterns that differ %s; counters %s, restated %s" % (
        what, len(hits), int((hits != want["hits"]).sum()), differ, gr.counters(report), gr.counters(want)))
    assert light.hits.dtype == torch.int32 and np.array_equal(hits, want["hits"])
    for k in OUTPUTS:
        if want[k] is None:
            assert got[k] is None, k
        else:
            assert got[k].dtype == torch.float32 and np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert gr.counters(report) == gr.counters(want)


# ---- 1: the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rays,sky,extra", [
    ("open_box", R, True, {}), ("crease", R, True, {}), ("fan", R, True, {}), ("blob", R, True, {}),
    ("open_box", 128, True, {}), ("open_box", R, False, {}), ("crease", R, True, dict(max_distance=4.0))])
def test_gather_points_equals_the_restatement(name, rays, sky, extra):
    import mesh
    v, f, n, kw, _ = _case(name)
    p, pn, mask = _points(name)
    kw = dict(kw, **extra)
    table = rr.direction_table(rays, K)
    cube = lr.hash_sky() if sky else None
    Q = gr.hash_radiosity(len(v))
    want = gr.gather_points(p, pn, v, f, table, cube, Q, mask=mask, **kw)
    light, report = mesh.gather_points(_dev(p), _dev(pn), _mesh(v, f, n), None if cube is None else _dev(cube), _dev(Q),
                                       directions=table, mask=_dev(mask), cell=want["grid"]["cell"], **kw)
    assert json.loads(json.dumps(report)) == report
    assert (report["n"], report["rays"], report["rotations"], report["seed"]) == (len(p), rays, K, kw.get("seed", 0))
    assert report["ao_distance"] == want["ao_distance"] and report["bias"] == want["bias"]
    assert report["max_distance"] == extra.get("max_distance") and report["sky_res"] == (8 if sky else None)
    _compare("%s R=%d sky=%s %s" % (name, rays, sky, extra), light, report, want)
    N = len(p)
    assert report["masked"] == (N + 4) // 5 and report["no_normal"] == 3
    assert report["misses"] + report["front_hits"] + report["back_hits"] == rays * (N - report["masked"] - 3)
    dead = (mask == 0) | np.isin(np.arange(N), (1, 2, 3))
    assert (light.hits.cpu().numpy()[dead] == 0).all() and (light.occlusion.cpu().numpy()[dead] == 1).all()
    if sky:
        assert (light.irradiance.cpu().numpy()[dead] == 0).all() and (light.indirect.cpu().numpy()[dead] == 0).all()
        assert float(light.irradiance.max()) > 0
        assert (light.indirect.cpu().numpy() <= light.irradiance.cpu().numpy()).all()
    if name == "open_box" and sky:
        assert report["front_hits"] > 0 and report["misses"] > 0 and float(light.indirect.max()) > 0
    if extra:  # a finite light distance: hits beyond it see the sky
        free, r0 = mesh.gather_points(_dev(p), _dev(pn), _mesh(v, f, n), _dev(cube), _dev(Q), directions=table, mask=_dev(mask),
                                      cell=want["grid"]["cell"], **dict(kw, max_distance=None))
        assert report["misses"] > r0["misses"] and r0["max_distance"] is None


# ---- 2: identities with the shipped kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open_box", "blob"])
def test_identities_with_the_bakes(name):
    import mesh
    v, f, n, kw, _ = _case(name)
    rho = _rho(len(v))
    m = _mesh(v, f, n, rho)
    table = rr.direction_table(R, K)
    D, bias = rr.bake_defaults(rr.build_grid(v, f))
    D = 3.0 * D
    common = dict(directions=table, seed=kw.get("seed", 0), bias=bias)
    occ, hits, rep = mesh._bake_occlusion(m, max_distance=D, **common)
    cube = _dev(lr.hash_sky())
    for c in (None, cube):
        light, r = mesh.gather_points(m.vertices, m.normals, m, c, ao_distance=D, **common)
        print("%s, cube %s: hits differ at %d of %d vertices (total %d)" % (name, c is not None, int((light.hits != hits).sum()),
                                                                            len(v), rep["hits_total"]))
        assert torch.equal(light.hits, hits) and np.array_equal(_bits(light.occlusion), _bits(occ))
        assert r["no_normal"] == rep["no_normal"] and r["masked"] == 0
    assert rep["hits_total"] > 0
    passes, _ = mesh.bake_light(m, cube, bounces=2, return_passes=True, **common)
    light, r = mesh.final_gather(m.vertices, m.normals, m, cube, bounces=2, **common)
    print("%s: final_gather against bake_light, irradiance bit patterns that differ: %d" % (
        name, int((_bits(light.irradiance) != _bits(passes[2])).sum())))
    assert np.array_equal(_bits(light.irradiance), _bits(passes[2])) and r["bounces"] == 2 and r["bake"]["passes"] == 2
    assert float(light.indirect.max()) > 0 and (passes[2] > passes[0]).any()
    zero, r0 = mesh.final_gather(m.vertices, m.normals, m, cube, bounces=0, **common)
    assert (zero.indirect == 0).all() and np.array_equal(_bits(zero.irradiance), _bits(passes[0])) and r0["bake"] is None
    assert r0["front_hits"] == r["front_hits"] > 0


# ---- 3: the grid does not show -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open_box", "blob"])
def test_grid_independence(name):
    import mesh
    v, f, n, kw, _ = _case(name)
    p, pn, mask = _points(name)
    m = _mesh(v, f, n)
    g = rr.build_grid(v, f)
    D, bias = rr.bake_defaults(g)  # the defaults follow the grid's box: pin them
    args = dict(cube=_dev(lr.hash_sky()), radiosity=_dev(gr.hash_radiosity(len(v))), rays=R, rotations=K, ao_distance=2.0 * D,
                bias=bias, seed=kw.get("seed", 0), mask=_dev(mask))
    one, r1 = mesh.gather_points(_dev(p), _dev(pn), m, cell=1e6 * g["cell"], **args)
    assert r1["dims"] == [1, 1, 1] and r1["front_hits"] + r1["back_hits"] > 0
    for scale in (0.5, 1.0, 3.0):
        got, r = mesh.gather_points(_dev(p), _dev(pn), m, cell=scale * g["cell"], **args)
        assert torch.equal(got.hits, one.hits) and gr.counters(r) == gr.counters(r1), (name, scale)
        for k in OUTPUTS:
            assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(one, k))), (name, scale, k)


# ---- 4: known answers ----------------------------------------------------------------------------------------------------------
def _constant_sky(c, n=4):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), (6, n, n, 3)))


def test_known_answers_and_empty_inputs():
    import mesh
    c = np.array([0.5, 2.0, 0.25], np.float32)
    sky = _dev(_constant_sky(c))
    up = lambda k: np.repeat([[0.0, 0.0, 1.0]], k, 0).astype(np.float32)  # noqa: E731
    # above the plane, looking up: nothing but the sky, and a sum of R equal float32 values is exact in float64
    v, f, n, _, _ = _case("plane")
    m = _mesh(v, f, n, np.ones((len(v), 3), np.float32))
    xy = np.random.default_rng(1).uniform(0.2, 0.8, size=(37, 2))
    p = np.concatenate([xy, np.full((37, 1), 0.5)], 1).astype(np.float32)
    for rays in (64, 1024):
        light, rep = mesh.gather_points(_dev(p), _dev(up(37)), m, sky, _dev(gr.hash_radiosity(len(v))), rays=rays, rotations=K)
        assert (light.occlusion == 1).all() and (light.hits == 0).all() and (light.indirect == 0).all()
        assert np.array_equal(_bits(light.irradiance), _bits(np.broadcast_to(c, (37, 3)))) and rep["misses"] == rays * 37
    # inside the closed box: every ray ends on a wall, whose back it sees
    v, f, n, _, _ = _case("box")
    m = _mesh(v, f, n)
    p = np.random.default_rng(2).uniform(0.2, 0.8, size=(21, 3)).astype(np.float32)
    pn = lr.analytic_normals()[np.arange(21) % 9]
    light, rep = mesh.gather_points(_dev(p), _dev(pn), m, sky, rays=R, rotations=K, ao_distance=10.0, bias=0.0)
    assert (light.hits == R).all() and (light.occlusion == 0).all() and (light.irradiance == 0).all()
    assert (rep["misses"], rep["front_hits"], rep["back_hits"]) == (0, 0, R * 21)
    # a shorter occlusion distance: fewer hits, with and without a sky
    v, f, n, kw, _ = _case("crease")
    m = _mesh(v, f, n)
    p, pn = gr.face_points(v, f)
    for cube in (None, sky):
        far, _ = mesh.gather_points(_dev(p), _dev(pn), m, cube, rays=R, rotations=K, ao_distance=1e6, **kw)
        near, _ = mesh.gather_points(_dev(p), _dev(pn), m, cube, rays=R, rotations=K, ao_distance=4.0, **kw)
        assert (near.hits <= far.hits).all() and int(near.hits.sum()) < int(far.hits.sum())
    # N = 0; a mesh with no usable face: nothing is launched and every point is open
    e3 = torch.zeros((0, 3), device=DEV)
    light, rep = mesh.gather_points(e3, e3, m, sky, rays=R)
    assert tuple(light.occlusion.shape) == (0,) and tuple(light.irradiance.shape) == (0, 3) and gr.counters(rep) == (0,) * 5
    light, rep = mesh.gather_points(e3, e3, m, rays=R)
    assert light.irradiance is None and light.indirect is None and light.hits.dtype == torch.int32
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 1, 1]], np.int32)):
        flat = _mesh(np.zeros((3, 3), np.float32), faces, up(3))
        pn = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]], np.float32)
        light, rep = mesh.gather_points(_dev(np.ones((4, 3), np.float32)), _dev(pn), flat, sky, rays=R,
                                        mask=_dev(np.array([1, 1, 0, 1], np.uint8)))
        assert (light.occlusion == 1).all() and (light.hits == 0).all() and (light.irradiance == 0).all()
        assert gr.counters(rep) == (2 * R, 0, 0, 1, 1) and rep["pairs"] == 0 and rep["dims"] == [0, 0, 0]
    # what is refused
    p, pn = _dev(p), _dev(pn)
    ok = _dev(gr.face_points(v, f)[0])
    for bad in (dict(rays=100), dict(rotations=65), dict(ao_distance=-1.0), dict(ao_distance=float("inf")), dict(bias=-1.0),
                dict(max_distance=float("nan")), dict(cube=sky[:5]), dict(cube=-sky), dict(cube=sky.double()),
                dict(radiosity=torch.zeros((len(v), 2), device=DEV)), dict(radiosity=torch.full((len(v), 3), float("nan"), device=DEV)),
                dict(mask=torch.zeros(len(ok), device=DEV)), dict(mask=torch.zeros(3, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            mesh.gather_points(ok, ok, m, **dict(dict(rays=R), **bad))
    for a, b in ((ok[:, :2], ok), (ok, ok[:5]), (ok.double(), ok)):
        with pytest.raises(ValueError):
            mesh.gather_points(a, b, m, rays=R)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.gather_points(ok.cpu(), ok, m, rays=R)
    with pytest.raises(ValueError, match="bounces"):
        mesh.final_gather(ok, ok, m, sky, bounces=-1)
    with pytest.raises(ValueError, match="cube"):
        mesh.final_gather(ok, ok, m, None)


# ---- 5: an image ---------------------------------------------------------------------------------------------------------------
IW, IH = 32, 24


def _camera():
    import scenes
    cam = scenes.look_at_camera((1.9, 0.35, 1.7), (0.4, 0.5, 0.3), IW, IH, 0.9)
    return {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}, cam


@pytest.mark.parametrize("name", ["crease", "open_box"])
def test_raytraced_light_planes_equal_the_restatement(name):
    import mesh_render
    if name == "crease":
        v, f, n, _ = rr.crease(4, 1.0)
    else:
        v, f, n = lr.open_box()
    rho = 0.25 + 0.5 * _rho(len(v))
    m = _mesh(v, f, n, rho)
    sky = lr.hash_sky()
    cam, cam_np = _camera()
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, seed=6, cube=_dev(sky), bounces=1, light_rays=64, device=DEV) as tracer:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        t = tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover)
        rep = t["report"]
        assert json.loads(json.dumps(rep)) == rep
        n_cover = int(cover.sum())
        assert 100 < n_cover < IW * IH and rep["masked"] == IW * IH - n_cover and rep["n"] == IW * IH and rep["bounces"] == 1
        assert tuple(t["occlusion"].shape) == (1, IH, IW) and tuple(t["hits"].shape) == (IH, IW)
        assert tuple(t["irradiance"].shape) == (3, IH, IW) and tuple(t["indirect"].shape) == (3, IH, IW)
        assert torch.equal(t["mask"].reshape(IH, IW).bool(), cover) and (t["occlusion"][0][~cover] == 1).all()
        assert (t["hits"][~cover] == 0).all() and (t["irradiance"][:, ~cover] == 0).all()
        # the prepared arrays: a numpy float64 transform of the planes, within one float32 ulp
        wp, wn = gr.prepare(o["pos"].cpu().numpy(), o["normal"].cpu().numpy(), cam_np["viewmatrix"])
        live = cover.reshape(-1).cpu().numpy()
        for what, got, want in (("points", t["points"], wp), ("normals", t["normals"], wn)):
            got = got.cpu().numpy().astype(np.float64)[live]
            ulp = np.spacing(np.abs(want[live]).astype(np.float32)).astype(np.float64)
            print("%s, %s: largest error %.3g ulp" % (name, what, float((np.abs(got - want[live]) / ulp).max())))
            assert (np.abs(got - want[live]) <= ulp).all(), what
        # the restatement fed the prepared arrays
        want = gr.gather_points(t["points"].cpu().numpy(), t["normals"].cpu().numpy(), v, f, rr.direction_table(R, K), sky,
                                tracer.radiosity[0].cpu().numpy(), ao_distance=tracer.ao_distance, bias=tracer.bias, seed=6,
                                mask=t["mask"].cpu().numpy())
        light = type("L", (), dict(hits=t["hits"].reshape(-1), occlusion=t["occlusion"].reshape(-1),
                                   irradiance=t["irradiance"].reshape(3, -1).t(), indirect=t["indirect"].reshape(3, -1).t()))
        _compare("%s image" % name, light, rep, want)
        assert rep["front_hits"] > 0 and float(t["indirect"].max()) > 0 and int(t["hits"].max()) > 0
        # no bounce: the sky alone; a view-space normal plane gives the world normals back
        t0 = tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover, bounces=0)
        assert (t0["indirect"] == 0).all() and torch.equal(t0["hits"], t["hits"]) and t0["report"]["bounces"] == 0
        nv = -torch.einsum("chw,cd->dhw", o["normal"].double(), cam["viewmatrix"][:3, :3].double()).float()
        _, back, _ = tracer.prepare(o["pos"], nv, cam["viewmatrix"], cover, normal_space="view")
        assert float((back - t["normals"])[cover.reshape(-1)].abs().max()) <= 1e-6
        with pytest.raises(ValueError, match="normal_space"):
            tracer.prepare(o["pos"], o["normal"], cam["viewmatrix"], cover, normal_space="screen")
        with pytest.raises(ValueError, match="bounces"):
            tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover, bounces=2)
    with pytest.raises(RuntimeError, match="closed"):
        tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover)


# ---- 6: G-buffer sources -----------------------------------------------------------------------------------------------------
RW, RH = 64, 48


@functools.lru_cache(maxsize=None)
def _relight_setup():
    """A sphere over a ground plane, a camera, its view directions and a light.  Read-only."""
    import mesh_render
    import pipeline
    import relight
    import scenes
    m = dict(raster_ref.sphere_mesh()[0])
    m["normals"] = (m["vertices"] / np.linalg.norm(m["vertices"], axis=1, keepdims=True)).astype(np.float32)
    n = 5
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, n), np.linspace(-1.6, 1.6, n), indexing="xy")
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(n * n, -0.65)], axis=1).astype(np.float32)
    cell = np.array([(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, j * n + i, (j + 1) * n + i + 1, (j + 1) * n + i)
                     for j in range(n - 1) for i in range(n - 1)], np.int32).reshape(-1, 3)
    V0 = len(m["vertices"])
    m["vertices"] = np.concatenate([m["vertices"], ground])
    m["faces"] = np.concatenate([m["faces"], cell + V0])
    m["normals"] = np.concatenate([m["normals"], np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n * n, 1))])
    m["albedo"] = np.concatenate([m["albedo"], np.full((n * n, 3), 0.6, np.float32)])
    m["roughness"] = np.concatenate([m["roughness"], np.full(n * n, 0.4, np.float32)])
    m["metallic"] = np.concatenate([m["metallic"], np.zeros(n * n, np.float32)])
    cam = scenes.orbit_camera(1, 8, RW, RH, radius=3.5)
    c = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}
    vd = pipeline.view_dirs_for(c, pipeline.canonical_rays(cam, DEV), DEV)
    light = relight.make_light(_dev(scenes.synthetic_envmap(64, 128, seed=5)), res=64)
    return mesh_render.device_mesh(m, DEV), c, vd, light


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(), b.nan_to_num())


def test_raytraced_gbuffer_over_a_mesh():
    import mesh_render
    import relight
    import scenes
    m, cam, vd, light = _relight_setup()
    gi = scenes.GI_DEFAULTS
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, ao_distance=1.0, bias=0.05, device=DEV) as tracer:
        # the bias: depth_pos comes from the filtered depth and lies up to 0.04 off this sphere at 64 x 48; a point under the
        # surface would see its back
        source = mesh_render.RaytracedGBuffer(mesh_render.MeshGBuffer(gi), tracer)
        rl = relight.Relighter(light, gi, 0, source=source)
        out = {k: (x.clone() if isinstance(x, torch.Tensor) else x) for k, x in rl(cam, rast, vd).items()}
        b = mesh_render.MeshGBuffer(gi)(cam, rast)
        t = tracer.planes(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], normal_space="view")
        plane = t["occlusion"]
        assert plane.dtype == b["occlusion"].dtype and tuple(plane.shape) == tuple(b["occlusion"].shape) == (1, RH, RW)
        assert torch.equal(out["occlusion"], plane) and torch.equal(out["raytraced_occlusion"], plane)
        assert "raytraced_irradiance" not in out and out["tri_id"].dtype == torch.int32
        assert source.report == t["report"] and t["report"]["masked"] == int((b["mask_u8"] == 0).sum())
        # the top of the sphere sees the sky, its underside the ground: the normals point outward (inward ones would end on the
        # sphere's own back, and the plane's mean would be below 0.5)
        covered = b["mask_u8"] != 0
        print("traced occlusion: mean %.4f over %d pixels, SSAO mean %.4f; hits %d of %d rays" % (
            float(plane[0][covered].mean()), int(covered.sum()), float(b["occlusion"][0][covered].mean()),
            t["report"]["front_hits"] + t["report"]["back_hits"], R * int(covered.sum())))
        assert 0.8 < float(plane[0][covered].mean()) < 1.0 and float(plane[0][covered].min()) < 1.0
        assert t["report"]["back_hits"] < t["report"]["front_hits"]
        # the shade and the march behind it, on a G-buffer whose occlusion was replaced by hand
        hand = dict(b, occlusion=plane)
        with torch.no_grad():
            rd, irr, rgb = relight.shade_ssr(light, rl.brdf_lut, gi, False, False, False, cam, vd, hand, hand["albedo_map"],
                                             relight.Scratch())
        assert _same(out["render_direct"], rd) and _same(out["render_rgb"], rgb) and _same(out["IRR"], irr)
        assert float(rgb.nan_to_num().max()) > 0.05
        plain = mesh_render.MeshRelighter(light, gi)(cam, rast, vd)
        assert not _same(plain["render_direct"], rd)  # the occlusion does reach the shade
        ssao = plain["occlusion"].clone()
        both = relight.Relighter(light, gi, 0, source=mesh_render.RaytracedGBuffer(mesh_render.MeshGBuffer(gi), tracer, "multiply"))
        ob = both(cam, rast, vd)
        assert torch.equal(ob["occlusion"], ssao * plane) and torch.equal(ob["raytraced_occlusion"], plane)
        # the other relighters take the source too; a traced view replays no hipGraph
        with relight.TurntableRelighter([light], gi, 0, source=source) as tr:
            ot = tr(cam, rast, vd)
            assert torch.equal(ot["occlusion"], plane) and _same(ot["render_rgb"][0], rgb)
        for make in (lambda: relight.Relighter(light, gi, 0, graphs=True, source=source),
                     lambda: relight.MultiRelighter([light], gi, 0, graphs=True, source=source)):
            with pytest.raises(ValueError, match="graphs"):
                make()
        with pytest.raises(ValueError, match="occlusion"):
            mesh_render.RaytracedGBuffer(mesh_render.MeshGBuffer(gi), tracer, "both")
        with pytest.raises(ValueError, match="metallic"):
            relight.Relighter(light, gi, 0, metallic=True, source=source)


def test_raytraced_gbuffer_over_splats_and_with_a_cube():
    import mesh_render
    import relight
    import scenes
    m, _, _, light = _relight_setup()
    gi = scenes.GI_DEFAULTS
    sc, cam = helpers.small_scene(P=300, sh_degree=1, W=RW, H=RH)
    g = {k: _dev(sc[k]) for k in helpers.GAUSS_KEYS}
    cam = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}
    sky = _dev(lr.hash_sky(8, top=2.0))
    with mesh_render.RaytracedLight(m, rays=R, rotations=K, cube=sky, bounces=1, light_rays=64, device=DEV) as tracer:
        source = mesh_render.RaytracedGBuffer(relight.SplatGBuffer(gi, 1), tracer)
        assert source.replayable is False and source.metallic is False
        got = source(cam, g)
        plane, extra = got["occlusion"].clone(), {k: x.clone() for k, x in got["extra"].items()}
        b = relight.SplatGBuffer(gi, 1)(cam, g)
        t = tracer.planes(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], normal_space="view")
        assert torch.equal(plane, t["occlusion"]) and tuple(plane.shape) == tuple(b["occlusion"].shape)
        assert sorted(extra) == ["raytraced_indirect", "raytraced_irradiance", "raytraced_occlusion"]
        assert torch.equal(extra["raytraced_irradiance"], t["irradiance"]) and torch.equal(extra["raytraced_indirect"], t["indirect"])
        assert t["report"]["masked"] == int((b["mask_u8"] == 0).sum()) < RW * RH and float(t["irradiance"].max()) > 0
        assert got["radii"] is not None and torch.equal(got["depth_map"], b["depth_map"])


# ---- 7: tools ----------------------------------------------------------------------------------------------------------------
def test_tools(tmp_path):
    import densify
    import optim
    import relight
    import relight_scene
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    import train_iteration as ti
    from PIL import Image
    v, f, n = _blob()
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=1, size=32)
    out = str(tmp_path / "run")
    os.makedirs(out)
    scene_io.save_mesh_ply(os.path.join(out, "blob.ply"), *_mesh(v, f, n, 0.25 + 0.5 * _rho(len(v))))
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    base = ["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--split", "train"]
    folder = os.path.join(out, "mesh_train")
    plain = render_mesh.render_mesh(base)
    assert not any("raytraced" in x for x in os.listdir(folder)) and "raytraced_vs_screen" not in plain
    ssao = {x: np.array(Image.open(os.path.join(folder, x))) for x in os.listdir(folder) if x.endswith("_occlusion.png")}
    assert len(ssao) == 2
    # --occlusion raytraced: the same files, another occlusion plane
    res = render_mesh.render_mesh(base + ["--occlusion", "raytraced", "--ao_rays", "64", "--ao_distance", "0.5", "--ray_bias", "0.001"])
    assert json.loads(json.dumps(res)) == res and res["files"] == plain["files"] and "raytraced_vs_screen" not in res
    traced = {x: np.array(Image.open(os.path.join(folder, x))) for x in ssao}
    assert all(traced[x].shape == ssao[x].shape and int(traced[x].max()) > 0 for x in ssao)
    assert any(not np.array_equal(traced[x], ssao[x]) for x in ssao)
    # --lighting raytraced: a diffuse image per view and the comparison
    res = render_mesh.render_mesh(base + ["--lighting", "raytraced", "--bounces", "2", "--light_rays", "64", "--sky_res", "16"])
    assert json.loads(json.dumps(res)) == res and res["files"] == plain["files"]
    assert res["raytraced_vs_screen_json"] == os.path.join(folder, "raytraced_vs_screen.json")
    with open(res["raytraced_vs_screen_json"]) as fh:
        cmp = json.load(fh)
    print("ray-traced diffuse against screen-space and per-vertex baked:", json.dumps(cmp["average"]))
    keys = ["psnr_%s_bounces_%d" % (k, b) for k in ("baked", "screen") for b in (0, 2)]
    assert sorted(cmp["average"]) == keys and cmp["average"] == res["raytraced_vs_screen"] and len(cmp["views"]) == 2
    assert (cmp["bounces"], cmp["rays"], cmp["light_rays"], cmp["sky_res"]) == (2, 64, 64, 16)
    assert cmp["tracer"]["n"] == 32 * 32 and cmp["tracer"]["front_hits"] + cmp["tracer"]["misses"] > 0
    assert len(cmp["light"]["mean_irradiance"]) == 3
    for view in cmp["views"]:
        assert view["pixels_covered"] > 20 and all(np.isfinite(view[k]) and view[k] > 0 for k in keys)
    assert len(res["raytraced_diffuse"]) == 2
    for path in res["raytraced_diffuse"]:
        img = np.array(Image.open(path))
        assert path.endswith("_raytraced_diffuse.png") and img.shape[:2] == (32, 32) and int(img.max()) > 0
    res0 = render_mesh.render_mesh(base + ["--lighting", "raytraced", "--bounces", "0", "--light_rays", "64"])
    assert sorted(res0["raytraced_vs_screen"]) == ["psnr_baked_bounces_0", "psnr_screen_bounces_0"]
    for bad in (["-m", out, "--mesh", "blob.ply", "--checkpoint", "none.pth", "--lighting", "raytraced"],
                ["-m", out, "--mesh", "x.obj", "--hdri", hdr, "--lighting", "raytraced"],
                base + ["--lighting", "raytraced", "--bounces", "-1"], base + ["--occlusion", "raytraced", "--ao_rays", "100"],
                base + ["--occlusion", "raytraced", "--ao_distance", "-1"]):
        with pytest.raises(ValueError, match="lighting raytraced|bounces|ao_rays|ao_distance"):
            render_mesh.render_mesh(bad)
    # relight_scene.py --occluder: the occlusion PNG is the traced plane
    g = ti.raw_from_scene(scenes.surface_scene(P=2000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [g[k]], "lr": 0.0, "name": k} for k in g], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(64, 128)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, g, densify.DensifyState(g["xyz"].shape[0], DEV), opt, 1.0), light.state_dict(), {}, 7)
    common = ["-m", out, "--checkpoint", ck, "--hdri", hdr, "--skip_train"]
    a = relight_scene.relight_scene(common)
    files = sorted(x for x in os.listdir(os.path.join(out, "test", "ours_7", "relight")) if x.endswith("_occlusion.png"))
    assert len(files) == 1 and "occluder" not in a["test"]
    before = np.array(Image.open(os.path.join(out, "test", "ours_7", "relight", files[0])))
    b = relight_scene.relight_scene(common + ["--occluder", "blob.ply", "--ao_rays", "64", "--occluder_mode", "replace"])
    after = np.array(Image.open(os.path.join(out, "test", "ours_7", "relight", files[0])))
    assert json.loads(json.dumps(b)) == b and b["test"]["files"] == a["test"]["files"]
    assert b["test"]["occluder"]["n"] == 32 * 32 and b["test"]["occluder"]["rays"] == 64
    assert after.shape == before.shape and not np.array_equal(after, before)
    for bad in (common + ["--ao_rays", "128"], common + ["--occluder", "blob.ply", "--ao_rays", "65"],
                common + ["--occluder_mode", "multiply"]):
        with pytest.raises(ValueError, match="occluder|ao_rays"):
            relight_scene.relight_scene(bad)
