"""GPU: light baking (csrc/mesh_light.hip through mesh.trace_hemispheres / mesh.gather_light / mesh.bake_light, bake_mesh.py
--light, bake_atlas(extra=)) against its numpy restatement (tests/mesh_light_ref.py).  Records by array_equal, weights,
irradiance and radiosity as bit patterns: the arithmetic is float64 + - * / without contraction and the summation order is
fixed, so there is no tolerance anywhere but in the analytic test, whose bound is derived in mesh_light_ref.analytic_irradiance.
The blob is held against the restatement on every 8th vertex; the grid-independence tests run everything against the GPU's
one-cell grid, its own brute force."""
import functools
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import mesh_clean_ref as cr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
R, K = 64, 4


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _rho(V, seed=3):
    """[V,3] float32 in [0, 1): a hash-random reflectance."""
    import mesh_distance_ref as dr
    return dr.uniform(seed, np.arange(3 * V, dtype=np.uint64), 1).astype(np.float32).reshape(V, 3)


def _mesh(v, f, normals, rho=None):
    """A mesh.Mesh whose default reflectance albedo * (1 - metallic) is `rho` (metallic 0), or 0."""
    import mesh
    v = _dev(np.asarray(v, np.float32).reshape(-1, 3))
    f = _dev(np.asarray(f, np.int32).reshape(-1, 3))
    z1 = torch.zeros(v.shape[0], device=DEV)
    albedo = torch.zeros_like(v) if rho is None else _dev(np.asarray(rho, np.float32))
    return mesh.Mesh(v, f, _dev(np.asarray(normals, np.float32).reshape(-1, 3)), albedo, z1, z1.clone())


@functools.lru_cache(maxsize=None)
def _blob():
    """(vertices, faces, normals) of the extracted blob mesh.  Read-only."""
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    assert (int(m.vertices.shape[0]), int(m.faces.shape[0])) == (980, 1944)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, normals, trace arguments, the vertices the restatement traces or None for all).  Read-only."""
    if name == "box":
        return rr.box_interior() + ({}, None)
    if name == "open_box":
        return lr.open_box() + ({}, None)
    if name == "plane":
        v, f = sr.plane_grid()
        return v, f, np.repeat([[0.0, 0.0, 1.0]], len(v), 0).astype(np.float32), {}, None
    if name == "crease":
        v, f, n, _ = rr.crease()
        return v, f, n, dict(bias=1e-3, seed=9), None
    if name == "blob":
        v, f, n = _blob()
        return v, f, n, dict(seed=2), np.arange(0, len(v), 8)
    d = sr.shared_cases()[name][0]
    v, f = d["vertices"], d["faces"]
    return v, f, lr.vertex_normals(v, f), dict(seed=5), None


@functools.lru_cache(maxsize=None)
def _traced(name, rays=R):
    """The restatement's records of a case with the default grid.  Read-only."""
    v, f, n, kw, subset = _case(name)
    return lr.trace(v, f, n, rr.direction_table(rays, K), subset=subset, **kw)


def _counters(report):
    return tuple(report[k] for k in ("misses", "front_hits", "back_hits", "no_normal"))


# ---- 1: the trace ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rays", [("box", R), ("plane", R), ("crease", R), ("fan", R), ("debris", R), ("blob", R), ("open_box", R),
                                       ("fan", 128)])
def test_trace_equals_the_restatement(name, rays):
    import mesh
    v, f, n, kw, subset = _case(name)
    table = rr.direction_table(rays, K)
    want = _traced(name, rays)
    m = _mesh(v, f, n)
    hits, report = mesh.trace_hemispheres(m, directions=table, cell=want["grid"]["cell"], **kw)
    assert json.loads(json.dumps(report)) == report
    assert (hits.rays, hits.rotations, hits.seed, report["n"]) == (rays, K, kw.get("seed", 0), len(v))
    assert hits.face.dtype == torch.int32 and tuple(hits.face.shape) == (len(v), rays)
    assert hits.bary.dtype == torch.float32 and tuple(hits.bary.shape) == (len(v), rays, 2)
    assert report["bias"] == want["bias"] and report["max_distance"] is None and report["record_bytes"] == 12 * len(v) * rays
    rows = np.arange(len(v)) if subset is None else subset
    face, bary = hits.face.cpu().numpy(), hits.bary.cpu().numpy()
    print("%s R=%d: %d vertices, %d compared, %d records and %d weight bit patterns differ; misses %d front %d back %d no_normal %d" % (
        name, rays, len(v), len(rows), int((face[rows] != want["face"][rows]).sum()),
        int((_bits(bary[rows]) != _bits(want["bary"][rows])).sum()), *_counters(report)))
    assert np.array_equal(face[rows], want["face"][rows])
    assert np.array_equal(_bits(bary[rows]), _bits(want["bary"][rows]))
    F = len(f)
    assert ((face >= -1 - F) & (face < F)).all() and (bary[face == -1] == 0).all()
    assert _counters(report)[:3] == (int((face[want["valid"]] == -1).sum()), int((face >= 0).sum()), int((face <= -2).sum()))
    assert sum(_counters(report)[:3]) == rays * (len(v) - report["no_normal"])
    assert (face[~want["valid"]] == -1).all() and report["no_normal"] == int((~want["valid"]).sum())
    if subset is None:
        assert _counters(report) == _counters(want)
    if name == "debris":
        assert report["no_normal"] == 4 and report["faces_skipped"] == 3
    if name == "box":  # outward faces seen from inside: every ray ends on a back
        assert report["back_hits"] == rays * len(v)
    if name == "plane":
        assert report["misses"] == rays * len(v)
    if name == "open_box":
        assert report["misses"] > 0 and report["front_hits"] > 0 and report["back_hits"] == 0
    # a finite distance: a hit beyond it is a miss
    if name == "crease":
        near, r2 = mesh.trace_hemispheres(m, directions=table, cell=want["grid"]["cell"], max_distance=4.0, **kw)
        lim = lr.trace(v, f, n, table, max_distance=4.0, **kw)
        assert np.array_equal(near.face.cpu().numpy(), lim["face"]) and np.array_equal(_bits(near.bary), _bits(lim["bary"]))
        assert _counters(r2) == _counters(lim) and r2["misses"] > report["misses"] and r2["max_distance"] == 4.0


# ---- 2: the gather -----------------------------------------------------------------------------------------------------------
SKIES = dict(faces=lr.face_colour_sky, hash=lr.hash_sky)


@pytest.mark.parametrize("sky", sorted(SKIES))
@pytest.mark.parametrize("name", ["open_box", "crease", "fan"])
def test_gather_equals_the_restatement(name, sky):
    import mesh
    v, f, n, kw, _ = _case(name)
    table = rr.direction_table(R, K)
    want = _traced(name)
    cube, rho = SKIES[sky](), _rho(len(v))
    m = _mesh(v, f, n, rho)
    hits = mesh.HemisphereHits(_dev(want["face"]), _dev(want["bary"]), table, kw.get("seed", 0), R, K)
    I, Q, report = mesh._gather_light(m, hits, _dev(cube), bounces=2)
    wI, wQ = lr.light(v, f, n, table, kw.get("seed", 0), want["face"], want["bary"], cube, rho, bounces=2)
    print("%s, %s sky: irradiance bit patterns that differ per pass %s, radiosity %s; mean irradiance %s" % (
        name, sky, [int((_bits(I[b]) != _bits(wI[b])).sum()) for b in range(3)],
        [int((_bits(Q[b]) != _bits(wQ[b])).sum()) for b in range(3)], report["mean_irradiance"]))
    assert np.array_equal(_bits(I), _bits(wI)) and np.array_equal(_bits(Q), _bits(wQ))
    assert (report["passes"], report["bounces"], report["sky_res"], report["rays"]) == (3, 2, cube.shape[1], R)
    assert np.allclose(report["mean_irradiance"], wI.astype(np.float64).mean(axis=(1, 2)), rtol=1e-12)
    assert (wI[2] > wI[0]).any()  # the bounces bring light
    # the public entry point: the last pass, or all of them; the default reflectance is albedo * (1 - metallic)
    last, _ = mesh.gather_light(m, hits, _dev(cube), bounces=2, reflectance=_dev(rho))
    every, _ = mesh.gather_light(m, hits, _dev(cube), bounces=2, return_passes=True)
    assert np.array_equal(_bits(last), _bits(wI[2])) and np.array_equal(_bits(every), _bits(wI))


# ---- 3: the grid does not show -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open_box", "blob"])
def test_grid_independence(name):
    import mesh
    v, f, n, kw, _ = _case(name)
    m = _mesh(v, f, n, _rho(len(v)))
    cell = rr.build_grid(v, f)["cell"]
    cube = _dev(lr.hash_sky())
    kw = dict(kw, bias=lr.default_bias(rr.build_grid(v, f)))  # the default bias follows the grid's box: pin it
    one, r1 = mesh.trace_hemispheres(m, rays=R, rotations=K, cell=1e6 * cell, **kw)
    assert r1["dims"] == [1, 1, 1]
    I1, Q1, _ = mesh._gather_light(m, one, cube, bounces=2)
    for scale in (0.5, 1.0, 3.0):
        got, r = mesh.trace_hemispheres(m, rays=R, rotations=K, cell=scale * cell, **kw)
        assert torch.equal(got.face, one.face) and np.array_equal(_bits(got.bary), _bits(one.bary)), (name, scale)
        assert _counters(r) == _counters(r1)
        I, Q, _ = mesh._gather_light(m, got, cube, bounces=2)
        assert np.array_equal(_bits(I), _bits(I1)) and np.array_equal(_bits(Q), _bits(Q1))


# ---- 4: known answers ----------------------------------------------------------------------------------------------------------
def _constant_sky(c, n=4):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), (6, n, n, 3)))


def test_known_answers_and_empty_inputs():
    import mesh
    c = np.array([0.7, 1.3, 1e-3], np.float32)
    sky = _dev(_constant_sky(c))
    # the plane sees nothing but the sky: a sum of R equal float32 values is exact in float64
    v, f, n, _, _ = _case("plane")
    for rays in (64, 1024):
        I, rep = mesh.bake_light(_mesh(v, f, n, _rho(len(v))), sky, rays=rays, rotations=K, bounces=2, return_passes=True)
        assert np.array_equal(_bits(I), _bits(np.broadcast_to(c, (3, len(v), 3)))) and rep["misses"] == rays * len(v)
    # the closed box seen from inside: no ray escapes and every hit is a back
    v, f, n, _, _ = _case("box")
    I, rep = mesh.bake_light(_mesh(v, f, n, np.ones((len(v), 3), np.float32)), sky, rays=R, rotations=K, bounces=3, return_passes=True)
    assert (I == 0).all() and tuple(I.shape) == (4, len(v), 3) and rep["misses"] == 0 and rep["mean_irradiance"] == [0.0] * 4
    # bounces = 0: one pass, the shadowed sky
    v, f, n, _, _ = _case("open_box")
    m = _mesh(v, f, n, np.ones((len(v), 3), np.float32))
    hits, _ = mesh.trace_hemispheres(m, rays=R, rotations=K)
    I0, rep = mesh.gather_light(m, hits, sky, bounces=0, return_passes=True)
    assert tuple(I0.shape) == (1, len(v), 3) and rep["passes"] == 1
    share = (hits.face == -1).sum(1).double() / R
    assert np.array_equal(_bits(I0[0]), _bits((share[:, None] * torch.from_numpy(c.astype(np.float64)).to(DEV)).float()))
    # V = 0; F = 0; no usable face
    e3, ei = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    hits, rep = mesh.trace_hemispheres(_mesh(e3, ei, e3), rays=R)
    assert tuple(hits.face.shape) == (0, R) and tuple(hits.bary.shape) == (0, R, 2) and _counters(rep) == (0, 0, 0, 0)
    I, rep = mesh.gather_light(_mesh(e3, ei, e3), hits, sky, bounces=2, return_passes=True)
    assert tuple(I.shape) == (3, 0, 3) and rep["mean_irradiance"] == [0.0] * 3
    up = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 0]], np.float32)
    for faces in (ei, np.array([[0, 1, 1]], np.int32)):
        m = _mesh(np.zeros((3, 3), np.float32), faces, up, np.ones((3, 3), np.float32))
        hits, rep = mesh.trace_hemispheres(m, rays=R)
        assert (hits.face == -1).all() and _counters(rep) == (2 * R, 0, 0, 1) and rep["pairs"] == 0
        I, rep = mesh.gather_light(m, hits, sky, bounces=1)
        assert np.array_equal(_bits(I), _bits(np.stack([c, c, np.zeros(3, np.float32)])))
    # what is refused
    m = _mesh(*_case("plane")[:3])
    hits, _ = mesh.trace_hemispheres(m, rays=R)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.gather_light(m, hits, sky.cpu())
    with pytest.raises(ValueError, match="records"):
        mesh.gather_light(_mesh(*_case("box")[:3]), hits, sky)
    with pytest.raises(ValueError, match="memory_limit"):
        mesh.trace_hemispheres(m, rays=R, memory_limit=12 * R * int(m.vertices.shape[0]) - 1)


# ---- 5: the white furnace ------------------------------------------------------------------------------------------------------
def test_white_furnace_is_monotone_and_bounded():
    """Reflectance 1 under a constant sky c: I(b+1) >= I(b) with no slack (the weights are >= 0 and every operation used is
    monotone), and I(b) <= c (1 + 2^-20) (the float32 rounding of the weights)."""
    import mesh
    v, f, n, _, _ = _case("open_box")
    c = np.array([0.7, 1.3, 5e3], np.float32)
    m = _mesh(v, f, n, np.ones((len(v), 3), np.float32))
    I, rep = mesh.bake_light(m, _dev(_constant_sky(c)), rays=R, rotations=K, bounces=4, return_passes=True)
    I = I.cpu().numpy()
    print("white furnace: mean irradiance / c per pass", [float((I[b] / c).mean()) for b in range(5)], "max", float((I / c).max()))
    assert (I[1:] >= I[:-1]).all() and (I[1:] > I[:-1]).any()
    assert (I.astype(np.float64) <= c.astype(np.float64) * (1.0 + 2.0 ** -20)).all()
    assert (I[0] > 0).any() and rep["front_hits"] > 0


# ---- 6, 7: the cube's convention -------------------------------------------------------------------------------------------------
FAR = np.array([[1000, 1000, 1000], [1000.5, 1000, 1000], [1000, 1000.5, 1000]], np.float32)  # a tiny triangle no ray meets


def _free_vertices(normals):
    """Free-standing vertices at the origin with `normals`, and FAR's triangle after them."""
    V = len(normals)
    v = np.concatenate([np.zeros((V, 3), np.float32), FAR])
    nrm = np.concatenate([np.asarray(normals, np.float32), np.repeat([[0.0, 0.0, 1.0]], 3, 0).astype(np.float32)])
    return v, np.array([[V, V + 1, V + 2]], np.int32), nrm


def test_sky_lookup_is_cube_texture_s():
    """A cube that is constant per face, n = 4: the kernel's texel of the texel-centre directions away from the face edges is
    pbr.texture.cube_texture's, exactly.  Every vertex looks along its normal with all its 64 rays."""
    import mesh
    from pbr.texture import cube_texture
    n = 4
    cube = lr.face_colour_sky(n)
    centre = lr.texel_centres(n)[:, 1:3, 1:3].reshape(-1, 3)  # (1, +-1/4, +-1/4) and the like: exact in float32
    dirs = (centre / np.sqrt((centre ** 2).sum(axis=1, keepdims=True))).astype(np.float32)
    v, f, nrm = _free_vertices(dirs)
    table = np.repeat(np.array([[[0.0, 0.0, 1.0]]], np.float32), 64, 1)  # K = 1, R = 64 copies of the normal itself
    I, rep = mesh.bake_light(_mesh(v, f, nrm), _dev(cube), directions=table, bounces=0)
    assert rep["misses"] == 64 * len(v) and rep["no_normal"] == 0
    want = cube_texture(_dev(cube), _dev(centre.astype(np.float32)))
    assert np.array_equal(_bits(I[:len(dirs)]), _bits(want))
    assert np.array_equal(_bits(want), _bits(np.repeat(cube[:, 0, 0], 4, 0)))
    # every texel its own value: the (u, v) signs too are cube_texture's (its four taps carry the weights 1, 0, 0, 0 at a centre)
    cube = lr.hash_sky(n, top=10.0)
    I, _ = mesh.bake_light(_mesh(v, f, nrm), _dev(cube), directions=table, bounces=0)
    want = cube_texture(_dev(cube), _dev(centre.astype(np.float32)))
    assert np.array_equal(_bits(I[:len(dirs)]), _bits(want))
    assert np.array_equal(_bits(want), _bits(cube[:, 1:3, 1:3].reshape(-1, 3))) and len(np.unique(_bits(want))) == want.numel()


def test_analytic_irradiance():
    """L(d) = a + b . d at the texel centres of a 256^2 cube, nothing to hit, R = 1024, K = 16: a + (2/3) b . n within the
    derived bound of mesh_light_ref.analytic_irradiance.  A wrong face, flip or axis gives an error of order |b|."""
    import mesh
    nrm = lr.analytic_normals()
    v, f, n = _free_vertices(nrm)
    sky = lr.linear_sky(lr.ANALYTIC_A, lr.ANALYTIC_B, 256)
    I, rep = mesh.bake_light(_mesh(v, f, n), _dev(sky), rays=1024, rotations=16, bounces=0)
    assert rep["misses"] == 1024 * len(v)
    want, bound = lr.analytic_irradiance(nrm)
    err = np.abs(I.cpu().numpy()[:len(nrm)].astype(np.float64) - want)
    print("analytic irradiance: largest error per channel", err.max(axis=0), "bound", bound)
    assert (err <= bound).all()
    table = rr.direction_table(1024, 16)
    ref, _ = lr.gather(v, f, n, table, 0, np.full((len(v), 1024), -1, np.int32), np.zeros((len(v), 1024, 2), np.float32), sky,
                       np.zeros((len(v), 3), np.float32))
    assert np.array_equal(_bits(I), _bits(ref))


# ---- 8: one trace, many lights -----------------------------------------------------------------------------------------------
def test_one_trace_many_lights():
    import mesh
    v, f, n = _blob()
    m = _mesh(v, f, n, _rho(len(v)))
    skies = [_dev(lr.hash_sky(8, seed=s)) for s in (1, 2)]
    hits, _ = mesh.trace_hemispheres(m, rays=R, rotations=K, seed=4)
    for sky in skies:
        a, ra = mesh.gather_light(m, hits, sky, bounces=2)
        b, rb = mesh.bake_light(m, sky, rays=R, rotations=K, seed=4, bounces=2)
        c, rc = mesh.bake_light(m, sky, rays=R, rotations=K, seed=4, bounces=2)
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(b), _bits(c)) and rb == rc
        assert ra["mean_irradiance"] == rb["mean_irradiance"] and float(a.max()) > 0
    again, _ = mesh.trace_hemispheres(m, rays=R, rotations=K, seed=4)
    assert torch.equal(again.face, hits.face) and np.array_equal(_bits(again.bary), _bits(hits.bary))


# ---- 9: tools ----------------------------------------------------------------------------------------------------------------
def test_tools(tmp_path):
    import bake_mesh
    import clean_mesh
    import image_writer
    import mesh
    import relight
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    v, f, n = _blob()
    src = _mesh(v, f, n, _rho(len(v)))
    raw = str(tmp_path / "blob.ply")
    scene_io.save_mesh_ply(raw, *src)
    hdr = str(tmp_path / "sky.hdr")
    image_writer.write_hdr(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    # without the new options: the parent's bytes (the PLY of --rays alone is save_mesh_ply(occlusion=) of bake_occlusion)
    plain = bake_mesh.bake_mesh([raw, "-o", str(tmp_path / "plain.ply"), "--rays", "64"])
    assert "light" not in plain
    m = mesh.Mesh(*(_dev(scene_io.read_mesh_ply(raw)[k]) for k in mesh.Mesh._fields))
    occ, _ = mesh.bake_occlusion(m, rays=64)
    scene_io.save_mesh_ply(str(tmp_path / "want.ply"), *m, occlusion=occ)
    with open(plain["path"], "rb") as a, open(str(tmp_path / "want.ply"), "rb") as b:
        plain_bytes = a.read()
        assert plain_bytes == b.read() and b"irradiance" not in plain_bytes
    # --light: the irradiance of bake_light in the file, bit for bit
    rep = bake_mesh.bake_mesh([raw, "-o", str(tmp_path / "lit.ply"), "--rays", "64", "--light", hdr, "--light_rays", "64", "--bounces", "2",
                               "--sky_res", "16"])
    assert json.loads(json.dumps(rep)) == rep
    cube = mesh.sky_cube(relight.latlong_to_cubemap(_dev(image_writer.load_latlong(hdr)), [256, 256]), 16)
    assert tuple(cube.shape) == (6, 16, 16, 3)
    want, wrep = mesh.bake_light(m, cube, rays=64, bounces=2)
    lit = scene_io.read_mesh_ply(rep["path"])
    assert np.array_equal(_bits(lit["irradiance"]), _bits(want)) and np.array_equal(_bits(lit["occlusion"]), _bits(occ))
    assert float(want.mean()) > 0 and len(rep["light"]["mean_irradiance"]) == 3
    assert all(rep["light"][k] == wrep[k] for k in ("misses", "front_hits", "back_hits", "no_normal", "mean_irradiance"))
    # the siblings read the file and drop the channels
    c = clean_mesh.clean_mesh([rep["path"], "-o", str(tmp_path / "clean.ply"), "--keep_largest", "1"])
    assert c["faces"] > 0 and "irradiance" not in scene_io.read_mesh_ply(c["path"])
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=1, n_test=1, size=32)
    out = str(tmp_path / "run")
    os.makedirs(out)
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    res = render_mesh.render_mesh(["-m", out, "--mesh", rep["path"], "--hdri", hdr, "--split", "train"])
    assert res["n_views"] == 1 and res["faces"] == len(f)
    # a light-map: bake_atlas(extra=) is transfer_attributes of the same values at the atlas points
    v, f, n, _, _ = _case("crease")
    m = _mesh(v, f, n, _rho(len(v)))
    irr, _ = mesh.bake_light(m, _dev(lr.hash_sky()), rays=R, rotations=K, bounces=1, bias=1e-3)
    base, r0 = mesh.bake_atlas(m, m, block=4)
    atlas, r1 = mesh.bake_atlas(m, m, block=4, extra=irr)
    assert base.extra is None and r0 == r1 and tuple(atlas.extra.shape) == (3,) + tuple(atlas.albedo.shape[1:])
    for name in ("albedo", "orm", "normal", "coverage", "uvs"):  # the nine channels are what they were
        assert torch.equal(getattr(base, name), getattr(atlas, name)), name
    points, _, _, dest = mesh.atlas_points(m, atlas.layout)
    got, _, _, _, _ = mesh.transfer_attributes(points, m, irr)
    keep = dest >= 0
    assert int(keep.sum()) == r1["baked"] > 0
    assert np.array_equal(_bits(atlas.extra.reshape(3, -1)[:, dest[keep]].T), _bits(got[keep]))
    with pytest.raises(ValueError, match="extra"):
        mesh.bake_atlas(m, m, block=4, extra=torch.zeros((len(v), 8), device=DEV))


def test_texture_mesh_and_extract_mesh_light(tmp_path):
    """texture_mesh.py --light writes the light-map of bake_atlas(extra=bake_light) beside files that are otherwise the same
    bytes; extract_mesh.py --bake_light puts bake_light's irradiance into the PLY it writes, and nothing else changes."""
    import densify
    import extract_mesh
    import image_writer
    import mesh
    import mesh_render
    import optim
    import relight
    import scene_io
    import scenes
    import synthetic_dataset
    import texture_mesh
    import train_iteration as ti
    from bake_mesh import load_sky
    v, f, n = _blob()
    raw = str(tmp_path / "blob.ply")
    scene_io.save_mesh_ply(raw, *_mesh(v, f, n, _rho(len(v))))
    hdr = str(tmp_path / "sky.hdr")
    image_writer.write_hdr(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    common = [raw, "--cell_edges", "2.5", "--block", "4"]
    plain = texture_mesh.texture_mesh(common + ["-o", str(tmp_path / "a" / "low.obj")])
    lit = texture_mesh.texture_mesh(common + ["-o", str(tmp_path / "b" / "low.obj"), "--light", hdr, "--light_rays", "64", "--sky_res", "16"])
    assert "lightmap" not in plain["files"] and "light" not in plain and json.loads(json.dumps(lit)) == lit
    assert sorted(os.listdir(str(tmp_path / "a"))) == sorted(x for x in os.listdir(str(tmp_path / "b")) if x != "low_lightmap.hdr")
    for name in os.listdir(str(tmp_path / "a")):
        with open(str(tmp_path / "a" / name), "rb") as a, open(str(tmp_path / "b" / name), "rb") as b:
            assert a.read() == b.read(), name
    assert lit["files"]["lightmap"] == str(tmp_path / "b" / "low_lightmap.hdr") and lit["atlas"] == plain["atlas"]
    src = mesh_render.device_mesh(raw, DEV)
    irr, rep = mesh.bake_light(src, load_sky(hdr, 16, DEV), rays=64)
    assert all(lit["light"][k] == rep[k] for k in ("misses", "front_hits", "back_hits", "mean_irradiance"))
    dst, _ = mesh.simplify(src, 2.5 * mesh.median_edge(src))
    atlas, _ = mesh.bake_atlas(dst, src, block=4, extra=irr)
    want = atlas.extra.permute(1, 2, 0).cpu().numpy()
    got = image_writer.read_hdr(lit["files"]["lightmap"])
    assert got.shape == want.shape and float(want.max()) > 0
    # RGBE keeps 8 bits of the largest channel: one part in 128 of it, per texel
    assert (np.abs(got - want) <= want.max(axis=2, keepdims=True) / 128.0 + 1e-30).all()
    # from a checkpoint
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=6, size=64)
    out = str(tmp_path / "run")
    os.makedirs(out)
    g = ti.raw_from_scene(scenes.surface_scene(P=4000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [g[k]], "lr": 0.0, "name": k} for k in g], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, g, densify.DensifyState(g["xyz"].shape[0], DEV), opt, 1.0), light.state_dict(), {}, 7)
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    base = ["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test", "--bake_occlusion", "64"]
    assert extract_mesh.parse_args(base).bake_light is None
    r0 = extract_mesh.extract_mesh(base + ["-o", "ao.ply"])
    r1 = extract_mesh.extract_mesh(base + ["-o", "lit.ply", "--bake_light", hdr, "--light_rays", "64", "--bounces", "2"])
    assert "light" not in r0 and json.loads(json.dumps(r1)) == r1 and len(r1["light"]["mean_irradiance"]) == 3
    a0, a1 = scene_io.read_mesh_ply(r0["path"]), scene_io.read_mesh_ply(r1["path"])
    assert "irradiance" not in a0 and sorted(a1) == sorted(list(a0) + ["irradiance"])
    for k in a0:
        assert np.array_equal(a0[k], a1[k], equal_nan=True), k
    # the bake reads positions, normals and faces, which the PLY keeps exactly, and the reflectance before the PLY's 8 bits:
    # pass 0 does not read the reflectance at all
    m = mesh_render.device_mesh(a0, DEV)
    I0, rep0 = mesh.bake_light(m, load_sky(hdr, 32, DEV), rays=64, bounces=0)
    assert rep0["mean_irradiance"][0] == r1["light"]["mean_irradiance"][0] and (a1["irradiance"] >= I0.cpu().numpy()).all()
    assert all(r1["light"][k] == rep0[k] for k in ("misses", "front_hits", "back_hits", "no_normal"))


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_light")


def test_option_less_tools_write_the_parents_bytes(tmp_path):
    """bake_mesh.py and texture_mesh.py without a light option on the crease: the PLY is the file the parent commit wrote
    (golden/mesh_light/parent_crease_ao.ply) and every file of the atlas has the hash the parent's had (parent_hashes.json)."""
    import hashlib

    import bake_mesh
    import mesh_distance_ref as dr
    import scene_io
    import texture_mesh
    out = str(tmp_path)
    v, f, n, _ = rr.crease()
    V = len(v)
    u = lambda k, c: dr.uniform(21, np.arange(c * V, dtype=np.uint64), k).astype(np.float32)  # noqa: E731
    src = os.path.join(out, "crease.ply")
    scene_io.save_mesh_ply(src, v, f, n, u(0, 3).reshape(V, 3), u(1, 1), u(2, 1))
    rep = bake_mesh.bake_mesh([src, "-o", os.path.join(out, "crease_ao.ply"), "--rays", "64", "--distance", "4.0", "--bias", "0.001",
                               "--seed", "9"])
    texture_mesh.texture_mesh([rep["path"], "-o", os.path.join(out, "tex", "low.obj"), "--target", rep["path"], "--block", "4"])
    with open(os.path.join(GOLDEN, "parent_hashes.json")) as fh:
        want = json.load(fh)
    with open(rep["path"], "rb") as a, open(os.path.join(GOLDEN, "parent_crease_ao.ply"), "rb") as b:
        assert a.read() == b.read()
    got = {"crease.ply": src, "crease_ao.ply": rep["path"]}
    got.update({"tex/" + name: os.path.join(out, "tex", name) for name in os.listdir(os.path.join(out, "tex"))})
    assert sorted(got) == sorted(want)
    for name, path in got.items():
        with open(path, "rb") as fh:
            assert hashlib.sha256(fh.read()).hexdigest() == want[name], name


def test_render_mesh_baked_lighting(tmp_path):
    """render_mesh.py --lighting baked: a baked_diffuse image per view and baked_vs_screen.json with the PSNR against the
    screen-space diffuse for 0 bounces and for --bounces.  The figures are printed, not bounded: they are a report."""
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    from PIL import Image
    v, f, n = _blob()
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=1, size=64)
    out = str(tmp_path / "run")
    os.makedirs(out)
    scene_io.save_mesh_ply(os.path.join(out, "blob.ply"), *_mesh(v, f, n, 0.25 + 0.5 * _rho(len(v))))
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    base = ["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--split", "train"]
    plain = render_mesh.render_mesh(base)
    assert "baked_vs_screen" not in plain and not any("baked" in x for x in os.listdir(os.path.join(out, "mesh_train")))
    res = render_mesh.render_mesh(base + ["--lighting", "baked", "--bounces", "2", "--light_rays", "64", "--sky_res", "16"])
    assert json.loads(json.dumps(res)) == res and res["files"] == plain["files"]
    with open(res["baked_vs_screen_json"]) as fh:
        cmp = json.load(fh)
    print("baked against screen-space diffuse:", json.dumps(cmp["average"]), [x["pixels_covered"] for x in cmp["views"]])
    assert res["baked_vs_screen_json"] == os.path.join(out, "mesh_train", "baked_vs_screen.json")
    assert sorted(cmp["average"]) == ["psnr_bounces_0", "psnr_bounces_2"] and cmp["average"] == res["baked_vs_screen"]
    assert len(cmp["views"]) == 2 and (cmp["bounces"], cmp["rays"], cmp["sky_res"]) == (2, 64, 16)
    assert len(cmp["light"]["mean_irradiance"]) == 3 and cmp["light"]["misses"] > 0
    for view in cmp["views"]:
        assert view["pixels_covered"] > 100 and np.isfinite(view["psnr_bounces_0"]) and np.isfinite(view["psnr_bounces_2"])
        assert view["psnr_bounces_0"] > 0 and view["psnr_bounces_2"] > 0
    assert len(res["baked_diffuse"]) == 2
    for path in res["baked_diffuse"]:
        img = np.array(Image.open(path))
        assert path.endswith("_baked_diffuse.png") and img.shape[:2] == (64, 64) and int(img.max()) > 0
    # no bounce: one figure; and what the mode needs
    res0 = render_mesh.render_mesh(base + ["--lighting", "baked", "--bounces", "0", "--light_rays", "64"])
    assert sorted(res0["baked_vs_screen"]) == ["psnr_bounces_0"]
    for bad in (["-m", out, "--mesh", "blob.ply", "--checkpoint", "none.pth", "--lighting", "baked"],
                ["-m", out, "--mesh", "x.obj", "--hdri", hdr, "--lighting", "baked"], base + ["--lighting", "baked", "--bounces", "-1"]):
        with pytest.raises(ValueError, match="lighting baked|bounces"):
            render_mesh.render_mesh(bad)
