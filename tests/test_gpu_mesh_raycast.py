"""GPU: ray casting and occlusion baking (csrc/mesh_raycast.hip through mesh.raycast / mesh.bake_occlusion, extract_mesh.py
--bake_occlusion, bake_mesh.py) against their numpy restatement (tests/mesh_raycast_ref.py).  face by array_equal, t and
bary as bit patterns, the bake's hit counts exactly: the arithmetic is float64 + - * / without contraction, so there is no
tolerance and no exemption anywhere in this file.  Against the restatement the large cases keep every 8th ray and the
blob's bake every 8th vertex (the restatement of a one-cell grid tests every face for every ray); the grid-independence
tests run everything against the GPU's one-cell grid, its own brute force."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as cr
import mesh_distance_ref as dr
import mesh_raycast_ref as rr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASES = dr.B_CASES + ("blob",)


def _mesh(v, f, normals=None):
    import mesh
    v = torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1, 3)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(f, np.int32).reshape(-1, 3)).to(DEV)
    n = torch.zeros_like(v) if normals is None else torch.from_numpy(np.ascontiguousarray(normals, np.float32)).to(DEV)
    z1 = torch.zeros(v.shape[0], device=DEV)
    return mesh.Mesh(v, f, n, torch.zeros_like(v), z1, z1.clone())


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


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


def _vf(name):
    if name == "blob":
        return _blob()[:2]
    d = sr.shared_cases()[name][0]
    return d["vertices"], d["faces"]


def _rays_of(v, f, grid, stride=None, thin=1):
    sets = rr.ray_sets(v, f, grid, stride=stride)
    sets = {k: s if k == "bad" else (s[0][::thin], s[1][::thin]) for k, s in sets.items()}
    return np.concatenate([s[0] for s in sets.values()]), np.concatenate([s[1] for s in sets.values()]), len(sets["bad"][0])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, the restatement's default grid, origins, directions, the restatement's answer).  Read-only."""
    v, f = _vf(name)
    grid = dr.build_grid(v, f)
    o, d, n_bad = _rays_of(v, f, grid, thin=8 if len(f) >= 1000 else 1)
    return v, f, grid, o, d, n_bad, rr.raycast(o, d, v, f, grid=grid)


@pytest.mark.parametrize("name", CASES)
def test_raycast_equals_the_restatement(name):
    import mesh
    v, f, grid, o, d, n_bad, want = _case(name)
    m = _mesh(v, f)
    t, face, bary, report = mesh.raycast(_dev(o), _dev(d), m, cell=grid["cell"])
    assert json.loads(json.dumps(report)) == report
    assert (report["cell"], report["dims"], report["pairs"]) == (grid["cell"], list(grid["G"]), grid["pairs"])
    assert t.dtype == torch.float32 and face.dtype == torch.int32 and bary.dtype == torch.float32
    assert tuple(t.shape) == (len(o),) and tuple(face.shape) == (len(o),) and tuple(bary.shape) == (len(o), 2)
    differ = int((face.cpu().numpy() != want["face"]).sum())
    print("%s: %d rays, %d hits (restatement %d), %d faces differ, %d t and %d bary bit patterns differ" % (
        name, len(o), report["hits"], want["hits"], differ, int((_bits(t) != _bits(want["t"])).sum()),
        int((_bits(bary) != _bits(want["bary"])).sum())))
    assert np.array_equal(face.cpu().numpy(), want["face"])
    assert np.array_equal(_bits(t), _bits(want["t"])) and np.array_equal(_bits(bary), _bits(want["bary"]))
    assert (report["n"], report["hits"], report["rays_invalid"]) == (len(o), want["hits"], n_bad) == (len(o), want["hits"], want["rays_invalid"])
    assert report["faces_skipped"] == grid["faces_skipped"] == (3 if name == "debris" else 0)
    assert want["hits"] > 0
    miss = want["face"] < 0
    assert np.isposinf(t.cpu().numpy()[miss]).all() and (bary.cpu().numpy()[miss] == 0).all()
    # a limit on t
    lim = float(np.median(want["t64"][~miss]))
    t2, face2, _, r2 = mesh.raycast(_dev(o), _dev(d), m, t_max=lim, cell=grid["cell"])
    keep = want["t64"] <= lim
    assert np.array_equal(face2.cpu().numpy(), np.where(keep, want["face"], -1)) and r2["hits"] == int(keep.sum())
    assert np.array_equal(_bits(t2)[keep], _bits(want["t"])[keep])


@pytest.mark.parametrize("name", CASES)
def test_grid_independence(name):
    """Three cell sizes give the bits of the one-cell grid, the GPU's own brute force; every ray of the case, unthinned."""
    import mesh
    v, f, grid, _, _, _, _ = _case(name)
    o, d, _ = _rays_of(v, f, grid, stride=1)
    o, d = _dev(o), _dev(d)
    m = _mesh(v, f)
    t1, f1, b1, r1 = mesh.raycast(o, d, m, cell=1e6 * grid["cell"])
    assert r1["dims"] == [1, 1, 1] and r1["pairs"] == int(grid["usable"].sum())
    for scale in (0.5, 1.0, 3.0):
        g = mesh.triangle_grid(m, scale * grid["cell"])
        t, face, bary, r = mesh.raycast(o, d, m, grid=g)
        assert torch.equal(face, f1) and np.array_equal(_bits(t), _bits(t1)) and np.array_equal(_bits(bary), _bits(b1)), (name, scale, r)
        assert (r["hits"], r["rays_invalid"]) == (r1["hits"], r1["rays_invalid"])
        t2, face2, bary2, r2 = mesh.raycast(o, d, m, grid=g)
        assert torch.equal(face2, face) and np.array_equal(_bits(t2), _bits(t)) and np.array_equal(_bits(bary2), _bits(bary)) and r2 == r


def test_known_answers_and_empty_inputs():
    import mesh
    v, f = sr.cube()
    edge = float(np.asarray(v).max())
    m = _mesh(v, f)
    c = np.full((6, 3), edge / 2, np.float32)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)
    t, face, bary, report = mesh.raycast(_dev(c), _dev(axes), m)
    assert t.cpu().tolist() == [edge / 2] * 6 and report["hits"] == 6
    assert np.array_equal(face.cpu().numpy(), rr.brute_force(c, axes, v, f)["face"])
    # nothing to cast, nothing to hit: no launch
    f32 = dict(dtype=torch.float32, device=DEV)
    t, face, bary, report = mesh.raycast(torch.empty((0, 3), **f32), torch.empty((0, 3), **f32), m)
    assert tuple(t.shape) == (0,) and tuple(face.shape) == (0,) and tuple(bary.shape) == (0, 2)
    assert report == dict(n=0, hits=0, rays_invalid=0, faces_skipped=None, cell=0.0, dims=[0, 0, 0], pairs=0)
    for empty in (_mesh(np.zeros((0, 3)), np.zeros((0, 3))), _mesh(np.zeros((3, 3)), [[0, 1, 2]])):
        o = _dev(np.array([[0, 0, 1], [np.nan, 0, 0]], np.float32))
        d = _dev(np.array([[0, 0, -1], [0, 0, 1]], np.float32))
        t, face, bary, report = mesh.raycast(o, d, empty)
        assert np.isposinf(t.cpu().numpy()).all() and face.cpu().tolist() == [-1, -1] and (bary == 0).all()
        assert (report["n"], report["hits"], report["rays_invalid"], report["pairs"]) == (2, 0, 1, 0)
        assert report["faces_skipped"] == int(empty.faces.shape[0])
        occ, rep = mesh.bake_occlusion(empty, rays=64)
        assert (occ == 1).all() and rep["hits_total"] == 0 and rep["no_normal"] == int(empty.vertices.shape[0])
    # CPU tensors fail loudly
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.raycast(torch.zeros((1, 3)), torch.ones((1, 3), **f32), m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.raycast(torch.zeros((1, 3), **f32), torch.ones((1, 3)), m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.bake_occlusion(mesh.Mesh(*(x.cpu() for x in m)))
    with pytest.raises(ValueError):
        mesh.raycast(torch.zeros((2, 3), **f32), torch.ones((1, 3), **f32), m)
    for bad in (dict(rays=65), dict(rays=32), dict(rays=2048), dict(rotations=0), dict(rotations=65), dict(max_distance=-1.0)):
        with pytest.raises(ValueError):
            mesh.bake_occlusion(m, **bad)


def _vertex_normals(v, f):
    """Area-weighted vertex normals of the usable faces, float32; zero where a vertex has none."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    use = dr.face_areas(v, f)[0] > 0
    n = np.zeros_like(v64)
    fn = np.cross(v64[f[use, 1]] - v64[f[use, 0]], v64[f[use, 2]] - v64[f[use, 0]])
    for k in range(3):
        np.add.at(n, f[use, k], fn)
    ln = np.sqrt((n ** 2).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ln > 0, n / ln, 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _bake_case(name):
    """(vertices, faces, normals, bake arguments, the vertices the restatement bakes or None for all).  Read-only."""
    if name == "box":
        return rr.box_interior() + (dict(max_distance=8.0), None)
    if name == "plane":
        v, f = sr.plane_grid()
        return v, f, np.repeat([[0.0, 0.0, 1.0]], len(v), 0).astype(np.float32), {}, None
    if name == "crease":
        v, f, n, _ = rr.crease()
        return v, f, n, dict(max_distance=4.0, bias=1e-3, seed=9), None
    if name == "blob":
        v, f, n = _blob()
        return v, f, n, dict(seed=2), np.arange(0, len(v), 8)
    v, f = _vf(name)
    return v, f, _vertex_normals(v, f), dict(seed=5), None


@pytest.mark.parametrize("name,R,K", [("box", 64, 4), ("plane", 64, 4), ("crease", 64, 4), ("fan", 64, 4), ("debris", 64, 4),
                                      ("blob", 64, 4), ("blob", 128, 4)])
def test_bake_equals_the_restatement(name, R, K):
    import mesh
    v, f, n, kw, subset = _bake_case(name)
    table = rr.direction_table(R, K)
    assert np.array_equal(mesh.occlusion_directions(R, K).view(np.uint32), table.view(np.uint32))
    want = rr.bake(v, f, n, table, subset=subset, **kw)
    m = _mesh(v, f, n)
    occ, hits, report = mesh._bake_occlusion(m, directions=table, cell=want["grid"]["cell"], **kw)
    assert json.loads(json.dumps(report)) == report
    assert (report["rays"], report["rotations"], report["n"]) == (R, K, len(v))
    assert (report["max_distance"], report["bias"]) == (want["max_distance"], want["bias"])
    rows = np.arange(len(v)) if subset is None else subset
    got = hits.cpu().numpy()
    print("%s R=%d: %d vertices, %d compared, %d hit counts differ; mean occlusion %.4f, no_normal %d" % (
        name, R, len(v), len(rows), int((got[rows] != want["hits"][rows]).sum()), float(occ.mean()), report["no_normal"]))
    assert np.array_equal(got[rows], want["hits"][rows])
    assert np.array_equal(_bits(occ)[rows], _bits(want["occlusion"])[rows])
    assert ((got >= 0) & (got <= R)).all() and report["hits_total"] == int(got.sum())
    assert np.array_equal(_bits(occ), _bits(((R - got).astype(np.float64) / R).astype(np.float32)))
    if subset is None:
        assert (report["no_normal"], report["hits_total"]) == (want["no_normal"], want["hits_total"])
    else:
        assert report["no_normal"] == int((~want["valid"]).sum())
    if name == "box":
        assert (got == R).all() and (occ == 0).all()
    if name == "plane":
        assert (got == 0).all() and (occ == 1).all()
    if name == "debris":
        assert report["no_normal"] >= 4 and report["faces_skipped"] == 3  # the unreferenced vertices and the NaN one
    # the one-cell grid, the GPU's own brute force, on every vertex; and the public entry point with the default table
    occ1, hits1, r1 = mesh._bake_occlusion(m, directions=table, cell=1e6 * want["grid"]["cell"], **dict(
        kw, max_distance=report["max_distance"], bias=report["bias"]))
    assert r1["dims"] == [1, 1, 1] and torch.equal(hits1, hits) and np.array_equal(_bits(occ1), _bits(occ))
    occ2, r2 = mesh.bake_occlusion(m, rays=R, rotations=K, cell=want["grid"]["cell"], **kw)
    assert np.array_equal(_bits(occ2), _bits(occ)) and r2 == report


def test_bake_seeds_and_ray_counts():
    import mesh
    v, f, n = _blob()
    m = _mesh(v, f, n)
    grid = mesh.triangle_grid(m)
    a, ha, ra = mesh._bake_occlusion(m, rays=64, rotations=4, seed=1, grid=grid)
    b, hb, rb = mesh._bake_occlusion(m, rays=64, rotations=4, seed=1, grid=grid)
    assert np.array_equal(_bits(a), _bits(b)) and torch.equal(ha, hb) and ra == rb
    c, hc, rc = mesh._bake_occlusion(m, rays=64, rotations=4, seed=2, grid=grid)
    same_turn = rr.rotation_of(1, np.arange(len(v)), 4) == rr.rotation_of(2, np.arange(len(v)), 4)
    assert 0 < same_turn.sum() < len(v)
    assert np.array_equal(ha.cpu().numpy()[same_turn], hc.cpu().numpy()[same_turn])  # the seed picks the rotation, nothing else
    assert not torch.equal(ha, hc) and rc["no_normal"] == ra["no_normal"]
    one, h1, _ = mesh._bake_occlusion(m, rays=64, rotations=1, seed=1, grid=grid)
    two, h2, _ = mesh._bake_occlusion(m, rays=64, rotations=1, seed=77, grid=grid)
    assert torch.equal(h1, h2)
    unsorted_, hu, _ = mesh._bake_occlusion(m, rays=64, rotations=4, seed=1, grid=grid, sort=False)
    assert torch.equal(hu, ha)
    for R in (64, 1024):
        occ, hits, rep = mesh._bake_occlusion(m, rays=R, rotations=16, grid=grid)
        h = hits.cpu().numpy()
        assert ((h >= 0) & (h <= R)).all() and rep["hits_total"] == int(h.sum()) and rep["rays"] == R
        assert np.array_equal(_bits(occ), _bits(((R - h).astype(np.float64) / R).astype(np.float32)))
        print("blob R=%d: mean occlusion %.4f, no_normal %d" % (R, float(occ.mean()), rep["no_normal"]))
    # more rays, the same integral: the two means agree to a few rays' worth
    assert abs(float(occ.mean()) - float(a.mean())) < 0.05


def test_extract_mesh_bake_and_bake_mesh_tool(tmp_path):
    """extract_mesh.py --bake_occlusion 64 on the blob scene of test_gpu_mesh_simplify.py's set-up, bake_mesh.py on its PLY,
    and the sibling tools on a PLY that carries the channel."""
    from argparse import Namespace

    import bake_mesh
    import clean_mesh
    import compare_mesh
    import densify
    import extract_mesh
    import mesh
    import mesh_render
    import optim
    import relight
    import scene_io
    import scenes
    import simplify_mesh
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
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=src, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    assert extract_mesh.parse_args(["-m", out, "--checkpoint", ck]).bake_occlusion == 0
    base = ["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test"]
    r0 = extract_mesh.extract_mesh(base + ["-o", "raw.ply"])
    r1 = extract_mesh.extract_mesh(base + ["--bake_occlusion", "0", "-o", "raw0.ply"])
    assert "occlusion" not in r0 and "occlusion" not in r1 and sorted(r0) == sorted(r1)
    plain = open(r0["path"], "rb").read()
    assert open(r1["path"], "rb").read() == plain
    # today's bytes: the file is the one save_mesh_ply writes without the argument
    arrays = scene_io.read_mesh_ply(r0["path"])
    assert "occlusion" not in arrays
    r2 = extract_mesh.extract_mesh(base + ["--bake_occlusion", "64", "-o", "baked.ply"])
    assert json.loads(json.dumps(r2)) == r2 and r2["occlusion"]["rays"] == 64 and r2["bake_s"] >= 0
    assert (r2["vertices"], r2["faces"]) == (r0["vertices"], r0["faces"])
    baked = scene_io.read_mesh_ply(r2["path"])
    for k in mesh_render.MESH_KEYS:
        assert np.array_equal(baked[k], arrays[k], equal_nan=True), k
    # the same bake on the device mesh the tool had: extract again through the API pieces is the PLY's arrays but for the
    # albedo's 8 bits, which the bake does not read
    m = mesh_render.device_mesh(arrays, DEV)
    occ, rep = mesh.bake_occlusion(m, rays=64)
    assert np.array_equal(_bits(baked["occlusion"]), _bits(occ)) and rep == r2["occlusion"]
    assert 0.0 < float(occ.mean()) < 1.0
    # bake_mesh.py on the plain file
    rep = bake_mesh.bake_mesh([r0["path"], "-o", str(tmp_path / "tool.ply"), "--rays", "64"])
    assert json.loads(json.dumps(rep)) == rep and rep["vertices"] == r0["vertices"] and sum(rep["histogram"]) == r0["vertices"]
    tool = scene_io.read_mesh_ply(rep["path"])
    assert np.array_equal(_bits(tool["occlusion"]), _bits(occ))
    rep2 = bake_mesh.bake_mesh([r0["path"], "-o", str(tmp_path / "tool2.ply"), "--rays", "128", "--distance", "0.2", "--bias", "0.001",
                                "--seed", "3"])
    occ2, _ = mesh.bake_occlusion(m, rays=128, max_distance=0.2, bias=0.001, seed=3)
    assert np.array_equal(_bits(scene_io.read_mesh_ply(rep2["path"])["occlusion"]), _bits(occ2))
    assert (rep2["rays"], rep2["max_distance"], rep2["bias"], rep2["seed"]) == (128, 0.2, 0.001, 3)
    # the siblings read a file with the channel and drop it
    c = clean_mesh.clean_mesh([r2["path"], "-o", str(tmp_path / "clean.ply"), "--keep_largest", "1"])
    s = simplify_mesh.simplify_mesh([r2["path"], "-o", str(tmp_path / "simple.ply"), "--cell_edges", "2.5"])
    d = compare_mesh.compare_mesh([r2["path"], r0["path"], "--samples", "2000"])
    assert c["faces"] > 0 and s["faces"] > 0 and d["hausdorff"] < 1e-5
    assert "occlusion" not in scene_io.read_mesh_ply(str(tmp_path / "clean.ply"))
    assert sorted(mesh_render.mesh_arrays(r2["path"])) == sorted(mesh_render.MESH_KEYS)
