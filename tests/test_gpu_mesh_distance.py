"""GPU: mesh comparison (csrc/mesh_distance.hip through mesh.sample_surface / mesh.closest_point / mesh.distance,
compare_mesh.py, simplify_mesh.py --distance) against its numpy restatement (tests/mesh_distance_ref.py).  Samples: face by
array_equal, points and barycentrics as bit patterns (the inputs have no sample within 2^-40 A of a boundary of the
cumulative areas).  Closest triangle: face by array_equal except where the restatement's two best d^2 are within 2^-40
relative; distance within 2^-22 max(d, cell): a float64 sqrt that need not be correctly rounded and one float32 rounding
that may fall either way.  The measured maxima are printed.  Measured on an MI355X: 0 faces differ, no open tie, the largest
distance difference 0.248 of the tolerance (the float32 rounding itself).  Against the restatement the strip keeps every 64th
and the blob every 4th of its vertex, second-mesh and random queries (mesh_distance_ref.default_stride: the restatement tests
every face of a one-cell grid for every query); test_grid_independence runs all of them against the GPU's one-cell grid."""
import ctypes as C
import functools
import json
import math

import numpy as np
import pytest
import torch

import mesh_clean_ref as cr
import mesh_distance_ref as dr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _mesh(v, f):
    """A device Mesh over positions and faces, the attributes zero."""
    import mesh
    v = torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(-1, 3)).to(DEV)
    f = torch.from_numpy(np.ascontiguousarray(f, np.int32).reshape(-1, 3)).to(DEV)
    z3, z1 = torch.zeros_like(v), torch.zeros(v.shape[0], device=DEV)
    return mesh.Mesh(v, f, z3, z3.clone(), z1, z1.clone())


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _blob():
    """(the extracted blob mesh on the device, vertices, faces, h).  Read-only for the tests."""
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    return m, m.vertices.cpu().numpy(), m.faces.cpu().numpy(), float(h)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, the restatement's default grid, the queries, the restatement's answer to them).  Read-only."""
    if name == "blob":
        _, v, f, _ = _blob()
        assert (len(v), len(f)) == (980, 1944)
    else:
        d = sr.shared_cases()[name][0]
        v, f = d["vertices"], d["faces"]
    grid = dr.build_grid(v, f)
    q = dr.queries(v, f, grid)
    points = np.concatenate(list(q.values()))
    return v, f, grid, q, points, dr.closest(points, v, f, grid=grid)


def _compare(got_d, got_f, want, cell, what):
    d, f = got_d.cpu().numpy(), got_f.cpu().numpy()
    assert d.dtype == np.float32 and f.dtype == np.int32 and d.shape == want["distance"].shape
    inf = np.isinf(want["d"])
    assert np.array_equal(np.isinf(d), inf) and (d[inf] > 0).all()
    err = np.abs(d[~inf].astype(np.float64) - want["d"][~inf]) / dr.distance_tolerance(want["d"][~inf], cell)
    open_ties = want["tie"]
    print("%s: %d queries, largest distance difference %.3f of its tolerance (2^-22 max(d, cell) = 1); %d open ties, %d faces "
          "differ" % (what, len(d), err.max() if len(err) else 0.0, int(open_ties.sum()), int((f != want["face"]).sum())))
    assert (err <= 1.0).all(), what
    assert np.array_equal(f[~open_ties], want["face"][~open_ties]), what
    return float(err.max()) if len(err) else 0.0


@pytest.mark.parametrize("name", dr.B_CASES + ("blob",))
def test_closest_point_equals_the_restatement(name):
    import mesh
    v, f, grid, q, points, want = _case(name)
    assert int(want["tie"].sum()) == 0, "the inputs are chosen to leave no tie open"
    m = _mesh(v, f)
    d, face, report = mesh.closest_point(torch.from_numpy(points).to(DEV), m, cell=grid["cell"])
    assert json.loads(json.dumps(report)) == report
    assert (report["cell"], report["dims"], report["pairs"]) == (grid["cell"], list(grid["G"]), grid["pairs"])
    invalid = 4 if name == "debris" else 3  # its NaN vertex is a query too
    assert (report["n"], report["far"], report["queries_invalid"]) == (len(points), 0, invalid) == (len(points), want["far"], want["queries_invalid"])
    assert report["faces_skipped"] == grid["faces_skipped"] == (3 if name == "debris" else 0)
    _compare(d, face, want, grid["cell"], name)
    # its own vertices, where a usable face references them: exactly 0, and the smallest face around the vertex
    nv = len(q["vertices"])
    used = np.zeros(len(v), bool)
    used[np.asarray(f, np.int64)[grid["usable"]].reshape(-1)] = True
    own = used[::dr.default_stride(f)]
    assert (d.cpu().numpy()[:nv][own] == 0.0).all() and (face.cpu().numpy()[:nv][own] >= 0).all()
    # the default cell is the restatement's up to the float32 subtraction in median_edge
    _, _, default = mesh.closest_point(torch.from_numpy(points[:8]).to(DEV), m)
    assert abs(default["cell"] - grid["cell"]) <= 1e-5 * grid["cell"]


@pytest.mark.parametrize("name", dr.B_CASES + ("blob",))
def test_grid_independence(name):
    """Every cell size gives the bits of the one-cell grid, the GPU's own brute force; every query of the case, unthinned."""
    import mesh
    v, f, grid, _, _, _ = _case(name)
    points = torch.from_numpy(np.concatenate(list(dr.queries(v, f, grid, stride=1).values()))).to(DEV)
    m = _mesh(v, f)
    d1, f1, r1 = mesh.closest_point(points, m, cell=1e6 * grid["cell"])
    assert r1["dims"] == [1, 1, 1] and r1["pairs"] == int(grid["usable"].sum())
    for scale in (0.5, 1.0, 3.0):
        d, face, r = mesh.closest_point(points, m, cell=scale * grid["cell"])
        assert np.array_equal(_bits(d), _bits(d1)) and torch.equal(face, f1), (name, scale, r)
        d2, face2, r2 = mesh.closest_point(points, m, cell=scale * grid["cell"])
        assert np.array_equal(_bits(d2), _bits(d)) and torch.equal(face2, face) and r2 == r


def test_ties_go_to_the_smaller_face_index():
    import mesh
    # sheets: the point midway between two sheets' coinciding flaps is as far from the one as from the other
    # (the same-winding pair 0 / 1 and the back-to-back pair 1 / 2); cell 2.5 puts the sheets at z = 0.75, 1, 1.25
    v, f = sr.sheets(2.5)
    assert sorted(set(v[:, 2].tolist())) == [0.75, 1.0, 1.25]
    pts = np.array([[2.0, 3.0, 0.875], [3.5, 2.25, 0.875], [1.5, 1.5, 0.875], [2.0, 3.0, 1.125], [5.0, 4.5, 1.125]], np.float32)
    want = dr.brute_force(pts, v, f)
    assert (want["second2"] == want["d2"]).all() and (want["d2"] == 0.125 ** 2).all()
    assert (want["face"][:3] < 8).all() and ((want["face"][3:] >= 8) & (want["face"][3:] < 16)).all()
    d, face, _ = mesh.closest_point(torch.from_numpy(pts).to(DEV), _mesh(v, f))
    assert np.array_equal(face.cpu().numpy(), want["face"]) and np.array_equal(_bits(d), _bits(want["distance"]))
    # a duplicated triangle behind other faces: the copy with the smaller index
    cv, cf = sr.cube()
    dup = np.concatenate([cf, cf[5:6], cf[:5]])
    pts = dr.sample_surface(cv, cf[5:6], 64, 1)["points"] + np.float32(0.0)
    want = dr.brute_force(pts, cv, dup)
    d, face, _ = mesh.closest_point(torch.from_numpy(pts).to(DEV), _mesh(cv, dup))
    got = face.cpu().numpy()
    assert np.array_equal(got, want["face"]) and (got < len(cf)).all() and (got == 5).sum() > 32


def test_max_distance():
    import mesh
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    h = 0.375
    pts = np.array([[0.25, 0.25, h], [0.25, 0.25, -h], [0.25, 0.25, np.nextafter(np.float32(h), np.float32(1))],
                    [0.25, 0.25, 40.0], [-30.0, 0.5, 0.0]], np.float32)
    d, face, report = mesh.closest_point(torch.from_numpy(pts).to(DEV), _mesh(v, f), max_distance=h)
    assert face.tolist() == [0, 0, -1, -1, -1] and d.tolist() == [h] * 5 and report["far"] == 3
    for name in ("fan", "blob"):
        v, f, grid, _, points, want = _case(name)
        limit = float(np.median(want["d"][np.isfinite(want["d"])]))
        capped = dr.closest(points, v, f, grid=grid, max_distance=limit)
        d, face, report = mesh.closest_point(torch.from_numpy(points).to(DEV), _mesh(v, f), cell=grid["cell"], max_distance=limit)
        assert report["far"] == capped["far"] > 0 and report["queries_invalid"] == 3 == capped["queries_invalid"]
        _compare(d, face, capped, grid["cell"], name + " with a limit")
        far = capped["face"] < 0
        assert (d.cpu().numpy()[far & np.isfinite(points).all(axis=1)] == np.float32(limit)).all()
    with pytest.raises(ValueError, match="max_distance"):
        mesh.closest_point(torch.from_numpy(pts).to(DEV), _mesh(v, f), max_distance=-1.0)


@pytest.mark.parametrize("name", dr.B_CASES + ("blob",))
def test_sampling_equals_the_restatement(name):
    import mesh
    v, f, _, _, _, _ = _case(name)
    m = _mesh(v, f)
    for n in dr.SAMPLE_SIZES:
        for seed in dr.SAMPLE_SEEDS:
            want = dr.sample_surface(v, f, n, seed)
            assert len(want["ambiguous"]) == 0, (name, n, seed)
            points, face, bary = mesh.sample_surface(m, n, seed)
            assert points.dtype == torch.float32 and face.dtype == torch.int32 and bary.dtype == torch.float32
            assert tuple(points.shape) == (n, 3) and tuple(face.shape) == (n,) and tuple(bary.shape) == (n, 2)
            assert np.array_equal(face.cpu().numpy(), want["face"]), (name, n, seed)
            assert np.array_equal(_bits(points), _bits(want["points"])), (name, n, seed)
            assert np.array_equal(_bits(bary), _bits(want["bary"])), (name, n, seed)
    again = mesh.sample_surface(m, 4097, 7)
    assert all(torch.equal(a, b) for a, b in zip(again, (points, face, bary)))


def test_metrics_with_known_answers():
    import mesh
    pv, pf = sr.plane_grid()
    h = 0.125
    shifted = pv + np.array([0, 0, h], np.float32)
    r = mesh.distance(_mesh(pv, pf), _mesh(shifted, pf), samples=5000, seed=2, taus=(0.1, h, 0.2))
    assert json.loads(json.dumps(r)) == r
    for side in ("a_to_b", "b_to_a"):
        assert r[side] == dict(n=5000, far=0, mean=h, rms=h, median=h, max=h), r[side]
    assert r["chamfer"] == h and r["hausdorff"] == h and r["seed"] == 2 and r["samples"] == 5000
    assert [(t["tau"], t["precision"], t["recall"], t["fscore"]) for t in r["taus"]] == [(0.1, 0.0, 0.0, 0.0), (h, 1.0, 1.0, 1.0),
                                                                                         (0.2, 1.0, 1.0, 1.0)]
    assert r["faces_skipped"] == dict(a=0, b=0) and r["grid"]["a"]["dims"] == r["grid"]["b"]["dims"]
    # a mesh against itself: the samples are float32 roundings of points of the surface
    m, v, f, hb = _blob()
    r = mesh.distance(m, m, samples=20000, seed=1)
    extent = float((v.max(axis=0) - v.min(axis=0)).max())
    print("blob against itself: max %.3e, allowed 2^-22 extent = %.3e" % (r["hausdorff"], 2.0 ** -22 * extent))
    assert r["hausdorff"] <= 2.0 ** -22 * extent and r["a_to_b"] == r["b_to_a"]
    # DESIGN.md's distance bound of mesh.simplify: a point of the simplified surface is within sqrt(3) cell of the raw one
    cell = float(np.float32(2) * np.float32(hb))
    simple, _ = mesh.simplify(m, cell)
    pts = mesh.sample_surface(simple, 20000, 0)[0]
    d, _, _ = mesh.closest_point(pts, m)
    bound = math.sqrt(3.0) * cell
    r = mesh.distance(simple, m, samples=20000, seed=0)
    print("simplified (2 h) -> raw: mean %.5f max %.5f; raw -> simplified: mean %.5f max %.5f; sqrt(3) cell = %.5f, h = %.5f"
          % (r["a_to_b"]["mean"], r["a_to_b"]["max"], r["b_to_a"]["mean"], r["b_to_a"]["max"], bound, hb))
    assert float(d.max()) <= bound + 2.0 ** -22 * max(bound, extent)
    assert r["a_to_b"]["max"] == float(d.max())


def test_empty_and_degenerate_inputs_launch_nothing():
    import mesh
    _, v, f, _ = _blob()
    pts = torch.from_numpy(np.array([[0, 0, 0], [np.nan, 0, 0]], np.float32)).to(DEV)
    flat = np.zeros_like(v)  # every face without area
    for m in (_mesh(v[:0], f[:0]), _mesh(v, f[:0]), _mesh(v[:0], f), _mesh(flat, f)):
        points, face, bary = mesh.sample_surface(m, 100, 0)
        assert tuple(points.shape) == (0, 3) and tuple(face.shape) == (0,) and tuple(bary.shape) == (0, 2)
        d, face, report = mesh.closest_point(pts, m)
        assert torch.isinf(d).all() and (d > 0).all() and face.tolist() == [-1, -1]
        assert report["queries_invalid"] == 1 and report["far"] == 0 and report["faces_skipped"] == int(m.faces.shape[0])
        assert report["dims"] == [0, 0, 0] and report["pairs"] == 0
    m = _mesh(v, f)
    assert tuple(mesh.sample_surface(m, 0, 0)[0].shape) == (0, 3)
    d, face, report = mesh.closest_point(pts[:0], m)
    assert tuple(d.shape) == (0,) and tuple(face.shape) == (0,) and report["n"] == 0
    r = mesh.distance(_mesh(v, f[:0]), m, samples=100)
    assert r["a_to_b"]["n"] == 0 and r["b_to_a"]["n"] == 100 and r["b_to_a"]["max"] == float("inf")
    assert r["faces_skipped"] == dict(a=0, b=0) and r["grid"]["a"] is None
    with pytest.raises(ValueError, match="float32"):
        mesh.closest_point(pts.double(), m)


def test_invalid_faces_touch_nothing_outside_the_arrays():
    """Every entry point through the C ABI on the debris mesh (a NaN vertex, a face on an index == V, one on -1) with pads
    of -7 around every array; then gigs_mesh_closest with a cell_start entry past the end."""
    import gigs_lib
    d = sr.shared_cases()["debris"][0]
    v, f = d["vertices"], d["faces"]
    V, F = len(v), len(f)
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    pad = 64

    def padded(n, dtype, fill=-7):
        t = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
        return t, t[pad:pad + n]

    def untouched(t, n, fill=-7):
        return bool((t[:pad] == fill).all()) and bool((t[pad + n:] == fill).all())

    vert_all, vert = padded(3 * V, torch.float32, -7.0)
    vert.copy_(torch.from_numpy(v.reshape(-1)))
    faces_all, faces = padded(3 * F, torch.int32)
    faces.copy_(torch.from_numpy(f.reshape(-1)))
    areas_all, areas = padded(F, torch.float64, -7.0)
    skip_all, skip = padded(1, torch.int32)
    gigs_lib.check(lib.gigs_mesh_face_areas(V, F, vert.data_ptr(), faces.data_ptr(), areas.data_ptr(), skip.data_ptr(), s), "areas")
    want_areas, want_skipped = dr.face_areas(v, f)
    assert untouched(areas_all, F, -7.0) and untouched(skip_all, 1) and skip.tolist() == [want_skipped] == [3]
    got_areas = areas.cpu().numpy()
    assert np.array_equal(got_areas > 0, want_areas > 0) and np.allclose(got_areas, want_areas, rtol=2.0 ** -50, atol=0)

    n = 257
    cum = torch.cumsum(areas, 0)
    pts_all, pts = padded(3 * n, torch.float32, -7.0)
    sf_all, sf = padded(n, torch.int32)
    bary_all, bary = padded(2 * n, torch.float32, -7.0)
    flag_all, flag = padded(1, torch.int32)
    flag.zero_()
    gigs_lib.check(lib.gigs_mesh_sample_surface(V, F, vert.data_ptr(), faces.data_ptr(), cum.data_ptr(), n, 5, pts.data_ptr(),
                                                sf.data_ptr(), bary.data_ptr(), flag.data_ptr(), s), "sample")
    want = dr.sample_surface(v, f, n, 5)
    assert len(want["ambiguous"]) == 0
    assert untouched(pts_all, 3 * n, -7.0) and untouched(sf_all, n) and untouched(bary_all, 2 * n, -7.0) and untouched(flag_all, 1)
    assert flag.tolist() == [0] and np.array_equal(sf.cpu().numpy(), want["face"])
    assert np.array_equal(_bits(pts).reshape(n, 3), _bits(want["points"]))

    g = dr.build_grid(v, f, cell=0.5)
    lo, dims = (C.c_float * 3)(*g["lo"].tolist()), (C.c_int * 3)(*g["G"])
    counts_all, counts = padded(F, torch.int32)
    gigs_lib.check(lib.gigs_mesh_grid_count(V, F, vert.data_ptr(), faces.data_ptr(), areas.data_ptr(), lo, g["cell"], dims,
                                            counts.data_ptr(), s), "count")
    assert untouched(counts_all, F) and int(counts.sum()) == g["pairs"] and bool((counts[~(areas > 0)] == 0).all())
    total = g["pairs"]
    offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts
    pairs_all, pairs = padded(total, torch.int64)
    gigs_lib.check(lib.gigs_mesh_grid_pairs(V, F, vert.data_ptr(), faces.data_ptr(), areas.data_ptr(), lo, g["cell"], dims,
                                            offsets.data_ptr(), total, pairs.data_ptr(), flag.data_ptr(), s), "pairs")
    assert untouched(pairs_all, total) and untouched(flag_all, 1) and flag.tolist() == [0]
    spairs_all, spairs = padded(total, torch.int64)
    spairs.copy_(torch.sort(pairs).values)
    assert np.array_equal((spairs & 0xFFFFFFFF).cpu().numpy(), g["pair_face"])
    cells = g["G"][0] * g["G"][1] * g["G"][2]
    start_all, start = padded(cells + 1, torch.int64)
    start.copy_(torch.searchsorted(spairs, torch.arange(cells + 1, dtype=torch.int64, device=DEV) << 32))
    assert np.array_equal(start.cpu().numpy(), g["cell_start"])
    # offsets that leave the pairs: the flag, and nothing stored
    pairs.fill_(-7)
    gigs_lib.check(lib.gigs_mesh_grid_pairs(V, F, vert.data_ptr(), faces.data_ptr(), areas.data_ptr(), lo, g["cell"], dims,
                                            (offsets + total).data_ptr(), total, pairs.data_ptr(), flag.data_ptr(), s), "pairs")
    assert flag.tolist() == [1] and bool((pairs_all == -7).all())
    flag.zero_()

    q = np.concatenate(list(dr.queries(v, f, g).values()))
    N = len(q)
    q_all, qd = padded(3 * N, torch.float32, -7.0)
    qd.copy_(torch.from_numpy(q.reshape(-1)))
    dist_all, dist = padded(N, torch.float32, -7.0)
    face_all, face = padded(N, torch.int32)
    cnt_all, cnt = padded(2, torch.int32)
    order_all, order = padded(N, torch.int64)
    order.copy_(torch.arange(N - 1, -1, -1, device=DEV))

    def closest(cell_start):
        return lib.gigs_mesh_closest(V, F, vert.data_ptr(), faces.data_ptr(), lo, g["cell"], dims, cell_start.data_ptr(),
                                     spairs.data_ptr(), total, N, qd.data_ptr(), order.data_ptr(), float("inf"), dist.data_ptr(),
                                     face.data_ptr(), cnt.data_ptr(), flag.data_ptr(), s)

    gigs_lib.check(closest(start), "closest")
    want = dr.closest(q, v, f, grid=g)
    assert all(untouched(t, k, fill) for t, k, fill in ((dist_all, N, -7.0), (face_all, N, -7), (cnt_all, 2, -7), (flag_all, 1, -7),
                                                       (vert_all, 3 * V, -7.0), (faces_all, 3 * F, -7), (q_all, 3 * N, -7.0)))
    assert flag.tolist() == [0] and cnt.tolist() == [0, 4] == [want["far"], want["queries_invalid"]]
    assert int(want["tie"].sum()) == 0
    _compare(dist, face, want, g["cell"], "debris through the C ABI")
    # a cell_start entry past the end: the flag is raised, the threads that met it store nothing
    broken = start.clone()
    broken[-1] = total + 5
    dist.fill_(-7.0)
    face.fill_(-7)
    gigs_lib.check(closest(broken), "closest")
    assert flag.tolist() == [1] and untouched(dist_all, N, -7.0) and untouched(face_all, N) and untouched(cnt_all, 2)
    assert bool((dist == -7.0).any()) and bool(((dist == -7.0) == (face == -7)).all())
    kept = (dist != -7.0).cpu().numpy()
    assert np.array_equal(face.cpu().numpy()[kept], want["face"][kept])


def test_tools(tmp_path):
    import compare_mesh
    import mesh
    import mesh_render
    import scene_io
    import simplify_mesh
    m, v, f, h = _blob()
    raw = str(tmp_path / "raw.ply")
    scene_io.save_mesh_ply(raw, *m)
    cell = repr(2.0 * h)
    plain = simplify_mesh.simplify_mesh([raw, "-o", str(tmp_path / "plain.ply"), "--cell", cell])
    timed = simplify_mesh.simplify_mesh([raw, "-o", str(tmp_path / "measured.ply"), "--cell", cell, "--distance", "2000"])
    assert sorted(timed) == sorted(list(plain) + ["distance"]) and json.loads(json.dumps(timed)) == timed
    assert open(plain["path"], "rb").read() == open(timed["path"], "rb").read()
    assert all(timed[k] == plain[k] for k in plain if k not in ("path", "simplify_s"))
    assert timed["distance"]["samples"] == 2000 and 0 < timed["distance"]["chamfer"] < timed["distance"]["hausdorff"] < 1.0
    out = str(tmp_path / "report.json")
    rep = compare_mesh.compare_mesh([raw, plain["path"], "--samples", "3000", "--seed", "4", "--tau", "0.01", "0.05",
                                     "--max_distance", "0.5", "-o", out])
    assert json.load(open(out)) == rep == json.loads(json.dumps(rep))

    def load(path):
        return mesh_render.device_mesh(path, DEV)

    direct = mesh.distance(load(raw), load(plain["path"]), samples=3000, seed=4, taus=(0.01, 0.05), max_distance=0.5)
    assert {k: rep[k] for k in direct} == direct and rep["a"] == raw and rep["b"] == plain["path"]
    assert [t["tau"] for t in rep["taus"]] == [0.01, 0.05] and 0 < rep["taus"][0]["fscore"] <= rep["taus"][1]["fscore"] <= 1
