"""CPU: the restatement of mesh simplification (tests/mesh_simplify_ref.py) against independent code -- clustering with a
dict, one np.linalg.solve per cluster, a brute-force set of rotated triples -- and against what the definition promises on
a cube, a plane and the blob field's spheres; the argument checks of mesh.simplify / mesh.cluster_grid."""
import functools

import numpy as np
import pytest

import mesh_clean_ref as cr
import mesh_ref
import mesh_simplify_ref as sr

REG = 1e-3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _independent(mesh, cell, origin, reg=REG):
    """The definition once more, vertex by vertex and face by face in plain Python.  -> dict(cluster_of, C, faces (before
    compaction), vertices, normals, albedo, roughness, metallic ([C,..] float32), counts)."""
    v = np.asarray(mesh["vertices"], np.float32)
    V = len(v)
    cell32 = np.float32(cell)
    inv = np.float32(1) / cell32
    finite = [bool(np.isfinite(p).all()) for p in v]
    org = np.asarray(origin, np.float32) if origin is not None else np.min([p for p, ok in zip(v, finite) if ok], axis=0)
    cell_of = {}
    for i in range(V):
        if not finite[i]:
            continue
        c = tuple(int(np.floor(np.float32(np.float32(v[i, a] - org[a]) * inv))) for a in range(3))
        if all(0 <= x < (1 << 21) for x in c):
            cell_of[i] = c
    cells = sorted(set(cell_of.values()), key=lambda c: (c[2], c[1], c[0]))  # the key: z most significant
    number = {c: k for k, c in enumerate(cells)}
    C = len(cells)
    cluster_of = np.array([number[cell_of[i]] if i in cell_of else -1 for i in range(V)], np.int32).reshape(V)
    members = [[] for _ in range(C)]
    for i in range(V):
        if cluster_of[i] >= 0:
            members[cluster_of[i]].append(i)
    faces = np.asarray(mesh["faces"], np.int64).reshape(-1, 3)
    seen, out_faces = set(), []
    counts = dict(invalid=0, collapsed=0, duplicate=0)
    touching = [[] for _ in range(C)]
    for fi, f in enumerate(faces.tolist()):
        if not all(0 <= i < V for i in f) or any(cluster_of[i] < 0 for i in f):
            counts["invalid"] += 1
            out_faces.append((-1, -1, -1))
            continue
        k = [int(cluster_of[i]) for i in f]
        for c in dict.fromkeys(k):
            touching[c].append(fi)
        if len(set(k)) < 3:
            counts["collapsed"] += 1
            out_faces.append((-1, -1, -1))
            continue
        s = k.index(min(k))
        t = (k[s], k[(s + 1) % 3], k[(s + 2) % 3])
        if t in seen:
            counts["duplicate"] += 1
            out_faces.append((-1, -1, -1))
            continue
        seen.add(t)
        out_faces.append(t)
    p64 = v.astype(np.float64)
    cell64 = float(cell32)
    pos, nrm, alb, rgh, met = (np.zeros((C, 3), np.float32), np.zeros((C, 3), np.float32), np.zeros((C, 3), np.float32),
                               np.zeros(C, np.float32), np.zeros(C, np.float32))
    for k in range(C):
        g = org.astype(np.float64) + (np.array(cells[k], np.float64) + 0.5) * cell64
        A, b = np.zeros((3, 3)), np.zeros(3)
        for fi in touching[k]:
            q = p64[faces[fi]] - g
            n = np.cross(q[1] - q[0], q[2] - q[0])
            length = np.sqrt(n @ n)
            if length == 0:
                continue
            u = n / length
            A += 0.5 * length * np.outer(u, u)
            b += 0.5 * length * -(u @ q[0]) * u
        m = np.zeros(3)
        for i in members[k]:
            m = m + (p64[i] - g)
        m = m / len(members[k])
        lam = reg * np.trace(A) / 3.0
        x = np.linalg.solve(A + lam * np.eye(3), lam * m - b) if lam > 0 else m
        pos[k] = (g + np.clip(x, -0.5 * cell64, 0.5 * cell64)).astype(np.float32)
        s = np.zeros(3)
        for i in members[k]:
            s = s + np.asarray(mesh["normals"][i], np.float64)
        nl = np.sqrt(s @ s)
        nrm[k] = (s / nl).astype(np.float32) if nl > 0 else 0
        for name, dst in (("albedo", alb), ("roughness", rgh), ("metallic", met)):
            acc = np.zeros_like(np.asarray(mesh[name][0], np.float64))
            for i in members[k]:
                acc = acc + np.asarray(mesh[name][i], np.float64)
            dst[k] = (acc / len(members[k])).astype(np.float32)
    return dict(cluster_of=cluster_of, C=C, faces=np.array(out_faces, np.int32).reshape(-1, 3), vertices=pos, normals=nrm,
                albedo=alb, roughness=rgh, metallic=met, counts=counts, members=members)


def _check_against_independent(mesh, cell, origin):
    out, report, det = sr.simplify(mesh, cell, origin, REG)
    ind = _independent(mesh, cell, origin)
    assert det["C"] == ind["C"] == report["clusters"] and np.array_equal(det["cluster_of"], ind["cluster_of"])
    assert det["cluster_of"].dtype == np.int32 and det["faces"].dtype == np.int32
    assert np.array_equal(det["faces"], ind["faces"])
    assert report["faces_invalid"] == ind["counts"]["invalid"] and report["faces_collapsed"] == ind["counts"]["collapsed"]
    assert report["faces_duplicate"] == ind["counts"]["duplicate"]
    assert report["vertices_unclustered"] == int((ind["cluster_of"] < 0).sum())
    assert sorted(report) == sorted(sr.REPORT_KEYS)
    for k in ("albedo", "roughness", "metallic"):
        assert np.array_equal(_bits(det[k]), _bits(ind[k])), k
    assert (np.abs(det["vertices"].astype(np.float64) - ind["vertices"]) <= sr.position_tolerance(ind["vertices"], cell)).all()
    assert (np.abs(det["normals"].astype(np.float64) - ind["normals"]) <= sr.NORMAL_TOLERANCE).all()
    # the compaction: the kept faces in their order over the referenced clusters in theirs
    kept = ind["faces"][ind["faces"][:, 0] >= 0]
    used = np.unique(kept)
    assert report["faces"] == len(kept) == len(out["faces"]) and report["vertices"] == len(used) == len(out["vertices"])
    assert np.array_equal(out["faces"], np.searchsorted(used, kept)) and out["faces"].dtype == np.int32
    for k in ("vertices", "normals", "albedo", "roughness", "metallic"):
        assert np.array_equal(_bits(out[k]), _bits(det[k][used])), k
    if len(out["faces"]):  # nothing references a dropped cluster, nothing kept is unreferenced
        assert out["faces"].min() >= 0 and out["faces"].max() < len(out["vertices"])
        assert len(np.unique(out["faces"])) == len(out["vertices"])
    return out, report, det, ind


@functools.lru_cache(maxsize=None)
def _blob():
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    return mesh_ref.surface_nets(tsdf, weight, attr_weight, attr, lo, h, 1), h


def test_cube_representatives_sit_on_corners_edges_and_sides():
    """The unit cube, 4 x 4 quads per side, cell 0.5 from -0.25: three cells per axis, 26 of the 27 occupied.  All faces that
    touch a corner, edge or side cell lie on the cube's planes through it, so A = diag(w) there (w_i = 0 for an axis no
    plane is normal to) and, before the float32 rounding,
        x_i - plane_i = lam / (w_i + lam) (m_i - plane_i),    lam = reg (w_0 + w_1 + w_2) / 3,
    which is at most reg (w_mean / w_i) |m_i - plane_i|, and at most reg |m_i - plane_i| where the weights are equal.  The
    coordinates 0.25 and 0.75 fall on cell boundaries and go to the upper cell, so only two of the eight corner cells,
    (0,0,0) and (2,2,2), have equal weights; the six others have w = (1, 1.5, 1.5) / 16 or (1.5, 1.5, 4) / 16 and reach
    1.33 reg and 1.55 reg (measured: 1.664e-4 and 1.941e-4 against reg |m - corner| = 1.25e-4).  The factor w_mean / w_i is
    therefore part of the bound below; where the weights are equal it is the bound reg |m - corner|_inf itself (measured
    in cell (2,2,2): 1.0705e-4 against 1.0714e-4).  The member mean misses by more than ten times as much."""
    mesh, cell, origin = sr.shared_cases()["cube"]
    assert mesh["vertices"].shape == (98, 3) and mesh["faces"].shape == (192, 3)
    assert (mesh_ref.edge_counts(mesh["faces"])[1] == 2).all()
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    assert report["clusters"] == 26 and report["vertices"] == 26 and report["faces_invalid"] == 0
    rounding = 2.0 ** -23 * 1.25
    kinds = {0: 0, 1: 0, 2: 0, 3: 0}
    for k in range(det["C"]):
        c = det["cells"][k]
        on = [a for a in range(3) if c[a] != 1]  # the axes whose plane (coordinate c / 2) passes through the cell
        kinds[len(on)] += 1
        A, mean, pos = det["A"][k], det["mean"][k].astype(np.float64), det["vertices"][k].astype(np.float64)
        w = np.diag(A)
        assert np.abs(A - np.diag(w)).max() == 0 and all(w[a] > 0 for a in on) and all(w[a] == 0 for a in range(3) if a not in on)
        for a in on:
            plane = c[a] / 2.0
            miss, mean_miss = abs(pos[a] - plane), abs(mean[a] - plane)
            assert miss <= REG * (w.sum() / 3.0 / w[a]) * mean_miss + rounding, (c, a, miss, mean_miss)
            if w[on].min() == w[on].max() and len(on) == 3:
                assert miss <= REG * np.abs(mean - c / 2.0).max() + rounding
            if det["count"][k] > 1 and len(on) == 3:
                assert np.abs(mean - c / 2.0).max() > 10 * (REG * np.abs(mean - c / 2.0).max() + rounding)
        for a in range(3):  # along an edge or within a side nothing pulls: the mean's coordinate
            if a not in on:
                assert abs(pos[a] - mean[a]) <= rounding
    assert kinds == {0: 0, 1: 6, 2: 12, 3: 8}
    corner = det["vertices"][np.all(det["cells"] == 2, axis=1)][0].astype(np.float64)
    mean = det["mean"][np.all(det["cells"] == 2, axis=1)][0].astype(np.float64)
    print("corner cell (2,2,2): placed misses by %.4e, bound %.4e, member mean by %.4e" % (
        np.abs(corner - 1).max(), REG * np.abs(mean - 1).max(), np.abs(mean - 1).max()))


def test_plane_stays_a_plane():
    mesh, cell, origin = sr.shared_cases()["plane"]
    assert mesh["vertices"].shape == (81, 3)
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    assert 4 < report["clusters"] < 81 and report["faces"] > 0
    assert np.abs(det["vertices"][:, 2].astype(np.float64) - 0.25).max() <= 2.0 ** -23  # one float32 rounding of 0.25 + x
    assert np.abs(out["vertices"][:, 2].astype(np.float64) - 0.25).max() <= 2.0 ** -23


def test_a_cell_below_the_vertex_spacing_changes_nothing_but_the_order():
    mesh, cell, origin = sr.shared_cases()["identity"]
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    V = len(mesh["vertices"])
    assert report["clusters"] == V and report["faces_collapsed"] == 0 and report["faces_duplicate"] == 0
    want, _ = cr.clean(mesh)
    perm = np.argsort(det["cluster_of"])  # cluster k is vertex perm[k]
    assert sorted(det["cluster_of"].tolist()) == list(range(V)) and not np.array_equal(perm, np.arange(V))
    tol = sr.position_tolerance(want["vertices"][perm], cell)
    assert (np.abs(out["vertices"].astype(np.float64) - want["vertices"][perm]) <= tol).all()
    for k in ("albedo", "roughness", "metallic"):
        assert np.array_equal(_bits(out[k]), _bits(want[k][perm])), k
    n = want["normals"][perm].astype(np.float64)
    n /= np.sqrt((n * n).sum(axis=1, keepdims=True))
    assert (np.abs(out["normals"] - n) <= sr.NORMAL_TOLERANCE).all()
    # the faces: the same triangles with the new numbers, each rotated to lead with its smallest
    f = det["cluster_of"][want["faces"]]
    s = np.argmin(f, axis=1)
    r = np.arange(len(f))
    assert np.array_equal(out["faces"], np.stack([f[r, s], f[r, (s + 1) % 3], f[r, (s + 2) % 3]], 1))


def test_debris_and_a_nan_vertex():
    mesh, cell, origin = sr.shared_cases()["debris"]
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    assert report["faces_invalid"] == 3 and report["vertices_unclustered"] == 1 and det["cluster_of"][11] == -1
    assert report["faces_in"] == 11 and report["vertices_in"] == 12
    assert report["faces"] + report["faces_collapsed"] + report["faces_duplicate"] + report["faces_invalid"] == 11
    assert np.isfinite(out["vertices"]).all() and np.isfinite(det["vertices"]).all()
    # an explicit origin inside the mesh: what lies below it on an axis is unclustered too
    below = int((mesh["vertices"][:11] < np.float32(-0.6)).any(axis=1).sum())
    _, report, det, _ = _check_against_independent(mesh, cell, (-0.6, -0.6, -0.6))
    assert report["vertices_unclustered"] == below + 1 and 0 < below < 11


def test_same_winding_duplicates_go_and_opposite_ones_stay():
    mesh, cell, origin = sr.shared_cases()["sheets"]
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    assert report["clusters"] == 9 and report["faces_in"] == 24 and report["faces_collapsed"] == 0
    assert report["faces_duplicate"] == 8 and report["faces"] == 16 and report["vertices"] == 9
    assert (det["faces"][:8, 0] >= 0).all() and (det["faces"][8:16] == -1).all() and (det["faces"][16:, 0] >= 0).all()
    first = {tuple(t) for t in det["faces"][:8].tolist()}
    for t in det["faces"][16:].tolist():  # the third sheet: every triple reversed is one of the first sheet's
        a, b, c = t
        assert {(a, c, b), (c, b, a), (b, a, c)} & first and tuple(t) not in first


def test_a_crowded_cell():
    mesh, cell, origin = sr.shared_cases()["fan"]
    out, report, det, ind = _check_against_independent(mesh, cell, origin)
    assert max(len(m) for m in ind["members"]) == 301 and report["faces_collapsed"] >= 300  # the whole fan
    assert report["clusters"] > 4 and report["faces"] > 0


def test_random_strip_many_clusters():
    mesh, cell, origin = sr.shared_cases()["strip"]
    out, report, det, _ = _check_against_independent(mesh, cell, origin)
    assert report["vertices_in"] == 8194 and report["clusters"] > 256 and report["faces"] > 1000


@pytest.mark.parametrize("ratio,clusters,surviving,referenced,largest", [(2, 195, 376, 193, 16), (3, 89, 166, 86, 24)])
def test_blob_mesh(ratio, clusters, surviving, referenced, largest):
    """Measured with the restatement: mean distance to the analytic spheres 0.00227 (placed), 0.00541 (member means of the
    referenced clusters) and 0.00275 (raw vertices) at 2 h; 0.00635 against 0.00856 at 3 h."""
    m, h = _blob()
    assert (len(m["vertices"]), len(m["faces"])) == (980, 1944)
    cell = np.float32(ratio) * h
    out, report, det, ind = _check_against_independent(m, cell, None)
    assert report["clusters"] == clusters and report["faces"] == surviving and report["faces_duplicate"] == 0
    assert report["vertices"] == referenced and max(len(x) for x in ind["members"]) == largest
    assert report["faces_collapsed"] == 1944 - surviving and report["faces_invalid"] == 0
    used = np.unique(det["faces"][det["faces"][:, 0] >= 0])
    placed, mean = sr.sphere_distance(out["vertices"]).mean(), sr.sphere_distance(det["mean"][used]).mean()
    print("cell = %d h: placed %.5f, member mean %.5f, raw %.5f" % (ratio, placed, mean, sr.sphere_distance(m["vertices"]).mean()))
    assert placed < (0.6 if ratio == 2 else 1.0) * mean
    # the clamp: every representative lies in its cell
    lo = det["origin"].astype(np.float64) + det["cells"] * float(cell)
    assert (det["vertices"] >= lo - 1e-6).all() and (det["vertices"] <= lo + float(cell) + 1e-6).all()


def test_empty_inputs_of_the_restatement():
    m, h = _blob()
    for case, V, F in (({k: np.asarray(v)[:0] for k, v in m.items()}, 0, 0), (dict(m, faces=m["faces"][:0]), 980, 0)):
        out, report, det = sr.simplify(case, 0.1)
        assert len(out["vertices"]) == 0 and out["faces"].shape == (0, 3) and report["clusters"] == 0
        assert report["vertices_in"] == V and report["faces_in"] == F and sorted(report) == sorted(sr.REPORT_KEYS)


def test_argument_checks():
    import torch

    import mesh
    d = sr.shared_cases()["cube"][0]
    cpu = mesh.Mesh(*(torch.from_numpy(d[k]) for k in mesh.Mesh._fields))
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="cell must be positive"):
            mesh.simplify(cpu, bad)
        with pytest.raises(ValueError, match="cell must be positive"):
            mesh.cluster_map(cpu, bad)
        with pytest.raises(ValueError):
            sr.simplify(d, bad)
    with pytest.raises(ValueError, match="reg"):
        mesh.simplify(cpu, 0.5, reg=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.simplify(cpu, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.cluster_map(cpu, 0.5)
    # the extent: 2^21 cells per axis and no more
    lo, hi = np.zeros(3, np.float32), np.array([1.0, 1.0, 1.5], np.float32)
    org, inv = mesh.cluster_grid(lo, hi, 2.0 ** -20)
    assert org.dtype == np.float32 and org.tolist() == [0, 0, 0] and inv == np.float32(2.0 ** 20)
    with pytest.raises(ValueError, match="2\\^21 cells"):
        mesh.cluster_grid(lo, hi, 2.0 ** -21)
    far = dict(d, vertices=d["vertices"] * np.float32(2.0 ** 22))
    with pytest.raises(ValueError, match="2\\^21 cells"):
        sr.simplify(far, 1.0)
    with pytest.raises(ValueError, match="2\\^21 cells"):
        mesh.cluster_grid(far["vertices"].min(axis=0), far["vertices"].max(axis=0), 1.0)
    for args in ((lo, hi, 1e-42), (lo, hi, 0.5, (0.0, np.inf, 0.0))):
        with pytest.raises(ValueError):
            mesh.cluster_grid(*args)
    # the same origin and reciprocal as the restatement's, an explicit origin taken as it is
    v = sr.shared_cases()["strip"][0]["vertices"]
    for origin in (None, (-1.5, -1.25, -2.0)):
        a, b = mesh.cluster_grid(v.min(axis=0), v.max(axis=0), 0.25, origin), sr.cluster_grid(v, 0.25, origin)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    org, _ = mesh.cluster_grid(np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32), 0.5)  # no finite vertex
    assert org.tolist() == [0, 0, 0]
