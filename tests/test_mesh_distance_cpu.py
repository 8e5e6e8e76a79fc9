"""CPU: the numpy restatement of mesh comparison (tests/mesh_distance_ref.py) against hand-computed values and against
itself: the point-triangle distance in every Voronoi region of a triangle, the counter hash, the stratification of the
samples, and the grid search against the brute force over all faces (the L(r) argument, before any kernel runs)."""
import functools

import numpy as np
import pytest

import mesh_distance_ref as dr

CASES = dr.B_CASES + ("blob",)


@functools.lru_cache(maxsize=None)
def _meshes():
    return dr.b_meshes()


def test_single_triangle_in_every_region():
    P = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float64)
    idx = np.array([[0, 1, 2]])
    want = [((0.25, 0.25, 0.5), 0.25),    # above the interior: the plane
            ((0.25, 0.25, -2.0), 4.0),    # below it
            ((0.5, -1.0, 0.0), 1.0),      # the three edge regions
            ((-1.0, 0.5, 0.0), 1.0),
            ((1.0, 1.0, 0.0), 0.5),
            ((-1.0, -1.0, 0.0), 2.0),     # the three vertex regions
            ((2.0, -1.0, 0.0), 2.0),
            ((-1.0, 2.0, 0.0), 2.0),
            ((0.5, 0.0, 0.0), 0.0),       # on an edge, on a vertex, above an edge, above a vertex
            ((1.0, 0.0, 0.0), 0.0),
            ((0.0, 1.0, 0.0), 0.0),
            ((0.5, 0.0, 2.0), 4.0),
            ((0.5, 0.5, 1.0), 1.0),
            ((0.0, 0.0, -3.0), 9.0),
            ((2.0, 0.0, 1.0), 2.0)]
    p = np.array([w[0] for w in want], np.float64)
    got = dr.triangle_d2(p, np.broadcast_to(P, (len(p), 3, 3)), np.broadcast_to(idx, (len(p), 3)))
    assert got.tolist() == [w[1] for w in want]
    # the winding and the numbering of the vertices change nothing here, and the reversed face shares every bit
    for perm in ((1, 2, 0), (2, 0, 1), (0, 2, 1)):
        again = dr.triangle_d2(p, np.broadcast_to(P[:, perm], (len(p), 3, 3)), np.broadcast_to(idx[:, perm], (len(p), 3)))
        assert np.array_equal(again, got), perm
    # a face without area is unusable; one with a NaN corner or an index out of range too
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [np.nan, 0, 0]], np.float32)
    areas, skipped = dr.face_areas(v, [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 0, 3], [-1, 1, 3]])
    assert areas.tolist() == [0.0, 0.5, 0.0, 0.0, 0.0, 0.0] and skipped == 5


def test_hash_values():
    gamma = 0x9E3779B97F4A7C15  # splitmix64 from state 0 gives mix(gamma), mix(2 gamma), mix(3 gamma)
    got = dr.mix64(np.array([gamma, (2 * gamma) % 2 ** 64, (3 * gamma) % 2 ** 64, 0], np.uint64))
    assert [int(x) for x in got] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0]

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return z ^ (z >> 31)

    for seed, i, k in ((0, 0, 0), (0, 1, 0), (1, 2, 3), (7, 4096, 2), (2 ** 40 + 5, 2 ** 31 - 1, 1), (-1, 3, 0)):
        want = (mix((((seed % 2 ** 64) * 2 ** 32 + i) * 4 + k) % 2 ** 64) >> 11) * 2.0 ** -53
        got = float(dr.uniform(seed, np.array([i], np.uint64), k)[0])
        assert got == want and 0.0 <= got < 1.0, (seed, i, k)
    assert float(dr.uniform(0, np.array([0], np.uint64), 0)[0]) == 0.0
    u = dr.uniform(5, np.arange(100000, dtype=np.uint64), 1)
    assert abs(u.mean() - 0.5) < 0.005 and abs((u * u).mean() - 1.0 / 3.0) < 0.005


@pytest.mark.parametrize("name", CASES)
def test_samples_are_stratified_and_unambiguous(name):
    v, f = _meshes()[name]
    areas, skipped = dr.face_areas(v, f)
    assert (areas > 0).any()
    for n in dr.SAMPLE_SIZES:
        for seed in dr.SAMPLE_SEEDS:
            s = dr.sample_surface(v, f, n, seed)
            assert len(s["ambiguous"]) == 0, (name, n, seed)
            assert s["points"].shape == (n, 3) and s["points"].dtype == np.float32 and s["bary"].shape == (n, 2)
            assert np.abs(s["counts"] - s["expected"]).max() <= 2.0, (name, n, seed)
            assert (areas[s["face"]] > 0).all()
            assert (s["bary"] >= 0).all() and (s["bary"].astype(np.float64).sum(axis=1) <= 1.0 + 2.0 ** -23).all()
            # the point lies on its face: its distance to that triangle is a float32 rounding
            _, P = dr._corners(v, f)
            d2 = dr.triangle_d2(s["points"].astype(np.float64), P[s["face"]], np.asarray(f, np.int64)[s["face"]])
            scale = np.abs(P[s["face"]]).max(axis=(1, 2))
            assert (np.sqrt(d2) <= 2.0 ** -22 * np.maximum(scale, 1e-30)).all()
    if name == "debris":
        assert skipped == 3
    assert np.array_equal(dr.sample_surface(v, f, 63, 7)["points"], dr.sample_surface(v, f, 63, 7)["points"])
    assert len(dr.sample_surface(v, f, 0, 0)["points"]) == 0
    assert len(dr.sample_surface(v, np.asarray(f)[:0], 5, 0)["points"]) == 0


@pytest.mark.parametrize("name", CASES)
def test_grid_search_equals_brute_force(name):
    v, f = _meshes()[name]
    base = dr.build_grid(v, f)
    assert base["pairs"] <= 8 * len(f) + 4096 and all(1 <= G <= 256 for G in base["G"])
    # the one-cell run and the brute force test every face for every query: fewer queries where the faces are many
    q = dr.queries(v, f, base, stride=512 if len(f) >= dr.LARGE else 32 if len(f) >= 1000 else 8)
    points = np.concatenate(list(q.values()))
    want = dr.brute_force(points, v, f)
    assert want["queries_invalid"] == 3 and want["far"] == 0
    for scale in (0.5, 1.0, 3.0, 1e6):
        got = dr.closest(points, v, f, cell=scale * base["cell"])
        assert np.array_equal(got["d2"], want["d2"]), (name, scale)
        assert np.array_equal(got["face"], want["face"]), (name, scale)
        assert np.array_equal(got["distance"].view(np.uint32), want["distance"].view(np.uint32))
        if scale == 1e6:
            assert got["grid"]["G"] == [1, 1, 1] and got["shells"] == 1
    # with a limit: the same faces below it, the limit and -1 above it
    limit = float(np.median(want["d"][np.isfinite(want["d"])]))
    got = dr.closest(points, v, f, max_distance=limit)
    capped = dr.brute_force(points, v, f, max_distance=limit)
    assert got["far"] == capped["far"] > 0 and np.array_equal(got["face"], capped["face"])
    assert np.array_equal(got["distance"].view(np.uint32), capped["distance"].view(np.uint32))
    far = (got["face"] < 0) & np.isfinite(points).all(axis=1)
    assert (got["distance"][far] == np.float32(limit)).all() and np.isinf(got["distance"][-3:]).all()
    near = capped["face"] >= 0
    assert np.array_equal(got["d2"][near], want["d2"][near])


def test_own_vertices_are_at_distance_zero_and_shared_edges_tie_exactly():
    v, f = _meshes()["blob"]
    got = dr.closest(v, v, f)
    assert (got["d2"] == 0.0).all() and (got["second2"] == 0.0).all()
    first = np.full(len(v), len(f), np.int64)
    np.minimum.at(first, np.asarray(f, np.int64).reshape(-1), np.repeat(np.arange(len(f)), 3))
    assert np.array_equal(got["face"], first)  # the smallest face index among the faces around the vertex
