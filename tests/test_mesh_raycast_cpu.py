"""CPU: the numpy restatement of ray casting and occlusion baking (tests/mesh_raycast_ref.py) against hand-computed values and
against itself -- the slab traversal of the triangle grid against the brute force over all faces at four cell sizes (the
completeness argument of DESIGN.md, "Baking occlusion", before any kernel runs), watertightness along shared edges, the
grazing guard, the bake on shapes whose occlusion is known -- and the PLY layout with and without the occlusion channel."""
import functools
import io
import os
import struct

import numpy as np
import pytest

import mesh_distance_ref as dr
import mesh_raycast_ref as rr
import mesh_simplify_ref as sr

CASES = dr.B_CASES + ("blob",)


@functools.lru_cache(maxsize=None)
def _meshes():
    return dr.b_meshes()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, what):
    assert np.array_equal(a["face"], b["face"]), what
    assert np.array_equal(a["t64"].view(np.uint64), b["t64"].view(np.uint64)), what
    assert np.array_equal(_bits(a["t"]), _bits(b["t"])) and np.array_equal(_bits(a["bary"]), _bits(b["bary"])), what
    assert (a["hits"], a["rays_invalid"]) == (b["hits"], b["rays_invalid"]), what


@pytest.mark.parametrize("name", CASES)
def test_traversal_equals_brute_force(name):
    v, f = _meshes()[name]
    base = dr.build_grid(v, f)
    sets = rr.ray_sets(v, f, base, n_random=256)
    o = np.concatenate([s[0] for s in sets.values()])
    d = np.concatenate([s[1] for s in sets.values()])
    thin = 16 if len(f) >= dr.LARGE else 4 if len(f) >= 1000 else 1
    if thin > 1:  # the strip has a one-cell grid at every cell size, so every ray tests every face; the blob's rays walk far
        sets = {k: (s[0], s[1]) if k == "bad" else (s[0][::thin], s[1][::thin]) for k, s in sets.items()}
        o = np.concatenate([s[0] for s in sets.values()])
        d = np.concatenate([s[1] for s in sets.values()])
    want = rr.brute_force(o, d, v, f)
    assert want["rays_invalid"] == len(sets["bad"][0]) and want["hits"] > 0
    n_aimed = len(sets["aimed"][0])
    at = len(sets["random"][0])
    # most rays aimed at a vertex, an edge midpoint or a centroid from outside hit (float32 rounding of the direction lets
    # one aimed at the silhouette pass by; test_known_answers_on_the_cube has the rays that cannot miss)
    assert (want["face"][at:at + n_aimed] >= 0).mean() > 0.5, name
    away = slice(len(o) - len(sets["bad"][0]) - len(sets["away"][0]), len(o) - len(sets["bad"][0]))
    assert (want["face"][away] == -1).all() and np.isinf(want["t"][away]).all()
    seen = set()
    for cell in rr.cell_sizes(v, f):
        g = dr.build_grid(v, f, cell)
        seen.add(tuple(g["G"]))
        got = rr.raycast(o, d, v, f, grid=g)
        _same(got, want, (name, cell, g["G"]))
        assert got["tests"] <= len(o) * max(int(g["usable"].sum()), 1) * 27 and got["slabs"] <= len(o) * max(g["G"])
    assert (1, 1, 1) in seen
    # a limit on t: the hits beyond it go, the others keep their bits
    lim = float(np.median(want["t64"][want["face"] >= 0]))
    short = rr.raycast(o, d, v, f, t_max=lim, grid=base)
    _same(short, rr.brute_force(o, d, v, f, t_max=lim), (name, "t_max"))
    keep = want["t64"] <= lim
    assert np.array_equal(short["face"][keep], want["face"][keep]) and (short["face"][~keep] == -1).all()


def test_known_answers_on_the_cube():
    v, f = sr.cube()
    v = v.astype(np.float32)
    edge = float(v.max())
    c = np.full(3, edge / 2)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    got = rr.raycast(np.repeat(c[None], 6, 0).astype(np.float32), axes.astype(np.float32), v, f)
    assert got["t64"].tolist() == [edge / 2] * 6
    P = v[np.asarray(f, np.int64)].astype(np.float64)
    for k, a in enumerate(axes):
        p = c + a * edge / 2
        # the centre of a side is a vertex that several of its triangles share: the smallest index among them wins
        on = [i for i in range(len(f)) if np.allclose(np.linalg.det(np.stack([P[i, 1] - P[i, 0], P[i, 2] - P[i, 0], p - P[i, 0]])), 0)
              and (P[i].min(0) <= p).all() and (p <= P[i].max(0)).all()]
        assert len(on) >= 2 and got["face"][k] == min(on), (k, on)
    # watertight: rays from outside at every vertex and every edge midpoint always hit
    E = np.concatenate([P[:, 0], P[:, 1], P[:, 2], (P[:, 0] + P[:, 1]) / 2, (P[:, 1] + P[:, 2]) / 2, (P[:, 2] + P[:, 0]) / 2])
    i = np.arange(len(E), dtype=np.uint64)
    out = c + (np.stack([dr.uniform(5, i, k) for k in range(3)], 1) - 0.5) * 0.9 * edge  # inside: aim outwards through E
    o = (E + 3.0 * (E - out)).astype(np.float32)
    d = (E - o.astype(np.float64)).astype(np.float32)
    for cell in (None, edge / 8, 100.0 * edge):
        hit = rr.raycast(o, d, v, f, cell=cell)
        assert (hit["face"] >= 0).all() and hit["hits"] == len(o)
        assert np.array_equal(hit["face"], rr.brute_force(o, d, v, f)["face"])
    # grazing: a ray in the plane of a side misses that side; it hits the sides it crosses at their edges instead
    o = np.array([[-1.0, edge / 3, 0.0], [-1.0, edge / 3, edge]], np.float32)
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]], np.float32)
    hit = rr.raycast(o, d, v, f)
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    for k in range(2):
        assert hit["face"][k] >= 0 and n[hit["face"][k], 2] == 0 and hit["t64"][k] == 1.0
    # one triangle, both sides, the barycentrics of the hit
    tv = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    one = rr.raycast(np.array([[1, 2, 5], [1, 2, -5], [3, 3, 5]], np.float32), np.array([[0, 0, -1], [0, 0, 2], [0, 0, -1]], np.float32),
                     tv, [[0, 1, 2]])
    assert one["face"].tolist() == [0, 0, -1] and one["t"].tolist() == [5.0, 2.5, np.inf]
    assert one["bary"].tolist() == [[0.25, 0.5], [0.25, 0.5], [0.0, 0.0]]


def test_bake_on_known_shapes():
    table = rr.direction_table(64, 4)
    assert table.dtype == np.float32 and table.shape == (4, 64, 3) and (table[..., 2] >= 0).all()
    assert np.abs((table.astype(np.float64) ** 2).sum(-1) - 1).max() < 1e-6
    assert abs(table[0, :, 2].astype(np.float64).mean() - 2.0 / 3.0) < 0.01  # cosine-weighted: E[z] = 2/3
    T, B = rr.frame(np.array([[0, 0, 1.0], [0, 0, -1.0], [0.6, 0, 0.8], [1.0, 0, 0]]))
    n = np.array([[0, 0, 1.0], [0, 0, -1.0], [0.6, 0, 0.8], [1.0, 0, 0]])
    for a, b in ((T, T), (B, B), (T, B), (T, n), (B, n)):
        assert np.allclose((a * b).sum(-1), 1.0 if a is b else 0.0, atol=1e-15)
    assert np.allclose(np.cross(T, B), n, atol=1e-15)
    # a closed box seen from inside: nothing is open
    v, f, nrm = rr.box_interior()
    got = rr.bake(v, f, nrm, table, max_distance=8.0)
    assert (got["hits"] == 64).all() and (got["occlusion"] == 0).all() and got["no_normal"] == 0
    assert np.array_equal(got["hits"], rr.bake(v, f, nrm, table, max_distance=8.0, brute=True)["hits"])
    # a plane: everything is open
    pv, pf = sr.plane_grid()
    pn = np.repeat([[0.0, 0.0, 1.0]], len(pv), 0).astype(np.float32)
    got = rr.bake(pv, pf, pn, table)
    assert (got["hits"] == 0).all() and (got["occlusion"] == 1).all()
    # a crease: a floor vertex at the foot of a wall loses the directions that point into the wall, as the table counts them
    cv, cf, cn, rows = rr.crease()
    got = rr.bake(cv, cf, cn, table, max_distance=4.0, bias=1e-3, seed=9)
    for r in rows:
        n = cn[r].astype(np.float64)[None]
        T, B = rr.frame(n)
        t = table[got["rotation"][r]].astype(np.float64)
        d = (t[:, 0:1] * T + t[:, 1:2] * B) + t[:, 2:3] * n  # the directions in the world
        assert (np.abs(d[:, 0]) > 1e-4).all()  # none so close to the wall's plane that max_distance decides
        blocked = int(((d[:, 0] < 0) | (d[:, 2] < -1e-3)).sum())  # into the wall, or (the lean) into the floor
        assert not ((d[:, 2] < 0) & (d[:, 2] >= -1e-3)).any()
        assert 16 < blocked < 48 and got["hits"][r] == blocked, (r, got["hits"][r], blocked)
    assert np.array_equal(got["occlusion"], ((64 - got["hits"]) / 64.0).astype(np.float32))
    assert (got["hits"][len(cv) // 2 + 6:] >= 0).all()
    # vertices without a usable normal are open and counted
    bad = cn.copy()
    bad[0], bad[1], bad[2] = 0.0, (0.0, 0.0, 1.01), (np.nan, 0.0, 1.0)
    bv = cv.copy()
    bv[3, 1] = np.inf
    got = rr.bake(bv, cf, bad, table, max_distance=4.0)
    assert got["no_normal"] == 4 and (got["hits"][:4] == 0).all() and (got["occlusion"][:4] == 1).all()
    # the rotation is a function of (seed, vertex)
    assert rr.rotation_of(3, np.arange(5), 4).tolist() == [int(dr.mix64(np.uint64((3 << 32) + i)) % 4) for i in range(5)]


def _mesh_dict(V, F, seed=0):
    rng = np.random.default_rng(seed)
    return dict(vertices=rng.normal(size=(V, 3)).astype(np.float32), faces=rng.integers(0, V, size=(F, 3)).astype(np.int32),
                normals=rng.normal(size=(V, 3)).astype(np.float32), albedo=rng.uniform(size=(V, 3)).astype(np.float32),
                roughness=rng.uniform(size=V).astype(np.float32), metallic=rng.uniform(size=V).astype(np.float32))


def test_ply_with_and_without_occlusion(tmp_path):
    import scene_io
    m = _mesh_dict(7, 5)
    args = [m[k] for k in ("vertices", "faces", "normals", "albedo", "roughness", "metallic")]
    plain, with_ao = str(tmp_path / "a.ply"), str(tmp_path / "b.ply")
    scene_io.save_mesh_ply(plain, *args)
    # the layout of a file without the channel, assembled here: the header; per vertex six floats, three colour bytes
    # (trunc(clamp(albedo 255 + 0.5, 0, 255))) and two floats; per face the byte 3 and three ints
    names = ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "roughness", "metallic")
    head = "ply\nformat binary_little_endian 1.0\nelement vertex 7\n"
    head += "".join("property %s %s\n" % ("uchar" if n in ("red", "green", "blue") else "float", n) for n in names)
    head += "element face 5\nproperty list uchar int vertex_indices\nend_header\n"
    colour = np.clip(m["albedo"] * np.float32(255.0) + np.float32(0.5), 0, 255).astype(np.uint8)
    body = io.BytesIO()
    for i in range(7):
        body.write(struct.pack("<6f3B2f", *m["vertices"][i], *m["normals"][i], *(int(c) for c in colour[i]), m["roughness"][i],
                               m["metallic"][i]))
    for tri in m["faces"]:
        body.write(struct.pack("<B3i", 3, *[int(x) for x in tri]))
    assert open(plain, "rb").read() == head.encode("ascii") + body.getvalue()
    scene_io.save_mesh_ply(plain + "2", *args, occlusion=None)
    assert open(plain + "2", "rb").read() == open(plain, "rb").read()
    back = scene_io.read_mesh_ply(plain)
    m["albedo"] = colour.astype(np.float32) / np.float32(255.0)  # what the colour bytes keep of it
    assert "occlusion" not in back and all(np.array_equal(back[k], m[k]) for k in m)
    ao = np.linspace(0, 1, 7).astype(np.float32)
    scene_io.save_mesh_ply(with_ao, *args, occlusion=ao)
    text = open(with_ao, "rb").read()
    assert b"property float metallic\nproperty float occlusion\nelement face" in text
    assert len(text) == len(open(plain, "rb").read()) + len(b"property float occlusion\n") + 4 * 7
    back = scene_io.read_mesh_ply(with_ao)
    assert np.array_equal(back["occlusion"], ao) and back["occlusion"].dtype == np.float32
    assert all(np.array_equal(back[k], m[k]) for k in m)
    with pytest.raises(ValueError):
        scene_io.save_mesh_ply(with_ao, *args, occlusion=ao[:3])
    # every other layout still raises
    other = text.replace(b"property float occlusion\n", b"property float occlusiom\n")
    open(with_ao, "wb").write(other)
    with pytest.raises(Exception):
        scene_io.read_mesh_ply(with_ao)
    assert os.path.exists(plain)
