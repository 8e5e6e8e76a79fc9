"""CPU: the host half of mesh texturing -- the atlas layout (mesh.atlas_layout, mesh.face_uvs) with the property it exists
for, the OBJ / MTL writer and reader (scene_io), and the restatement of the transfer (tests/mesh_atlas_ref.py) against a brute
force of its own.  The device half is tests/test_gpu_mesh_atlas.py."""
import math
import os

import numpy as np
import pytest

import mesh_atlas_ref as ar
import mesh_distance_ref as dr

LATTICE = 64  # a power of two: every lattice point of a UV triangle is exact in float64


def _lattice(n):
    a, b = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = a + b <= n
    return a[keep] / float(n), b[keep] / float(n)


def _taps(x, y):
    """The bilinear taps of the points (x, y) in texel INDEX coordinates (a texel centre is an integer): -> [(ix, iy, w)]."""
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    return [(x0.astype(np.int64) + dx, y0.astype(np.int64) + dy, (fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy))
            for dx in (0, 1) for dy in (0, 1)]


@pytest.mark.parametrize("B", [3, 4, 5, 8])
def test_every_bilinear_tap_of_a_uv_triangle_is_owned_by_its_face(B):
    own = ar.owner(B)
    assert own.shape == (B, B + 1) and int((own == 0).sum()) == int((own == 1).sum()) == B * (B + 1) // 2
    w1, w2 = _lattice(LATTICE)
    w0 = (1.0 - w1) - w2
    assert len(w1) == (LATTICE + 1) * (LATTICE + 2) // 2
    checked = 0
    for half in (0, 1):
        c = ar.corners(B)[half].astype(np.float64)
        x = (w0 * c[0, 0] + w1 * c[1, 0]) + w2 * c[2, 0]  # index coordinates: the centre of texel (i, j) is (i, j)
        y = (w0 * c[0, 1] + w1 * c[1, 1]) + w2 * c[2, 1]
        assert np.array_equal(x * LATTICE, np.round(x * LATTICE)) and np.array_equal(y * LATTICE, np.round(y * LATTICE))
        for ix, iy, w in _taps(x, y):
            hit = w > 0
            assert ((ix[hit] >= 0) & (ix[hit] <= B) & (iy[hit] >= 0) & (iy[hit] <= B - 1)).all(), (B, half)
            assert (own[iy[hit], ix[hit]] == half).all(), (B, half)
            checked += int(hit.sum())
        # the corners are texel centres of the half
        for i, j in ar.corners(B)[half]:
            assert own[j, i] == half
    assert checked > 2 * len(w1)
    # the reflection that defines the upper half
    j, i = np.meshgrid(np.arange(B), np.arange(B + 1), indexing="ij")
    assert np.array_equal(own[B - 1 - j, B - i], 1 - own)
    lo, up = ar.corners(B)
    assert np.array_equal(up, np.stack([B - lo[:, 0], B - 1 - lo[:, 1]], 1))


def test_ownership_in_the_image_with_margin_columns():
    """Six faces, B = 4 in a 16 x 4 image (both powers of two, so the float32 UVs are exact): three blocks and one margin
    column.  Every tap of every face's UV triangle is a texel whose texel_face is that face."""
    import mesh
    F, B = 5, 4
    lay = mesh.atlas_layout(F, B, width=16)
    assert lay == mesh.AtlasLayout(4, 16, 4, 3, 3) and ar.atlas_layout(F, B, 16) == lay._asdict()
    v = np.random.default_rng(0).uniform(-1, 1, (3 * F, 3)).astype(np.float32)
    faces = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    pts = ar.atlas_points(v, faces, lay._asdict())
    image = np.full(lay.width * lay.height, -2, np.int64)
    baked = pts["dest"] >= 0
    assert len(set(pts["dest"][baked].tolist())) == int(baked.sum()) == F * B * (B + 1) // 2
    image[pts["dest"][baked]] = pts["texel_face"][baked]
    assert (pts["texel_face"][~baked] == -1).all() and np.isnan(pts["points"][~baked]).all()
    image = image.reshape(lay.height, lay.width)
    assert (image[:, 15] == -2).all()
    uv = mesh.face_uvs(F, lay).numpy().astype(np.float64)
    w1, w2 = _lattice(LATTICE)
    w0 = (1.0 - w1) - w2
    for f in range(F):
        u = (w0 * uv[f, 0, 0] + w1 * uv[f, 1, 0]) + w2 * uv[f, 2, 0]
        t = (w0 * uv[f, 0, 1] + w1 * uv[f, 1, 1]) + w2 * uv[f, 2, 1]
        for ix, iy, w in _taps(u * lay.width - 0.5, (1.0 - t) * lay.height - 0.5):
            hit = w > 0
            assert (image[iy[hit], ix[hit]] == f).all(), f
    # the texel points: the corners' texels hold the corners, the weights sum to one
    P = v[faces].astype(np.float64)
    for f in range(F):
        for k in range(3):
            x, y = uv[f, k, 0] * lay.width - 0.5, (1.0 - uv[f, k, 1]) * lay.height - 0.5
            assert x == round(x) and y == round(y)
            q = np.nonzero(pts["dest"] == int(y) * lay.width + int(x))[0]
            assert len(q) == 1 and np.array_equal(pts["points"][q[0]], P[f, k].astype(np.float32))
    b = pts["bary"].astype(np.float64)
    assert (b >= 0).all() and ((1.0 - b[:, 0]) - b[:, 1] >= -1.0 / (B - 2) - 1e-7).all()


def test_atlas_layout_cases():
    import mesh
    for B in ar.BLOCKS + (5, 16):
        for F in (0, 1, 2, 3, 1945):
            lay = mesh.atlas_layout(F, B)
            assert lay._asdict() == ar.atlas_layout(F, B)
            W = lay.width
            assert W & (W - 1) == 0 and W >= B + 1 and lay.n_blocks == (F + 1) // 2 and lay.blocks_per_row == W // (B + 1)
            assert lay.height == math.ceil(lay.n_blocks / lay.blocks_per_row) * B and lay.height <= W
            assert W == B + 1 or W // 2 < B + 1 or ((W // 2) // (B + 1)) * ((W // 2) // B) < lay.n_blocks  # the smallest
            assert tuple(mesh.face_uvs(F, lay).shape) == (F, 3, 2)
    assert mesh.atlas_layout(0, 8).height == 0
    for F, B, W in ((1945, 8, 1000), (3, 3, 7), (7, 4, 14), (2, 8, 9)):  # widths that are no multiple of B + 1
        lay = mesh.atlas_layout(F, B, width=W)
        assert lay._asdict() == ar.atlas_layout(F, B, W) and lay.width == W and lay.blocks_per_row == W // (B + 1)
        uv = mesh.face_uvs(F, lay).numpy()
        assert np.array_equal(uv, ar.face_uvs(F, lay._asdict())) and uv.dtype == np.float32
        assert (uv > 0).all() and (uv < 1).all()
        x, y = uv[..., 0].astype(np.float64) * W - 0.5, (1.0 - uv[..., 1].astype(np.float64)) * lay.height - 0.5
        assert np.abs(x - np.round(x)).max() <= W * 2.0 ** -24 and np.abs(y - np.round(y)).max() <= lay.height * 2.0 ** -24
        assert (np.round(x) <= lay.blocks_per_row * (B + 1) - 1).all()
    for bad in (dict(F=4, block=2), dict(F=4, block=0), dict(F=4, block=8, width=8), dict(F=4, block=3, width=3)):
        with pytest.raises(ValueError):
            mesh.atlas_layout(**bad)
        with pytest.raises(ValueError):
            ar.atlas_layout(**bad)


def test_obj_round_trip(tmp_path):
    import mesh
    import mesh_simplify_ref as sr
    import scene_io
    d = sr.shared_cases()["cube"][0]
    v, f, n = d["vertices"], d["faces"], d["normals"]
    F = len(f)
    lay = mesh.atlas_layout(F, 4)
    uvs = mesh.face_uvs(F, lay)
    path = str(tmp_path / "sub" / "cube.obj")
    scene_io.save_mesh_obj(path, v, f, uvs, normals=n)
    got = scene_io.read_mesh_obj(path)
    assert len(got["vt"]) == 3 * F and np.array_equal(got["uv_faces"], np.arange(3 * F).reshape(F, 3))
    assert np.array_equal(got["faces"], f) and got["faces"].dtype == np.int32
    for a, b in ((got["vertices"], v), (got["normals"], n), (got["uvs"], uvs.numpy())):
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
    assert got["mtllib"] == "cube.mtl" and got["textures"] == scene_io.obj_texture_names(path)
    assert got["textures"]["albedo"] == "cube_albedo.png" and got["textures"]["orm"] == "cube_orm.png"
    mtl = open(str(tmp_path / "sub" / "cube.mtl")).read()
    for key, name in (("map_Kd", "cube_albedo.png"), ("map_Pr", "cube_roughness.png"), ("map_Pm", "cube_metallic.png"),
                      ("norm", "cube_normal.png")):
        assert "%s %s\n" % (key, name) in mtl
    text = open(path).read()
    assert text.startswith("mtllib cube.mtl\n") and "usemtl " in text and text.count("\nvt ") == 3 * F
    assert "f 1/1/1 " in text
    # without normals, and other file names
    plain = str(tmp_path / "plain.obj")
    scene_io.save_mesh_obj(plain, v, f, uvs, textures=dict(albedo="a.png"))
    got = scene_io.read_mesh_obj(plain)
    assert got["normals"] is None and got["textures"]["albedo"] == "a.png" and np.array_equal(got["faces"], f)
    assert "f 1/1 " in open(plain).read()
    with pytest.raises(ValueError):
        scene_io.save_mesh_obj(plain, v, f, uvs[:-1])
    with pytest.raises(ValueError):
        scene_io.save_mesh_obj(plain, v, f + len(v), uvs)
    with open(plain, "a") as fh:
        fh.write("g group\n")
    with pytest.raises(ValueError):
        scene_io.read_mesh_obj(plain)
    # an empty mesh
    empty = str(tmp_path / "empty.obj")
    scene_io.save_mesh_obj(empty, v[:0], f[:0], uvs[:0])
    got = scene_io.read_mesh_obj(empty)
    assert got["vertices"].shape == (0, 3) and got["faces"].shape == (0, 3) and got["uvs"].shape == (0, 3, 2)
    assert os.path.exists(str(tmp_path / "empty.mtl"))


@pytest.mark.parametrize("name", sorted(ar.TRIANGLES))
def test_restated_weights_minimise_the_distance(name):
    """The restated closest point against the minimum over a barycentric lattice of n = 256 steps.  A point of the triangle
    is within L / n of a lattice point (L the longest edge), so the lattice minimum d_n satisfies
    d <= d_n <= d + L / n for the true distance d; the restatement must sit in that band (with 2^-40 L for rounding),
    its weights must be a convex combination, and its d^2 must be mesh_distance_ref.triangle_d2's bit for bit."""
    P, idx = ar.TRIANGLES[name]
    P = np.asarray(P, np.float32).astype(np.float64)
    idx = np.asarray(idx, np.int64)
    q = ar.voronoi_queries(P).astype(np.float64)
    N = len(q)
    w, d2 = ar.triangle_weights(q, np.broadcast_to(P, (N, 3, 3)), np.broadcast_to(idx, (N, 3)))
    assert np.array_equal(d2, dr.triangle_d2(q, P[None], idx[None]))
    assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1.0).max() <= 2.0 ** -50
    regions = {tuple(r) for r in (w > 0).tolist()}
    assert len(regions) == 7, regions  # three vertices, three edges, the interior
    c = np.einsum("nk,kc->nc", w, P)
    d = np.sqrt(((q - c) ** 2).sum(axis=1))
    assert np.abs(d * d - d2).max() <= 2.0 ** -40 * max(1.0, float(d2.max()))
    n = 256
    a, b = _lattice(n)
    lattice = (1.0 - a - b)[:, None] * P[0] + a[:, None] * P[1] + b[:, None] * P[2]
    dn = np.sqrt(((q[:, None, :] - lattice[None]) ** 2).sum(axis=2).min(axis=1))
    L = math.sqrt(max(float(((P[i] - P[j]) ** 2).sum()) for i, j in ((0, 1), (1, 2), (2, 0))))
    print("%s: lattice minimum above the restatement by at most %.3e (allowed L / n = %.3e), below by %.3e"
          % (name, (dn - d).max(), L / n, (d - dn).max()))
    assert (d <= dn + 2.0 ** -40 * L).all() and (dn <= d + L / n).all()


def test_restated_transfer_interpolates_and_skips():
    P, idx = ar.TRIANGLES["tilted"]
    v = np.zeros((8, 3), np.float32)
    v[idx] = np.asarray(P, np.float32)
    faces = np.array([idx, [0, 1, 2]], np.int32)
    values = np.random.default_rng(1).uniform(-2, 2, (8, 5)).astype(np.float32)
    q = ar.voronoi_queries(v[idx].astype(np.float64))
    face = np.zeros(len(q), np.int64)
    face[::5] = -1
    q[3] = np.nan
    t = ar.transfer(q, face, v, faces, values)
    skipped = (face < 0) | ~np.isfinite(q).all(axis=1)
    assert t["skipped"] == int(skipped.sum()) and t["transferred"] == len(q) - t["skipped"]
    assert (t["out"][skipped] == 0).all() and (t["bary"][skipped] == 0).all() and np.array_equal(t["done"], ~skipped)
    w = t["w"][~skipped]
    want = np.einsum("nk,kc->nc", w, values[idx].astype(np.float64))
    assert np.abs(t["out"][~skipped] - want).max() <= 2.0 ** -22 * 2.0
    # with destinations: planes, coverage
    dest = np.where(skipped, -1, np.arange(len(q))[::-1] + 7)
    s = ar.transfer(q, face, v, faces, values, dest=dest, plane=len(q) + 9)
    assert s["out"].shape == (5, len(q) + 9) and int(s["coverage"].sum()) == t["transferred"]
    assert np.array_equal(s["out"][:, dest[~skipped]].T, t["out"][~skipped]) and (s["out"][:, s["coverage"] == 0] == 0).all()
