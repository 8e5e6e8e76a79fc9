"""CPU: the numpy restatement of the mesh rasterizer (tests/mesh_raster_ref.py) against the analytic sphere, the owner rule
on edges through pixel centres, the PLY -> mesh round trip and render_mesh.py's argument parsing.

The closed sphere mesh (radius 0.6, 1710 vertices, 3416 faces) seen from six orbit cameras at 40 x 56: a ray through a
closed surface crosses it twice, so every covered pixel centre is covered by exactly two triangles (front and back) --
the count of an exact, hole-free, overlap-free coverage rule.  Against the analytic sphere the covered set may differ at
silhouette pixels only (<= 1 % of the image) and the depth by at most half a voxel (the vertices lie within h / 4 of the
sphere, tests/mesh_ref.check_closed_sphere, and a chord sags below its arc by less than that again)."""
import functools

import numpy as np

import mesh_raster_ref as rr


@functools.lru_cache(maxsize=None)
def _sphere():
    return rr.sphere_mesh()


@functools.lru_cache(maxsize=None)
def _renders():
    m, _ = _sphere()
    return [rr.render(m, c, counts=True) for c in rr.sphere_cameras()]


def test_sphere_mesh_is_the_one_the_tests_expect():
    import mesh_ref
    m, h = _sphere()
    assert m["vertices"].shape == (1710, 3) and m["faces"].shape == (3416, 3)
    mesh_ref.check_closed_sphere(m["vertices"], m["faces"], h)


def test_every_covered_pixel_is_covered_twice():
    for v, r in enumerate(_renders()):
        assert set(np.unique(r["cover"]).tolist()) <= {0, 2}, (v, np.unique(r["cover"], return_counts=True))
        assert (r["cover"] == 2).sum() > 100, v
        assert not r["flags"].any()
        assert np.array_equal(r["tri_id"] >= 0, r["cover"] == 2)


def test_coverage_and_depth_against_the_analytic_sphere():
    _, h = _sphere()
    for v, (cam, r) in enumerate(zip(rr.sphere_cameras(), _renders())):
        hit, depth = rr.analytic_sphere(cam)
        cov = r["tri_id"] >= 0
        differ = int((cov != hit).sum())
        both = cov & hit
        err = float(np.abs(r["depth"][0][both].astype(np.float64) - depth[both]).max()) / h
        print("view %d: covered %d, differ from the analytic sphere at %d of %d pixels, depth error %.3f h" % (
            v, int(cov.sum()), differ, cov.size, err))
        assert differ <= 0.01 * cov.size, (v, differ)
        assert err <= 0.5, (v, err)


def test_planes_of_the_restatement():
    """Background as the blend kernel leaves it, attributes inside the hull of the vertex attributes, the front triangle wins."""
    m, _ = _sphere()
    cam, r = rr.sphere_cameras()[0], _renders()[0]
    cov = r["tri_id"] >= 0
    bg = ~cov
    assert (r["opacity"][0][bg] == 0).all() and (r["depth"][0][bg] == 0).all() and (r["roughness"][0][bg] == 1).all()
    assert (r["albedo"][:, bg] == 0).all() and (r["normal"][:, bg] == 0).all() and np.isnan(r["normal_view"][:, bg]).all()
    assert (r["opacity"][0][cov] == 1).all() and np.isfinite(r["normal_view"][:, cov]).all()
    assert np.allclose(np.linalg.norm(r["normal_view"][:, cov], axis=0), 1.0, atol=1e-5)
    for k in ("albedo", "roughness", "metallic"):
        assert r[k][:, cov].min() >= m[k].min() - 1e-5 and r[k][:, cov].max() <= m[k].max() + 1e-5, k
    assert np.abs(r["pos"][2][cov] - r["depth"][0][cov]).max() <= 1e-5
    # the winner faces the camera: the orientation test of the screen integers (y points down, so outward-facing
    # counter-clockwise triangles have a negative doubled area on screen)
    s = r["screen"].astype(np.int64)
    f = m["faces"][np.unique(r["tri_id"][cov])]
    A = (s[f[:, 1], 0] - s[f[:, 0], 0]) * (s[f[:, 2], 1] - s[f[:, 0], 1]) - (s[f[:, 1], 1] - s[f[:, 0], 1]) * (
        s[f[:, 2], 0] - s[f[:, 0], 0])
    assert (A < 0).all() or (A > 0).all()


def test_owner_rule_on_edges_through_pixel_centres():
    screen, faces, interior, (W, H) = rr.owner_rule_case()
    V = len(screen)
    view_pos = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (V, 1))
    vis, cover = rr.raster(faces, view_pos, screen, np.zeros(V, np.uint8), W, H, counts=True)
    assert cover.max() == 1, "a pixel centre on a shared edge has two owners"
    assert (cover[interior] == 1).all()
    # the quad: of its closed square [4,14]^2 the rule keeps a half-open one (one horizontal and one vertical border)
    q = cover[4:15, 4:15]
    assert q.sum() == 100 and q[1:-1, 1:-1].all()
    # the fan: a closed octagon has no gap, and its centre vertex -- on all eight spokes -- has exactly one owner
    assert cover[30, 22] == 1 and cover[26:35, 19:26].all()
    tri = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert set(np.unique(tri[4:15, 4:15][q == 1]).tolist()) == {0, 1}
    assert len(np.unique(tri[cover == 1])) == 10  # every triangle owns something


def test_ties_and_drops_in_the_restatement():
    W, H = 16, 12
    S = rr.SUB
    screen = np.array([(2 * S, 2 * S), (12 * S, 3 * S), (5 * S, 10 * S), (0, 0)], np.int32)
    view_pos = np.array([[0, 0, 1.0], [0, 0, 2.0], [0, 0, 1.5], [0, 0, 0.1]], np.float32)
    flags = np.array([0, 0, 0, 1], np.uint8)
    one = rr.raster(np.array([[0, 1, 2], [0, 1, 2]]), view_pos, screen, flags, W, H)
    tri = (one & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (one != rr.EMPTY).sum() > 20 and (tri[one != rr.EMPTY] == 0).all()  # identical triangles: the lower index wins
    for faces in ([[0, 1, 1]], [[0, 1, 4]], [[0, -1, 2]], [[0, 1, 3]], np.zeros((0, 3), np.int32)):
        assert (rr.raster(np.array(faces, np.int32).reshape(-1, 3), view_pos, screen, flags, W, H) == rr.EMPTY).all(), faces


def test_ply_round_trip_to_mesh_arrays(tmp_path):
    import mesh_render
    import scene_io
    m, _ = _sphere()
    path = str(tmp_path / "sphere.ply")
    scene_io.save_mesh_ply(path, *(m[k] for k in mesh_render.MESH_KEYS))
    a = mesh_render.mesh_arrays(path)
    assert a["faces"].dtype == np.int32 and all(a[k].dtype == np.float32 for k in mesh_render.MESH_KEYS if k != "faces")
    assert np.array_equal(a["vertices"], m["vertices"]) and np.array_equal(a["faces"], m["faces"])
    assert np.array_equal(a["normals"], m["normals"]) and np.array_equal(a["roughness"], m["roughness"])
    assert np.abs(a["albedo"] - np.clip(m["albedo"], 0, 1)).max() <= 1.0 / 255.0
    b = mesh_render.mesh_arrays(tuple(m[k] for k in mesh_render.MESH_KEYS))  # mesh.Mesh's field order
    assert all(np.array_equal(b[k], m[k]) for k in mesh_render.MESH_KEYS)
    cam = rr.sphere_cameras()[1]
    assert np.array_equal(rr.render(a, cam)["tri_id"], _renders()[1]["tri_id"])  # geometry survives the file exactly
    import pytest
    with pytest.raises(ValueError, match="rows"):
        mesh_render.mesh_arrays(dict(m, roughness=m["roughness"][:-1]))
    with pytest.raises(ValueError, match="lacks"):
        mesh_render.mesh_arrays({k: m[k] for k in ("vertices", "faces")})


def test_render_mesh_arguments():
    import pytest
    import render_mesh
    a = render_mesh.parse_args(["-m", "out", "--mesh", "mesh.ply"])
    assert (a.model_path, a.mesh, a.checkpoint, a.hdri, a.rotations, a.compare, a.split) == (
        "out", "mesh.ply", None, None, 0, False, "test")
    assert (a.radius, a.step, a.start) == (0.8, 16, 8) and a.metallic is False
    a = render_mesh.parse_args(["-m", "o", "--mesh", "m.ply", "--checkpoint", "o/chkpnt7.pth", "--hdri", "a.hdr", "b.hdr",
                                "--rotations", "4", "--compare", "--split", "train"])
    assert a.hdri == ["a.hdr", "b.hdr"] and a.rotations == 4 and a.compare and a.split == "train"
    assert render_mesh.light_names(["x/a.hdr", "b.npy"], 0) == ["a", "b"]
    assert render_mesh.light_names(["a.hdr"], 2) == ["a_rot000", "a_rot001"] and render_mesh.light_names(None, 0) == ["trained"]
    with pytest.raises(SystemExit):
        render_mesh.parse_args(["-m", "out"])  # --mesh is required
    with pytest.raises(ValueError, match="--compare"):
        render_mesh.render_mesh(["-m", "out", "--mesh", "m.ply", "--hdri", "a.hdr", "--compare"])
    with pytest.raises(ValueError, match="--checkpoint or --hdri"):
        render_mesh.render_mesh(["-m", "out", "--mesh", "m.ply"])
    p = render_mesh.view_paths("out", "test", "r_3", ["a", "b"])
    assert p["depth"].endswith("out/mesh_test/r_3_depth.png") and p["relit"] == ["out/mesh_test/r_3_a.png", "out/mesh_test/r_3_b.png"]
