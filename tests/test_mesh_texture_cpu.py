"""CPU: the numpy restatement of the textured resolve (tests/mesh_texture_ref.py) on cases with a known answer, and the
loader of a textured mesh (mesh_render.load_textured_mesh).  mesh_render.py binds the shared library when it is imported,
which needs no GPU (tests/test_mesh_render_cpu.py imports it the same way), so the loader test runs here and is not
marked gpu."""
import numpy as np
import pytest

import mesh_raster_ref as rr
import mesh_texture_ref as tr


@pytest.mark.parametrize("back", [False, True])
def test_a_texture_linear_in_uv_is_reproduced_at_pixel_centres(back):
    """The quad of mesh_texture_ref.quad_case: t = u + 3 v on an 8 x 8 texture, UVs on texel centres, so every lookup falls
    between texel centres, where bilinear interpolation is exact for a function linear in the texel coordinates.  What is
    left is float32; mesh_texture_ref derives 138 units of 2^-24 beside QUAD_BOUND, and 2^-16 is asserted.  Both
    triangles -- one of them takes the set-up's A < 0 path, the other one from behind -- are covered and checked at every
    pixel they own."""
    mesh, uvs, planes, cam = tr.quad_case(back=back)
    o = tr.render_textured(mesh, uvs, planes, planes, None, cam)
    want = tr.quad_expected(o["pos"], cam)
    for t in (0, 1):
        own = o["tri_id"] == t
        assert own.sum() > 300, t
        err = np.abs(o["albedo"][0] - want)[own].max()
        print("back %s, triangle %d: %d pixels, largest error %.3g = %.1f units of 2^-24" % (back, t, own.sum(), err, err / 2.0 ** -24))
        assert err <= tr.QUAD_BOUND
        assert np.abs(o["roughness"][0] - 0.25 * want)[own].max() <= tr.QUAD_BOUND  # the ORM planes: t / 4, 1 - t / 8
        assert np.abs(o["metallic"][0] - (1.0 - 0.125 * want))[own].max() <= tr.QUAD_BOUND
        assert np.abs(o["occlusion"][0] - want)[own].max() <= tr.QUAD_BOUND
    # the flipped triangle is the second from the front and the first from behind
    view_pos, screen, flags = o["view_pos"], o["screen"], o["flags"]
    flipped = [tuple(rr._setup(t, mesh["faces"], 4, screen, flags, view_pos)[0]) != tuple(mesh["faces"][t]) for t in (0, 1)]
    assert flipped == ([True, False] if back else [False, True])
    # the corner UVs swapped WITHOUT the vertices: the flipped triangle is wrong by texels
    wrong = uvs.copy()
    t = flipped.index(True)
    wrong[t, [1, 2]] = wrong[t, [2, 1]]
    bad = tr.render_textured(mesh, wrong, planes, planes, None, cam)
    assert np.abs(bad["albedo"][0] - want)[o["tri_id"] == t].max() > 0.1
    # background
    bg = o["tri_id"] < 0
    assert bg.sum() > 100 and (o["occlusion"][0][bg] == 1).all() and (o["roughness"][0][bg] == 1).all()
    assert (o["albedo"][:, bg] == 0).all() and np.isnan(o["normal_view"][:, bg]).all()


def test_listing_a_face_with_the_opposite_winding_changes_no_value():
    """The same two triangles with the second listed the other way round (and its corner UVs with it): the set-up brings both
    listings to one vertex order, so every plane has the same bits."""
    mesh, uvs, planes, cam = tr.quad_case()
    rng = np.random.default_rng(1)
    tex = [rng.uniform(0, 1, (3, 7, 5)).astype(np.float32) for _ in range(2)] + [rng.uniform(-1, 1, (3, 7, 5)).astype(np.float32)]
    a = tr.render_textured(mesh, uvs, *tex, cam)
    other = dict(mesh, faces=mesh["faces"].copy())
    other["faces"][1] = other["faces"][1][[0, 2, 1]]
    uv2 = uvs.copy()
    uv2[1] = uv2[1][[0, 2, 1]]
    b = tr.render_textured(other, uv2, *tex, cam)
    assert (a["tri_id"] == 1).sum() > 300
    for k in ("tri_id", "albedo", "roughness", "metallic", "occlusion", "normal", "depth", "pos"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["normal_view"], b["normal_view"], equal_nan=True)


def test_nan_and_huge_uvs_are_clamped_to_minus_one_and_the_size():
    """The definition, spelled out: a coordinate is brought into [-1, n] before anything is converted, and a NaN becomes
    -1.  At -1 both taps are texel 0 (weight 0 on the second); at n both are texel n - 1."""
    a, b, f = tr.tex_axis(np.array([np.nan, -1e30, 1e30, -0.25, 3.0, 4.75, -np.inf, np.inf], np.float32), 5)
    assert a.tolist() == [0, 0, 4, 0, 3, 4, 0, 4] and b.tolist() == [0, 0, 4, 0, 4, 4, 0, 4]
    assert f.tolist() == [0.0, 0.0, 0.0, 0.75, 0.0, 0.75, 0.0, 0.0]
    planes = np.random.default_rng(2).uniform(0, 1, (3, 4, 5)).astype(np.float32)
    u = np.array([np.nan, 1e30, -1e30, np.nan, 0.5], np.float32)
    v = np.array([np.nan, 1e30, -1e30, 0.5, np.nan], np.float32)
    got = tr.bilinear(planes, u, v)
    assert np.isfinite(got).all()
    # u: NaN -> x = -1 -> column 0; 1e30 -> column 4; -1e30 -> column 0.  v: NaN -> y = -1 -> row 0 (the top); v = 1e30 ->
    # y = -1e30 -> row 0; v = -1e30 -> y = 4 -> row 3
    assert np.array_equal(got[:, 0], planes[:, 0, 0]) and np.array_equal(got[:, 1], planes[:, 0, 4])
    assert np.array_equal(got[:, 2], planes[:, 3, 0])
    # u = 0.5 of five texels: x = 2, exactly texel 2; v = 0.5 of four rows: y = 1.5, half of rows 1 and 2
    half = lambda c: (np.float32(0.5) * planes[:, 1, c] + np.float32(0.5) * planes[:, 2, c]).astype(np.float32)  # noqa: E731
    assert np.array_equal(got[:, 3], half(0)) and np.array_equal(got[:, 4], planes[:, 0, 2])
    # through the whole resolve: a face with NaN UVs and one with +-1e30, on a 1 x 1 texture too
    mesh, uvs, _, cam = tr.quad_case()
    hostile = uvs.copy()
    hostile[0] = np.nan
    hostile[1] = np.array([(1e30, -1e30), (-1e30, 1e30), (1e30, 1e30)], np.float32)
    for shape in ((3, 4, 5), (3, 1, 1)):
        tex = np.random.default_rng(3).uniform(0.25, 1, shape).astype(np.float32)
        o = tr.render_textured(mesh, hostile, tex, tex, tex, cam)
        hit = o["tri_id"] >= 0
        assert hit.sum() > 600
        for k in ("albedo", "normal"):
            assert np.isfinite(o[k]).all(), k
        assert (o["albedo"][:, o["tri_id"] == 0] == tex[:, 0, 0][:, None]).all()  # NaN, NaN -> the top left texel
        if shape[1:] == (1, 1):
            assert (o["albedo"][:, hit] == tex[:, 0, 0][:, None]).all()


def test_load_textured_mesh_reads_back_what_was_written(tmp_path):
    from PIL import Image

    import mesh_render
    import scene_io
    rng = np.random.default_rng(4)
    Wt, Ht = 5, 4
    images = {k: rng.integers(0, 256, (Ht, Wt, 3), dtype=np.uint8) for k in ("albedo", "orm", "normal")}
    images["normal"][0, 0] = (0, 255, 128)
    path = str(tmp_path / "m" / "quad.obj")
    mesh, uvs, _, _ = tr.quad_case()
    scene_io.save_mesh_obj(path, mesh["vertices"], mesh["faces"], uvs, normals=mesh["normals"])
    names = scene_io.obj_texture_names(path)
    for k, img in images.items():
        Image.fromarray(img, "RGB").save(str(tmp_path / "m" / names[k]))
    got = mesh_render.load_textured_mesh(path)
    assert sorted(got) == ["albedo", "mesh", "normal", "orm", "uvs"]
    planes = {k: img.transpose(2, 0, 1).astype(np.float32) for k, img in images.items()}
    for k in ("albedo", "orm"):
        assert got[k].dtype == np.float32 and got[k].shape == (3, Ht, Wt) and got[k].flags["C_CONTIGUOUS"]
        assert np.array_equal(got[k], planes[k] / np.float32(255.0)), k
    assert got["normal"].dtype == np.float32
    assert np.array_equal(got["normal"], np.float32(2.0) * planes["normal"] / np.float32(255.0) - np.float32(1.0))
    assert got["normal"][:, 0, 0].tolist() == [-1.0, 1.0, np.float32(256.0) / np.float32(255.0) - np.float32(1.0)]
    assert np.array_equal(got["uvs"], uvs) and got["uvs"].dtype == np.float32
    assert np.array_equal(got["mesh"]["vertices"], mesh["vertices"]) and np.array_equal(got["mesh"]["faces"], mesh["faces"])
    assert np.array_equal(got["mesh"]["normals"], mesh["normals"])
    # without vn statements the normals are None: the normal texture carries them
    scene_io.save_mesh_obj(path, mesh["vertices"], mesh["faces"], uvs)
    assert mesh_render.load_textured_mesh(path)["mesh"]["normals"] is None
    # images of different sizes are refused
    Image.fromarray(images["orm"][:3], "RGB").save(str(tmp_path / "m" / names["orm"]))
    with pytest.raises(ValueError, match="differ in size"):
        mesh_render.load_textured_mesh(path)
