"""GPU: the textured resolve (gigs_mesh_resolve_textured through mesh_render.TexturedMeshRasterizer) against its numpy
restatement (tests/mesh_texture_ref.py) and, independently of it, against the per-vertex rasterizer on meshes baked onto
themselves; the occlusion modes of mesh_planes, the mesh relighters over a textured rasterizer, and render_mesh.py on an
OBJ.

The restatement runs on the GPU's own projected arrays and key plane, so coverage is not in question here
(tests/test_gpu_mesh_render.py); tri_id, opacity, depth and pos are compared with gigs_mesh_resolve's as bit patterns."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_raster_ref as rr
import mesh_texture_ref as tr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
PW, PH = rr.PW, rr.PH
ATLAS_WIDTH = 64


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cam_t(cam):
    return {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}


def _host(planes):
    return {k: v.cpu().numpy() for k, v in planes.items()}


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)


@functools.lru_cache(maxsize=None)
def _mesh():
    return rr.sphere_mesh()[0]


@functools.lru_cache(maxsize=None)
def _cams():
    return rr.sphere_cameras(seventh=True)


@functools.lru_cache(maxsize=None)
def _plain():
    import mesh_render
    return mesh_render.MeshRasterizer(_mesh(), device=DEV)


@functools.lru_cache(maxsize=None)
def _random_atlas(block):
    """(uvs, albedo, orm in [0, 1], normal in [-1, 1]) on atlas_layout(F, block, 64), random texel by texel.  Read-only."""
    import mesh
    F = len(_mesh()["faces"])
    lay = mesh.atlas_layout(F, block, ATLAS_WIDTH)
    rng = np.random.default_rng(20 + block)
    shape = (3, lay.height, lay.width)
    return (mesh.face_uvs(F, lay).numpy(), rng.uniform(0, 1, shape).astype(np.float32), rng.uniform(0, 1, shape).astype(np.float32),
            rng.uniform(-1, 1, shape).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _textured(block):
    import mesh_render
    uvs, albedo, orm, normal = _random_atlas(block)
    return mesh_render.TexturedMeshRasterizer(_mesh(), uvs, albedo, orm, normal, device=DEV)


def _adjacent_difference(planes):
    return max(float(np.abs(np.diff(planes, axis=1)).max()) if planes.shape[1] > 1 else 0.0,
               float(np.abs(np.diff(planes, axis=2)).max()) if planes.shape[2] > 1 else 0.0)


def _bound(planes):
    """1e-5 (the mesh tests' bound) plus four ulps of a texel coordinate times the steepest step between adjacent texels."""
    return 1e-5 + 4 * 2.0 ** -23 * max(planes.shape[1:]) * _adjacent_difference(planes)


# ---- 1: against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [3, 8])
@pytest.mark.parametrize("view", range(7))
def test_textured_resolve_matches_the_restatement(view, block):
    m, rast, cam = _mesh(), _textured(block), _cams()[view]
    uvs, albedo, orm, normal = _random_atlas(block)
    assert albedo.shape[2] == ATLAS_WIDTH
    got = _host(rast(cam_t(cam)))
    view_pos, screen, flags = rast._view_pos.cpu().numpy(), rast._screen.cpu().numpy(), rast._flags.cpu().numpy()
    vis_t = rast._vis.clone()
    vis = vis_t.cpu().numpy().view(np.uint64)
    # gigs_mesh_resolve on the same key plane: the planes no texture touches have its bits
    plain = _plain()
    plain.project(cam_t(cam))
    base = _host(plain.resolve(cam_t(cam), vis=vis_t))
    for k in ("tri_id", "opacity", "depth", "pos"):
        assert np.array_equal(_bits(got[k]), _bits(base[k])), k
    ref = tr.resolve_textured(vis, m["faces"], view_pos, screen, flags, uvs, albedo, orm, normal, None, cam["viewmatrix"])
    assert np.array_equal(got["tri_id"], ref["tri_id"])
    covered = int((ref["tri_id"] >= 0).sum())
    assert covered == PW * PH if view == 6 else 300 < covered < PW * PH
    for k, planes in (("albedo", albedo), ("occlusion", orm), ("roughness", orm), ("metallic", orm), ("normal", normal)):
        err = float(np.abs(got[k] - ref[k]).max())
        print("view %d block %d %s: %.4f bit-equal, largest error %.3g (bound %.3g)"
              % (view, block, k, float((_bits(got[k]) == _bits(ref[k])).mean()), err, _bound(planes)))
        assert err <= _bound(planes), k
    for k in ("opacity", "depth", "pos"):
        assert np.abs(got[k] - ref[k]).max() <= 1e-5, k
    assert np.allclose(got["normal_view"], ref["normal_view"], rtol=0, atol=1e-5, equal_nan=True)
    assert np.array_equal(np.isnan(got["normal_view"]).any(0), ref["tri_id"] < 0)
    assert (got["occlusion"][0][ref["tri_id"] < 0] == 1.0).all()


# ---- 2: winding --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("back", [False, True])
def test_corner_uvs_follow_the_vertices_when_the_set_up_swaps_them(back):
    """mesh_texture_ref.quad_case: two triangles seen head-on, one of them listed clockwise (the A < 0 path; from behind it
    is the other), t = u + 3 v with UVs on texel centres.  Both reproduce the function within QUAD_BOUND (derived beside
    it) at every pixel they cover; with the corner UVs of the flipped triangle swapped and its vertices not, it is off by
    texels."""
    import mesh_render
    mesh, uvs, planes, cam = tr.quad_case(back=back)
    with mesh_render.TexturedMeshRasterizer(mesh, uvs, planes, planes, None, device=DEV) as rast:
        o = _host(rast(cam_t(cam)))
        flipped = 0 if back else 1
        s = rast._screen.cpu().numpy().astype(np.int64)
        for t in (0, 1):
            i0, i1, i2 = mesh["faces"][t]
            A = (s[i1, 0] - s[i0, 0]) * (s[i2, 1] - s[i0, 1]) - (s[i1, 1] - s[i0, 1]) * (s[i2, 0] - s[i0, 0])
            assert (A < 0) == (t == flipped)
    want = tr.quad_expected(o["pos"], cam)
    for t in (0, 1):
        own = o["tri_id"] == t
        assert own.sum() > 300
        err = float(np.abs(o["albedo"][0] - want)[own].max())
        print("back %s triangle %d: %d pixels, largest error %.3g = %.1f units of 2^-24" % (back, t, own.sum(), err, err * 2.0 ** 24))
        assert err <= tr.QUAD_BOUND
        assert np.abs(o["occlusion"][0] - want)[own].max() <= tr.QUAD_BOUND
        assert np.abs(o["roughness"][0] - 0.25 * want)[own].max() <= tr.QUAD_BOUND
        assert np.abs(o["metallic"][0] - (1.0 - 0.125 * want))[own].max() <= tr.QUAD_BOUND
    wrong = uvs.copy()
    wrong[flipped, [1, 2]] = wrong[flipped, [2, 1]]
    with mesh_render.TexturedMeshRasterizer(mesh, wrong, planes, planes, None, device=DEV) as rast:
        bad = _host(rast(cam_t(cam)))
    assert np.abs(bad["albedo"][0] - want)[o["tri_id"] == flipped].max() > 0.1
    assert np.abs(bad["albedo"][0] - want)[o["tri_id"] == 1 - flipped].max() <= tr.QUAD_BOUND


# ---- 3: independent of the restatement -----------------------------------------------------------------------------------------
def _device_mesh(d):
    import mesh
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(d[k], dt)).to(DEV)  # noqa: E731
    return mesh.Mesh(t("vertices", np.float32).reshape(-1, 3), t("faces", np.int32).reshape(-1, 3), t("normals", np.float32),
                     t("albedo", np.float32), t("roughness", np.float32), t("metallic", np.float32))


def _linear_attributes(d, seed=4):
    """Attributes a . x + b, a, b > 0, on the mesh dict's vertices; occlusion gets the roughness row."""
    rng = np.random.default_rng(seed)
    A, b = rng.uniform(0.25, 1.0, (8, 3)), rng.uniform(0.5, 1.0, 8)
    lin = (d["vertices"].astype(np.float64) @ A.T + b).astype(np.float32)
    return dict(d, albedo=lin[:, 0:3], roughness=lin[:, 3].copy(), metallic=lin[:, 4].copy(), normals=lin[:, 5:8])


def _baked_onto_itself(d, block):
    import mesh
    import mesh_render
    m = _device_mesh(d)
    atlas, report = mesh.bake_atlas(m, m, block=block, width=ATLAS_WIDTH, occlusion=m.roughness)
    assert report["baked"] == len(d["faces"]) * block * (block + 1) // 2 and atlas.layout.width == ATLAS_WIDTH
    return m, atlas, mesh_render.TexturedMeshRasterizer.from_atlas(m, atlas), mesh_render.MeshRasterizer(m, device=DEV)


def _compare_with_vertex_render(textured, plain, cams, keep):
    """-> (pixels compared, the largest difference over the nine channels, the largest value) over `cams`; keep(t, cam) ->
    [H,W] bool: the pixels whose lookups the bilinear-reproduction argument covers."""
    n, worst, M = 0, 0.0, 0.0
    for cam in cams:
        t, p = textured(cam_t(cam)), plain(cam_t(cam))
        assert torch.equal(t["tri_id"], p["tri_id"]) and torch.equal(t["depth"], p["depth"])
        ok = keep(t, cam) & (t["tri_id"] >= 0)
        n += int(ok.sum())
        for a, b in (("albedo", "albedo"), ("roughness", "roughness"), ("metallic", "metallic"), ("occlusion", "roughness"),
                     ("normal", "normal")):
            worst = max(worst, float((t[a] - p[b]).abs()[:, ok].max()))
            M = max(M, float(p[b].abs()[:, ok].max()))
    return n, worst, M


@pytest.mark.parametrize("block", [4, 8])
def test_a_plane_baked_onto_itself_renders_like_its_vertices(block):
    """Independent of the restatement: the jittered plane with attributes linear in the position, baked onto itself.  A
    linear function survives the interpolation on the source face, the extrapolated gutter points of a face whose
    neighbours lie in the same plane, and the bilinear lookup (the layout's property: every tap of non-zero weight is a
    texel of the face's own half), so the textured render equals the per-vertex render, which interpolates the same table
    perspective-correctly.  Bound: tests/test_gpu_mesh_atlas.py's derived 2^-20 max|value| for the bake and the lookup plus
    the render tests' 1e-5 for the two interpolations.  Faces with a vertex on the border are left out, as there: their
    gutter points leave the mesh.  Every other covered pixel of three oblique views is compared, all nine channels.
    Measured on an MI355X (profiles/r21/mesh_texture_tests_figures.txt): 0.087 of the bound at block 4, 0.058 at block 8."""
    import mesh_simplify_ref as sr
    import scenes
    d = _linear_attributes(dict(sr.shared_cases()["plane"][0]))
    m, atlas, textured, plain = _baked_onto_itself(d, block)
    n = int(round(len(d["vertices"]) ** 0.5))
    i, j = np.arange(n * n) // n, np.arange(n * n) % n
    inner_vertex = (i > 0) & (i < n - 1) & (j > 0) & (j < n - 1)
    inner = tt(inner_vertex[d["faces"]].all(axis=1))
    cams = [scenes.look_at_camera(eye, (0.5, 0.5, 0.25), PW, PH, rr.FOVX, up=(0.0, 1.0, 0.0))
            for eye in ((1.1, 0.2, 1.6), (-0.1, 1.0, 1.5), (0.6, 0.4, -1.2))]  # the last from below: every face flips
    count, worst, M = _compare_with_vertex_render(textured, plain, cams, lambda t, cam: inner[t["tri_id"].clamp(min=0).long()])
    bound = 2.0 ** -20 * M + 1e-5
    print("plane, block %d: %d pixels on inner faces, largest difference %.3e = %.3f of the bound %.3e" % (block, count, worst,
                                                                                                         worst / bound, bound))
    assert count > 1500 and worst <= bound


@pytest.mark.parametrize("block", [4, 8])
def test_the_blob_baked_onto_itself_renders_like_its_vertices(block):
    """The same on a curved mesh (the blob, 1944 faces), where the argument covers fewer lookups: a gutter texel stands for
    the extrapolated point of its face's plane, which on a curved surface is not on the mesh, so the bake stores the value
    at the closest point of the neighbouring face instead and a lookup that gives a gutter texel weight is off by the
    gradient times that distance.  Those lookups are left out and nothing else is: a second render through a probe atlas
    whose albedo holds the texel's own column and row gives every pixel its texel coordinates, and a pixel is compared iff
    none of its four taps is a gutter texel (local li + lj = block - 1), a tap within 1e-3 texel of having weight counted
    as having it.  No plane needs the vertex normals' path: the normal texture is compared like the other channels, at
    silhouette pixels too.  The compared share is asserted against the share of a chart's unit cells that touch no gutter
    texel -- 1 of 2 at block 4, 15 of 18 at block 8 -- with room for the pixels' sampling of the charts: 0.3 and 0.6.
    Measured on an MI355X: 388 and 606 of 734 covered pixels compared, 0.156 and 0.767 of the bound."""
    import mesh
    import mesh_clean_ref as cr
    import mesh_render
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    raw = vol.extract(1)
    d = _linear_attributes({k: v.cpu().numpy() for k, v in zip(mesh.Mesh._fields, raw)})
    m, atlas, textured, plain = _baked_onto_itself(d, block)
    lay = atlas.layout
    B, W, H = lay.block, lay.width, lay.height
    probe = torch.zeros((3, H, W), dtype=torch.float32, device=DEV)
    probe[0] = torch.arange(W, device=DEV, dtype=torch.float32)[None, :]
    probe[1] = torch.arange(H, device=DEV, dtype=torch.float32)[:, None]
    prober = mesh_render.TexturedMeshRasterizer(m, atlas.uvs, probe, probe, probe, device=DEV)

    def keep(t, cam):
        p = prober(cam_t(cam))
        assert torch.equal(p["tri_id"], t["tri_id"])
        f = p["tri_id"].clamp(min=0).long()
        b, upper = f // 2, (f % 2) == 1
        x = p["albedo"][0].double() - ((b % lay.blocks_per_row) * (B + 1)).double()  # in the block, texel centres at integers
        y = p["albedo"][1].double() - ((b // lay.blocks_per_row) * B).double()
        li, lj = torch.where(upper, B - x, x), torch.where(upper, (B - 1) - y, y)
        return (li + 1e-3).floor() + (lj + 1e-3).floor() + 2 <= B - 2

    import scenes
    cams = [scenes.orbit_camera(k, 6, PW, PH, radius=2.0, fovx=rr.FOVX, elevation=e) for k, e in ((0, 0.5), (3, -0.6))]
    count, worst, M = _compare_with_vertex_render(textured, plain, cams, keep)
    covered = sum(int((plain(cam_t(c))["tri_id"] >= 0).sum()) for c in cams)
    bound = 2.0 ** -20 * M + 1e-5
    print("blob, block %d: %d of %d covered pixels compared, largest difference %.3e = %.3f of the bound %.3e"
          % (block, count, covered, worst, worst / bound, bound))
    assert count >= (0.3 if block == 4 else 0.6) * covered and covered > 400
    assert worst <= bound


# ---- 4: hostile inputs ---------------------------------------------------------------------------------------------------------
def test_hostile_inputs_in_one_call_each():
    """NaN UVs, +-1e30 UVs, a 1 x 1 texture, no normal texture, an empty key plane and a mesh without faces: every index is
    clamped by construction, the outputs equal the restatement's and are finite where its are."""
    import mesh_render
    from test_gpu_mesh_render import _assert_background
    mesh, uvs, _, cam = tr.quad_case()
    hostile = uvs.copy()
    hostile[0] = np.nan
    hostile[1] = np.array([(1e30, -1e30), (-1e30, 1e30), (1e30, 1e30)], np.float32)
    rng = np.random.default_rng(6)
    c = cam_t(cam)
    for shape, with_normal in (((3, 4, 5), True), ((3, 1, 1), False), ((3, 1, 7), True)):
        tex = [rng.uniform(0.25, 1, shape).astype(np.float32) for _ in range(3)]
        normal = tex[2] if with_normal else None
        with mesh_render.TexturedMeshRasterizer(mesh, hostile, tex[0], tex[1], normal, device=DEV) as rast:
            got = _host(rast(c))
            vis = rast._vis.cpu().numpy().view(np.uint64)
            ref = tr.resolve_textured(vis, mesh["faces"], rast._view_pos.cpu().numpy(), rast._screen.cpu().numpy(),
                                      rast._flags.cpu().numpy(), hostile, tex[0], tex[1], normal, mesh["normals"], cam["viewmatrix"])
            assert np.array_equal(got["tri_id"], ref["tri_id"]) and (got["tri_id"] >= 0).sum() > 600
            for k in ("albedo", "occlusion", "roughness", "metallic", "normal", "opacity", "depth", "pos"):
                assert np.array_equal(np.isfinite(got[k]), np.isfinite(ref[k])) and np.isfinite(ref[k]).all(), (shape, k)
                assert np.abs(got[k] - ref[k]).max() <= 1e-5, (shape, k)
            assert np.allclose(got["normal_view"], ref["normal_view"], rtol=0, atol=1e-5, equal_nan=True)
            hit = got["tri_id"] == 0  # NaN, NaN -> (-1, -1) -> the top left texel
            assert (got["albedo"][:, hit] == tex[0][:, 0, 0][:, None]).all()
            # an empty key plane: the background, and occlusion 1
            empty = torch.full((PH, PW), -1, dtype=torch.int64, device=DEV)
            bg = rast.resolve(c, vis=empty)
            _assert_background(bg)
            assert bool((bg["occlusion"] == 1).all())
    none = dict(mesh, faces=np.zeros((0, 3), np.int32))
    with mesh_render.TexturedMeshRasterizer(none, np.zeros((0, 3, 2), np.float32), tex[0], tex[1], tex[2], device=DEV) as rast:
        bg = rast(c)
        _assert_background(bg)
        assert bool((bg["occlusion"] == 1).all())
    # what the constructor refuses
    for bad in (lambda: mesh_render.TexturedMeshRasterizer(mesh, uvs[:1], tex[0], tex[1], tex[2], device=DEV),
                lambda: mesh_render.TexturedMeshRasterizer(mesh, uvs.astype(np.float64), tex[0], tex[1], tex[2], device=DEV),
                lambda: mesh_render.TexturedMeshRasterizer(mesh, uvs, tex[0], tex[1][:, :, :3], tex[2], device=DEV),
                lambda: mesh_render.TexturedMeshRasterizer(mesh, uvs, tex[0][0], tex[1], tex[2], device=DEV),
                lambda: mesh_render.TexturedMeshRasterizer(dict(vertices=mesh["vertices"], faces=mesh["faces"]), uvs, tex[0], tex[1],
                                                           None, device=DEV)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_render.TexturedMeshRasterizer(mesh, uvs, tex[0], tex[1], tex[2], device="cpu")


# ---- 5 and 6: occlusion modes and relighters -------------------------------------------------------------------------------------
RW, RH, RES = 176, 144, 64  # tests/test_gpu_relight.py's small case


@functools.lru_cache(maxsize=None)
def _relight_setup():
    """tests/test_gpu_mesh_render.py's sphere over a ground plane, once with per-vertex materials and once with random
    textures (block 4, 64 wide) and the same vertex normals, so both give the same normal_view and depth."""
    import mesh
    import mesh_render
    import pipeline
    import relight
    import scenes
    m = dict(_mesh())
    m["normals"] = (m["vertices"] / np.linalg.norm(m["vertices"], axis=1, keepdims=True)).astype(np.float32)
    n = 7
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, n), np.linspace(-1.6, 1.6, n), indexing="xy")
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(n * n, -0.65)], axis=1).astype(np.float32)
    cell = np.array([(j * n + i, j * n + i + 1, (j + 1) * n + i + 1, j * n + i, (j + 1) * n + i + 1, (j + 1) * n + i)
                     for j in range(n - 1) for i in range(n - 1)], np.int32).reshape(-1, 3)
    rng = np.random.default_rng(11)
    V0 = len(m["vertices"])
    m["vertices"] = np.concatenate([m["vertices"], ground])
    m["faces"] = np.concatenate([m["faces"], cell + V0])
    m["normals"] = np.concatenate([m["normals"], np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (n * n, 1))])
    m["albedo"] = np.concatenate([m["albedo"], rng.uniform(0.2, 0.9, size=(n * n, 3)).astype(np.float32)])
    m["roughness"] = np.concatenate([m["roughness"], rng.uniform(0.1, 0.6, size=n * n).astype(np.float32)])
    m["metallic"] = np.concatenate([m["metallic"], rng.uniform(0.0, 1.0, size=n * n).astype(np.float32)])
    F = len(m["faces"])
    lay = mesh.atlas_layout(F, 4, ATLAS_WIDTH)
    shape = (3, lay.height, lay.width)
    albedo, orm = rng.uniform(0.2, 0.9, shape).astype(np.float32), rng.uniform(0.1, 0.9, shape).astype(np.float32)
    plain = mesh_render.MeshRasterizer(m, device=DEV)
    textured = mesh_render.TexturedMeshRasterizer(m, mesh.face_uvs(F, lay), albedo, orm, None, device=DEV)
    cam = scenes.orbit_camera(1, 8, RW, RH, radius=3.5)
    lights = [relight.make_light(tt(scenes.synthetic_envmap(128, 256, seed=5 + k)), res=RES) for k in range(3)]
    c = cam_t(cam)
    vd = pipeline.view_dirs_for(c, pipeline.canonical_rays(cam, DEV), DEV)
    return plain, textured, c, vd, lights


def test_occlusion_modes():
    import mesh_render
    import scenes
    plain, textured, cam, _, _ = _relight_setup()
    gi = scenes.GI_DEFAULTS
    base = {k: v.clone() for k, v in mesh_render.mesh_planes(plain, cam, gi).items()}
    assert "baked_occlusion" not in base
    ssao = {k: v.clone() for k, v in mesh_render.mesh_planes(textured, cam, gi, "ssao").items()}
    default = mesh_render.mesh_planes(textured, cam, gi)
    baked_plane = textured(cam)["occlusion"]
    for k in ("occlusion_map", "depth_map", "out_normal_view", "normal_map_from_depth", "depth_pos", "tri_id", "opacity_map"):
        assert np.array_equal(_bits(ssao[k]), _bits(base[k])), k  # the same normal_view and depth: the same SSAO, bit for bit
        assert np.array_equal(_bits(default[k]), _bits(base[k])), k
    assert torch.equal(ssao["baked_occlusion"], baked_plane) and float(baked_plane.std()) > 0.05
    assert float((ssao["occlusion_map"] - 1.0).abs().max()) > 0.05, "an SSAO that occludes nothing tells the modes apart by nothing"
    baked = mesh_render.mesh_planes(textured, cam, gi, "baked")
    assert torch.equal(baked["occlusion_map"], baked_plane) and torch.equal(baked["baked_occlusion"], baked_plane)
    assert bool((baked["occlusion_map"][0][baked["tri_id"] < 0] == 1).all())
    both = mesh_render.mesh_planes(textured, cam, gi, "both")
    assert torch.equal(both["occlusion_map"], ssao["occlusion_map"] * baked_plane)
    for mode in ("baked", "both"):
        with pytest.raises(ValueError, match="TexturedMeshRasterizer"):
            mesh_render.mesh_planes(plain, cam, gi, mode)
    with pytest.raises(ValueError, match="occlusion"):
        mesh_render.mesh_planes(textured, cam, gi, "none")
    with pytest.raises(ValueError, match="occlusion"):
        mesh_render.MeshGBuffer(gi, occlusion="none")


@pytest.mark.parametrize("occlusion", ["baked", "ssao"])
def test_mesh_relighter_over_textures_equals_the_op_sequence_on_the_same_planes(occlusion):
    """tests/test_gpu_mesh_render.py's test of the same name, over the textured rasterizer: relight.Relighter._unfused's
    sequence spelled with the drop-in operators on mesh_planes' output; the bound is its 2e-6."""
    import mesh_render
    import pipeline
    import scenes
    from diff_gaussian_rasterization import Gaussian_SSR, filters
    from pbr import get_brdf_lut, pbr_shading
    _, rast, cam, vd, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    light = lights[0]
    rl = mesh_render.MeshRelighter(light, gi, occlusion=occlusion)
    out = rl(cam, rast, vd)
    assert int((out["tri_id"] >= 0).sum()) > 2000

    r = mesh_render.mesh_planes(rast, cam, gi, occlusion)
    _, _, normals_view, normal_mask, onv = pipeline.gbuffer_post(r["normal_map_from_depth"], r["normal_map"],
                                                                 r["out_normal_view"], r["viewmatrix"])
    albedo_map, roughness_map, metallic_map = r["albedo_map"], r["roughness_map"], r["metallic_map"]
    res = pbr_shading(light=light, normals=normals_view.permute(1, 2, 0), view_dirs=vd, mask=normal_mask.permute(1, 2, 0),
                      albedo=albedo_map.permute(1, 2, 0), roughness=roughness_map.permute(1, 2, 0), metallic=None, tone=False,
                      occlusion=r["occlusion_map"].permute(1, 2, 0), gamma=False, brdf_lut=get_brdf_lut().to(DEV))
    render_direct = torch.where(normal_mask, res["render_rgb"].permute(2, 0, 1), torch.zeros(3, device=DEV)[:, None, None])
    ssr = Gaussian_SSR(cam["tanfovx"], cam["tanfovy"], RW, RH, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"],
                       gi["start"])
    F0, metallic_in = 0.04 + albedo_map * metallic_map, metallic_map
    IRR, _ = ssr(onv, r["depth_pos"], pipeline.srgb_to_linear(render_direct), albedo_map, roughness_map, metallic_in, F0)
    render_rgb = render_direct + filters.median_blur(pipeline.linear_to_srgb(IRR)[None, ...], (3, 3))[0]
    for k, w in dict(render_direct=render_direct, IRR=IRR, render_rgb=render_rgb).items():
        d = float((out[k].nan_to_num() - w.nan_to_num()).abs().max())
        print("occlusion %s, %s: max difference %.3g" % (occlusion, k, d))
        assert d <= 2e-6, k
    assert torch.equal(out["occlusion"], r["occlusion_map"]) and torch.equal(out["baked_occlusion"], r["baked_occlusion"])
    if occlusion == "baked":
        assert torch.equal(out["occlusion"], out["baked_occlusion"])
    assert float(out["render_rgb"].nan_to_num().max()) > 0.2 and out["radii"] is None


def test_multi_and_turntable_over_textures_equal_the_single_light_relighter():
    import mesh_render
    import scenes
    _, rast, cam, vd, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    for occlusion in ("baked", "both"):
        single = []
        for light in lights:
            o = mesh_render.MeshRelighter(light, gi, occlusion=occlusion)(cam, rast, vd)
            single.append({k: o[k].clone() for k in ("render_rgb", "render_direct", "IRR")})
        multi = mesh_render.MeshMultiRelighter(lights, gi, occlusion=occlusion)(cam, rast, vd)
        with mesh_render.MeshTurntableRelighter(lights, gi, occlusion=occlusion) as turn_rl:
            turn = turn_rl(cam, rast, vd)
        for name, o in (("multi", multi), ("turntable", turn)):
            assert tuple(o["render_rgb"].shape) == (3, 3, RH, RW) and "baked_occlusion" in o
            for k, want in enumerate(single):
                for key, w in want.items():
                    a = o[key][k]
                    assert torch.equal(torch.isnan(a), torch.isnan(w)) and torch.equal(a.nan_to_num(), w.nan_to_num()), (
                        occlusion, name, k, key)


# ---- 7: the tools ----------------------------------------------------------------------------------------------------------------
def test_render_mesh_tool_on_a_textured_mesh(tmp_path):
    """texture_mesh.py on the blob PLY, then render_mesh.py --mesh light.obj --reference_mesh blob.ply --occlusion baked on a
    scene folder whose cameras look at the origin.  The files exist, mesh_vs_mesh.json has its keys, and the albedo rendered
    from the 8-bit PNGs is within half a quantisation step (bilinear is a convex combination of texels) plus the render
    tests' 1e-5 of the albedo rendered from the float atlas."""
    from argparse import Namespace

    import mesh
    import mesh_clean_ref as cr
    import mesh_render
    import render_mesh
    import scene_io
    import scenes
    import simplify_mesh
    import synthetic_dataset
    import texture_mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    src = vol.extract(1)
    out = str(tmp_path / "run")
    os.makedirs(out)
    raw = os.path.join(out, "blob.ply")
    fields = {k: t.cpu().numpy() for k, t in zip(mesh.Mesh._fields, src)}
    for k in ("albedo", "roughness", "metallic"):  # the blob's random attributes lie in [-1, 1]; an 8-bit image holds [0, 1]
        fields[k] = np.abs(fields[k])
    scene_io.save_mesh_ply(raw, *(fields[k] for k in mesh.Mesh._fields))
    low = simplify_mesh.simplify_mesh([raw, "-o", os.path.join(out, "low.ply"), "--cell_edges", "2"])
    obj = os.path.join(out, "light.obj")
    rep = texture_mesh.texture_mesh([raw, "-o", obj, "--target", low["path"], "--block", "4", "--width", str(ATLAS_WIDTH)])
    scene = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=6, size=64)
    with open(os.path.join(out, "cfg_args"), "w") as f:
        f.write(str(Namespace(sh_degree=3, source_path=scene, model_path=out, images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    res = render_mesh.render_mesh(["-m", out, "--mesh", "light.obj", "--reference_mesh", "blob.ply", "--occlusion", "baked",
                                   "--hdri", hdr, "--split", "train"])
    assert res["n_views"] == 2 and res["faces"] == rep["faces"] and res["lights"] == ["sky"]
    folder = os.path.join(out, "mesh_train")
    names = sorted(os.listdir(folder))
    assert len(names) == 2 * 8 + 1 and res["files"] == 16 and sum(n.endswith("_baked_occlusion.png") for n in names) == 2
    with open(os.path.join(folder, "mesh_vs_mesh.json")) as f:
        cmp = json.load(f)
    assert res["mesh_vs_mesh_json"] == os.path.join(folder, "mesh_vs_mesh.json") and cmp["occlusion"] == "baked"
    assert len(cmp["views"]) == 2 and cmp["lights"] == ["sky"]
    for v in cmp["views"] + [cmp["average"]]:
        for k in ("coverage_iou", "albedo_psnr", "roughness_psnr", "metallic_psnr", "normal_angle_deg"):
            assert np.isfinite(v[k]), (k, v)
        assert list(v["relit_psnr"]) == ["sky"] and np.isfinite(v["relit_psnr"]["sky"])
    assert all(v["pixels_both_cover"] > 100 and 0.5 < v["coverage_iou"] <= 1.0 for v in cmp["views"])
    print("light textured mesh against the blob:", json.dumps(cmp["average"]))
    # a PLY against a PLY: the "vertices" column
    res2 = render_mesh.render_mesh(["-m", out, "--mesh", "low.ply", "--reference_mesh", raw, "--hdri", hdr, "--split", "train"])
    assert np.isfinite(res2["mesh_vs_mesh"]["albedo_psnr"])
    print("light per-vertex mesh against the blob:", json.dumps(res2["mesh_vs_mesh"]))
    # --occlusion baked with a PLY is an argument error
    with pytest.raises(SystemExit) as e:
        render_mesh.main(["-m", out, "--mesh", "low.ply", "--occlusion", "baked", "--hdri", hdr])
    assert e.value.code not in (0, None)
    parsed = render_mesh.parse_args(["-m", out, "--mesh", "low.ply", "--hdri", hdr])
    parsed.occlusion = "both"  # past the parser: the API refuses it too
    with pytest.raises(ValueError, match="occlusion"):
        render_mesh.render_mesh(parsed)
    # the PNGs against the float atlas
    load = lambda p: _device_mesh(mesh_render.mesh_arrays(p))  # noqa: E731
    dst = load(low["path"])
    atlas, _ = mesh.bake_atlas(dst, load(raw), block=4, width=ATLAS_WIDTH)
    loaded = mesh_render.load_textured_mesh(obj)
    assert np.array_equal(loaded["uvs"], atlas.uvs.cpu().numpy()) and loaded["albedo"].shape == tuple(atlas.albedo.shape)
    cam = cam_t(scenes.orbit_camera(0, 6, PW, PH, radius=2.0, fovx=rr.FOVX, elevation=0.5))
    with mesh_render.TexturedMeshRasterizer(**loaded, device=DEV) as from_png, \
            mesh_render.TexturedMeshRasterizer.from_atlas(dst, atlas) as from_atlas:
        a, b = from_png(cam), from_atlas(cam)
        assert torch.equal(a["tri_id"], b["tri_id"]) and int((a["tri_id"] >= 0).sum()) > 200
        worst = float((a["albedo"] - b["albedo"]).abs().max())
        print("albedo from the PNGs against the float atlas: largest difference %.5f = %.3f of a quantisation step" % (worst, worst * 255))
        assert worst <= 0.5 / 255 + 1e-5
