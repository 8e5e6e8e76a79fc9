"""CPU: the numpy restatement of ray-traced light per point (tests/mesh_gather_ref.py) against known answers and against its
own one-cell grid, the new symbol's place in the C ABI, and the arguments of render_mesh.py and relight_scene.py."""
import os
import re

import numpy as np
import pytest

import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
import mesh_simplify_ref as sr

R, K = 64, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _constant_sky(c, n=4):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), (6, n, n, 3)))


def test_restatement_known_answers():
    table = rr.direction_table(R, K)
    c = np.array([0.5, 2.0, 0.25], np.float32)
    # above a plane, looking up: the sky alone, exactly; a masked point, a NaN position and a zero normal get no rays
    v, f = sr.plane_grid()
    p = np.array([[0.3, 0.4, 0.5], [0.6, 0.2, 0.5], [np.nan, 0.5, 0.5], [0.5, 0.5, 0.5], [0.7, 0.7, 0.5]], np.float32)
    n = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 1]], np.float32)
    got = gr.gather_points(p, n, v, f, table, _constant_sky(c), gr.hash_radiosity(len(v)), mask=np.array([1, 1, 1, 1, 0], np.uint8))
    assert gr.counters(got) == (2 * R, 0, 0, 2, 1)
    assert np.array_equal(got["hits"], np.zeros(5, np.int32)) and (got["occlusion"] == 1).all() and (got["indirect"] == 0).all()
    assert np.array_equal(_bits(got["irradiance"]), _bits(np.stack([c, c, 0 * c, 0 * c, 0 * c])))
    # below the plane, looking up at its back: every ray is a back hit within reach, and brings nothing
    down = gr.gather_points(np.array([[0.5, 0.5, 0.2]], np.float32), n[:1], v, f, table, _constant_sky(c), ao_distance=10.0, bias=0.0)
    assert 0 < down["hits"][0] <= R and down["back_hits"] == down["hits"][0] and down["front_hits"] == 0
    assert down["occlusion"][0] == np.float32((R - down["hits"][0]) / R)
    # the same from the other side of a flipped plane: front hits that bring the radiosity, constant here
    Q = np.broadcast_to(np.array([3.0, 0.5, 1.0], np.float32), (len(v), 3))
    flip = gr.gather_points(np.array([[0.5, 0.5, 0.2]], np.float32), n[:1], v, f[:, [0, 2, 1]], table, _constant_sky(0 * c), Q,
                            ao_distance=10.0, bias=0.0)
    assert flip["front_hits"] == down["hits"][0] and flip["back_hits"] == 0 and np.array_equal(flip["hits"], down["hits"])
    want = flip["hits"][0] / R * Q[0].astype(np.float64)
    assert np.allclose(flip["irradiance"][0], want, rtol=1e-6) and np.array_equal(_bits(flip["irradiance"]), _bits(flip["indirect"]))
    # no sky: no light outputs, the same count
    bare = gr.gather_points(np.array([[0.5, 0.5, 0.2]], np.float32), n[:1], v, f, table, ao_distance=10.0, bias=0.0)
    assert bare["irradiance"] is None and bare["indirect"] is None and np.array_equal(bare["hits"], down["hits"])


def test_restatement_does_not_depend_on_the_grid_or_on_the_light_distance():
    v, f, nrm = lr.open_box(2)
    p, n = gr.face_points(v, f, 3)
    table = rr.direction_table(R, K)
    g = rr.build_grid(v, f)
    D, bias = rr.bake_defaults(g)
    args = dict(sky=lr.hash_sky(), radiosity=gr.hash_radiosity(len(v)), ao_distance=3.0 * D, bias=bias, seed=4)
    a = gr.gather_points(p, n, v, f, table, **args)
    b = gr.gather_points(p, n, v, f, table, cell=1e6 * g["cell"], **args)
    assert tuple(int(x) for x in b["grid"]["G"]) == (1, 1, 1)
    assert np.array_equal(a["hits"], b["hits"]) and gr.counters(a) == gr.counters(b) and a["front_hits"] > 0 and a["misses"] > 0
    for k in ("occlusion", "irradiance", "indirect"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    # occlusion only stops the rays at ao_distance: the count is the one of the rays that run on
    c = gr.gather_points(p, n, v, f, table, **dict(args, sky=None))
    assert np.array_equal(c["hits"], a["hits"]) and np.array_equal(_bits(c["occlusion"]), _bits(a["occlusion"]))
    assert 0 < int(a["hits"].sum()) < a["front_hits"] + a["back_hits"]
    # with points = vertices and the vertex radiosity this is one pass of the light bake
    rec = lr.trace(v, f, nrm, table, bias=bias, seed=4)
    rho = np.full((len(v), 3), 0.5, np.float32)
    I, Qs = lr.light(v, f, nrm, table, 4, rec["face"], rec["bary"], args["sky"], rho, bounces=1)
    d = gr.gather_points(v, nrm, v, f, table, args["sky"], Qs[0], ao_distance=3.0 * D, bias=bias, seed=4)
    assert np.array_equal(_bits(d["irradiance"]), _bits(I[1])) and (I[1] > I[0]).any()
    assert (d["misses"], d["front_hits"], d["back_hits"], d["no_normal"]) == tuple(rec[k] for k in ("misses", "front_hits", "back_hits", "no_normal"))


def test_prepare_inverts_the_view_transform():
    import scenes
    cam = scenes.look_at_camera((1.9, 0.35, 1.7), (0.4, 0.5, 0.3), 8, 6, 0.9)
    M = cam["viewmatrix"].astype(np.float64)
    rng = np.random.default_rng(0)
    pw = rng.uniform(-1, 1, size=(48, 3))
    nw = rng.normal(size=(48, 3))
    nw /= np.linalg.norm(nw, axis=1, keepdims=True)
    pv = (pw @ M[:3, :3] + M[3, :3]).astype(np.float32).T.reshape(3, 6, 8)
    for space, plane in (("world", nw), ("view", -(nw @ M[:3, :3]))):
        p, n = gr.prepare(pv, plane.astype(np.float32).T.reshape(3, 6, 8), cam["viewmatrix"], space)
        assert np.abs(p - pw).max() <= 1e-6 and np.abs(n - nw).max() <= 1e-6, space
    _, n = gr.prepare(pv, np.zeros((3, 6, 8), np.float32), cam["viewmatrix"])
    assert np.isnan(n).all()


def test_the_symbol_is_declared_bound_and_built():
    import build
    import gigs_lib
    with open(os.path.join(ROOT, "include", "gigs_hip.h")) as fh:
        header = fh.read()
    proto = re.search(r"int gigs_mesh_gather_points\(([^;]*)\);", header)
    assert proto is not None and "mesh_gather.hip" in build.SOURCES
    res, args = gigs_lib.SIGNATURES["gigs_mesh_gather_points"]
    assert len(args) == len(proto.group(1).split(",")) == 33
    with open(os.path.join(ROOT, "gi-gs_amd", "csrc", "mesh_gather.hip")) as fh:
        src = fh.read()
    assert re.sub(r"\s+", " ", proto.group(1)) in re.sub(r"\s+", " ", src)
    assert "Ray-traced light per point" in header and "sqrt" not in src.replace("no sqrt", "")


def test_render_mesh_raytraced_arguments():
    import render_mesh
    base = ["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr"]
    a = render_mesh.parse_args(base)
    assert (a.occlusion, a.lighting, a.ao_rays, a.ao_distance, a.ray_bias) == ("ssao", "screen", 64, None, None)
    assert render_mesh._check(a) == 0
    a = render_mesh.parse_args(base + ["--occlusion", "raytraced", "--ao_rays", "128", "--ao_distance", "0.5", "--ray_bias", "0.01"])
    assert (a.occlusion, a.ao_rays, a.ao_distance, a.ray_bias) == ("raytraced", 128, 0.5, 0.01) and render_mesh._check(a) == 0
    a = render_mesh.parse_args(["-m", "o", "--mesh", "m.obj", "--checkpoint", "c.pth", "--occlusion", "raytraced"])
    assert render_mesh._check(a) == 0  # an OBJ, and no --hdri: the occlusion needs neither
    a = render_mesh.parse_args(base + ["--lighting", "raytraced", "--bounces", "3", "--light_rays", "64", "--sky_res", "16"])
    assert (a.lighting, a.bounces, a.light_rays, a.sky_res) == ("raytraced", 3, 64, 16) and render_mesh._check(a) == 0
    assert render_mesh.LIGHTING_MODES == ("screen", "baked", "raytraced") and render_mesh.OCCLUSION_MODES == ("ssao", "baked", "both")
    for argv in (["-m", "o", "--mesh", "m.ply", "--checkpoint", "c.pth", "--lighting", "raytraced"],
                 ["-m", "o", "--mesh", "m.obj", "--hdri", "a.hdr", "--lighting", "raytraced"],
                 base + ["--lighting", "raytraced", "--bounces", "-1"], base + ["--lighting", "raytraced", "--ao_rays", "96"],
                 base + ["--occlusion", "raytraced", "--ao_rays", "2048"], base + ["--occlusion", "raytraced", "--ray_bias", "-1"],
                 base + ["--occlusion", "raytraced", "--ao_distance", "inf"]):
        with pytest.raises(ValueError, match="lighting raytraced|bounces|ao_rays|ray_bias|ao_distance"):
            render_mesh._check(render_mesh.parse_args(argv))
    for argv in (base + ["--lighting", "both"], base + ["--occlusion", "traced"], base + ["--occlusion", "baked"]):
        with pytest.raises(SystemExit):
            render_mesh.parse_args(argv)


def test_relight_scene_occluder_arguments():
    import relight_scene
    base = ["-m", "o", "--checkpoint", "c.pth", "--hdri", "a.hdr"]
    a = relight_scene.parse_args(base)
    assert (a.occluder, a.ao_rays, a.ao_distance, a.ray_bias, a.occluder_mode) == (None, 64, None, None, "replace")
    assert relight_scene.check_occluder(a) is False
    a = relight_scene.parse_args(base + ["--occluder", "mesh.ply", "--ao_rays", "256", "--ao_distance", "0.3", "--ray_bias", "0.002",
                                         "--occluder_mode", "multiply"])
    assert (a.occluder, a.ao_rays, a.ao_distance, a.ray_bias, a.occluder_mode) == ("mesh.ply", 256, 0.3, 0.002, "multiply")
    assert relight_scene.check_occluder(a) is True
    for argv in (base + ["--ao_rays", "128"], base + ["--ao_distance", "1"], base + ["--ray_bias", "0"],
                 base + ["--occluder_mode", "multiply"], base + ["--occluder", "m.ply", "--ao_rays", "100"],
                 base + ["--occluder", "m.ply", "--ao_distance", "-2"], base + ["--occluder", "m.ply", "--ray_bias", "nan"]):
        with pytest.raises(ValueError, match="occluder|ao_rays|ao_distance|ray_bias"):
            relight_scene.check_occluder(relight_scene.parse_args(argv))
    with pytest.raises(SystemExit):
        relight_scene.parse_args(base + ["--occluder_mode", "both"])
