"""CPU: the numpy restatement of ray-traced reflections per point (tests/mesh_reflect_ref.py) against known answers, the table
of GGX half vectors, the new symbols' place in the C ABI and the arguments of render_mesh.py."""
import os
import re

import numpy as np
import pytest

import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
import mesh_reflect_ref as fr
import mesh_simplify_ref as sr

R, K = 64, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _constant_sky(c, n=4):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(c, np.float32), (6, n, n, 3)))


def test_table_of_half_vectors():
    import mesh
    t = mesh.ggx_directions(128, 4, 8)
    assert t.shape == (8, 4, 128, 3) and t.dtype == np.float32
    assert np.array_equal(_bits(t), _bits(fr.ggx_table(128, 4, 8)))
    assert mesh.ggx_directions().shape == (16, 16, 64, 3)
    length = np.sqrt((t.astype(np.float64) ** 2).sum(-1))
    assert np.abs(length - 1.0).max() <= 3 * 2.0 ** -24  # three float32 roundings of a unit vector's components
    assert (t[..., 2] > 0).all()
    mean_z = t[..., 2].astype(np.float64).mean(axis=(1, 2))
    assert (np.diff(mean_z) < 0).all() and mean_z[0] > 0.9999 and mean_z[-1] < 0.8  # the lobe widens with the roughness
    # every rotation is the same lattice turned about z
    assert np.array_equal(t[:, 0, :, 2], t[:, 3, :, 2])
    for bad in (dict(rays=100), dict(rays=2048), dict(rotations=0), dict(rotations=65), dict(levels=0), dict(levels=65)):
        with pytest.raises(ValueError, match="rays|rotations|levels"):
            mesh.ggx_directions(**bad)


def test_level_rule():
    L = 16
    exact = (np.arange(L + 1, dtype=np.float64) / L).astype(np.float32)  # l / L is a float32 for L = 16
    assert np.array_equal(fr.level_of(exact, L), np.minimum(np.arange(L + 1), L - 1))
    assert list(fr.level_of(np.array([1.0, np.nan, -1.0, 2.0, -0.0, np.inf, -np.inf], np.float32), L)) == [15, 0, 0, 15, 0, 15, 0]
    below = np.nextafter(exact[1:], np.float32(0), dtype=np.float32)
    assert np.array_equal(fr.level_of(below, L), np.arange(L))
    assert list(fr.level_of(np.array([0.0, 0.3, 0.999], np.float32), 1)) == [0, 0, 0]


def test_constant_sky_and_closed_box():
    table = fr.ggx_table(R, K, 4)
    c = np.array([0.5, 2.0, 0.25], np.float32)
    # above a plane, looking down on it from any side: every valid ray rises and escapes; the weighted mean of a constant
    # is the constant: the float64 quotient lies within R 2^-53 of a float32, so the float32 rounding is exact
    v, f = sr.plane_grid()
    xy = np.random.default_rng(1).uniform(0.2, 0.8, size=(23, 2))
    p = np.concatenate([xy, np.full((23, 1), 0.5)], 1).astype(np.float32)
    n = np.repeat([[0.0, 0.0, 1.0]], 23, 0).astype(np.float32)
    views = fr.hash_views(n, below_every=10 ** 6)
    rough = fr.hash_roughness(23)
    got = fr.reflect_points(p, n, views, rough, v, f, table, _constant_sky(c), gr.hash_radiosity(len(v)), bias=1e-3)
    assert (got["valid"] > 0).all() and (got["blocked"] == 0).all() and (got["visibility"] == 1).all()
    assert np.array_equal(_bits(got["specular"]), _bits(np.broadcast_to(c, (23, 3)))) and (got["reflected"] == 0).all()
    assert got["misses"] == int(got["valid"].sum()) and got["misses"] + got["below_horizon"] == 23 * R
    assert fr.counters(got)[1:3] == (0, 0) and fr.counters(got)[4:] == (0, 0, 0)
    # inside the closed box every ray ends on a wall, whose back it sees: nothing escapes and nothing is brought
    v, f, _ = rr.box_interior()
    p = np.random.default_rng(2).uniform(0.2, 0.8, size=(11, 3)).astype(np.float32)
    n = lr.analytic_normals()[np.arange(11) % 9].astype(np.float32)
    got = fr.reflect_points(p, n, fr.hash_views(n, below_every=10 ** 6), fr.hash_roughness(11), v, f, table, _constant_sky(c),
                            gr.hash_radiosity(len(v)), bias=0.0)
    assert (got["valid"] > 0).all() and np.array_equal(got["blocked"], got["valid"]) and (got["visibility"] == 0).all()
    assert np.array_equal(_bits(got["reflected"]), _bits(got["specular"])) and got["misses"] == 0
    # no sky: the light outputs are None, the rest is the same
    bare = fr.reflect_points(p, n, fr.hash_views(n, below_every=10 ** 6), fr.hash_roughness(11), v, f, table, bias=0.0)
    assert bare["specular"] is None and bare["reflected"] is None and fr.counters(bare) == fr.counters(got)
    assert np.array_equal(bare["blocked"], got["blocked"]) and np.array_equal(_bits(bare["visibility"]), _bits(got["visibility"]))


def _wall(x):
    """A quad in the plane x = `x` about (x, 0, 1), one unit a side."""
    v = np.array([[x, -0.5, 0.5], [x, 0.5, 0.5], [x, 0.5, 1.5], [x, -0.5, 1.5]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_mirror_case():
    L = 64
    table = fr.ggx_table(R, K, L)
    s = np.float32(np.sqrt(0.5))
    p = np.zeros((K * 3, 3), np.float32)  # several points: the rotation follows the point's index
    n = np.repeat([[0.0, 0.0, 1.0]], len(p), 0).astype(np.float32)
    views = np.repeat([[-s, 0.0, s]], len(p), 0).astype(np.float32)  # 45 degrees: the mirror direction is (s, 0, s)
    rough = np.full(len(p), 0.5 / L, np.float32)
    assert (fr.level_of(rough, L) == 0).all()
    # from the table alone: every valid ray meets the plane x = 1 well inside the quad
    q = fr.rays_of(p, n, views, rough, table, 0)
    assert q["ok_normal"].all() and q["ok_view"].all() and len(set(q["rotation"])) > 1
    live = q["live"]
    assert live.sum() > 0.9 * live.size
    l = q["l"][live]
    assert (l[:, 0] > 0).all()
    y, z = l[:, 1] / l[:, 0], l[:, 2] / l[:, 0]
    assert np.abs(y).max() < 0.4 and np.abs(z - 1.0).max() < 0.4
    v, f = _wall(1.0)
    got = fr.reflect_points(p, n, views, rough, v, f, table, _constant_sky([1.0, 1.0, 1.0]), bias=1e-3)
    assert np.array_equal(got["valid"], live.sum(axis=1)) and np.array_equal(got["blocked"], got["valid"])
    assert (got["visibility"] == 0).all() and got["misses"] == 0
    v, f = _wall(-1.0)
    got = fr.reflect_points(p, n, views, rough, v, f, table, _constant_sky([1.0, 1.0, 1.0]), bias=1e-3)
    assert np.array_equal(got["valid"], live.sum(axis=1)) and (got["blocked"] == 0).all() and (got["visibility"] == 1).all()
    assert np.array_equal(_bits(got["specular"]), _bits(np.ones((len(p), 3), np.float32)))


def test_counters_and_dead_points():
    v, f, _ = lr.open_box(2)
    p, n = gr.face_points(v, f, 3)
    p, n = p.copy(), n.copy()
    N = len(p)
    assert N >= 12
    mask = (np.arange(N) % 5 != 0).astype(np.uint8)
    p[1, 0] = np.nan
    n[2] = 0.0
    n[3] = n[3] * np.float32(1.01)
    views = fr.hash_views(n)
    views[4] = views[4] * np.float32(1.01)
    views[6] = np.nan
    rough = fr.hash_roughness(N)
    table = fr.ggx_table(R, K, 4)
    args = dict(sky=lr.hash_sky(), radiosity=gr.hash_radiosity(len(v)), seed=4, mask=mask)
    got = fr.reflect_points(p, n, views, rough, v, f, table, **args)
    dead = (mask == 0) | np.isin(np.arange(N), (1, 2, 3, 4, 6))
    assert got["masked"] == int((mask == 0).sum()) and got["no_normal"] == 3 and got["no_view"] == 2
    assert (got["valid"][dead] == 0).all() and (got["blocked"][dead] == 0).all() and (got["visibility"][dead] == 1).all()
    assert (got["specular"][dead] == 0).all() and (got["reflected"][dead] == 0).all()
    live = int((~dead).sum())
    assert int(got["valid"].sum()) + got["below_horizon"] == R * live
    assert got["misses"] + got["front_hits"] + got["back_hits"] == int(got["valid"].sum())
    assert got["front_hits"] > 0 and got["misses"] > 0 and got["below_horizon"] > 0 and (got["blocked"] <= got["valid"]).all()
    assert (got["reflected"] <= got["specular"]).all() and float(got["reflected"].max()) > 0
    # the one-cell grid gives the same bits
    one = fr.reflect_points(p, n, views, rough, v, f, table, cell=1e6 * got["grid"]["cell"], bias=got["bias"], **args)
    assert tuple(int(x) for x in one["grid"]["G"]) == (1, 1, 1) and fr.counters(one) == fr.counters(got)
    for k in fr.OUTPUTS:
        assert np.array_equal(_bits(one[k]), _bits(got[k])), k
    # a mesh with no usable face: nothing is traced and no ray is counted
    none = fr.reflect_points(p, n, views, rough, np.zeros((3, 3), np.float32), np.array([[0, 1, 1]], np.int32), table, **args)
    assert fr.counters(none) == (0, 0, 0, 0, 3, 2, got["masked"]) and (none["visibility"] == 1).all() and (none["specular"] == 0).all()


def test_compose_and_views():
    rng = np.random.default_rng(5)
    N = 50
    n = rng.normal(size=(N, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    views = fr.hash_views(n)
    lut = rng.uniform(0, 1, size=(8, 16, 2)).astype(np.float32)
    rough, rad = rng.uniform(0, 1, N).astype(np.float32), rng.uniform(0, 4, (N, 3)).astype(np.float32)
    # a constant table: fg is the constant within the roundings of four weights that sum to 1
    flat = np.broadcast_to(np.array([0.75, 0.125], np.float32), (8, 16, 2))
    out = fr.compose(n, views, rough, rad, flat)
    assert out.dtype == np.float32 and np.allclose(out, rad * (0.04 * 0.75 + 0.125), rtol=1e-6)
    mask = (np.arange(N) % 3 != 0).astype(np.uint8)
    alb, met, vis = rng.uniform(0, 1, (N, 3)).astype(np.float32), rng.uniform(0, 1, N).astype(np.float32), rng.uniform(0, 1, N).astype(np.float32)
    out = fr.compose(n, views, rough, rad, lut, alb, met, mask, vis)
    assert (out[mask == 0] == 0).all() and (out[mask != 0] > 0).all()
    f64 = lambda x: x.astype(np.float64)  # noqa: E731
    ones = fr.compose(n, views, rough, np.ones((N, 3), np.float32), lut, alb, met)
    assert np.allclose(out[mask != 0], (f64(rad) * f64(vis)[:, None] * f64(ones))[mask != 0], rtol=1e-6)
    # the views point from the surface towards the eye and have unit length
    p = rng.uniform(-1, 1, (N, 3)).astype(np.float32)
    c = np.array([0.5, 3.0, -2.0], np.float32)
    w = fr.prepare_views(p, c)
    assert np.abs((w ** 2).sum(1) - 1.0).max() < 1e-14 and np.allclose(np.cross(w, f64(c) - f64(p)), 0.0, atol=1e-12)
    assert ((w * (f64(c) - f64(p))).sum(1) > 0).all() and np.isnan(fr.prepare_views(c[None], c)).all()


def test_the_symbols_are_declared_bound_and_built():
    import build
    import gigs_lib
    with open(os.path.join(ROOT, "include", "gigs_hip.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "gi-gs_amd", "csrc", "mesh_reflect.hip")) as fh:
        src = fh.read()
    assert "mesh_reflect.hip" in build.SOURCES and "Ray-traced reflections per point" in header
    for symbol, count in (("gigs_mesh_reflect_points", 36), ("gigs_reflect_compose", 14)):
        proto = re.search(r"int %s\(([^;]*)\);" % symbol, header)
        assert proto is not None, symbol
        res, args = gigs_lib.SIGNATURES[symbol]
        assert len(args) == len(proto.group(1).split(",")) == count, symbol
        assert re.sub(r"\s+", " ", proto.group(1)) in re.sub(r"\s+", " ", src), symbol
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "sqrt" not in code and "atomicAdd(a.counts" in code and "__shared__" not in code


def test_render_mesh_reflection_arguments():
    import render_mesh
    base = ["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr"]
    a = render_mesh.build_parser().parse_args(base)
    assert (a.reflections, a.reflection_rays, a.roughness_levels, a.reflection_sky_res) == (False, 64, 16, 128)
    assert render_mesh._check(a) == 0
    a = render_mesh.build_parser().parse_args(base + ["--lighting", "raytraced", "--reflections", "--reflection_rays", "128",
                                                      "--roughness_levels", "8", "--reflection_sky_res", "64"])
    assert (a.reflections, a.reflection_rays, a.roughness_levels, a.reflection_sky_res) == (True, 128, 8, 64)
    assert render_mesh._check(a) == 0
    for argv in (base + ["--reflections"], base + ["--lighting", "baked", "--reflections"],
                 base + ["--lighting", "raytraced", "--reflections", "--reflection_rays", "96"],
                 base + ["--lighting", "raytraced", "--reflections", "--roughness_levels", "0"],
                 base + ["--lighting", "raytraced", "--reflections", "--reflection_sky_res", "0"]):
        with pytest.raises(ValueError, match="reflections needs --lighting raytraced|reflection_rays|roughness_levels|reflection_sky_res"):
            render_mesh._check(render_mesh.parse_args(argv))
