"""CPU: analytic lights and their shadows -- the two new symbols' place in the C ABI, the lights file, the table of ball
offsets, the numpy restatement's grid walk against its brute force over all faces (the any-hit identity on the host), and the
conditions of the BSDF fixture tests/golden/lights_bsdf.npz."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest

import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
import mesh_shadow_ref as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lights_bsdf.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_symbols_are_declared_bound_and_built():
    import build
    import gigs_lib
    with open(os.path.join(ROOT, "include", "gigs_hip.h")) as fh:
        header = fh.read()
    for symbol, unit, n_args in (("gigs_mesh_shadow_points", "mesh_shadow.hip", 29), ("gigs_shade_lights", "shade_lights.hip", 15)):
        proto = re.search(r"int %s\(([^;]*)\);" % symbol, header)
        assert proto is not None and unit in build.SOURCES
        res, args = gigs_lib.SIGNATURES[symbol]
        assert len(args) == len(proto.group(1).split(",")) == n_args
        with open(os.path.join(ROOT, "gi-gs_amd", "csrc", unit)) as fh:
            src = fh.read()
        assert re.sub(r"\s+", " ", proto.group(1)) in re.sub(r"\s+", " ", src)
    assert "Shadows of analytic lights" in header and "Shading under analytic lights" in header
    assert re.search(r"#define GIGS_LIGHT_ROW 8\b", header)
    with open(os.path.join(ROOT, "gi-gs_amd", "csrc", "mesh_shadow.hip")) as fh:
        assert "sqrt" not in fh.read()  # float64 + - * / only
    with open(os.path.join(ROOT, "gi-gs_amd", "csrc", "mesh_ray.h")) as fh:
        ray = fh.read()
    assert "bool occluded(" in ray and "bool traverse(" in ray


def test_parse_lights_and_pack(tmp_path):
    import analytic_lights as al
    entries = [dict(kind="point", position=[1, 2, 3], color=[1, 0.5, 0.25], intensity=4, radius=0.5),
               dict(kind="directional", direction=[0, 3, -4], angle=45.0), dict(kind="point", position=[0, 0, 0])]
    lights = al.parse_lights(entries)
    assert [x.kind for x in lights] == ["point", "directional", "point"] and lights[1].vector == (0.0, 0.6, -0.8)
    assert lights[2].color == (1.0, 1.0, 1.0) and lights[2].intensity == 1.0 and lights[2].extent == 0.0
    rows, radiance = al.pack(lights)
    assert rows.dtype == radiance.dtype == np.float32 and rows.shape == (3, al.LIGHT_ROW) and radiance.shape == (3, 3)
    assert np.array_equal(rows[0], np.array([0, 1, 2, 3, 0.5, 0, 0, 0], np.float32))
    assert rows[1, 0] == 1 and np.array_equal(rows[1, 1:4], np.array([0, 0.6, -0.8], np.float32)) and rows[1, 4] == np.float32(1.0)
    assert np.array_equal(radiance, np.array([[4, 2, 1], [1, 1, 1], [1, 1, 1]], np.float32))
    # parsing what was parsed, and packing either, changes no bit; the file and the echo round-trip
    assert al.parse_lights(list(lights)) == lights and np.array_equal(al.pack(entries)[0], rows)
    assert np.array_equal(al.light_rows(lights), rows) and np.array_equal(al.light_rows(rows), rows)
    path = str(tmp_path / "lights.json")
    with open(path, "w") as fh:
        json.dump([al.light_entry(x) for x in lights], fh)
    assert al.load_lights(path) == lights
    with open(path, "w") as fh:
        fh.write("[{")
    with pytest.raises(ValueError, match="not JSON"):
        al.load_lights(path)
    point, sun = entries[0], entries[1]
    for bad, field in (([], "1 to 16"), ([point] * 17, "1 to 16"), ({"kind": "point"}, "list"), ([3], r"lights\[0\]: an object"),
                       ([dict(point, kind="spot")], "kind"), ([dict(kind="point")], "position"),
                       ([dict(point, position=[1, 2])], "position"), ([dict(point, position=[1, 2, float("nan")])], "position"),
                       ([dict(point, position="here")], "position"), ([dict(point, color=[1, -1, 1])], "color"),
                       ([dict(point, color=[1, 1])], "color"), ([dict(point, intensity=-1)], "intensity"),
                       ([dict(point, intensity="bright")], "intensity"), ([dict(point, radius=-0.5)], "radius"),
                       ([dict(point, radius=float("inf"))], "radius"), ([dict(point, angle=3)], "angle"),
                       ([dict(point, direction=[0, 0, 1])], "direction"), ([dict(sun, direction=[0, 0, 0])], "direction"),
                       ([dict(sun, angle=90)], "angle"), ([dict(sun, radius=1)], "radius"), ([point, dict(sun, angel=1)], r"lights\[1\].*angel")):
        with pytest.raises(ValueError, match=field):
            al.parse_lights(bad)
    for bad in (np.zeros((0, 8), np.float32), np.zeros((17, 8), np.float32), np.zeros((2, 5), np.float32),
                np.array([[2, 0, 0, 0, 0, 0, 0, 0]], np.float32), np.array([[0, np.nan, 0, 0, 0, 0, 0, 0]], np.float32),
                np.array([[0, 0, 0, 0, -1, 0, 0, 0]], np.float32), np.array([[1, 0, np.inf, 0, 0, 0, 0, 0]], np.float32)):
        with pytest.raises(ValueError, match="light rows"):
            al.light_rows(bad)


def test_ball_offsets():
    import analytic_lights as al
    one = al.ball_offsets(1, 5)
    assert one.shape == (5, 1, 3) and one.dtype == np.float32 and not one.any()
    for S, K in ((2, 1), (16, 4), (64, 64)):
        t = al.ball_offsets(S, K)
        assert t.shape == (K, S, 3) and t.dtype == np.float32 and np.isfinite(t).all()
        norm = np.sqrt((t.astype(np.float64) ** 2).sum(-1))
        assert norm.max() <= 1.0 and norm.max() > 0.5
        assert np.array_equal(_bits(t), _bits(al.ball_offsets(S, K)))  # a pure function of its arguments
        assert len(np.unique(t.reshape(-1, 3), axis=0)) == S * K
    big = al.ball_offsets(64, 64).astype(np.float64).reshape(-1, 3)
    assert np.abs(big.mean(axis=0)).max() < 0.03 and abs((big ** 2).sum(-1).mean() - 0.6) < 0.03  # a uniform ball: E r^2 = 3/5
    for S, K in ((0, 4), (65, 4), (4, 0), (4, 65)):
        with pytest.raises(ValueError, match="ball_offsets"):
            al.ball_offsets(S, K)


def _case(name):
    if name == "open_box":
        return lr.open_box(4)
    if name == "box":
        return rr.box_interior(4)
    return rr.crease(4)[:3]


@pytest.mark.parametrize("name", ["open_box", "crease", "box"])
def test_restatement_grid_walk_equals_its_brute_force(name):
    import analytic_lights as al
    v, f, _ = _case(name)
    p, n = gr.face_points(v, f)
    if name == "box":  # the closed box is wound outward: look inward, where the walls block what comes from outside
        n = -n
    rows, _ = al.pack(sh.lights_for(v))
    mask =(np.arange(len(p)) % 5 != 0).astype(np.uint8)
    for S in (1, 16):
        table = al.ball_offsets(S, 4)
        a = sh.shadow_points(p, n, v, f, rows, table, seed=3, mask=mask)
        b = sh.shadow_points(p, n, v, f, rows, table, seed=3, mask=mask, brute=False)
        assert np.array_equal(a["lit"], b["lit"]) and np.array_equal(_bits(a["visibility"]), _bits(b["visibility"]))
        assert sh.counters(a) == sh.counters(b) and np.array_equal(a["ray_blocked"], b["ray_blocked"])
        live = int(mask.sum())
        assert a["masked"] == len(p) - live and a["no_normal"] == 0 and a["rays"] + a["below_horizon"] == live * 3 * S
        assert 0 < a["blocked"] < a["rays"] and a["below_horizon"] > 0, (name, S)
        assert (a["lit"][mask == 0] == S).all() and (a["visibility"][mask == 0] == 1).all()
        # one cell: the walk IS a brute force (the default bias follows the grid's box: pin it)
        c = sh.shadow_points(p, n, v, f, rows, table, seed=3, mask=mask, cell=1e6 * a["grid"]["cell"], brute=False, bias=a["bias"])
        assert tuple(int(x) for x in c["grid"]["G"]) == (1, 1, 1) and np.array_equal(c["lit"], a["lit"])


def test_restatement_known_answers():
    import analytic_lights as al
    v, f, _ = lr.open_box(4)
    top = float(v.max())
    floor = np.array([[0.5 * top, 0.5 * top, 0.0]], np.float32)
    up = np.array([[0.0, 0.0, 1.0]], np.float32)
    one = al.ball_offsets(1, 4)
    above = al.pack([dict(kind="point", position=[0.5 * top, 0.5 * top, 2.0 * top])])[0]
    beside = al.pack([dict(kind="point", position=[3.0 * top, 0.5 * top, 0.5 * top])])[0]
    under = al.pack([dict(kind="point", position=[0.5 * top, 0.5 * top, -1.0 * top]), dict(kind="directional", direction=[0, 0, 1])])[0]
    a = sh.shadow_points(floor, up, v, f, above, one)
    assert a["visibility"][0, 0] == 1 and sh.counters(a) == (1, 0, 0, 0, 0)
    b = sh.shadow_points(floor, up, v, f, beside, one)
    assert b["visibility"][0, 0] == 0 and sh.counters(b) == (1, 1, 0, 0, 0)
    c = sh.shadow_points(floor, up, v, f, under, one)
    assert not c["visibility"].any() and sh.counters(c) == (0, 0, 2, 0, 0)
    # a light exactly at the ray's origin: d = 0 is below the horizon
    at = al.pack([dict(kind="point", position=[float(x) for x in floor[0]])])[0]
    d = sh.shadow_points(floor, up, v, f, at, one, bias=0.0)
    assert d["visibility"][0, 0] == 0 and sh.counters(d) == (0, 0, 1, 0, 0)


def _generator():
    spec = importlib.util.spec_from_file_location("make_lights_golden", os.path.join(ROOT, "tests", "golden", "make_lights_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_bsdf_fixture_keeps_its_conditions():
    gen = _generator()
    z = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 512 * 1024
    N, L = z["points"].shape[0], z["light_rows"].shape[0]
    assert N >= 2048 and L == 4 and z["want"].shape == (N, L, 3) and z["want"].dtype == np.float64
    assert sorted(set(z["light_rows"][:, 0].tolist())) == [0.0, 1.0]
    # the inputs are the generator's, so the stored results are results of THESE inputs
    for k, x in zip(("points", "normals", "albedo", "roughness", "metallic"), gen.inputs()):
        assert np.array_equal(_bits(z[k]), _bits(x)), k
    assert np.array_equal(z["light_rows"], gen.LIGHT_ROWS) and np.array_equal(z["campos"], gen.CAMPOS)
    # coverage: normals over the whole sphere, the ends of the roughness range and values below min_roughness, metallic
    # over [0, 1], grazing and back-facing lights
    n = z["normals"].astype(np.float64)
    assert np.abs((n ** 2).sum(1) - 1).max() < 2.0 ** -10
    assert all(((n * np.array(s)) > 0.3).all(axis=1).any() for s in [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)])
    r, m = z["roughness"], z["metallic"]
    assert (r == 0).sum() >= 64 and (r == 1).sum() >= 64 and ((r > 0) & (r < 0.08)).sum() >= 64 and r.min() >= 0 and r.max() <= 1
    assert (m == 0).any() and (m == 1).any() and m.min() >= 0 and m.max() <= 1 and ((m > 0.25) & (m < 0.75)).sum() > N // 4
    wi = gen.incident(z["points"], z["light_rows"], __import__("torch").float64).numpy()
    cos = (n[:, None, :] * wi).sum(-1)
    assert ((cos > 0) & (cos < 0.05)).sum() >= 100 and (cos < -0.5).sum() >= 100 and (cos > 0.5).sum() >= 100
    # the band: at most 1 % of the pairs, re-derived from the stored inputs
    out = gen.excluded(z["points"], z["normals"], z["light_rows"], z["campos"])
    assert out.shape == (N, L) and float(out.mean()) <= float(z["band_cap"]) == 0.01
    assert float(z["band"]) == 1e-5 and float(z["floor"]) == 1e-3
    want = z["want"]
    assert np.isfinite(want).all() and (want >= 0).all() and float(want.max()) > 1.0
    # both terms carry the cosine; in front of a surface that is not a pure metal the Lambert term is never 0
    assert (want[cos < 0] == 0).all() and (want[(cos > 1e-3) & (m[:, None] < 1)] > 0).all()
    assert 1e-6 < float(z["ref32_err"]) < 1e-2
    # the project's text of the formulas, in float64 on the CPU, is the reference's: 1e-12 apart at most by the floor measure
    rows, campos = z["light_rows"], z["campos"]
    total = np.zeros_like(want)
    for l in range(L):
        one = np.ones((1, 3), np.float32)
        d, s = sh.shade_lights(z["points"], z["normals"], z["albedo"], r, m, campos, rows[l:l + 1], one, dtype=__import__("torch").float64)
        v = rows[l, 1:4].astype(np.float64) - z["points"].astype(np.float64)
        scale = (v * v).sum(1, keepdims=True) if rows[l, 0] == 0 else 1.0
        total[:, l] = (d + s) * scale
    err = np.abs(total - want) / np.maximum(np.abs(want), float(z["floor"]))
    print("the restated formulas in float64 against the reference's: largest error %.3g; in float32: %.3g (ref32_err %.3g)" % (
        float(err[~out].max()), _float32_error(z, out), float(z["ref32_err"])))
    assert float(err[~out].max()) <= 1e-12


def _float32_error(z, out):
    """The restatement evaluated in float32 by torch on the CPU: what an independent float32 evaluation is off by."""
    rows, want = z["light_rows"], z["want"]
    total = np.zeros_like(want)
    for l in range(len(rows)):
        d, s = sh.shade_lights(z["points"], z["normals"], z["albedo"], z["roughness"], z["metallic"], z["campos"], rows[l:l + 1],
                               np.ones((1, 3), np.float32))
        v = rows[l, 1:4].astype(np.float64) - z["points"].astype(np.float64)
        scale = (v * v).sum(1, keepdims=True) if rows[l, 0] == 0 else 1.0
        total[:, l] = (d.astype(np.float64) + s.astype(np.float64)) * scale
    err = np.abs(total - want) / np.maximum(np.abs(want), float(z["floor"]))
    return float(err[~out].max())


def test_tool_arguments():
    import relight_scene
    import render_mesh
    base = ["-m", "o", "--mesh", "m.ply", "--hdri", "a.hdr"]
    a = render_mesh.parse_args(base)
    assert (a.lights, a.shadow_samples, a.no_shadows) == (None, 1, False) and render_mesh._check(a) == 0
    a = render_mesh.parse_args(["-m", "o", "--mesh", "m.obj", "--checkpoint", "c.pth", "--lights", "l.json", "--shadow_samples", "16"])
    assert (a.lights, a.shadow_samples, a.no_shadows) == ("l.json", 16, False) and render_mesh._check(a) == 0
    a = render_mesh.parse_args(base + ["--lights", "l.json", "--no_shadows"])
    assert a.no_shadows is True and render_mesh._check(a) == 0
    for argv in (base + ["--shadow_samples", "4"], base + ["--no_shadows"], base + ["--lights", "l.json", "--shadow_samples", "0"],
                 base + ["--lights", "l.json", "--shadow_samples", "65"]):
        with pytest.raises(ValueError, match="lights|shadow_samples"):
            render_mesh._check(render_mesh.parse_args(argv))
    base = ["-m", "o", "--checkpoint", "c.pth", "--hdri", "a.hdr"]
    a = relight_scene.parse_args(base)
    assert (a.lights, a.shadow_samples) == (None, 1) and relight_scene.check_lights(a) is False
    a = relight_scene.parse_args(base + ["--lights", "l.json"])
    assert relight_scene.check_lights(a) is True and relight_scene.check_occluder(a) is False
    a = relight_scene.parse_args(base + ["--lights", "l.json", "--occluder", "m.ply", "--shadow_samples", "8", "--ray_bias", "0.01"])
    assert relight_scene.check_lights(a) is True and relight_scene.check_occluder(a) is True and a.shadow_samples == 8
    for argv in (base + ["--shadow_samples", "4"], base + ["--lights", "l.json", "--shadow_samples", "4"],
                 base + ["--lights", "l.json", "--occluder", "m.ply", "--shadow_samples", "100"]):
        with pytest.raises(ValueError, match="lights|shadow_samples|occluder"):
            relight_scene.check_lights(relight_scene.parse_args(argv))
