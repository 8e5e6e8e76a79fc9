"""GPU: analytic lights and their ray-traced shadows (csrc/mesh_shadow.hip through mesh.shadow_points, csrc/shade_lights.hip
through analytic_lights.shade_lights, mesh_render.RaytracedLight.shadows, analytic_lights.AnalyticRelighter, render_mesh.py and
relight_scene.py --lights).  The shadows against their numpy restatement (tests/mesh_shadow_ref.py, a brute force over all
faces): lit and the counters by array_equal, visibility as bit patterns -- float64 + - * / without contraction, so there is
no tolerance.  The any-hit walk against the nearest-hit kernel on the same rays.  The float32 shade against the reference's
bsdf_pbr in float64 (tests/golden/lights_bsdf.npz) within 4 x the error of the reference's own float32 evaluation.

Figures of the shade against the fixture, measured on an MI355X (2048 points x 4 lights, no pair in the band):
ref32_err 1.27e-4, bound 5.09e-4, the kernel's worst error 1.89e-4 (the test prints it)."""
import functools
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import helpers
import mesh_clean_ref as cr
import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
import mesh_shadow_ref as sh
from mesh_raycast_ref import _dot

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K = 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _rho(V, seed=3):
    import mesh_distance_ref as dr
    return dr.uniform(seed, np.arange(3 * V, dtype=np.uint64), 1).astype(np.float32).reshape(V, 3)


def _mesh(v, f, normals, rho=None):
    import mesh
    v = _dev(np.asarray(v, np.float32).reshape(-1, 3))
    f = _dev(np.asarray(f, np.int32).reshape(-1, 3))
    z1 = torch.zeros(v.shape[0], device=DEV)
    albedo = torch.zeros_like(v) if rho is None else _dev(np.asarray(rho, np.float32))
    return mesh.Mesh(v, f, _dev(np.asarray(normals, np.float32).reshape(-1, 3)), albedo, z1 + 0.5, z1.clone())


@functools.lru_cache(maxsize=None)
def _blob():
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    assert (int(m.vertices.shape[0]), int(m.faces.shape[0])) == (980, 1944)
    return m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices, faces, normals, every: the stride of the faces whose centroids are the points).  Read-only."""
    if name == "open_box":
        return lr.open_box(4) + (1,)
    if name == "box":
        return rr.box_interior(4) + (1,)
    if name == "crease":
        return rr.crease(4)[:3] + (1,)
    return _blob() + (8,)


@functools.lru_cache(maxsize=None)
def _points(name):
    """The face centroids of a case with unit face normals, every 5th masked, and three that get no rays: a NaN position, a
    zero normal and a normal of length 1.01.  -> (points, normals, mask uint8).  Read-only."""
    v, f, _, every = _case(name)
    p, n = gr.face_points(v, f, every)
    p, n = p.copy(), n.copy()
    mask = (np.arange(len(p)) % 5 != 0).astype(np.uint8)
    p[1, 0] = np.nan
    n[2] = 0.0
    n[3] = n[3] * np.float32(1.01)
    return p, n, mask


def _grid(m, v, f, scale=1.0):
    """The device grid at `scale` times the restatement's default cell, and that cell."""
    import mesh
    cell = float(np.float32(rr.build_grid(v, f)["cell"] * scale))
    return mesh.triangle_grid(m, cell)


def _compare(what, visibility, lit, report, want):
    got = lit.cpu().numpy()
    print("%s: %d x %d, lit differs at %d, visibility bit patterns that differ %d; counters %s, restated %s" % (
        what, got.shape[0], got.shape[1], int((got != want["lit"]).sum()), int((_bits(visibility) != _bits(want["visibility"])).sum()),
        sh.counters(report), sh.counters(want)))
    assert lit.dtype == torch.int32 and visibility.dtype == torch.float32
    assert np.array_equal(got, want["lit"]) and np.array_equal(_bits(visibility), _bits(want["visibility"]))
    assert sh.counters(report) == sh.counters(want)


# ---- 1: the restatement -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated(name, S, bias, max_distance):
    """The restatement of a case, computed once.  -> (rows, want).  Read-only."""
    import analytic_lights as al
    v, f, _, _ = _case(name)
    p, n, mask = _points(name)
    entries = sh.lights_for(v)
    if name == "open_box":  # a fourth light exactly at the origin of point 7's rays: d = 0, below the horizon
        o = p[7].astype(np.float64) + bias * n[7].astype(np.float64)
        assert (o == o.astype(np.float32).astype(np.float64)).all()
        entries.append(dict(kind="point", position=[float(x) for x in o], radius=0.0))
    rows, _ = al.pack(entries)
    return rows, sh.shadow_points(p, n, v, f, rows, al.ball_offsets(S, K), bias=bias, max_distance=max_distance, seed=5, mask=mask)


def _bias(name):
    v = _case(name)[0]
    return float(2.0 ** -7 * (v.max() - v.min()))


@pytest.mark.parametrize("name,S,max_distance", [("open_box", 1, None), ("open_box", 16, None), ("crease", 1, None), ("crease", 16, None),
                                                  ("blob", 1, None), ("blob", 16, None), ("open_box", 1, "short")])
def test_shadow_points_equals_the_restatement(name, S, max_distance):
    import mesh
    v, f, n, _ = _case(name)
    p, pn, mask = _points(name)
    extent = float(v.max() - v.min())
    if max_distance == "short":  # the directional light's blocked rays of the open box meet a wall at t >= 0.27 extents
        max_distance = 0.2 * extent
    bias = _bias(name)
    rows, want = _restated(name, S, bias, max_distance)
    m = _mesh(v, f, n)
    args = dict(samples=S, rotations=K, bias=bias, max_distance=max_distance, seed=5, mask=_dev(mask))
    visibility, lit, report = mesh.shadow_points(_dev(p), _dev(pn), m, rows, grid=_grid(m, v, f), **args)
    assert json.loads(json.dumps(report)) == report
    L, N = len(rows), len(p)
    assert (report["n"], report["lights"], report["samples"], report["rotations"], report["seed"]) == (N, L, S, K, 5)
    assert report["bias"] == bias and report["max_distance"] == max_distance
    _compare("%s S=%d max_distance=%s" % (name, S, max_distance), visibility, lit, report, want)
    assert report["masked"] == (N + 4) // 5 and report["no_normal"] == 3
    assert report["rays"] + report["below_horizon"] == L * S * (N - report["masked"] - 3)
    assert 0 < report["blocked"] < report["rays"] and report["below_horizon"] > 0
    dead = (mask == 0) | np.isin(np.arange(N), (1, 2, 3))
    assert (lit.cpu().numpy()[dead] == S).all() and (visibility.cpu().numpy()[dead] == 1).all()
    if name == "open_box":  # the light at point 7's origin is dark there, without a ray
        assert int(lit[7, 3]) == 0 and float(visibility[7, 3]) == 0
    if max_distance is not None:  # a finite distance turns shadows of the directional light into light
        _, free = _restated(name, S, bias, None)
        sun = 2
        assert (visibility[:, sun].cpu().numpy() >= free["visibility"][:, sun]).all()
        assert float(visibility[:, sun].sum()) > float(free["visibility"][:, sun].sum()) and report["blocked"] < free["blocked"]
        assert np.array_equal(_bits(visibility[:, :2]), _bits(free["visibility"][:, :2]))  # the point lights have t_max = 1
    # the grid does not show: cells of 0.5 and 3 times the default; nor does the order of the points
    for scale in (0.5, 3.0):
        vis2, lit2, rep2 = mesh.shadow_points(_dev(p), _dev(pn), m, rows, grid=_grid(m, v, f, scale), **args)
        assert torch.equal(lit2, lit) and np.array_equal(_bits(vis2), _bits(visibility)) and sh.counters(rep2) == sh.counters(report), scale
    import analytic_lights as al
    lit3, vis3 = torch.full_like(lit, -1), torch.full_like(visibility, -1.0)
    counts = mesh._shadow_points(_dev(p), _dev(pn), m, _grid(m, v, f), rows, al.ball_offsets(S, K), 5, bias, max_distance, _dev(mask),
                                 lit3, vis3, sort=False)
    assert torch.equal(lit3, lit) and np.array_equal(_bits(vis3), _bits(visibility))
    assert tuple(int(x) for x in counts.cpu()) == sh.counters(report) + (0,)


# ---- 2: any hit = nearest hit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open_box", "blob"])
def test_any_hit_equals_nearest_hit(name):
    """Rays that float32 holds exactly: origins and point lights on a lattice of 2^-10 of the extent, bias 0, one sample at
    the light's centre, so that mesh.raycast can be given the very rays (o, d, t_max) shadow_points casts."""
    import analytic_lights as al
    import mesh
    v, f, n, every = _case(name)
    extent = float(2.0 ** math.ceil(math.log2(float(v.max() - v.min()))))
    q = extent * 2.0 ** -10
    p, pn = gr.face_points(v, f, max(1, every // 4))
    o = (np.round((p.astype(np.float64) + 0.01 * extent * pn) / q) * q).astype(np.float32)
    centre = np.round(0.5 * (v.max(axis=0) + v.min(axis=0)).astype(np.float64) / q) * q
    entries = [dict(kind="point", position=list(centre + np.array([0.125, -0.0625, 0.25]) * extent)),
               dict(kind="point", position=list(centre + np.array([-1.5, 0.25, 0.5]) * extent)),
               dict(kind="directional", direction=[-0.3, 0.2, -1.0])]
    rows, _ = al.pack(entries)
    m = _mesh(v, f, n)
    grid = _grid(m, v, f)
    max_distance = 0.75 * extent
    visibility, lit, report = mesh.shadow_points(_dev(o), _dev(pn), m, rows, samples=1, rotations=K, bias=0.0, max_distance=max_distance,
                                                 grid=grid)
    lit = lit.cpu().numpy()
    total = 0
    for l in range(3):
        if rows[l, 0] == 0:
            d64, t_max = rows[l, 1:4].astype(np.float64) - o.astype(np.float64), 1.0
        else:
            d64, t_max = np.broadcast_to(-rows[l, 1:4].astype(np.float64), o.shape), max_distance
        d = d64.astype(np.float32)
        assert np.array_equal(d.astype(np.float64), d64)  # the very rays
        cast = _dot(d64, pn.astype(np.float64)) > 0
        _, face, _, rep = mesh.raycast(_dev(o), _dev(d), m, t_max=t_max, grid=grid)
        found = face.cpu().numpy() >= 0
        differ = int((found[cast] != (lit[cast, l] == 0)).sum())
        print("%s light %d: %d rays, nearest-hit finds %d faces, any-hit reports %d blocked, they differ at %d" % (
            name, l, int(cast.sum()), int(found[cast].sum()), int((lit[cast, l] == 0).sum()), differ))
        assert differ == 0 and (lit[~cast, l] == 0).all()  # below the horizon: dark without a ray
        total += int(found[cast].sum())
    assert report["blocked"] == total and 0 < total < report["rays"] and report["no_normal"] == 0


# ---- 3: known answers ----------------------------------------------------------------------------------------------------------
def test_known_answers():
    import analytic_lights as al
    import mesh
    v, f, n, _ = _case("open_box")
    m = _mesh(v, f, n)
    top = float(v.max())
    floor = _dev(np.array([[0.5 * top, 0.5 * top, 0.0], [0.25 * top, 0.625 * top, 0.0]], np.float32))
    up = _dev(np.array([[0.0, 0.0, 1.0]] * 2, np.float32))
    point = lambda x, y, z, **kw: dict(kind="point", position=[x * top, y * top, z * top], **kw)  # noqa: E731
    # a point light above the opening reaches the floor; beside a wall outside the box it does not
    vis, lit, rep = mesh.shadow_points(floor, up, m, al.parse_lights([point(0.5, 0.5, 2.0)]))
    assert (vis == 1).all() and (lit == 1).all() and sh.counters(rep) == (2, 0, 0, 0, 0)
    vis, lit, rep = mesh.shadow_points(floor, up, m, al.parse_lights([point(3.0, 0.5, 0.5)]))
    assert (vis == 0).all() and (lit == 0).all() and sh.counters(rep) == (2, 2, 0, 0, 0)
    # a light on the far side of the tangent plane: dark, and no ray is cast
    vis, lit, rep = mesh.shadow_points(floor, up, m, al.parse_lights([point(0.5, 0.5, -1.0), dict(kind="directional", direction=[0, 0, 1])]))
    assert (vis == 0).all() and sh.counters(rep) == (0, 0, 4, 0, 0)
    # inside the closed box with the light outside: dark
    v, f, n, _ = _case("box")
    box = _mesh(v, f, n)
    inside = np.random.default_rng(2).uniform(0.2, 0.8, size=(21, 3)).astype(np.float32) * float(v.max())
    towards = np.array([3.0, 0.5, 0.5]) * float(v.max()) - inside
    towards = (towards / np.linalg.norm(towards, axis=1, keepdims=True)).astype(np.float32)
    vis, lit, rep = mesh.shadow_points(_dev(inside), _dev(towards), box, al.parse_lights([dict(kind="point", position=[3.0 * float(v.max()), 0.5 * float(v.max()), 0.5 * float(v.max())])]),
                                       samples=16, rotations=K)
    assert (vis == 0).all() and sh.counters(rep) == (21 * 16, 21 * 16, 0, 0, 0)
    # a sphere light half hidden by the top edge of the crease's wall: a penumbra, and the restatement's
    v, f, n, _ = _case("crease")
    size = float(v.max())
    crease = _mesh(v, f, n)
    p = np.array([[0.5 * size, 0.5 * size, 0.0]], np.float32)
    light = [dict(kind="point", position=[-0.5 * size, 0.5 * size, 2.0 * size], radius=0.15 * size)]
    vis, lit, rep = mesh.shadow_points(_dev(p), _dev(np.array([[0.0, 0.0, 1.0]], np.float32)), crease, al.parse_lights(light),
                                       samples=16, rotations=K, bias=1e-3 * size, seed=1)
    want = sh.shadow_points(p, np.array([[0.0, 0.0, 1.0]], np.float32), v, f, al.pack(light)[0], al.ball_offsets(16, K), bias=1e-3 * size, seed=1)
    print("the half-hidden sphere light: %d of 16 samples arrive" % int(lit[0, 0]))
    assert 0 < int(lit[0, 0]) < 16 and 0.0 < float(vis[0, 0]) < 1.0
    _compare("penumbra", vis, lit, rep, want)


def test_empty_and_refused_inputs():
    import analytic_lights as al
    import mesh
    v, f, n, _ = _case("open_box")
    m = _mesh(v, f, n)
    lights = al.parse_lights(sh.lights_for(v))
    e3 = torch.zeros((0, 3), device=DEV)
    vis, lit, rep = mesh.shadow_points(e3, e3, m, lights, samples=4)
    assert tuple(vis.shape) == tuple(lit.shape) == (0, 3) and sh.counters(rep) == (0,) * 5 and rep["dims"] == [0, 0, 0]
    up = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 1, 1]], np.int32)):
        flat = _mesh(np.zeros((3, 3), np.float32), faces, np.repeat([[0.0, 0.0, 1.0]], 3, 0))
        sun = al.parse_lights([dict(kind="directional", direction=[0, 0, -1])])
        vis, lit, rep = mesh.shadow_points(_dev(np.ones((4, 3), np.float32)), _dev(up), flat, sun, mask=_dev(np.array([1, 1, 0, 1], np.uint8)))
        assert vis[:, 0].tolist() == [1.0, 1.0, 1.0, 0.0] and lit[:, 0].tolist() == [1, 1, 1, 0]
        assert sh.counters(rep) == (1, 0, 1, 1, 1) and rep["pairs"] == 0 and rep["dims"] == [0, 0, 0]
    p, pn, _ = _points("open_box")
    ok, okn = _dev(np.nan_to_num(p)), _dev(pn)
    rows = al.pack(lights)[0]
    bad_rows = rows.copy()
    bad_rows[1, 2] = np.inf
    for bad in (dict(lights=[]), dict(lights=list(lights) * 6), dict(lights=rows[:0]), dict(lights=np.tile(rows, (6, 1))), dict(lights=bad_rows),
                dict(samples=0), dict(samples=65), dict(rotations=0), dict(rotations=65), dict(bias=-1.0), dict(bias=float("nan")),
                dict(max_distance=-1.0), dict(max_distance=float("inf")), dict(mask=torch.zeros(len(p), device=DEV)),
                dict(mask=torch.zeros(3, dtype=torch.uint8, device=DEV))):
        with pytest.raises(ValueError):
            mesh.shadow_points(ok, okn, m, **dict(dict(lights=lights), **bad))
    for a, b in ((ok[:, :2], okn), (ok, okn[:5]), (ok.double(), okn)):
        with pytest.raises(ValueError):
            mesh.shadow_points(a, b, m, lights)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.shadow_points(ok.cpu(), okn, m, lights)


# ---- 4: the shade --------------------------------------------------------------------------------------------------------------
def _entries(rows, radiance=None):
    """Light entries that pack to `rows` (extent 0) with the given radiance as the colour."""
    out = []
    for l, r in enumerate(rows):
        colour = [1.0, 1.0, 1.0] if radiance is None else [float(x) for x in radiance[l]]
        where = "position" if r[0] == 0 else "direction"
        out.append({"kind": "point" if r[0] == 0 else "directional", where: [float(x) for x in r[1:4]], "color": colour})
    return out


def test_shade_lights_against_the_reference_bsdf():
    import analytic_lights as al
    z = np.load(os.path.join(ROOT, "tests", "golden", "lights_bsdf.npz"))
    rows, want = z["light_rows"], z["want"]
    assert np.array_equal(al.pack(_entries(rows))[0], rows)  # the unit directions survive the host's normalisation
    p64 = z["points"].astype(np.float64)
    args = [_dev(z[k]) for k in ("points", "normals", "albedo", "roughness", "metallic")] + [_dev(z["campos"])]
    got = np.zeros_like(want)
    for l in range(len(rows)):  # one light at a time with radiance 1: f E, and E undone in float64
        d, s = al.shade_lights(*args, al.parse_lights(_entries(rows[l:l + 1])))
        v = rows[l, 1:4].astype(np.float64) - p64
        scale = (v * v).sum(1, keepdims=True) if rows[l, 0] == 0 else 1.0
        got[:, l] = (d.cpu().numpy().astype(np.float64) + s.cpu().numpy().astype(np.float64)) * scale
    n, wo = z["normals"].astype(np.float64), z["campos"].astype(np.float64) - p64
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    n_wo = (n * wo).sum(1)[:, None]
    wi = np.stack([(rows[l, 1:4] - p64) / np.linalg.norm(rows[l, 1:4] - p64, axis=1, keepdims=True) if rows[l, 0] == 0
                   else np.broadcast_to(-rows[l, 1:4].astype(np.float64), p64.shape) for l in range(len(rows))], 1)
    n_wi = (n[:, None, :] * wi).sum(-1)
    band = float(z["band"])
    out = (np.abs(n_wo - 1e-4) < band) | (np.abs(n_wi - 1e-4) < band) | (np.abs(n_wi) < band)
    assert float(out.mean()) <= 0.01
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-3)
    worst, bound = float(err[~out].max()), 4.0 * float(z["ref32_err"])
    print("shade_lights against bsdf_pbr in float64: %d pairs, %d left out, worst error %.4g, ref32_err %.4g, bound %.4g" % (
        out.size, int(out.sum()), worst, float(z["ref32_err"]), bound))
    assert worst <= bound
    # all four lights in one call: the float32 sums in light order of the four calls above
    radiance = np.array([[1.0, 0.5, 2.0], [3.0, 1.0, 0.25], [0.5, 0.75, 1.0], [2.0, 2.0, 0.125]], np.float32)
    lights = al.parse_lights(_entries(rows, radiance))
    d4, s4 = al.shade_lights(*args, lights)
    dsum, ssum = torch.zeros_like(d4), torch.zeros_like(s4)
    for l in range(len(rows)):
        d, s = al.shade_lights(*args, lights[l:l + 1])
        dsum, ssum = dsum + d, ssum + s
    assert np.array_equal(_bits(d4), _bits(dsum)) and np.array_equal(_bits(s4), _bits(ssum)) and float(s4.max()) > 0.1
    # a back-facing light gives exact zeros; so does a visibility of 0, and 0.5 halves
    back = n_wi[:, 2] < 0
    d, s = al.shade_lights(*args, lights[2:3])
    assert back.sum() > 500 and not d[_dev(back)].any() and not s[_dev(back)].any() and float(d[_dev(~back)].min()) >= 0
    N = len(p64)
    vis = torch.ones((N, 4), device=DEV)
    vis[:, 1] = 0.0
    vis[:, 3] = 0.5
    dv, sv = al.shade_lights(*args, lights, visibility=vis)
    d0, s0 = al.shade_lights(*args, lights[0:1])
    d2, s2 = al.shade_lights(*args, lights[2:3])
    d3, s3 = al.shade_lights(*args, al.parse_lights(_entries(rows[3:4], 0.5 * radiance[3:4])))
    assert np.array_equal(_bits(dv), _bits(d0 + d2 + d3)) and np.array_equal(_bits(sv), _bits(s0 + s2 + s3))
    # masked points and points without a unit normal get zeros
    mask = torch.ones(N, dtype=torch.uint8, device=DEV)
    mask[::3] = 0
    nrm = args[1].clone()
    nrm[1] = 0.0
    nrm[4] *= 1.01
    pts = args[0].clone()
    pts[7, 1] = float("nan")
    dm, sm = al.shade_lights(pts, nrm, *args[2:], lights, mask=mask)
    dead = (mask == 0)
    dead[[1, 4, 7]] = True
    assert not dm[dead].any() and not sm[dead].any() and np.array_equal(_bits(dm[~dead]), _bits(d4[~dead]))
    assert not torch.isnan(dm).any() and not torch.isnan(sm).any()
    for bad in (dict(points=args[0].double()), dict(normals=args[1][:5]), dict(roughness=args[3][:, None]), dict(visibility=vis[:, :3]),
                dict(mask=torch.ones(N, device=DEV))):
        kw = dict(points=args[0], normals=args[1], albedo=args[2], roughness=args[3], metallic=args[4], campos=args[5], lights=lights)
        with pytest.raises(ValueError):
            al.shade_lights(**dict(kw, **bad))
    with pytest.raises(RuntimeError, match="no CPU path"):
        al.shade_lights(args[0].cpu(), *args[1:], lights)
    e3 = torch.zeros((0, 3), device=DEV)
    d, s = al.shade_lights(e3, e3, e3, e3[:, 0], None, args[5], lights)
    assert tuple(d.shape) == tuple(s.shape) == (0, 3)


def test_lambert_known_answer():
    """Normal +z, metallic 0 (None), roughness 1, the camera below the horizon (no specular), a point light of intensity I at
    height h straight above: diffuse = albedo I / (pi h^2), to float32 rounding.  Pins pi and the inverse square."""
    import analytic_lights as al
    albedo = np.array([[0.8, 0.5, 0.25], [1.0, 0.125, 0.6]], np.float32)
    p = np.array([[0.25, -0.5, 0.0], [0.25, -0.5, 0.0]], np.float32)
    up = np.array([[0.0, 0.0, 1.0]] * 2, np.float32)
    for I, h in ((1.0, 1.0), (7.5, 2.0), (3.0, 0.375)):
        light = al.parse_lights([dict(kind="point", position=[0.25, -0.5, h], intensity=I)])
        d, s = al.shade_lights(_dev(p), _dev(up), _dev(albedo), _dev(np.ones(2, np.float32)), None, _dev(np.array([1.0, 1.0, -2.0], np.float32)), light)
        want = albedo.astype(np.float64) * I / (math.pi * h * h)
        err = np.abs(d.cpu().numpy().astype(np.float64) - want) / want
        print("Lambert I=%g h=%g: largest relative error %.3g" % (I, h, float(err.max())))
        assert float(err.max()) <= 4 * 2.0 ** -24 and not s.any()  # four float32 roundings: E, kd cos / pi (two), the product
        # seen from above there is a specular term as well, and a directional light of the same radiance at the point is I / pi
        d2, s2 = al.shade_lights(_dev(p), _dev(up), _dev(albedo), _dev(np.ones(2, np.float32)), None, _dev(np.array([1.0, 1.0, 2.0], np.float32)), light)
        assert np.array_equal(_bits(d2), _bits(d)) and float(s2.min()) > 0
    sun = al.parse_lights([dict(kind="directional", direction=[0, 0, -2], intensity=2.0)])
    d, _ = al.shade_lights(_dev(p), _dev(up), _dev(albedo), _dev(np.ones(2, np.float32)), None, _dev(np.array([1.0, 1.0, -2.0], np.float32)), sun)
    assert np.abs(d.cpu().numpy().astype(np.float64) - albedo.astype(np.float64) * 2.0 / math.pi).max() <= 4 * 2.0 ** -24


# ---- 5: in the image -----------------------------------------------------------------------------------------------------------
IW, IH = 32, 24


def _camera():
    import scenes
    cam = scenes.look_at_camera((1.9, 0.35, 1.7), (0.4, 0.5, 0.3), IW, IH, 0.9)
    return {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}, cam


def _image_lights():
    return [dict(kind="point", position=[0.6, 0.4, 0.9], color=[1.0, 0.9, 0.8], intensity=1.5, radius=0.05),
            dict(kind="point", position=[-0.8, 0.5, 0.4], intensity=2.0),
            dict(kind="directional", direction=[-0.4, 0.3, -1.0], color=[0.5, 0.6, 1.0], intensity=0.8, angle=2.0)]


def _tilted(v, n):
    """The unit-size mesh turned about the centre of [0, 1]^3 (20 degrees about x, then 15 about z): the G-buffer masks a pixel
    whose world normal has a zero component (gigs_gbuffer_post, the reference's rule), which is every pixel of an
    axis-aligned box."""
    a, b = math.radians(20.0), math.radians(15.0)
    Rx = np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Rz = np.array([[math.cos(b), -math.sin(b), 0], [math.sin(b), math.cos(b), 0], [0, 0, 1]])
    R = Rz @ Rx
    return ((v.astype(np.float64) - 0.5) @ R.T + 0.5).astype(np.float32), (n.astype(np.float64) @ R.T).astype(np.float32)


@pytest.mark.parametrize("name,S", [("crease", 1), ("open_box", 16)])
def test_shadows_and_relighter_in_the_image(name, S):
    import analytic_lights as al
    import mesh_render
    import scenes
    if name == "crease":
        v, f, n, _ = rr.crease(4, 1.0)
    else:
        v, f, n = lr.open_box()
    v, n = _tilted(v, n)
    m = _mesh(v, f, n, 0.25 + 0.5 * _rho(len(v)))
    lights = al.parse_lights(_image_lights())
    L = len(lights)
    cam, cam_np = _camera()
    gi = scenes.GI_DEFAULTS
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, mesh_render.RaytracedLight(m, rotations=K, seed=6, bias=0.05, device=DEV) as tracer:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        visibility, points, normals, mask, rep = tracer.shadows(o["pos"], o["normal"], cam["viewmatrix"], cover, lights, S)
        assert json.loads(json.dumps(rep)) == rep and tuple(visibility.shape) == (L, IH, IW)
        n_cover = int(cover.sum())
        assert 100 < n_cover < IW * IH and rep["masked"] == IW * IH - n_cover and rep["n"] == IW * IH and rep["samples"] == S
        assert torch.equal(mask.reshape(IH, IW).bool(), cover) and (visibility[:, ~cover] == 1).all()
        # the restatement fed the prepared arrays
        want = sh.shadow_points(points.cpu().numpy(), normals.cpu().numpy(), v, f, al.pack(lights)[0], al.ball_offsets(S, K), bias=0.05,
                                seed=6, mask=mask.cpu().numpy())
        flat = visibility.reshape(L, -1).t()
        print("%s image: visibility bit patterns that differ %d; counters %s, restated %s" % (
            name, int((_bits(flat) != _bits(want["visibility"])).sum()), sh.counters(rep), sh.counters(want)))
        assert np.array_equal(_bits(flat), _bits(want["visibility"])) and sh.counters(rep) == sh.counters(want)
        assert 0 < rep["blocked"] < rep["rays"]
        # the relighter over the mesh's G-buffer: its planes are shade_lights called by hand on the prepared arrays
        source = mesh_render.MeshGBuffer(gi)
        for trace in (tracer, None):
            rl = al.AnalyticRelighter(lights, source, tracer=trace, samples=S, gamma=True)
            assert rl.replayable is False
            out = rl(cam, rast)
            b = source(cam, rast)
            if trace is not None:
                vis, pts, nrm, mk, r = tracer.shadows(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], lights, S, normal_space="view")
                hand_vis = vis.reshape(L, -1).t().contiguous()
                assert out["report"] == dict(r, shadows=True)
            else:
                pts, nrm, mk = tracer.prepare(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], "view")
                vis, hand_vis = torch.ones((L, IH, IW), device=DEV), None
                assert out["report"]["shadows"] is False
            d, s = al.shade_lights(pts, nrm, b["albedo_map"].reshape(3, -1).t().contiguous(), b["roughness_map"].reshape(-1), None,
                                   cam["campos"], lights, hand_vis, mk)
            plane = lambda x: x.t().reshape(3, IH, IW)  # noqa: E731
            assert torch.equal(out["shadow"], vis) and torch.equal(out["lights_diffuse"], plane(d)) and torch.equal(out["lights_specular"], plane(s))
            from pipeline import linear_to_srgb
            assert torch.equal(out["lights_rgb"], linear_to_srgb((plane(d) + plane(s)).clamp(0.0, 1.0)))
            covered = b["mask_u8"] != 0
            assert 100 < int(covered.sum()) < IW * IH
            assert (out["lights_rgb"][:, ~covered] == 0).all() and (out["shadow"][:, ~covered] == 1).all()
            assert float(out["lights_rgb"].max()) > 0.05 and float(out["lights_rgb"].max()) <= 1.0
            linear = al.AnalyticRelighter(lights, source, tracer=trace, samples=S, gamma=False)(cam, rast)
            assert torch.equal(linear["lights_rgb"], (plane(d) + plane(s)).clamp(0.0, 1.0))
        with pytest.raises(ValueError, match="samples"):
            al.AnalyticRelighter(lights, source, samples=65)
        with pytest.raises(TypeError, match="tracer"):
            al.AnalyticRelighter(lights, source, tracer=rast)


def test_relighter_over_splats():
    import analytic_lights as al
    import mesh_render
    import relight
    import scenes
    import mesh_raster_ref as raster_ref
    RW, RH = 64, 48
    sphere = dict(raster_ref.sphere_mesh()[0])
    sphere["normals"] = (sphere["vertices"] / np.linalg.norm(sphere["vertices"], axis=1, keepdims=True)).astype(np.float32)
    m = mesh_render.device_mesh(sphere, DEV)
    gi = scenes.GI_DEFAULTS
    sc, cam = helpers.small_scene(P=300, sh_degree=1, W=RW, H=RH)
    g = {k: _dev(sc[k]) for k in helpers.GAUSS_KEYS}
    cam = {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}
    lights = al.parse_lights([dict(kind="point", position=[0.5, 1.0, 2.5], intensity=6.0, radius=0.1),
                              dict(kind="directional", direction=[0.2, -0.3, -1.0], intensity=0.7)])
    with mesh_render.RaytracedLight(m, rotations=K, bias=0.05, device=DEV) as tracer:
        for metallic in (False, True):
            source = relight.SplatGBuffer(gi, 1, metallic=metallic)
            out = al.AnalyticRelighter(lights, source, tracer=tracer, samples=4, gamma=False)(cam, g)
            out = {k: (x.clone() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}
            b = source(cam, g)
            vis, pts, nrm, mk, r = tracer.shadows(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], lights, 4, normal_space="view")
            d, s = al.shade_lights(pts, nrm, b["albedo_map"].reshape(3, -1).t().contiguous(), b["roughness_map"].reshape(-1),
                                   b["metallic_map"].reshape(-1) if metallic else None, cam["campos"], lights,
                                   vis.reshape(2, -1).t().contiguous(), mk)
            plane = lambda x: x.t().reshape(3, RH, RW)  # noqa: E731
            assert torch.equal(out["shadow"], vis) and torch.equal(out["lights_diffuse"], plane(d)) and torch.equal(out["lights_specular"], plane(s))
            assert torch.equal(out["lights_rgb"], (plane(d) + plane(s)).clamp(0.0, 1.0)) and out["report"] == dict(r, shadows=True)
            covered = b["mask_u8"] != 0
            assert 0 < int(covered.sum()) <= RW * RH and r["masked"] == int((~covered).sum())  # the splats' padded normals cover the frame
            assert (out["lights_rgb"][:, ~covered] == 0).all() and (out["shadow"][:, ~covered] == 1).all() and float(out["lights_rgb"].max()) > 0


# ---- 6: tools ------------------------------------------------------------------------------------------------------------------
def _report_is_finite(x):
    if isinstance(x, dict):
        return all(_report_is_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_report_is_finite(v) for v in x)
    return x is None or isinstance(x, (str, bool)) or math.isfinite(x)


def test_tools(tmp_path):
    import analytic_lights as al
    import densify
    import optim
    import relight
    import relight_scene
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    import train_iteration as ti
    from PIL import Image
    v, f, n = _blob()
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=1, size=32)
    out = str(tmp_path / "run")
    os.makedirs(out)
    scene_io.save_mesh_ply(os.path.join(out, "blob.ply"), *_mesh(v, f, n, 0.25 + 0.5 * _rho(len(v))))
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    centre, extent = 0.5 * (v.max(axis=0) + v.min(axis=0)), float((v.max(axis=0) - v.min(axis=0)).max())
    entries = [dict(kind="point", position=[float(x) for x in centre + np.array([0.0, 0.0, 2.0]) * extent], intensity=6.0 * extent * extent,
                    radius=0.1 * extent), dict(kind="directional", direction=[0.3, -0.2, -1.0], color=[1.0, 0.8, 0.6], angle=1.0)]
    lights_json = str(tmp_path / "lights.json")
    with open(lights_json, "w") as fh:
        json.dump(entries, fh)
    base = ["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--split", "train"]
    folder = os.path.join(out, "mesh_train")
    plain = render_mesh.render_mesh(base)
    before = sorted(os.listdir(folder))
    assert not any("_lights" in x or "_shadow_" in x or x == "lights_report.json" for x in before) and "lights_report_json" not in plain
    # --lights: an image and a shadow plane per light and view, and the report; the files of the plain run are what they were
    res = render_mesh.render_mesh(base + ["--lights", lights_json, "--shadow_samples", "4", "--ray_bias", "0.01"])
    assert json.loads(json.dumps(res)) == res and res["files"] == plain["files"]
    added = sorted(set(os.listdir(folder)) - set(before))
    names = sorted(x[:-len("_albedo.png")] for x in before if x.endswith("_albedo.png"))
    assert len(names) == 2
    assert added == sorted(["lights_report.json"] + ["%s_lights.png" % x for x in names] + ["%s_shadow_%d.png" % (x, l) for x in names for l in (0, 1)])
    assert sorted(res["lights_files"]) == sorted(os.path.join(folder, x) for x in added if x.endswith(".png"))
    for x in names:
        img = np.array(Image.open(os.path.join(folder, "%s_lights.png" % x)))
        shadow = np.array(Image.open(os.path.join(folder, "%s_shadow_1.png" % x)))
        assert img.shape[:2] == (32, 32) and int(img.max()) > 0 and shadow.shape[:2] == (32, 32) and int(shadow.max()) == 255
        assert int(shadow.min()) < 255  # the blob shades itself from the directional light
    with open(res["lights_report_json"]) as fh:
        rep = json.load(fh)
    assert res["lights_report_json"] == os.path.join(folder, "lights_report.json") and _report_is_finite(rep)
    assert all(np.array_equal(x, y) for x, y in zip(al.pack(rep["lights"]), al.pack(entries))) and rep["shadows"] is True and rep["shadow_samples"] == 4
    assert [x["image_name"] for x in rep["views"]] == names
    for view in rep["views"]:
        assert view["n"] == 32 * 32 and view["lights"] == 2 and view["samples"] == 4 and view["bias"] == 0.01 and view["shadows"] is True
        assert all(isinstance(view[k], int) for k in sh.COUNTERS) and 0 < view["blocked"] < view["rays"]
    # --no_shadows: no shadow planes, and the report says so
    for x in added:
        os.remove(os.path.join(folder, x))
    res = render_mesh.render_mesh(base + ["--lights", lights_json, "--no_shadows"])
    added = sorted(set(os.listdir(folder)) - set(before))
    assert added == sorted(["lights_report.json"] + ["%s_lights.png" % x for x in names])
    with open(res["lights_report_json"]) as fh:
        rep = json.load(fh)
    assert rep["shadows"] is False and all(view["shadows"] is False for view in rep["views"]) and _report_is_finite(rep)
    bad_json = str(tmp_path / "bad.json")
    with open(bad_json, "w") as fh:
        json.dump([dict(kind="point", position=[0, 0])], fh)
    for bad, match in ((base + ["--shadow_samples", "4"], "lights"), (base + ["--no_shadows"], "lights"),
                       (base + ["--lights", lights_json, "--shadow_samples", "65"], "shadow_samples"),
                       (base + ["--lights", lights_json, "--ray_bias", "-1"], "ray_bias"), (base + ["--lights", bad_json], "position")):
        with pytest.raises(ValueError, match=match):
            render_mesh.render_mesh(bad)
    # relight_scene.py --lights: unshadowed without --occluder, shadowed with it
    g = ti.raw_from_scene(scenes.surface_scene(P=2000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [g[k]], "lr": 0.0, "name": k} for k in g], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(64, 128)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, g, densify.DensifyState(g["xyz"].shape[0], DEV), opt, 1.0), light.state_dict(), {}, 7)
    common = ["-m", out, "--checkpoint", ck, "--hdri", hdr, "--skip_train"]
    folder = os.path.join(out, "test", "ours_7", "relight")
    a = relight_scene.relight_scene(common)
    before = sorted(os.listdir(folder))
    assert "analytic_lights" not in a["test"] and not any("_lights" in x or "_shadow_" in x for x in before)
    b = relight_scene.relight_scene(common + ["--lights", lights_json])
    assert json.loads(json.dumps(b)) == b and b["test"]["files"] == a["test"]["files"]
    added = sorted(set(os.listdir(folder)) - set(before))
    assert len(added) == 2 and added[0] == "lights_report.json" and added[1].endswith("_lights.png")
    assert b["test"]["analytic_lights"]["shadows"] is False and b["test"]["analytic_lights"]["files"] == [os.path.join(folder, added[1])]
    with open(b["test"]["analytic_lights"]["report_json"]) as fh:
        rep = json.load(fh)
    assert rep["shadows"] is False and rep["occluder"] is None and _report_is_finite(rep) and len(rep["views"]) == 1
    assert int(np.array(Image.open(os.path.join(folder, added[1]))).max()) > 0
    c = relight_scene.relight_scene(common + ["--lights", lights_json, "--occluder", "blob.ply", "--shadow_samples", "2", "--ray_bias", "0.02"])
    added = sorted(set(os.listdir(folder)) - set(before))
    image_name = added[1][:-len("_lights.png")]
    assert added == sorted(["lights_report.json", image_name + "_lights.png", image_name + "_shadow_0.png", image_name + "_shadow_1.png"])
    with open(c["test"]["analytic_lights"]["report_json"]) as fh:
        rep = json.load(fh)
    assert rep["shadows"] is True and rep["occluder"] == "blob.ply" and rep["shadow_samples"] == 2 and _report_is_finite(rep)
    assert rep["views"][0]["n"] == 32 * 32 and rep["views"][0]["samples"] == 2 and rep["views"][0]["bias"] == 0.02
    assert c["test"]["occluder"]["rays"] == 64  # --occluder still traces the occlusion, as before
    for bad, match in ((common + ["--shadow_samples", "4"], "lights"), (common + ["--lights", lights_json, "--shadow_samples", "4"], "occluder"),
                       (common + ["--lights", lights_json, "--occluder", "blob.ply", "--shadow_samples", "0"], "shadow_samples"),
                       (common + ["--lights", bad_json], "position")):
        with pytest.raises(ValueError, match=match):
            relight_scene.relight_scene(bad)
