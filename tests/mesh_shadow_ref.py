"""CPU restatement of the shadows of analytic lights (csrc/mesh_shadow.hip through mesh.shadow_points), as include/gigs_hip.h
states them under "Shadows of analytic lights": the masked and no_normal rules, the origin and the rotation of a point
(mesh_raycast_ref's), the direction of sample s of a point and of a directional light, the horizon test, and "blocked" as
"the ray has an accepted face within t_max".  The answer is a BRUTE FORCE over all usable faces
(mesh_raycast_ref.brute_force); brute=False walks the grid the way the nearest-hit kernel does (mesh_raycast_ref.raycast): the
CPU tests hold the two against each other, which is the any-hit identity on the host.  Every float64 expression is written
in the header's operation order, so lit, visibility and the counters are the kernel's bit for bit.

shade_lights() restates "Shading under analytic lights" in torch on the CPU, in the dtype it is given: the float64 yardstick
of the shade is the reference's own bsdf_pbr (tests/golden/make_lights_golden.py), this is the project's text of it."""
import math

import numpy as np

import mesh_raycast_ref as rr
from mesh_raycast_ref import _dot, build_grid

COUNTERS = ("rays", "blocked", "below_horizon", "no_normal", "masked")
EPS, MIN_ROUGHNESS = 1e-4, 0.08


def shadow_points(points, normals, vertices, faces, rows, offsets, bias=None, max_distance=None, seed=0, mask=None, cell=None,
                  grid=None, brute=True):
    """rows [L,8] float32 (analytic_lights.pack), offsets [K,S,3] float32 -> dict(lit [N,L] int32, visibility [N,L] float32,
    the five counters, bias, grid, and the rays that were cast: ray_o, ray_d [n,3] float64, ray_tmax [n], ray_blocked [n],
    ray_point, ray_light [n])."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    rows = np.asarray(rows, np.float32).astype(np.float64)
    table = np.asarray(offsets, np.float32).astype(np.float64)
    K, S = table.shape[:2]
    N, L = len(p), len(rows)
    live = np.ones(N, bool) if mask is None else np.asarray(mask).reshape(N) != 0
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = _dot(n, n)
        valid = np.isfinite(p).all(axis=1) & (n2 >= 1.0 - rr.NORMAL_BAND) & (n2 <= 1.0 + rr.NORMAL_BAND)
    g = build_grid(vertices, faces, cell) if grid is None else grid
    if bias is None:
        bias = rr.bake_defaults(g)[1]
    q = np.nonzero(live & valid)[0]
    u = table[rr.rotation_of(seed, q, K)]  # [n,S,3]
    o = p[q] + bias * n[q]
    lit = np.full((N, L), S, np.int32)
    rays = dict(o=[], d=[], tmax=[], blocked=[], point=[], light=[])
    below_n = 0
    for l in range(L):
        c, e = rows[l, 1:4], rows[l, 4]
        if rows[l, 0] == 0:
            d, tmax = (c + e * u) - o[:, None, :], 1.0
        else:
            d, tmax = (-c) + e * u, np.inf if max_distance is None else float(max_distance)
        with np.errstate(invalid="ignore"):
            below = ~(_dot(d, n[q][:, None, :]) > 0)
        below_n += int(below.sum())
        cast = ~below
        oo, dd = np.broadcast_to(o[:, None, :], d.shape)[cast], d[cast]
        got = (rr.brute_force(oo, dd, vertices, faces, tmax) if brute else rr.raycast(oo, dd, vertices, faces, tmax, grid=g))
        blocked = got["face"] >= 0
        assert got["rays_invalid"] == 0
        dark = below.copy()
        dark[cast] = blocked
        lit[q, l] = S - dark.sum(axis=1)
        who = np.broadcast_to(q[:, None], cast.shape)[cast]
        for k, x in (("o", oo), ("d", dd), ("tmax", np.full(len(oo), tmax)), ("blocked", blocked), ("point", who),
                     ("light", np.full(len(oo), l))):
            rays[k].append(x)
    out = dict(lit=lit, visibility=(lit.astype(np.float64) / float(S)).astype(np.float32), below_horizon=below_n,
               no_normal=int((live & ~valid).sum()), masked=int((~live).sum()), bias=float(bias), grid=g)
    for k, x in rays.items():
        out["ray_" + k] = np.concatenate(x) if x else np.zeros(0)
    out["rays"], out["blocked"] = len(out["ray_blocked"]), int(out["ray_blocked"].sum())
    return out


def counters(report):
    return tuple(int(report[k]) for k in COUNTERS)


def shade_lights(points, normals, albedo, roughness, metallic, campos, rows, radiance, visibility=None, mask=None, dtype=None):
    """"Shading under analytic lights" in torch on the CPU -> (diffuse [N,3], specular [N,3]) numpy, in `dtype` (default
    float32)."""
    import torch
    dt = dtype or torch.float32
    t = lambda x: torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float32))).to(dt)  # noqa: E731
    p, n, base, rough = t(points), t(normals), t(albedo), t(roughness)[:, None]
    N, L = len(p), len(rows)
    m = torch.zeros((N, 1), dtype=dt) if metallic is None else t(metallic)[:, None]
    vis = torch.ones((N, L), dtype=dt) if visibility is None else t(visibility)
    rows, radiance = t(rows), t(radiance)
    dot = lambda a, b: (a[:, 0:1] * b[:, 0:1] + a[:, 1:2] * b[:, 1:2]) + a[:, 2:3] * b[:, 2:3]  # noqa: E731
    clamp = lambda c: torch.clamp(c, EPS, 1.0 - EPS)  # noqa: E731
    normalize = lambda v: v / torch.clamp(torch.sqrt(dot(v, v)), min=1e-12)  # noqa: E731
    n2 = dot(n.double(), n.double())[:, 0]
    good = torch.isfinite(p).all(1) & (n2 >= 1.0 - rr.NORMAL_BAND) & (n2 <= 1.0 + rr.NORMAL_BAND)
    if mask is not None:
        good &= torch.from_numpy(np.asarray(mask).reshape(N) != 0)
    ks, kd = 0.04 * (1.0 - m) + base * m, base * (1.0 - m)
    alpha = torch.clamp(rough * rough, MIN_ROUGHNESS * MIN_ROUGHNESS, 1.0)
    a2 = alpha * alpha
    wo = normalize(t(campos)[None, :] - p)
    woN = dot(wo, n)

    def lam(x):
        c = clamp(x)
        return 0.5 * (torch.sqrt(1.0 + a2 * ((1.0 - c * c) / (c * c))) - 1.0)

    diffuse, specular = torch.zeros((N, 3), dtype=dt), torch.zeros((N, 3), dtype=dt)
    for l in range(L):
        if float(rows[l, 0]) == 0:
            v = rows[l, 1:4][None, :] - p
            v2 = dot(v, v)
            wi, E = v / torch.sqrt(v2), radiance[l][None, :] / torch.clamp(v2, min=1e-8)
        else:
            wi, E = (-rows[l, 1:4])[None, :].expand(N, 3), radiance[l][None, :].expand(N, 3)
        wiN = dot(wi, n)
        h = normalize(wo + wi)
        c = clamp(dot(n, h))
        d = (c * a2 - c) * c + 1.0
        D = a2 / (d * d * math.pi)
        G = 1.0 / (1.0 + lam(woN) + lam(wiN))
        f = 1.0 - clamp(dot(wo, h))
        F = ks + (1.0 - ks) * (((f * f) * (f * f)) * f)
        spec = torch.where((woN > EPS) & (wiN > EPS), F * D * G * 0.25 / torch.clamp(woN, min=EPS), torch.zeros_like(F))
        lambert = torch.where(wiN > 0, wiN, torch.zeros_like(wiN)) / math.pi
        w = vis[:, l:l + 1] * E
        diffuse = diffuse + w * (kd * lambert)
        specular = specular + w * spec
    zero = torch.zeros((), dtype=dt)
    return (torch.where(good[:, None], diffuse, zero).numpy(), torch.where(good[:, None], specular, zero).numpy())


def lights_for(vertices):
    """Three lights placed by the mesh's bounding box (lo, extent s): a point light inside it, one outside beside the side
    x = min (behind the crease's wall), one directional.  JSON entries of analytic_lights.parse_lights."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    lo, s = v.min(axis=0), float((v.max(axis=0) - v.min(axis=0)).max())
    at = lambda x, y, z: [float(np.float32(lo[0] + x * s)), float(np.float32(lo[1] + y * s)), float(np.float32(lo[2] + z * s))]  # noqa: E731
    return [dict(kind="point", position=at(0.4, 0.55, 0.6), color=[1.0, 0.9, 0.8], intensity=2.0 * s * s, radius=0.1 * s),
            dict(kind="point", position=at(-0.7, 0.45, 0.3), intensity=3.0 * s * s, radius=0.15 * s),
            dict(kind="directional", direction=[-0.3, 0.2, -1.0], color=[0.5, 0.6, 1.0], intensity=1.5, angle=4.0)]
