"""CPU restatement of ray-traced reflections per point (csrc/mesh_reflect.hip through mesh.reflect_points and
mesh_render.compose_reflections), as include/gigs_hip.h states it under "Ray-traced reflections per point": the table of GGX
half vectors, the level of a roughness, the masked, no_normal and no_view rules, the rays of a point (the frame and rotation
of mesh_light_ref.hemispheres, the view mirrored about each half vector), the traversal (mesh_raycast_ref.raycast), the
classification, the contribution of a miss (mesh_light_ref.sky_texel) and of a front hit with the weights rounded to
float32, the weighted per-lane sums in ascending chunk order and their butterfly (mesh_gather_ref._butterfly); the compose in
numpy float32; prepare_views.  Every expression is written in the header's operation order, so every output is the kernel's
bit for bit."""
import math

import numpy as np

import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_raycast_ref as rr
from mesh_raycast_ref import _corners, _cross, _dot, build_grid

WAVE = 64
COUNTERS = ("misses", "front_hits", "back_hits", "below_horizon", "no_normal", "no_view", "masked")
OUTPUTS = ("specular", "reflected", "visibility")


def counters(report):
    return tuple(report[k] for k in COUNTERS)


# ---- the table ---------------------------------------------------------------------------------------------------------------
def ggx_table(R, K, L):
    """[L,K,R,3] float32: GGX half vectors, z the normal.  Level l: alpha = ((l + 1/2) / L)^2; point i: u = (i + 1/2) / R,
    cos^2 = (1 - u) / (1 + (alpha^2 - 1) u), azimuth i golden + 2 pi k / K."""
    i = np.arange(R, dtype=np.float64)
    u = (i + 0.5) / R
    alpha = ((np.arange(L, dtype=np.float64) + 0.5) / L) ** 2
    cos2 = (1.0 - u)[None, :] / (1.0 + (alpha[:, None] ** 2 - 1.0) * u[None, :])
    z, r = np.sqrt(cos2), np.sqrt(1.0 - cos2)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    phi = i[None, :] * golden + (2.0 * math.pi * np.arange(K, dtype=np.float64) / K)[:, None]
    return np.stack([r[:, None, :] * np.cos(phi)[None], r[:, None, :] * np.sin(phi)[None],
                     np.broadcast_to(z[:, None, :], (L, K, R))], -1).astype(np.float32)


def level_of(roughness, L):
    """min(L - 1, floor(r L)) in float64 on the float32 roughness; a NaN or a negative product gives 0."""
    r = np.asarray(roughness, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.floor(r * float(L))
        return np.where(~(t >= 0.0), 0.0, np.where(t > float(L - 1), float(L - 1), t)).astype(np.int64)


# ---- the trace ---------------------------------------------------------------------------------------------------------------
def rays_of(points, normals, views, roughness, table, seed):
    """-> dict(p, n, v [N,3] float64, ok_normal, ok_view [N], level, rotation [N], l [N,R,3] (the ray directions), w [N,R] (n.l),
    live [N,R] (vh > 0 and w > 0)).  Rows of a dead point are whatever the expressions give and are not used."""
    table = np.asarray(table, np.float32)
    L, K, R = table.shape[:3]
    p, n, ok_normal, rot, _ = lr.hemispheres(points, normals, table[0], seed)
    v = np.asarray(views, np.float32).reshape(-1, 3).astype(np.float64)
    lev = level_of(np.asarray(roughness, np.float32).reshape(-1), L)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        vv = _dot(v, v)
        ok_view = np.isfinite(v).all(axis=1) & (vv >= 1.0 - rr.NORMAL_BAND) & (vv <= 1.0 + rr.NORMAL_BAND)
        T, B = rr.frame(n)
        rows = table[lev, rot].astype(np.float64)  # [N,R,3]
        x, y, z = rows[..., 0:1], rows[..., 1:2], rows[..., 2:3]
        h = (x * T[:, None, :] + y * B[:, None, :]) + z * n[:, None, :]
        vh = _dot(v[:, None, :], h)
        l = (2.0 * vh)[..., None] * h - v[:, None, :]
        w = _dot(n[:, None, :], l)
        live = (vh > 0.0) & (w > 0.0)
    return dict(p=p, n=n, v=v, ok_normal=ok_normal, ok_view=ok_view, level=lev, rotation=rot, l=l, w=w, live=live)


def reflect_points(points, normals, views, roughness, vertices, faces, table, sky=None, radiosity=None, max_distance=None,
                   bias=None, seed=0, mask=None, cell=None, grid=None):
    """-> dict(specular, reflected [N,3] float32 or None (no sky), visibility [N] float32, valid, blocked [N] int32, the
    seven counters, bias, grid).  bias defaults as mesh_raycast_ref.bake_defaults; max_distance None is no limit.  With no
    usable face nothing is traced and no ray is counted."""
    table = np.asarray(table, np.float32)
    R = table.shape[2]
    q = rays_of(points, normals, views, roughness, table, seed)
    N = len(q["p"])
    live_pt = np.ones(N, bool) if mask is None else np.asarray(mask).reshape(N) != 0
    g = build_grid(vertices, faces, cell) if grid is None else grid
    bias = rr.bake_defaults(g, None, bias)[1]
    tmax = np.inf if max_distance is None else float(max_distance)
    no_normal = live_pt & ~q["ok_normal"]
    no_view = live_pt & q["ok_normal"] & ~q["ok_view"]
    rows = np.nonzero(live_pt & q["ok_normal"] & q["ok_view"])[0]
    visibility = np.ones(N, np.float32)
    valid, blocked = np.zeros(N, np.int32), np.zeros(N, np.int32)
    specular = reflected = None
    if sky is not None:
        sky = np.asarray(sky, np.float32)
        specular, reflected = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    miss_n = front_n = back_n = below_n = 0
    if len(rows) and g is not None:
        n_rows = len(rows)
        use = q["live"][rows]  # [n,R]
        flat = np.nonzero(use.reshape(-1))[0]
        dd = q["l"][rows].reshape(-1, 3)[flat]
        o = np.broadcast_to((q["p"][rows] + bias * q["n"][rows])[:, None, :], (n_rows, R, 3)).reshape(-1, 3)[flat]
        got = rr.raycast(o, dd, vertices, faces, tmax, grid=g)
        f = got["face"].astype(np.int64)
        hit = f >= 0
        _, P = _corners(vertices, faces)
        Pf = P[np.maximum(f, 0)]
        s = _dot(dd, _cross(Pf[:, 1] - Pf[:, 0], Pf[:, 2] - Pf[:, 0]))
        front = hit & (s < 0)
        c = np.zeros((len(dd), 3), np.float64)
        if sky is not None:
            cf, iy, ix = lr.sky_texel(dd, sky.shape[1])
            miss = ~hit
            c[miss] = sky[cf[miss], iy[miss], ix[miss]].astype(np.float64)
            if radiosity is not None and front.any():
                Q = np.asarray(radiosity, np.float32).reshape(-1, 3).astype(np.float64)
                tri = np.asarray(faces, np.int64).reshape(-1, 3)[f[front]]
                b = got["bary"][front].astype(np.float64)  # float32(w1 / W), float32(w2 / W)
                b1, b2 = b[:, 0:1], b[:, 1:2]
                b0 = np.maximum(0.0, (1.0 - b1) - b2)
                c[front] = (b0 * Q[tri[:, 0]] + b1 * Q[tri[:, 1]]) + b2 * Q[tri[:, 2]]
        # per ray [n,R]: kind -1 below the horizon, 0 a miss, 1 a front hit, 2 a back hit; w is 0 below the horizon
        kind = np.full(n_rows * R, -1, np.int64)
        kind[flat] = np.where(hit, np.where(front, 1, 2), 0)
        w = np.zeros(n_rows * R, np.float64)
        w[flat] = q["w"][rows].reshape(-1)[flat]
        wc = np.zeros((n_rows * R, 3), np.float64)
        wc[flat] = w[flat, None] * c
        kind, w, wc = kind.reshape(n_rows, R), w.reshape(n_rows, R), wc.reshape(n_rows, R, 3)
        # the kernel adds +0.0 where a term does not apply; the sums start at +0.0, so the bits are the same
        S = gr._butterfly(wc, R)
        S_front = gr._butterfly(np.where((kind == 1)[..., None], wc, 0.0), R)
        Wm = gr._butterfly(np.stack([w, np.where(kind == 0, w, 0.0), np.zeros_like(w)], -1), R)
        W, W_miss = Wm[:, 0], Wm[:, 1]
        some = W > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            visibility[rows] = np.where(some, W_miss / W, 1.0).astype(np.float32)
            if sky is not None:
                specular[rows] = np.where(some[:, None], S / W[:, None], 0.0).astype(np.float32)
                reflected[rows] = np.where(some[:, None], S_front / W[:, None], 0.0).astype(np.float32)
        valid[rows] = (kind >= 0).sum(axis=1)
        blocked[rows] = (kind >= 1).sum(axis=1)
        miss_n, front_n, back_n, below_n = (int((kind == k).sum()) for k in (0, 1, 2, -1))
    return dict(specular=specular, reflected=reflected, visibility=visibility, valid=valid, blocked=blocked, misses=miss_n,
                front_hits=front_n, back_hits=back_n, below_horizon=below_n, no_normal=int(no_normal.sum()),
                no_view=int(no_view.sum()), masked=int((~live_pt).sum()), bias=float(bias), grid=g)


# ---- the compose (float32) -----------------------------------------------------------------------------------------------------
def compose(normals, views, roughness, radiance, lut, albedo=None, metallic=None, mask=None, visibility=None):
    """gigs_reflect_compose in numpy float32, every product and sum rounded on its own.  lut [h,w,2] float32."""
    f = np.float32
    n, v = np.asarray(normals, f).reshape(-1, 3), np.asarray(views, f).reshape(-1, 3)
    r, rad = np.asarray(roughness, f).reshape(-1), np.asarray(radiance, f).reshape(-1, 3)
    lut = np.asarray(lut, f)
    lut = lut.reshape(lut.shape[-3], lut.shape[-2], 2)
    h, w = lut.shape[:2]
    nov = np.minimum(np.maximum((n[:, 1] * v[:, 1] + n[:, 2] * v[:, 2]) + n[:, 0] * v[:, 0], f(1e-4)), f(1.0))
    fu, fv = nov * f(w) - f(0.5), r * f(h) - f(0.5)
    flu, flv = np.floor(fu), np.floor(fv)
    tu, tv = fu - flu, fv - flv
    x0, x1 = np.clip(flu.astype(np.int64), 0, w - 1), np.clip(flu.astype(np.int64) + 1, 0, w - 1)
    y0, y1 = np.clip(flv.astype(np.int64), 0, h - 1), np.clip(flv.astype(np.int64) + 1, 0, h - 1)
    one = f(1.0)
    w00, w10, w01, w11 = (one - tu) * (one - tv), tu * (one - tv), (one - tu) * tv, tu * tv
    fg = ((lut[y0, x0] * w00[:, None] + lut[y0, x1] * w10[:, None]) + lut[y1, x0] * w01[:, None]) + lut[y1, x1] * w11[:, None]
    assert fg.dtype == f
    if metallic is None:
        F0 = np.full((len(n), 3), f(0.04), f)
    else:
        m = np.asarray(metallic, f).reshape(-1, 1)
        F0 = (one - m) * f(0.04) + np.asarray(albedo, f).reshape(-1, 3) * m
    refl = F0 * fg[:, 0:1] + fg[:, 1:2]
    sp = rad if visibility is None else rad * np.asarray(visibility, f).reshape(-1, 1)
    out = sp * refl
    assert out.dtype == f
    if mask is not None:
        out = np.where((np.asarray(mask).reshape(-1) != 0)[:, None], out, f(0.0))
    return out


def prepare_views(points, campos):
    """mesh_render.prepare_views in numpy float64 -> [N,3] float64, NOT rounded."""
    p = np.asarray(points, np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(campos, np.float32).astype(np.float64).reshape(3)
    d = [c[i] - p[:, i] for i in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return np.stack([d[i] / length for i in range(3)], 1)


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------
def hash_views(normals, seed=23, below_every=11):
    """[N,3] float32 unit views from a counter hash on the upper hemisphere about each normal (cosine of the polar angle
    uniform in [0.05, 1)); every `below_every`-th is mirrored below it.  A normal that gives no finite view gets (0, 0, 1)."""
    import mesh_distance_ref as dr
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    N = len(n)
    i = np.arange(N, dtype=np.uint64)
    z = 0.05 + 0.95 * dr.uniform(seed, i, 0)
    phi = 2.0 * math.pi * dr.uniform(seed, i, 1)
    s = np.sqrt(1.0 - z * z)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        T, B = rr.frame(n)
        z = np.where(np.arange(N) % below_every == below_every - 1, -z, z)
        v = (s * np.cos(phi))[:, None] * T + (s * np.sin(phi))[:, None] * B + z[:, None] * n
        v = v / np.sqrt((v ** 2).sum(axis=1, keepdims=True))
    v[~np.isfinite(v).all(axis=1)] = (0.0, 0.0, 1.0)
    return v.astype(np.float32)


def hash_roughness(N, seed=29):
    """[N] float32 in [0, 1) from a counter hash; the last entries are the boundary values 0, 1, NaN, -1, 2, 0.25, 0.5."""
    import mesh_distance_ref as dr
    r = dr.uniform(seed, np.arange(N, dtype=np.uint64), 3).astype(np.float32)
    edge = np.array([0.0, 1.0, np.nan, -1.0, 2.0, 0.25, 0.5], np.float32)
    k = min(N, len(edge))
    r[N - k:] = edge[:k]  # at the END: the first points of the shared sets are the dead ones
    return r
