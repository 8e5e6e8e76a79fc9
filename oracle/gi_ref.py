"""NumPy float64 restatement of the screen-space GI passes, reporting every DECISION it takes.

*** TEST INFRASTRUCTURE ONLY *** (like oracle/gigs_oracle.cpp, whose orc_depth_to_normal / orc_ssao / orc_ssr / orc_median3x3 /
orc_bilateral3x3 it restates in float64).  Reference lines: R = submodules/diff-gaussian-rasterization/cuda_rasterizer.

  ray_table(delta)        the ray set of SSAOCUDA / SSRCUDA (R/forward.cu:679-681, 796-797) as csrc/gi.hip::get_ray_table
                          builds it: fp32 loop accumulation of phi and theta, sinf / cosf in fp32, the live rays first in
                          loop order and the identical zero-weight rays behind them.  The table is input data: the ray index
                          of `march` is the ray index of the recorded hit list (gigs_ssr_hits).
  march(...)              A7 / A8's march (R/forward.cu:679-716, 796-829; get_coord R/ssr.h:119-135): per (pixel, ray) the
                          outcome -- hit at step j on pixel q / left the image at step j / ran out of steps -- and the
                          margins of that outcome in pixels, depth and on the projection's denominator.
  ssao(...), ssr(...)     the sums over a set of hits (R/forward.cu:690, 711, 718-723; 824-909, fresnelSchlick R/ssr.h:13-16)
                          with the sum of |terms| a summation bound needs; `ssr` takes ANY hit set, float64's or a kernel's.
  depth_to_normal(...)    A6 (R/forward.cu:914-1032) with the early-out every pixel took.
  median3x3, bilateral3x3 the build's definition of the kornia filters (oracle/gigs_oracle.cpp).

Inputs are the fp32 values the kernels receive (settings included: bias = float32(0.01)); everything after is float64.
Non-finite inputs follow the oracle's conventions (saturating float -> int, roundf(NaN) -> pixel 0, comparisons with NaN
false); pixels whose frame or position is not finite are flagged (`nonfinite`) and get no float64 "decisions".

`mut` names ONE deliberate error (MUTATIONS): the tests use them to show that the cases tell a wrong march from a right one.
"""
import ctypes
import ctypes.util

import numpy as np

MISS, HIT, LEFT, NONFINITE = 0, 1, 2, 3
EDGES = ("x_low", "x_high", "y_low", "y_high")
MUTATIONS = ("lt_for_le", "bias_thick_swapped", "continue_on_leaving", "start_plus_1", "step_minus_1_end", "floor_for_round",
             "w_for_w_minus_1", "no_1e-7", "scale_once", "radius_over_step_minus_1", "weight_cos", "ssr_over_sum_w",
             "ssao_over_count", "kd_without_metallic", "a6_pad_1", "a6_centre_only")
F32 = np.float32
PI_F = F32(3.14159265358979323846)
EPS_DEN = float(F32(0.0000001))
DEPTH_THRESH = float(F32(0.01))


def _libm():
    lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for f in (lib.sinf, lib.cosf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return lib


_RAYS = {}


def ray_table(delta):
    """dict: ts [n,3], cos, sin, w [n] (fp32 values as float64), n, n_live, n_dead, sum_w (fp32, loop order), loop_index [n]"""
    key = float(F32(delta))
    if key in _RAYS:
        return _RAYS[key]
    m = _libm()
    sample_delta = F32(delta) * PI_F
    rows, sum_w = [], F32(0)
    phi = F32(0)
    while float(phi) < 2.0 * float(PI_F):
        theta = F32(0)
        while float(theta) <= 0.5 * float(PI_F):
            ct, st = F32(m.cosf(float(theta))), F32(m.sinf(float(theta)))
            tx, ty, tz = st * F32(m.cosf(float(phi))), st * F32(m.sinf(float(phi))), ct
            inv = F32(1) / np.sqrt(F32(F32(tx * tx + ty * ty) + tz * tz))
            w = ct * st
            sum_w = F32(sum_w + w)
            rows.append((F32(tx * inv), F32(ty * inv), F32(tz * inv), ct, st, w))
            theta = F32(float(theta) + float(sample_delta) * 0.5)
        phi = F32(phi + sample_delta)
    a = np.array(rows, np.float64)
    dead = np.flatnonzero((a[:, 4] == 0) & (a[:, 5] == 0) & (a[:, 0] == 0) & (a[:, 1] == 0))
    if len(dead) and not (np.all(a[dead, 2] == a[dead[0], 2]) and np.all(a[dead, 3] == a[dead[0], 3])):
        dead = dead[:0]
    live = np.setdiff1d(np.arange(len(a)), dead)
    order = np.concatenate([live, dead])
    a = a[order]
    t = dict(ts=a[:, :3].copy(), cos=a[:, 3].copy(), sin=a[:, 4].copy(), w=a[:, 5].copy(), n=len(a), n_live=len(live),
             n_dead=len(dead), sum_w=float(sum_w), loop_index=order)
    _RAYS[key] = t
    return t


def _normalize(v):
    """R/vec_math.h:538-541: v * (1 / sqrt(dot)); 0 -> NaN as 0 * inf"""
    with np.errstate(all="ignore"):
        return v * (1.0 / np.sqrt((v * v).sum(-1, keepdims=True)))


def frames(normal, pos):
    """[N,3] float64 tangent, bitangent, normal of R/forward.cu:660-677 and the pixels whose frame or position is not finite"""
    n = _normalize(normal)
    up = np.array([0.0, 1.0, 0.0])
    with np.errstate(all="ignore"):
        t = _normalize(up[None] - n * (n @ up)[:, None])
        b = _normalize(np.cross(n, t))
    bad = ~(np.isfinite(t).all(1) & np.isfinite(b).all(1) & np.isfinite(n).all(1) & np.isfinite(pos).all(1))
    return t, b, n, bad


def _f2i_round(t, floor=False):
    """f2i(roundf(t)): half away from zero, NaN -> 0, saturating (kept as float64 integers clipped to the int32 range)"""
    with np.errstate(all="ignore"):
        r = np.floor(t) if floor else np.sign(t) * np.floor(np.abs(t) + 0.5)
    return np.clip(np.where(np.isnan(r), 0.0, r), -2147483648.0, 2147483647.0)


def _coord_margin(t, i, size, out):
    """distance of a projected coordinate to the boundary that decides its pixel: the nearest k + 0.5 inside the image, the
    image's edge (-0.5 / size - 0.5: the same boundary, seen from outside) for a sample that has left"""
    with np.errstate(all="ignore"):
        inside = 0.5 - np.abs(t - i)
        outside = np.where(t < 0, -0.5 - t, t - (size - 0.5))
        m = np.where(out, outside, inside)
    return np.where(np.isnan(m), 0.0, m)


def march(W, H, fx, fy, radius, bias, thick, delta, step, start, normal, pos, mut=None, chunk=1 << 16):
    """normal, pos: [3,H,W] fp32.  Returns per (pixel, ray), [N,R]: outcome (MISS / HIT / LEFT / NONFINITE), step (the sample
    that ended the ray, -1 for a miss), hit_pix (-1 = none), edge (LEFT: index into EDGES), m_px, m_z, m_den (see the module
    text of tests/gi_cases.py), front_then_hit (a sample in front of the surface it landed on, a later one hit), passed_behind
    (a sample more than `thick` behind a surface), den_nonpos (a sample with sp.z + 1e-7 <= 0), hole_missed (a sample on a
    pixel of depth 0 that did not hit); per pixel [N]: nonfinite.
    Rays are marched in chunks of pixels to bound memory."""
    N = W * H
    nrm = np.asarray(normal, np.float64).reshape(3, N).T
    p = np.asarray(pos, np.float64).reshape(3, N).T
    z_plane = p[:, 2].copy()
    radius, bias, thick, fx, fy = (float(F32(v)) for v in (radius, bias, thick, fx, fy))
    if mut == "bias_thick_swapped":
        bias, thick = thick, bias
    tab = ray_table(delta)
    R = tab["n"]
    out = dict(outcome=np.zeros((N, R), np.int8), step=np.full((N, R), -1, np.int32), hit_pix=np.full((N, R), -1, np.int64),
               edge=np.full((N, R), -1, np.int8), m_px=np.full((N, R), np.inf), m_z=np.full((N, R), np.inf),
               m_den=np.full((N, R), np.inf), front_then_hit=np.zeros((N, R), bool), passed_behind=np.zeros((N, R), bool),
               den_nonpos=np.zeros((N, R), bool), hole_missed=np.zeros((N, R), bool))
    t, b, n, bad = frames(nrm, p)
    out["nonfinite"] = bad
    cx, cy = W / 2.0, H / 2.0
    j0 = start + 1 if mut == "start_plus_1" else start
    j1 = step - 1 if mut == "step_minus_1_end" else step
    eps = 0.0 if mut == "no_1e-7" else EPS_DEN
    for c0 in range(0, N, chunk):
        s = slice(c0, min(N, c0 + chunk))
        pc, zc = p[s], p[s, 2]
        ts = tab["ts"]
        with np.errstate(all="ignore"):
            # transformVec3x3(tangentSample, TBN) (R/auxiliary.h:90-98), rows t, b, n
            sv = t[s, None, :] * ts[None, :, 0:1] + b[s, None, :] * ts[None, :, 1:2] + n[s, None, :] * ts[None, :, 2:3]
            a = (1 + zc / 100) if mut == "scale_once" else (1 + zc / 100) * (1 + zc / 100)
            a = a * radius / ((step - 1) if mut == "radius_over_step_minus_1" else step)
        M = pc.shape[0]
        alive = np.ones((M, R), bool)
        front = np.zeros((M, R), bool)
        o = {k: v[s] for k, v in out.items() if k != "nonfinite"}
        for j in range(j0, j1):
            with np.errstate(all="ignore"):
                sp = pc[:, None, :] + sv * (j * a)[:, None, None]  # R/forward.cu:699-702
                den = sp[..., 2] + eps                             # get_coord, R/ssr.h:119-135
                tx = sp[..., 0] / den * fx + cx
                ty = sp[..., 1] / den * fy + cy
            fl = mut == "floor_for_round"
            ix, iy = _f2i_round(tx, fl), _f2i_round(ty, fl)
            xmax = W if mut == "w_for_w_minus_1" else W - 1
            ox, oy = (ix < 0) | (ix > xmax), (iy < 0) | (iy > H - 1)
            outside = ox | oy
            mx, my = _coord_margin(tx, ix, W, ox), _coord_margin(ty, iy, H, oy)
            with np.errstate(all="ignore"):
                # the x test comes first (R/forward.cu:705-706): a ray that has left in x is decided by x alone
                m = np.where(ox, mx, np.where(oy, my, np.minimum(mx, my)))
            m = np.where(np.isnan(m), 0.0, m)
            q = np.clip(iy, 0, H - 1).astype(np.int64) * W + np.clip(ix, 0, xmax).astype(np.int64)
            q = np.minimum(q, N - 1)
            sd = z_plane[q]
            with np.errstate(all="ignore"):
                hi, lo = sp[..., 2] + bias, sp[..., 2] - thick
                h = ((sd < hi) & (sd > lo)) if mut == "lt_for_le" else ((sd <= hi) & (sd >= lo))
                mz = np.minimum(np.abs(sd - hi), np.abs(sd - lo))
            # the ray's own pixel at j = 0: sp is pos itself, no arithmetic lies between sampleDepth and sp.z
            own = (j == 0) & (q == (np.arange(s.start, s.stop)[:, None]))
            mz = np.where(np.isnan(mz) | own, np.inf, mz)
            h &= ~outside
            ev = alive
            o["m_px"][ev] = np.minimum(o["m_px"][ev], m[ev])
            evz = alive & ~outside
            o["m_z"][evz] = np.minimum(o["m_z"][evz], mz[evz])
            with np.errstate(all="ignore"):
                # the denominator's margin: over the samples at or behind the camera plane
                behind = ev & ~(sp[..., 2] > 0)
                o["m_den"][behind] = np.minimum(o["m_den"][behind], np.where(np.isnan(den), 0.0, np.abs(den))[behind])
                o["den_nonpos"][ev] |= (den <= 0)[ev]
                o["passed_behind"][evz] |= (sd < lo)[evz]
                o["hole_missed"][evz] |= ((sd == 0) & ~h)[evz]
                landed = alive & h
                o["front_then_hit"][landed] = front[landed]
                front |= evz & (sd > hi)
            leaving = alive & outside
            if mut == "continue_on_leaving":
                leaving &= False
            o["outcome"][landed] = HIT
            o["step"][landed] = j
            o["hit_pix"][landed] = q[landed]
            o["outcome"][leaving] = LEFT
            o["step"][leaving] = j
            o["edge"][leaving] = np.where(ix < 0, 0, np.where(ix > xmax, 1, np.where(iy < 0, 2, 3)))[leaving].astype(np.int8)
            alive = alive & ~landed & ~leaving
            if not alive.any():
                break
        o["outcome"][bad[s]] = NONFINITE
    return out


def decided(m, W, H, max_z):
    """the rays whose outcome no fp32 evaluation of the same lines can change (the margin rule of tests/gi_cases.py)"""
    px, zz = 2.0 ** -19 * max(W, H), 2.0 ** -19 * max_z
    return (m["m_px"] > px) & (m["m_z"] > zz) & (m["m_den"] > zz) & (m["outcome"] != NONFINITE)


def ssao(delta, outcome, mut=None):
    """occlusion [N] of R/forward.cu:690, 711, 718-723 for a hit pattern (outcome == HIT, [N,R]); sum of |terms| [N]"""
    tab = ray_table(delta)
    w = tab["cos"] if mut == "weight_cos" else tab["w"]
    div = float(tab["n"]) if mut == "ssao_over_count" else (float(w.sum()) if mut == "weight_cos" else tab["sum_w"])
    terms = (outcome == HIT) * w[None, :]
    occ = terms.sum(1) / div
    res = np.clip(1.0 - occ, 0.0, 1.0) if div > 0 else np.ones(len(occ))
    return res, np.abs(terms).sum(1) / div


def fresnel(normal, pos, metallic, F0, mut=None):
    """kD [N,3] of R/forward.cu:832-842 (fresnelSchlick R/ssr.h:13-16) and the two clamps' arguments and distances"""
    N_ = _normalize(normal)
    with np.errstate(all="ignore"):
        V = _normalize(-pos)
        ndv = (N_ * V).sum(1)
        cos_t = np.fmax(ndv, EPS_DEN)
        arg = 1.0 - cos_t
        cl = np.fmin(np.fmax(arg, float(F32(0.000001))), 1.0)
        pw = cl ** 5
        F = F0 + (1.0 - F0) * pw[:, None]
        kD = 1.0 - F
        if mut != "kd_without_metallic":
            kD = kD * (1.0 - metallic)[:, None]
    det = dict(ndv=ndv, ndv_clamped=~(ndv >= EPS_DEN), ndv_dist=np.abs(ndv - EPS_DEN), arg=arg,
               arg_clamped=(arg < float(F32(0.000001))) | (arg > 1.0),
               arg_dist=np.minimum(np.abs(arg - float(F32(0.000001))), np.abs(arg - 1.0)))
    return kD, det


def ssr(delta, hit_pix, normal, pos, rgb, albedo, metallic, F0, mut=None):
    """colour, abd [3,N] and the sums of |terms| [3,N] of R/forward.cu:824-909 over the hits hit_pix [N,R] (-1 = no hit): ANY
    hit set, float64's own or the one a kernel recorded.  Planes are [3,H,W] / [1,H,W] fp32."""
    tab = ray_table(delta)
    Npix = hit_pix.shape[0]
    f = lambda a, c: np.asarray(a, np.float64).reshape(c, Npix).T  # noqa: E731
    rgb_, alb, F0_ = f(rgb, 3), f(albedo, 3), f(F0, 3)
    w_cos, w_sin = tab["cos"], (np.ones_like(tab["sin"]) if mut == "weight_cos" else tab["sin"])
    kD, det = fresnel(f(normal, 3), f(pos, 3), f(metallic, 1)[:, 0], F0_, mut)
    n_samples = tab["sum_w"] if mut == "ssr_over_sum_w" else float(tab["n"])
    hitm = hit_pix >= 0
    q = np.where(hitm, hit_pix, 0)
    col, abd, mag = np.zeros((3, Npix)), np.zeros((3, Npix)), np.zeros((3, Npix))
    with np.errstate(all="ignore"):
        for c in range(3):
            terms = np.where(hitm, rgb_[q, c] * w_cos[None, :] * w_sin[None, :], 0.0)  # rgb * cosf(theta) * sinf(theta)
            tail = float(PI_F) / n_samples * kD[:, c]
            abd[c] = terms.sum(1) * tail
            mag[c] = np.abs(np.where(np.isfinite(terms), terms, 0.0)).sum(1) * np.abs(tail)
            col[c] = abd[c] * alb[:, c]
    mag_col = mag * np.abs(alb.T)
    return col, abd, mag_col, mag, det


# ---- A6 and the 3x3 filters --------------------------------------------------------------------------
EARLY = ("none", "border", "depth", "pad")


def depth_to_normal(W, H, fx, fy, viewmatrix, depth, mut=None):
    """A6 (R/forward.cu:914-1032; get_position R/ssr.h:103-117).  Returns normal [3,H,W], depth_pos [3,H,W], early [H,W]
    (index into EARLY) and dist [H,W]: the smallest |d - 0.01| over the depths the pixel's early-out tests read."""
    d = np.asarray(depth, np.float64).reshape(H, W)
    vm = np.asarray(viewmatrix, np.float64).reshape(-1)
    fx, fy = float(F32(fx)), float(F32(fy))
    cx, cy = W / 2.0, H / 2.0
    normal, dpos = np.zeros((3, H, W)), np.zeros((3, H, W))
    early, dist = np.zeros((H, W), np.int8), np.full((H, W), np.inf)
    pad = 1 if mut == "a6_pad_1" else 2

    def gp(x, y):
        dd = d[y, x]
        return np.array([(x - cx) / fx, (y - cy) / fy, 1.0]) * dd

    for y in range(H):
        for x in range(W):
            if x <= 0 or x >= W - 1 or y <= 0 or y >= H - 1:
                early[y, x] = 1
                continue
            dpos[:, y, x] = gp(x, y)
            dist[y, x] = abs(d[y, x] - DEPTH_THRESH)
            if d[y, x] < DEPTH_THRESH:
                early[y, x] = 2
                continue
            skip = False
            if mut != "a6_centre_only":
                for dx in range(-pad, pad + 1):
                    if skip:
                        break
                    if x + dx < 0 or x + dx > W - 1:
                        skip = True
                        break
                    for dy in range(-pad, pad + 1):
                        if y + dy < 0 or y + dy > H - 1:
                            skip = True
                            break
                        dist[y, x] = min(dist[y, x], abs(d[y + dy, x + dx] - DEPTH_THRESH))
                        if d[y + dy, x + dx] < DEPTH_THRESH:
                            skip = True
                            break
            if skip:
                early[y, x] = 3
                continue
            aa, bb, cc, dd_ = gp(x, y - 1), gp(x + 1, y), gp(x, y + 1), gp(x - 1, y)
            ab, bc_, cd, da = gp(x + 1, y - 1), gp(x + 1, y + 1), gp(x - 1, y + 1), gp(x - 1, y - 1)
            ea, eb, ec, ed = da - ab, ab - bc_, bc_ - cd, cd - da
            eac, ebd, ecdab, ebcad = cc - aa, dd_ - bb, ab - cd, da - bc_
            ns = [np.cross(ea, ed), np.cross(ed, ec), np.cross(ec, eb), np.cross(eb, ea), np.cross(eac, ebd), np.cross(ebcad, ecdab)]
            nv = sum(_normalize(v) for v in ns) * (1.0 / 6.0)
            normal[:, y, x] = (vm[0:3] @ nv, vm[4:7] @ nv, vm[8:11] @ nv)
    return normal, dpos, early, dist


def median3x3(x):
    """zero padding, 5th smallest of the 9 taps, NaN-propagating.  Returns (out [C,H,W], tap [C,H,W]: the chosen tap's index
    dy * 3 + dx in 0..8, -1 where the window holds a NaN, and tied [C,H,W]: the median's value occurs more than once)"""
    x = np.asarray(x, np.float64)
    C, H, W = x.shape
    padded = np.zeros((C, H + 2, W + 2))
    padded[:, 1:-1, 1:-1] = x
    taps = np.stack([padded[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], -1)
    nan = np.isnan(taps).any(-1)
    order = np.argsort(np.where(np.isnan(taps), np.inf, taps), -1, kind="stable")
    tap = order[..., 4]
    out = np.take_along_axis(taps, tap[..., None], -1)[..., 0]
    tied = (taps == out[..., None]).sum(-1) > 1
    return np.where(nan, np.nan, out), np.where(nan, -1, tap), tied


def bilateral3x3(x, sigma_color=1.0, sigma_space=(3.0, 3.0)):
    """reflect border, L1 colour distance over the channels, separable Gaussian of the tap offsets (gigs_oracle.cpp)"""
    x = np.asarray(x, np.float64)
    C, H, W = x.shape
    sc, sy, sx = float(F32(sigma_color)), float(F32(sigma_space[0])), float(F32(sigma_space[1]))

    def k1d(s):
        k = np.exp(-np.array([1.0, 0.0, 1.0]) / (2.0 * s * s))
        return k / k.sum()

    ky, kx = k1d(sy), k1d(sx)
    refl = lambda i, n: np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))  # noqa: E731
    ys, xs = np.arange(H), np.arange(W)
    num, den = np.zeros_like(x), np.zeros((H, W))
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = np.clip(refl(ys + dy, H), 0, H - 1), np.clip(refl(xs + dx, W), 0, W - 1)
                t = x[:, yy][:, :, xx]
                dist = np.abs(t - x).sum(0)
                kk = ky[dy + 1] * kx[dx + 1] * np.exp((-0.5 / (sc * sc)) * dist * dist)
                num += t * kk
                den += kk
        return num / den
