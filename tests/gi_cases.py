"""Shared cases for the per-ray / per-pixel float64 checks of the screen-space GI passes (tests/test_gi_f64_cpu.py,
tests/test_gpu_gi_f64.py, tests/golden/make_gi_f64_bounds.py): csrc/gi.hip ssao_kernel, ssr_kernel (march, hit list),
csrc/ssr_apply.hip ssr_apply_kernel, csrc/normal_filters.hip depth_to_normal_kernel, median3x3(_bwd)_kernel,
bilateral3x3_kernel, derive_normal_fused_kernel.

A march case is an ANALYTIC G-buffer -- planes meeting in concave corners, a free-standing slab in front of them (depth edges
that rays pass behind), a floor at a grazing angle, holes (pos = 0, normal = 0), patches of NaN normals, of normals exactly
(0, -1, 0) (the NaN tangent frame) and of normals that engage the two Fresnel clamps -- with the GI settings it is marched
with, built so that it ENTERS the branches it is there for: `Case.needs` declares their minimum populations,
`populations()` measures them from the decisions the float64 restatement reports (oracle/gi_ref.march) and
`check_populations()` fails when a case has silently stopped entering one.  Plane normals are tilted well off (0, +-1, 0):
the tangent up - n (n.up) cancels there and fp32 loses the frame.

The margin rule.  A ray is DECIDED when no fp32 evaluation of the same lines can change its outcome:
  * pixels: every projected coordinate it evaluated is more than 2^-19 max(W, H) from the rounding boundary that decides it
    (k + 0.5 inside the image; the image's edge, the same boundary, for the sample that left) -- sixteen fp32 ulps of the
    largest coordinate an in-image projection produces, for a chain of about a dozen rounded operations plus the 1-ulp
    reciprocal of the projective march;
  * depth: sampleDepth is more than 2^-19 max|z| of the case from sp.z + bias and from sp.z - thick at every sample (the
    ray's own pixel at j = 0 is exempt: there sp.z IS sampleDepth, no arithmetic lies between them);
  * denominator: |sp.z + 1e-7| stays above 2^-19 max|z| at the samples at or behind the camera plane.
These are derived from the arithmetic; they were not measured on a device.  Undecided rays may differ between any two
evaluations; CAP_RAYS / CAP_WEIGHT bound how many a case may hold.

The summation bound.  Per pixel and plane (n + 8) 2^-24 sum|t_i|: n the marched rays, t_i the float64 terms of the pixel's sum
carried through its tail (/ sum w, or pi kD albedo / nrSamples) -- the a-priori bound of an fp32 sum in any order.
Where float64 is an exact zero the result has to be one.

A6 / median / bilateral cases are depth planes around the 0.01 threshold; their bound is BOUND_FACTOR x the C oracle's worst
per-pixel error against float64 per case and tensor (tests/golden/gi_f64_bounds.json).
"""
import json
import os

import numpy as np

from oracle import gi_ref as gr

F32 = np.float32
BOUND_FACTOR = 4.0
CAP_RAYS, CAP_WEIGHT, MIN_HIT_SHARE = 0.01, 0.10, 0.05
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gi_f64_bounds.json")
GI_DEFAULTS = dict(radius=0.8, bias=0.01, thick=0.05, delta=0.0625, step=16, start=8)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


class Case:
    def __init__(self, name, W, H, f, gi, g, needs, hit_share=MIN_HIT_SHARE):
        self.name, self.W, self.H, self.f, self.gi, self.g, self.needs, self.hit_share = name, W, H, float(F32(f)), gi, g, needs, hit_share

    @property
    def args(self):
        gi = self.gi
        return (self.W, self.H, self.f, self.f, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])

    @property
    def max_z(self):
        z = np.abs(self.g["pos"][2])
        return float(z[np.isfinite(z)].max())


# ---- analytic G-buffers ----------------------------------------------------------------------------------------
def gbuffer(W, H, f, planes, slabs=(), holes=(), seed=0):
    """planes: (normal, point) pairs, the visible one per pixel is the nearest front-facing one; slabs: (normal, point, (x0, x1,
    y0, y1) as fractions of the image) drawn over them where nearer; holes: pixel rectangles (x0, x1, y0, y1) with pos = 0 and
    normal = 0.  Positions are get_position's fp32 values (R/ssr.h:103-117), normals the planes' own."""
    f = F32(f)
    ys, xs = np.mgrid[0:H, 0:W]
    dx, dy = (xs.astype(F32) - F32(W / 2.0)) / f, (ys.astype(F32) - F32(H / 2.0)) / f
    r = np.stack([dx.astype(np.float64), dy.astype(np.float64), np.ones((H, W))], -1)
    depth = np.full((H, W), np.inf)
    normal = np.zeros((H, W, 3))

    def draw(n, p0, where):
        n = unit(n)
        with np.errstate(all="ignore"):
            nr = r @ n
            z = float(n @ np.asarray(p0, np.float64)) / nr
        ok = where & (nr < 0) & (z > 0) & (z < depth)
        depth[ok] = z[ok]
        normal[ok] = n

    for n, p0 in planes:
        draw(n, p0, np.ones((H, W), bool))
    for n, p0, (x0, x1, y0, y1) in slabs:
        draw(n, p0, (xs >= x0 * W) & (xs < x1 * W) & (ys >= y0 * H) & (ys < y1 * H))
    empty = ~np.isfinite(depth)
    for x0, x1, y0, y1 in holes:
        empty |= (xs >= x0) & (xs < x1) & (ys >= y0) & (ys < y1)
    depth[empty] = 0.0
    normal[empty] = 0.0
    d32 = depth.astype(F32)
    pos = np.stack([dx * d32, dy * d32, d32]).astype(F32)
    rng = np.random.default_rng(seed)
    g = dict(normal=np.ascontiguousarray(normal.transpose(2, 0, 1)).astype(F32), pos=pos,
             rgb=rng.uniform(0.0, 1.0, (3, H, W)).astype(F32), rgb2=rng.uniform(0.0, 2.0, (3, H, W)).astype(F32),
             albedo=rng.uniform(0.05, 0.95, (3, H, W)).astype(F32), roughness=rng.uniform(0.1, 0.9, (1, H, W)).astype(F32),
             metallic=rng.uniform(0.05, 0.95, (1, H, W)).astype(F32), F0=rng.uniform(0.02, 0.9, (3, H, W)).astype(F32))
    g["metallic"][0, :, : max(1, W // 3)] = 0.0
    g["metallic"][0, :, W - max(1, W // 3):] = 1.0
    return g


WALL = (unit([0.12, 0.2, -1.0]), (0.0, 0.0, 3.0))
FLOOR = (unit([0.3, -0.85, -0.3]), (0.0, 0.55, 3.0))
SIDE = (unit([0.9, 0.25, -0.35]), (-0.9, 0.0, 3.0))
SIDE_R = (unit([-0.9, 0.2, -0.3]), (1.0, 0.0, 3.0))
SLAB = (unit([0.05, 0.15, -1.0]), (0.0, 0.0, 2.55))
GRAZING = (unit([0.3, -0.9, 0.15]), (0.0, 0.45, 2.0))


def _patches(g, W, H, special=True):
    """the per-pixel specials of a case of at least 37 x 29 pixels, one kind per row (every second row from the bottom, 33
    or more pixels each): NaN normals, the degenerate frame, both Fresnel clamps"""
    if not special:
        return
    n, p = g["normal"], g["pos"]
    covered = p[2] > 0
    for kind, y0 in enumerate((H - 3, H - 5, H - 7, H - 9)):
        for x in range(2, W - 2):
            if not covered[y0, x]:
                continue
            if kind == 0:
                n[:, y0, x] = np.nan                      # a NaN normal on a covered pixel
            elif kind == 1:
                n[:, y0, x] = (0.0, -1.0, 0.0)            # up - n (n.up) = 0: the NaN frame
            elif kind == 2:
                n[:, y0, x] = -n[:, y0, x]                # faces away: dot(N, V) < 1e-7, the first clamp
            else:
                v = -p[:, y0, x].astype(np.float64)      # N = V: 1 - cosTheta < 1e-6, the second clamp
                n[:, y0, x] = (v / np.linalg.norm(v)).astype(F32)


def _poison(case, m):
    """non-finite radiance (R/forward.cu:824-826: rgb * cos * 0 = NaN) on a short band that live rays hit, and on pixels chosen
    so that for up to 64 pixels the ONLY non-finite hit is their zero-weight ray's: q is poisoned when the zero-weight ray of p
    lands there, no live ray of p lands on q or on anything poisoned before, and no pixel accepted before sees q.  No
    undecided ray of any pixel lands on a poisoned pixel or next to one: which radiance such a ray picks up is not decided,
    and a NaN must not hang on it."""
    tab = gr.ray_table(case.gi["delta"])
    rgb, W = case.g["rgb"], case.W
    hp = m["hit_pix"]
    live, dead = hp[:, :tab["n_live"]], hp[:, tab["n_live"]]
    und = hp[~gr.decided(m, W, case.H, case.max_z) & (hp >= 0)]
    near = np.zeros((case.H + 2, W + 2), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near[und // W + dy, und % W + dx] = True
    near = near[1:-1, 1:-1].reshape(-1)  # pixels with an undecided ray's hit in their 3 x 3 neighbourhood
    y = case.H // 2
    poisoned = {q for q in range(y * W + W // 4, y * W + W // 2) if not near[q]}
    for q in poisoned:
        rgb[1, q // W, q % W] = np.nan
    seen_by_accepted, accepted = set(), 0
    for p_ in np.flatnonzero((dead >= 0) & ~m["nonfinite"]):
        q = int(dead[p_])
        mine = set(live[p_][live[p_] >= 0].tolist())
        if accepted >= 64 or q == p_ or near[q] or q in mine or q in seen_by_accepted or mine & poisoned:
            continue
        if q not in poisoned:
            rgb[accepted % 3, q // W, q % W] = np.inf if accepted % 2 else np.nan
            poisoned.add(q)
        seen_by_accepted |= mine
        accepted += 1


def _march_case(name, W, H, f, gi, planes, slabs=(), holes=(), needs=None, special=True, poison=True, seed=0, **kw):
    g = gbuffer(W, H, f, planes, slabs, holes, seed)
    _patches(g, W, H, special and W >= 37 and H >= 29)
    case = Case(name, W, H, f, dict(GI_DEFAULTS, **gi), g, needs or {}, **kw)
    return case, poison


ROOM = [WALL, FLOOR, SIDE, SIDE_R]
SLABS = [SLAB + ((0.52, 0.78, 0.15, 0.7),)]
COMMON = dict(hit=32, miss=32, hit_first=32, hit_last=32, left_first=32, front_then_hit=32, passed_behind=32,
              left_x_low=32, left_x_high=32, left_y_low=32, left_y_high=32, nan_normal=32, degenerate_frame=32,
              ndv_clamped=32, ndv_free=32, arg_clamped=32, arg_free=32, metallic_0=32, metallic_1=32, metallic_mid=32)

MARCH_SPECS = {
    # defaults on a multiple of 8 that is no multiple of 16 or 32; holes, a slab, non-finite radiance under zero-weight rays
    "room_48x40": lambda: _march_case("room_48x40", 48, 40, 40.0, {}, ROOM, SLABS, [(0, 6, 0, 5)],
                                      dict(COMMON, all_missing=32, hole_pixels=16)),
    # ragged against every workgroup tile; 144 rays, a longer reach
    "room_37x29": lambda: _march_case("room_37x29", 37, 29, 30.0, dict(delta=0.125, start=4, radius=1.2), ROOM, SLABS, [(30, 37, 0, 4)],
                                      dict(COMMON, hole_pixels=16), seed=1),
    # a step that is no power of two
    "step12_37x29": lambda: _march_case("step12_37x29", 37, 29, 30.0, dict(delta=0.125, step=12, start=5), ROOM, SLABS, (),
                                        dict(COMMON), seed=2),
    # start = 0: every finite pixel hits itself at j = 0, occlusion is 0
    "start0_37x29": lambda: _march_case("start0_37x29", 37, 29, 30.0, dict(delta=0.125, start=0), ROOM, SLABS, [(0, 5, 0, 4)],
                                        dict(hit=32, hit_first=32, self_hit_all=32, nan_normal=32, degenerate_frame=32, hole_pixels=16), seed=3),
    # bias = thick = 0 with start = 0: an equality-only hit window
    "equal_5x3": lambda: _march_case("equal_5x3", 5, 3, 4.0, dict(delta=0.125, start=0, bias=0.0, thick=0.0), ROOM, (), (),
                                     dict(hit=1, hit_first=1, self_hit_all=1), poison=False, seed=4),
    # the camera close to the geometry: sp.z + 1e-7 passes through zero, rays land on holes (sampleDepth = 0)
    "near_37x29": lambda: _march_case("near_37x29", 37, 29, 30.0, dict(delta=0.125, start=2, radius=1.6, bias=0.03, thick=0.2),
                                      [(unit([0.15, 0.25, -1.0]), (0.0, 0.0, 0.46)), (unit([0.3, -0.85, -0.3]), (0.0, 0.3, 0.46)),
                                       (unit([0.9, 0.25, -0.35]), (-0.35, 0.0, 0.45))], (), [(10, 27, 6, 23)],
                                      dict(hit=32, miss=32, den_nonpos=32, hit_hole=32, hole_missed=32, hole_pixels=16), seed=5,
                                      hit_share=MIN_HIT_SHARE),
    # the room of room_37x29 at 1e-4 of its size: the 1e-7 of get_coord is 3e-4 of the denominator and decides pixels
    "micro_37x29": lambda: _march_case("micro_37x29", 37, 29, 30.0, dict(delta=0.125, start=4, radius=1.2e-4, bias=1e-6, thick=5e-6),
                                       [(n, tuple(1e-4 * np.asarray(p0))) for n, p0 in ROOM],
                                       [(n, tuple(1e-4 * np.asarray(p0)), r) for n, p0, r in SLABS], (),
                                       dict(hit=32, miss=32, hit_first=32, passed_behind=32, front_then_hit=32), seed=13),
    # a floor at a grazing angle in front of the wall
    "grazing_48x40": lambda: _march_case("grazing_48x40", 48, 40, 40.0, dict(delta=0.125), [WALL, GRAZING, SIDE], SLABS, (),
                                         dict(hit=32, miss=32, grazing_pixels=32, passed_behind=32, front_then_hit=32), seed=6),
    # the tiny images: ragged against every tile, and the largest ray set on the smallest ones
    "one_1x1": lambda: _march_case("one_1x1", 1, 1, 1.0, dict(delta=0.03125, start=0), [WALL], (), (), dict(hit=1, self_hit_all=1),
                                   poison=False, seed=7),
    "one_1x1_leaves": lambda: _march_case("one_1x1_leaves", 1, 1, 200.0, dict(delta=0.125), [WALL], (), (),
                                          dict(left_first=1, all_missing=1), poison=False, seed=8, hit_share=0.0),
    "tiny_5x3": lambda: _march_case("tiny_5x3", 5, 3, 6.0, dict(delta=0.03125, start=6), ROOM, (), (), dict(hit=1, miss=1, left_first=1),
                                    poison=False, seed=9),
    # more than 60 steps: the projective march falls back to the exact one
    "long_5x3": lambda: _march_case("long_5x3", 5, 3, 4.0, dict(delta=0.125, step=72, start=4), ROOM, (), (), dict(hit=1, miss=1),
                                    poison=False, seed=10),
    # aligned to every tile
    "room_64x64": lambda: _march_case("room_64x64", 64, 64, 52.0, {}, ROOM, SLABS, [(58, 64, 58, 64)], dict(COMMON, hole_pixels=16), seed=11),
    # 5 x 4 blocks of 16 pixels: the inner 3 x 2 can certify (gi_minmax_kernel: border and partly covered blocks never do)
    "cert_80x64": lambda: _march_case("cert_80x64", 80, 64, 64.0, dict(delta=0.125), ROOM, SLABS, [(0, 7, 0, 6)],
                                      dict(COMMON, dead_hits_nonfinite=32, dead_only_nan=32, hole_pixels=16), seed=12),
}
MARCH_CASES = list(MARCH_SPECS)
_BUILT = {}


def build(name):
    """the case and its float64 march (cached for the session; treat both as read-only)"""
    if name not in _BUILT:
        case, poison = MARCH_SPECS[name]()
        m = gr.march(*case.args, case.g["normal"], case.g["pos"])
        if poison:
            _poison(case, m)
        _BUILT[name] = (case, m)
    return _BUILT[name]


def reference(case, m=None, mut=None):
    """float64 outputs of the case: the march (recomputed under a mutation), occlusion, colour, abd, their bounds"""
    g = case.g
    if m is None or mut is not None:
        m = gr.march(*case.args, g["normal"], g["pos"], mut=mut)
    tab = gr.ray_table(case.gi["delta"])
    occ, occ_mag = gr.ssao(case.gi["delta"], m["outcome"], mut)
    col, abd, col_mag, abd_mag, det = gr.ssr(case.gi["delta"], m["hit_pix"], g["normal"], g["pos"], g["rgb"], g["albedo"],
                                             g["metallic"], g["F0"], mut)
    dec = gr.decided(m, case.W, case.H, case.max_z)
    und = ~dec & ~m["nonfinite"][:, None]
    share = (und * np.abs(tab["w"])[None, :]).sum(1) / tab["sum_w"]
    occ_bound, col_bound, abd_bound = bounds(case, occ_mag, col_mag, abd_mag)
    return dict(march=m, decided=dec, occ=occ, occ_bound=occ_bound, color=col, abd=abd, color_bound=col_bound,
                abd_bound=abd_bound, fresnel=det, undecided_share=share, finite=~m["nonfinite"])


U = 2.0 ** -24


def ssr_tail(case):
    """|pi kD / nrSamples| [3,N] in float64 (NaN -> 0)"""
    g = case.g
    N = case.W * case.H
    f = lambda a, c: np.asarray(a, np.float64).reshape(c, N).T  # noqa: E731
    kD, _ = gr.fresnel(f(g["normal"], 3), f(g["pos"], 3), f(g["metallic"], 1)[:, 0], f(g["F0"], 3))
    t = np.abs(float(gr.PI_F) / gr.ray_table(case.gi["delta"])["n"] * kD.T)
    return np.where(np.isfinite(t), t, 0.0)


def bounds(case, occ_mag, col_mag, abd_mag):
    """The summation bound (n + 8) u sum|t_i| of the module text, with the two roundings the tails add to it beyond the sum:
    occlusion = 1 - occ is rounded once as a number <= 1 (8 u, nothing where no ray hit: float64's 1 is exact), and
    kD = (1 - F)(1 - metallic) is a difference of numbers <= 1 whose ABSOLUTE error is F's -- 12 roundings from cosTheta to
    kD (R/ssr.h:13-16, R/forward.cu:836-842) -- so it adds 12 u (1 - metallic) pi / nrSamples sum|rgb w| where kD is small."""
    g = case.g
    N = case.W * case.H
    n = gr.ray_table(case.gi["delta"])["n"]
    k = (n + 8) * U
    occ_bound = np.where(occ_mag > 0, k * occ_mag + 8 * U, 0.0)
    tail = ssr_tail(case)
    metal = np.abs(1.0 - np.asarray(g["metallic"], np.float64).reshape(1, N))
    alb = np.abs(np.asarray(g["albedo"], np.float64).reshape(3, N))
    with np.errstate(all="ignore"):
        raw = np.where(tail > 0, abd_mag / np.where(tail > 0, tail, 1.0), 0.0)  # sum |rgb w|
    kd_term = 12 * U * np.where(np.isfinite(metal), metal, 0.0) * float(gr.PI_F) / n * raw
    abd_bound = k * abd_mag + kd_term
    return occ_bound, k * col_mag + kd_term * alb, abd_bound


def ssr_bound_for(case, hit_pix, rgb=None):
    """float64 colour / abd and their summation bounds over ANOTHER hit set (a kernel's own decisions)"""
    g = case.g
    col, abd, col_mag, abd_mag, _ = gr.ssr(case.gi["delta"], hit_pix, g["normal"], g["pos"], g["rgb"] if rgb is None else rgb,
                                           g["albedo"], g["metallic"], g["F0"])
    _, col_bound, abd_bound = bounds(case, np.zeros(1), col_mag, abd_mag)
    return col, abd, col_bound, abd_bound


def populations(case, ref):
    m, dec, g = ref["march"], ref["decided"], case.g
    W, H = case.W, case.H
    tab = gr.ray_table(case.gi["delta"])
    out, st = m["outcome"], m["step"]
    z = g["pos"][2].reshape(-1)
    hit, left = dec & (out == gr.HIT), dec & (out == gr.LEFT)
    finite = ref["finite"]
    fr = ref["fresnel"]
    nrm = g["normal"].reshape(3, -1).T
    metal = g["metallic"].reshape(-1)
    rgb_bad = ~np.isfinite(g["rgb"]).all(0).reshape(-1)
    dead_hit, live_hit = m["hit_pix"][:, tab["n_live"]:], m["hit_pix"][:, :tab["n_live"]]
    own = np.arange(W * H)[:, None]
    pop = dict(
        hit=int(hit.sum()), miss=int((dec & (out == gr.MISS)).sum()), hit_first=int((hit & (st == case.gi["start"])).sum()),
        hit_last=int((hit & (st == case.gi["step"] - 1)).sum()), left_first=int((left & (st == case.gi["start"])).sum()),
        front_then_hit=int((hit & m["front_then_hit"]).sum()), passed_behind=int((dec & m["passed_behind"]).sum()),
        den_nonpos=int((dec & m["den_nonpos"]).sum()), hit_hole=int((hit & (z[np.maximum(m["hit_pix"], 0)] == 0)).sum()),
        hole_missed=int((dec & m["hole_missed"]).sum()),
        self_hit_all=int((((out == gr.HIT) & (m["hit_pix"] == own) & (st == 0)).all(1) & finite).sum()),
        all_missing=int((finite & ~(out == gr.HIT).any(1)).sum()),
        dead_hits_nonfinite=int(((dead_hit >= 0) & rgb_bad[np.maximum(dead_hit, 0)]).any(1).sum()),
        # ... of which no live ray of the pixel lands on non-finite radiance: the NaN is the zero-weight ray's alone
        dead_only_nan=int((((dead_hit >= 0) & rgb_bad[np.maximum(dead_hit, 0)]).any(1) & finite
                           & ~((live_hit >= 0) & rgb_bad[np.maximum(live_hit, 0)]).any(1)).sum()),
        nan_normal=int(np.isnan(nrm).any(1).sum()), degenerate_frame=int(((nrm[:, 0] == 0) & (nrm[:, 2] == 0) & (nrm[:, 1] != 0)).sum()),
        hole_pixels=int(((z == 0) & (nrm == 0).all(1)).sum()),
        ndv_clamped=int((finite & fr["ndv_clamped"]).sum()), ndv_free=int((finite & ~fr["ndv_clamped"]).sum()),
        arg_clamped=int((finite & fr["arg_clamped"]).sum()), arg_free=int((finite & ~fr["arg_clamped"]).sum()),
        metallic_0=int((finite & (metal == 0)).sum()), metallic_1=int((finite & (metal == 1)).sum()),
        metallic_mid=int((finite & (metal > 0) & (metal < 1)).sum()),
        grazing_pixels=int((finite & (np.abs(fr["ndv"]) < 0.25)).sum()))
    for k, e in enumerate(gr.EDGES):
        pop["left_" + e] = int((left & (m["edge"] == k)).sum())
    n_pairs = int(finite.sum()) * tab["n"]
    pop["pairs"] = n_pairs
    pop["undecided"] = int((~dec & finite[:, None]).sum())
    pop["undecided_share"] = pop["undecided"] / max(1, n_pairs)
    pop["undecided_weight_worst"] = float(ref["undecided_share"].max())
    pop["hit_share"] = float(((out == gr.HIT) & finite[:, None]).sum() / max(1, n_pairs))
    return pop


def check_populations(case, ref):
    pop = populations(case, ref)
    for k, need in case.needs.items():
        assert pop[k] >= need, f"{case.name}: branch {k} entered by {pop[k]} decided rays / pixels, needs {need}"
    assert pop["undecided_share"] <= CAP_RAYS, (case.name, "undecided rays", pop["undecided_share"])
    assert pop["undecided_weight_worst"] <= CAP_WEIGHT, (case.name, "undecided weight of one pixel", pop["undecided_weight_worst"])
    assert pop["hit_share"] >= case.hit_share, (case.name, "hit share", pop["hit_share"])
    return pop


# ---- A6, median, bilateral -------------------------------------------------------------------------------------
def _depth_plane(W, H, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    return (2.0 + 0.03 * xs + 0.05 * ys + 0.02 * rng.uniform(-1, 1, (H, W))).astype(F32)


def normal_cases():
    """name -> dict(W, H, f, viewmatrix, depth): depth planes with values on both sides of 0.01 at the centre and at each of the
    25 pad positions of some pixel, pixels 1 and 2 from every edge, images narrower than the pad"""
    a = 0.3
    vm = np.array([[np.cos(a), 0, np.sin(a), 0.1], [0, 1, 0, -0.2], [-np.sin(a), 0, np.cos(a), 3.0], [0, 0, 0, 1]], F32).T.copy()
    out = {}
    # 25 pad positions + the centre: one probe pixel each on a 6 x 5 lattice of 7 x 7 cells, below / above the threshold
    W, H = 6 * 7 + 3, 5 * 7 + 3
    d = _depth_plane(W, H, 1)
    k = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            cx_, cy_ = 4 + 7 * (k % 6), 4 + 7 * (k // 6)
            d[cy_ + dy, cx_ + dx] = F32(0.0099) if k % 2 == 0 else F32(0.0101)
            k += 1
    d[4 + 7 * 4, 4 + 7 * 5] = np.nextafter(F32(0.01), F32(0))  # the centre, one ulp below
    d[4 + 7 * 4, 4 + 7 * 4] = F32(0.01)                         # ... and exactly on it (not below: no early-out)
    out["pad_45x38"] = dict(W=W, H=H, f=40.0, viewmatrix=vm, depth=d)
    for (w, h) in ((1, 1), (2, 5), (5, 2), (5, 5), (7, 6)):
        out["small_%dx%d" % (w, h)] = dict(W=w, H=h, f=6.0, viewmatrix=vm, depth=_depth_plane(w, h, 10 + w))
    d = _depth_plane(37, 29, 3)
    d[10:14, 20:25] = 0.0
    d[20, 5] = np.nan
    out["ragged_37x29"] = dict(W=37, H=29, f=30.0, viewmatrix=vm, depth=d)
    return out


def normal_chain(impl, c, dtype):
    """median3x3(depth) -> depth_to_normal -> bilateral3x3(normal, 1, (3, 3)), median3x3(pos) with `impl` = oracle/gi_ref (float64
    throughout) or the C oracle (fp32 throughout): what the rasterizer's forward derives its normals with"""
    d = impl.median3x3(np.asarray(c["depth"]).reshape(1, c["H"], c["W"]))
    d = d[0] if isinstance(d, tuple) else d
    out = impl.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], np.asarray(d, dtype).reshape(c["H"], c["W"]))
    nrm = impl.bilateral3x3(np.asarray(out[0], dtype), 1.0, (3.0, 3.0))
    pos = impl.median3x3(np.asarray(out[1], dtype))
    return nrm, (pos[0] if isinstance(pos, tuple) else pos)


def filter_cases():
    """name -> [C,H,W] fp32: median inputs with ties, with a NaN, at the zero-padded border; bilateral inputs constant / step"""
    rng = np.random.default_rng(5)
    out = {}
    x = rng.permutation(3 * 29 * 37).reshape(3, 29, 37).astype(F32) / F32(64.0) - F32(20.0)  # tie-free, both signs
    out["distinct_37x29"] = x
    t = rng.integers(0, 4, (3, 13, 11)).astype(F32)                                          # many ties
    out["ties_11x13"] = t
    n = x[:, :9, :10].copy()
    n[1, 4, 5] = np.nan
    out["nan_10x9"] = n
    out["const_9x7"] = np.full((3, 7, 9), 0.375, F32)
    s = np.zeros((3, 8, 12), F32)
    s[:, :, 6:] = 1.5
    s += (rng.uniform(-0.01, 0.01, s.shape)).astype(F32)
    out["step_12x8"] = s
    out["one_2x2"] = rng.uniform(-1, 1, (1, 2, 2)).astype(F32)
    return out


def load_bounds():
    with open(BOUNDS_JSON) as f:
        return json.load(f)


# ---- comparing an fp32 result with float64 ---------------------------------------------------------------------
def plane_errors(got, ref, bound, extra=None):
    """got (fp32) against ref (float64) with the per-element bound (+ extra): where ref is not finite the result has to be the
    same non-finite value, elsewhere |got - ref| <= bound -- so an exact zero with a zero bound has to be an exact zero.
    Returns dict(worst_abs, worst_ratio: of |error| to the bound where that is > 0, violations, pattern: mismatches of
    non-finite values, where: flat index of the worst violation or -1)."""
    got, ref, bound = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1), np.asarray(bound, np.float64).reshape(-1)
    allow = bound if extra is None else bound + np.asarray(extra, np.float64).reshape(-1)
    fin = np.isfinite(ref)
    with np.errstate(all="ignore"):
        pattern = int((~fin & ~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum()) + int((fin & ~np.isfinite(got)).sum())
        err = np.where(fin & np.isfinite(got), np.abs(got - ref), 0.0)
        viol = err > allow
        ratio = np.where(allow > 0, err / np.where(allow > 0, allow, 1.0), 0.0)
    where = int(np.argmax(np.where(viol, err, -1.0))) if viol.any() else -1
    return dict(worst_abs=float(err.max()) if err.size else 0.0, worst_ratio=float(ratio.max()) if err.size else 0.0,
                violations=int(viol.sum()), pattern=pattern, where=where)


def oracle_march(orc, case):
    """the C oracle's occlusion [N], colour and abd [3,N] of the case"""
    g = case.g
    occ = orc.ssao(*case.args, g["normal"], g["pos"]).reshape(-1)
    col, abd = orc.ssr(*case.args, g["normal"], g["pos"], g["rgb"], g["albedo"], g["roughness"], g["metallic"], g["F0"])
    return occ, col.reshape(3, -1), abd.reshape(3, -1)
