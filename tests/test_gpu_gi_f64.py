"""GPU tests: the screen-space GI kernels (csrc/gi.hip ssao_kernel, ssr_kernel and its hit list; csrc/ssr_apply.hip
ssr_apply_kernel; csrc/normal_filters.hip depth_to_normal_kernel, median3x3(_bwd)_kernel, bilateral3x3_kernel,
derive_normal_fused_kernel) against the float64
restatement oracle/gi_ref.py on the analytic cases of tests/gi_cases.py, which enter every branch of the march on purpose.

  * decisions: the default march's recorded hit list (gigs_ssr_hits) gives, per pixel, {ray -> hit pixel}; every DECIDED ray
    (gi_cases: the margin rule -- derived from the arithmetic, not measured) has exactly float64's outcome, in every
    combination of gi_cert, gi_interleave, gi_zero_rays and gi_tile_log2w; undecided rays may differ and are counted;
  * sums: colour and abd are held per pixel and channel to the float64 evaluation over the kernel's OWN hit list with the
    a-priori summation bound alone (gi_cases.bounds), the gather gigs_ssr_apply likewise with other radiance, two lights through
    gigs_ssr_multi / gigs_ssr_apply_multi; SSAO (no hit list) to float64 within the bound plus the weight share of the pixel's
    undecided rays; the exact march to the C oracle with the bound and no slack;
  * the non-finite population and every NaN of the radiance: the C oracle's pattern;
  * normal derivation: A6, the median, the bilateral filter and the fused kernel per pixel within BOUND_FACTOR x the C oracle's
    own error (tests/golden/gi_f64_bounds.json), early-outs exact zeros, depth_pos and the median bit-equal to the oracle, the
    median's backward to float64's chosen tap.
tests/golden/record_gi_f64_device.py writes the bounds file's "device" record with this module's helpers."""
import numpy as np
import pytest
import torch

import gi_cases as gc
from oracle import gi_ref as gr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = [dict(gi_cert=c, gi_interleave=i, gi_zero_rays=z, gi_tile_log2w=t) for c in (1, 0) for i in (1, 0) for z in (0, 1) for t in range(7)]


def tt(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


_REFS = {}


def get_ref(name):
    """case, float64 reference and its device copies: once per session"""
    if name not in _REFS:
        case, m = gc.build(name)
        ref = gc.reference(case, m)
        gc.check_populations(case, ref)
        g = {k: tt(v) for k, v in case.g.items()}
        px, zz = 2.0 ** -19 * max(case.W, case.H), 2.0 ** -19 * case.max_z
        rel = np.minimum(np.minimum(m["m_px"] / px, m["m_z"] / zz), m["m_den"] / zz)  # > 1: decided
        dev = dict(hit=tt(m["hit_pix"], torch.int64), decided=tt(ref["decided"]), rel=tt(np.minimum(rel, 1e30).astype(np.float32)),
                   finite=tt(ref["finite"]))
        _REFS[name] = (case, ref, g, dev)
    return _REFS[name]


def _scratch(lib, W, H):
    return torch.empty(max(16, int(lib.gigs_gi_scratch_bytes(W, H))), dtype=torch.uint8, device=DEV)


def record_hits(lib, ctx, case, g, rgb=None):
    """gigs_ssr_hits mode 1 (count), prefix, mode 2 (fill) -> colour, abd of the fill call, offsets, entries"""
    W, H = case.W, case.H
    N = W * H
    a = tuple(float(x) if isinstance(x, float) else int(x) for x in case.args)
    s = torch.cuda.current_stream().cuda_stream
    scratch = _scratch(lib, W, H)
    planes = (_p(g["normal"]), _p(g["pos"]), _p(g["rgb"] if rgb is None else rgb), _p(g["albedo"]), _p(g["roughness"]), _p(g["metallic"]),
              _p(g["F0"]))
    counts = torch.zeros(4 * N, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(4 * N + 1, dtype=torch.int32, device=DEV)
    c1, a1 = torch.full((3, H, W), 7.0, device=DEV), torch.full((3, H, W), 7.0, device=DEV)
    import gigs_lib
    gigs_lib.check(lib.gigs_ssr_hits(ctx, *a, *planes, _p(c1), _p(a1), 1, _p(counts), None, None, 0, _p(scratch), s), "ssr_hits (count)")
    torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
    total = int(offsets[-1])
    entries = torch.full((max(total, 1), 2), -1, dtype=torch.int32, device=DEV)
    c2, a2 = torch.full((3, H, W), 7.0, device=DEV), torch.full((3, H, W), 7.0, device=DEV)
    gigs_lib.check(lib.gigs_ssr_hits(ctx, *a, *planes, _p(c2), _p(a2), 2, None, _p(offsets), _p(entries), total, _p(scratch), s),
                   "ssr_hits (fill)")
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(a1.view(torch.int32), a2.view(torch.int32))
    return c2, a2, offsets, entries[:total]


def decode(case, offsets, entries, marched):
    """the hit list as a dense [N, R] map ray -> hit pixel (-1 = none); every entry valid, no ray twice in a pixel"""
    N, R = case.W * case.H, gr.ray_table(case.gi["delta"])["n"]
    dense = torch.full((N, R), -1, dtype=torch.int64, device=DEV)
    if entries.shape[0] == 0:
        return dense
    q, ray = entries[:, 0].long(), entries[:, 1].long()
    assert int(q.min()) >= 0 and int(q.max()) < N, "a hit pixel outside the image"
    assert int(ray.min()) >= 0 and int(ray.max()) < marched, ("a ray index beyond the marched rays", int(ray.max()), marched)
    slot = torch.searchsorted(offsets[1:].long().contiguous(), torch.arange(entries.shape[0], device=DEV), right=True)
    pix = slot // 4
    seen = torch.zeros(N * R, dtype=torch.int32, device=DEV)
    seen.index_add_(0, pix * R + ray, torch.ones_like(ray, dtype=torch.int32))
    assert int(seen.max()) == 1, "a ray is listed twice for one pixel"
    dense[pix, ray] = q
    return dense


def marched_rays(case, zero_rays):
    t = gr.ray_table(case.gi["delta"])
    return t["n_live"] + (t["n_dead"] if zero_rays else min(1, t["n_dead"]))


def compare_decisions(case, dev, dense, marched):
    """(decided rays that differ, undecided rays that differ, the largest relative margin among those: < 1 by definition)"""
    diff = (dense != dev["hit"])[:, :marched] & dev["finite"][:, None]
    bad = diff & dev["decided"][:, :marched]
    und = diff & ~dev["decided"][:, :marched]
    worst = float(dev["rel"][:, :marched][und].max()) if bool(und.any()) else 0.0
    where = torch.nonzero(bad)[:5].tolist()
    return int(bad.sum()), int(und.sum()), worst, where


def ssr_reference(case, dense, rgb=None):
    """float64 colour, abd and their bounds over a hit list: the expensive part, evaluated once per distinct list"""
    return gc.ssr_bound_for(case, dense, rgb)


def check_ssr(case, name, want, color, abd, what="march", quiet=False):
    col64, abd64, cb, ab = want
    N = case.W * case.H
    for k, got, w64, b in (("color", color, col64, cb), ("abd", abd, abd64, ab)):
        e = gc.plane_errors(got.reshape(3, N), w64, b)
        if not quiet:
            print(f"  {name} {what} {k}: worst |d| {e['worst_abs']:.3e}, {e['worst_ratio']:.3f} of the bound")
        assert e["violations"] == 0 and e["pattern"] == 0, (name, what, k, e, divmod(e["where"] % N, case.W) if e["where"] >= 0 else None)


@pytest.mark.parametrize("name", gc.MARCH_CASES)
def test_default_march_decides_every_decided_ray_as_float64(name):
    """Per mode: the hit list decoded and compared ray by ray; that call's colour and abd, and the gather's with other radiance,
    against float64 over the kernel's own hits (float64 is evaluated once per distinct list, every mode's planes are compared);
    SSAO against float64 with the undecided rays' weight share."""
    import gigs_lib
    lib = gigs_lib.lib()
    case, ref, g, dev = get_ref(name)
    W, H, N = case.W, case.H, case.W * case.H
    proj = case.gi["step"] - case.gi["start"] <= 60
    a = tuple(float(x) if isinstance(x, float) else int(x) for x in case.args)
    s = torch.cuda.current_stream().cuda_stream
    distinct, und_total, und_worst = [], 0, 0.0
    for mode in MODES:
        with gigs_lib.options(**mode) as cx:
            if proj:
                color, abd, offsets, entries = record_hits(lib, cx.ptr, case, g)
            occ = torch.full((1, H, W), 7.0, device=DEV)
            gigs_lib.check(lib.gigs_ssao_ex(cx.ptr, *a, _p(g["normal"]), _p(g["pos"]), _p(occ), _p(_scratch(lib, W, H)), s), "ssao")
        e = gc.plane_errors(occ.cpu().numpy().reshape(-1), ref["occ"], ref["occ_bound"], ref["undecided_share"])
        assert e["violations"] == 0 and e["pattern"] == 0, (name, mode, "occlusion", e)
        clean = ref["undecided_share"] == 0
        e = gc.plane_errors(occ.cpu().numpy().reshape(-1)[clean], ref["occ"][clean], ref["occ_bound"][clean])
        assert e["violations"] == 0, (name, mode, "occlusion of pixels without an undecided ray", e)
        if not proj:
            continue  # a march of more than 60 steps is the exact one: no hit list (test_exact_march_...)
        marched = marched_rays(case, mode["gi_zero_rays"])
        dense = decode(case, offsets, entries, marched)
        n_bad, n_und, worst, where = compare_decisions(case, dev, dense, marched)
        assert n_bad == 0, (f"{name} {mode}: {n_bad} DECIDED rays differ from float64 ({n_und} undecided ones do); first (pixel, ray): "
                            f"{where}")
        und_total, und_worst = und_total + n_und, max(und_worst, worst)
        known = [i for i, (x, _, _) in enumerate(distinct) if torch.equal(dense, x)]
        if not known:
            d = dense.cpu().numpy()
            distinct.append((dense, ssr_reference(case, d), ssr_reference(case, d, case.g["rgb2"])))
            known = [len(distinct) - 1]
        _, want, want2 = distinct[known[0]]
        quiet = mode != MODES[0]
        check_ssr(case, name, want, color.cpu().numpy(), abd.cpu().numpy(), what=f"march {mode}", quiet=quiet)
        c3, a3 = torch.full((3, H, W), 7.0, device=DEV), torch.full((3, H, W), 7.0, device=DEV)
        gigs_lib.check(lib.gigs_ssr_apply(W, H, float(case.gi["delta"]), _p(offsets), _p(entries), _p(g["normal"]), _p(g["pos"]),
                                          _p(g["rgb2"]), _p(g["albedo"]), _p(g["metallic"]), _p(g["F0"]), _p(c3), _p(a3), s), "ssr_apply")
        check_ssr(case, name, want2, c3.cpu().numpy(), a3.cpu().numpy(), what=f"gather {mode}", quiet=quiet)
    print(f"{name}: {len(MODES)} modes, {len(distinct)} distinct hit lists, undecided rays that differ from float64: {und_total} "
          f"(largest margin {und_worst:.3f} of the rule's)")


@pytest.mark.parametrize("name", gc.MARCH_CASES)
def test_exact_march_is_the_c_oracle_to_the_summation_bound(orc, name):
    """gi_march = exact claims the oracle's pixel choices bit for bit: every pixel of occlusion, colour and abd within the bound of
    the C oracle's value, no slack for undecided rays; the NaN pattern identical."""
    import gigs_lib
    import diff_gaussian_rasterization as dgr
    case, ref, g, _ = get_ref(name)
    N = case.W * case.H
    occ0, col0, abd0 = gc.oracle_march(orc, case)
    for mode in (dict(gi_zero_rays=z, gi_tile_log2w=t) for z in (0, 1) for t in range(7)):  # cert / interleave: projective march only
        with gigs_lib.options(gi_march="exact", **mode):
            occ = dgr._C.SSAO(*case.args, g["normal"], g["pos"])
            col, abd = dgr._C.SSR(*case.args, g["normal"], g["pos"], g["rgb"], g["albedo"], g["roughness"], g["metallic"], g["F0"])
        for k, got, want, b in (("occlusion", occ, occ0, ref["occ_bound"]), ("color", col, col0, ref["color_bound"]),
                                ("abd", abd, abd0, ref["abd_bound"])):
            e = gc.plane_errors(got.cpu().numpy().reshape(-1, N), np.asarray(want, np.float64).reshape(-1, N), b)
            assert e["violations"] == 0 and e["pattern"] == 0, (name, mode, k, e)
        np.testing.assert_array_equal(np.isnan(col.cpu().numpy().reshape(3, N)), np.isnan(col0))


@pytest.mark.parametrize("name", gc.MARCH_CASES)
def test_default_march_nan_pattern_is_the_c_oracles(orc, name):
    """SSR's NaNs -- non-finite radiance under a hit, the zero-weight ray's included -- and the non-finite population's values are
    the oracle's in every one of the 56 modes, on every pixel (gi_cases._poison keeps non-finite radiance away from the pixels an
    undecided ray lands on or next to)"""
    import gigs_lib
    import diff_gaussian_rasterization as dgr
    case, ref, g, _ = get_ref(name)
    N = case.W * case.H
    occ0, col0, abd0 = gc.oracle_march(orc, case)
    bad = ~ref["finite"]
    for mode in MODES:
        with gigs_lib.options(**mode):
            occ = dgr._C.SSAO(*case.args, g["normal"], g["pos"]).cpu().numpy().reshape(N)
            col, abd = (t.cpu().numpy().reshape(3, N) for t in dgr._C.SSR(*case.args, g["normal"], g["pos"], g["rgb"], g["albedo"],
                                                                         g["roughness"], g["metallic"], g["F0"]))
        np.testing.assert_array_equal(np.isnan(col), np.isnan(col0), err_msg=str(mode))
        np.testing.assert_array_equal(np.isnan(abd), np.isnan(abd0), err_msg=str(mode))
        for got, want in ((occ, occ0), (col, col0), (abd, abd0)):
            np.testing.assert_array_equal(got[..., bad], want[..., bad], err_msg=str(mode))
    if case.needs.get("dead_hits_nonfinite"):
        assert int(np.isnan(col0).any(0).sum()) > 0


def test_two_lights_through_the_multi_entry_points():
    """gigs_ssr_multi (marches itself) and gigs_ssr_apply_multi (gathers at a recorded list), K = 2: each light's planes against
    float64 over the default mode's hit list"""
    import gigs_lib
    lib = gigs_lib.lib()
    name = "room_37x29"
    case, ref, g, _ = get_ref(name)
    W, H = case.W, case.H
    a = tuple(float(x) if isinstance(x, float) else int(x) for x in case.args)
    s = torch.cuda.current_stream().cuda_stream
    ctx = gigs_lib.ctx_ptr()
    _, _, offsets, entries = record_hits(lib, ctx, case, g)
    dense = decode(case, offsets, entries, marched_rays(case, 0)).cpu().numpy()
    rgb = torch.stack([g["rgb"], g["rgb2"]]).contiguous()
    color, abd = torch.full((2, 3, H, W), 7.0, device=DEV), torch.full((2, 3, H, W), 7.0, device=DEV)
    gigs_lib.check(lib.gigs_ssr_multi(ctx, 2, *a, _p(g["normal"]), _p(g["pos"]), _p(rgb), _p(g["albedo"]), _p(g["roughness"]),
                                      _p(g["metallic"]), _p(g["F0"]), _p(color), _p(abd), _p(_scratch(lib, W, H)), s), "ssr_multi")
    packed = torch.empty(max(16, int(lib.gigs_ssr_apply_multi_scratch_bytes(2, W, H))), dtype=torch.uint8, device=DEV)
    color2, abd2 = torch.full((2, 3, H, W), 7.0, device=DEV), torch.full((2, 3, H, W), 7.0, device=DEV)
    gigs_lib.check(lib.gigs_ssr_apply_multi(2, W, H, float(case.gi["delta"]), _p(offsets), _p(entries), _p(g["normal"]), _p(g["pos"]),
                                            _p(rgb), _p(g["albedo"]), _p(g["metallic"]), _p(g["F0"]), _p(color2), _p(abd2), _p(packed), s),
                   "ssr_apply_multi")
    for k, plane in enumerate((None, case.g["rgb2"])):
        want = ssr_reference(case, dense, plane)
        check_ssr(case, name, want, color[k].cpu().numpy(), abd[k].cpu().numpy(), what=f"multi march light {k}")
        check_ssr(case, name, want, color2[k].cpu().numpy(), abd2[k].cpu().numpy(), what=f"multi gather light {k}")


# ---- normal derivation -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    return gc.load_bounds()


@pytest.mark.parametrize("name", list(gc.normal_cases()))
def test_depth_to_normal_and_the_fused_chain(orc, recorded, name):
    import gigs_lib
    import diff_gaussian_rasterization as dgr
    c = gc.normal_cases()[name]
    W, H, f = c["W"], c["H"], c["f"]
    rec = recorded["normal"][name]["comparator_worst"]
    n64, p64, early, _ = gr.depth_to_normal(W, H, f, f, c["viewmatrix"], c["depth"])
    n32, p32 = orc.depth_to_normal(W, H, f, f, c["viewmatrix"], c["depth"])
    vm, d = tt(c["viewmatrix"]), tt(c["depth"].reshape(1, H, W))
    nrm, pos = (t.cpu().numpy() for t in dgr._C.depth_to_normal(W, H, f, f, vm, d))
    e = gc.plane_errors(nrm, n64, np.full(n64.shape, gc.BOUND_FACTOR * rec["normal"]))
    assert e["violations"] == 0 and e["pattern"] == 0, (name, "normal", e)
    assert np.all(nrm[:, early != 0] == 0) and np.all(pos[:, early == 1] == 0)  # early-outs: exact zeros
    np.testing.assert_array_equal(pos.view(np.uint32), p32.view(np.uint32))     # depth_pos: the oracle's bits
    if min(W, H) < 2:
        return
    cn64, cp64 = gc.normal_chain(gr, c, np.float64)
    for fused in (1, 0):
        with gigs_lib.options(fused_derive=fused):
            if fused:
                cn, cp = dgr._derive_normal(W, H, f, f, vm, d)
            else:
                dfil = dgr.filters.median_blur(d[None], (3, 3))[0]
                n0, p0 = dgr._C.depth_to_normal(W, H, f, f, vm, dfil)
                cn, cp = dgr.filters.bilateral_blur(n0[None], (3, 3), 1, (3, 3))[0], dgr.filters.median_blur(p0[None], (3, 3))[0]
        for k, got, want in (("chain_normal", cn, cn64), ("chain_pos", cp, cp64)):
            e = gc.plane_errors(got.cpu().numpy(), want, np.full(want.shape, gc.BOUND_FACTOR * rec[k]))
            assert e["violations"] == 0 and e["pattern"] == 0, (name, "fused" if fused else "chain", k, e)


@pytest.mark.parametrize("name", list(gc.filter_cases()))
def test_median_and_bilateral(orc, recorded, name):
    import diff_gaussian_rasterization as dgr
    x = gc.filter_cases()[name]
    rec = recorded["filters"][name]["comparator_worst"]
    med, tap, tied = gr.median3x3(x)
    xd = tt(x)
    got = dgr.filters.median_blur(xd[None], (3, 3))[0].cpu().numpy()
    np.testing.assert_array_equal(got.view(np.uint32), orc.median3x3(x).view(np.uint32))  # bit-equal to the oracle, NaNs included
    np.testing.assert_array_equal(got, med.astype(np.float32))
    if "bilateral" in rec:
        b64 = gr.bilateral3x3(x)
        gb = dgr.filters.bilateral_blur(xd[None], (3, 3), 1.0, (3.0, 3.0))[0].cpu().numpy()
        e = gc.plane_errors(gb, b64, np.full(b64.shape, gc.BOUND_FACTOR * rec["bilateral"]))
        assert e["violations"] == 0 and e["pattern"] == 0, (name, e)
    if not np.isnan(x).any():
        # the backward routes each output's gradient to float64's chosen tap (outputs whose median is tied get no gradient here)
        C_, H, W = x.shape
        rng = np.random.default_rng(3)
        gout = np.where(tied, 0.0, rng.uniform(-1, 1, x.shape)).astype(np.float32)
        want, mag = np.zeros((C_, H + 2, W + 2)), np.zeros((C_, H + 2, W + 2))
        cc, yy, xx = np.nonzero(~tied)
        ty, tx = tap[cc, yy, xx] // 3, tap[cc, yy, xx] % 3
        np.add.at(want, (cc, yy + ty, xx + tx), gout[cc, yy, xx].astype(np.float64))
        np.add.at(mag, (cc, yy + ty, xx + tx), np.abs(gout[cc, yy, xx].astype(np.float64)))
        assert np.all(mag[:, 0] == 0) and np.all(mag[:, -1] == 0) and np.all(mag[:, :, 0] == 0) and np.all(mag[:, :, -1] == 0)
        xg = xd.clone().requires_grad_(True)
        dgr.filters.median_blur(xg[None], (3, 3))[0].backward(tt(gout))
        e = gc.plane_errors(xg.grad.cpu().numpy(), want[:, 1:-1, 1:-1], 9 * 2.0 ** -24 * mag[:, 1:-1, 1:-1])
        assert e["violations"] == 0 and e["pattern"] == 0, (name, "median backward", e)
