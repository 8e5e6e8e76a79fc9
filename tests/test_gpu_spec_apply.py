"""The table-driven GGX pre-filter (specular_apply_* in csrc/light_filter.hip) on ragged shapes, against the table-free kernels.

The table-free kernels compute every pair weight with the IEEE sequence the tables cache ("bit-identical per term"),
so the two paths differ in summation order only: the tolerance is the one test_gpu_pbr.py uses against the oracle
(rtol 2e-5 / atol 2e-6 forward, 2e-5 of the peak backward).  The shapes are chosen so that the last wave of a level is
partly empty, windows have empty faces and no candidates at all, and candidate counts are not multiples of the
kLanes * kU candidates a group of lanes consumes per iteration -- for each of the three kLanes variants, which the
spec_max8 / spec_max16 options select.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_U = 4  # candidates per lane and iteration (kU of specular_apply_body)

# (res, roughness): 6 res^2 is never a multiple of the 8 texels a wave of 8-lane groups holds.  Window sizes (computed
# from the bounds in `window_counts` and asserted below): 65..89 and 225..303 candidates with 0-2 empty faces at
# roughness 1; 0..44 at (7, 0.4), incl. counts of 32 and 33 = kLanes kU (+1) for 8 lanes; 0..24 at (9, 0.3); single
# candidates and empty windows at (5, 0.2).
CASES = [(5, 1.0), (9, 1.0), (9, 0.5), (7, 0.4), (9, 0.3), (5, 0.2)]
LANES = {8: dict(spec_max8=1 << 30, spec_max16=1 << 30), 16: dict(spec_max8=0, spec_max16=1 << 30),
         64: dict(spec_max8=0, spec_max16=0)}


@pytest.fixture(autouse=True)
def _fresh_tables():
    """No test leaves its cached (or refused) weight tables to the next one."""
    from pbr.renderutils import ops
    ops._weightTables.clear()
    yield
    ops._weightTables.clear()


def tt(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.requires_grad_(True) if grad else t


def rel_peak(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-20)


def spec_lanes_for(avg_window, max8, max16):
    """spec_lanes_for of csrc/light_filter.hip."""
    return 8 if 0 < avg_window <= max8 else 16 if 0 < avg_window <= max16 else 64


def window_counts(bounds):
    """Candidates per texel and empty faces per texel, from the [6, res, res, 24] bounds tensor."""
    b = bounds.detach().cpu().numpy().reshape(-1, 6, 4)
    w = np.where(b[..., 0] <= b[..., 1], b[..., 1] - b[..., 0] + 1, 0)
    h = np.where(b[..., 2] <= b[..., 3], b[..., 3] - b[..., 2] + 1, 0)
    cnt = (w * h).astype(np.int64)
    return cnt.sum(1), (cnt == 0).sum(1)


def level(ops, res, rough):
    cc = ops._ndf_cutoff(rough, 0.99)
    _, bounds = ops._ndf_bounds(res, rough, 0.99, torch.device(DEV))
    tables = ops._weight_tables(res, rough, 0.99, torch.device(DEV))
    assert tables is not None and tables[3] is not None, "the cached tables are what this test is about"
    return cc, bounds, tables


def fallback(ops, monkeypatch):
    """Selects the table-free kernels for ops.specular_cubemap (the environment variable is read once, at import)."""
    monkeypatch.setattr(ops, "_TABLE_MAX_BYTES", 0)
    ops._weightTables.clear()


def under(lanes, avg):
    """The library context that serves a mean window of `avg` candidates with `lanes`-lane groups."""
    import gigs_lib
    ctx = gigs_lib.options(**LANES[lanes])
    assert spec_lanes_for(avg, ctx.ctx.option("spec_max8"), ctx.ctx.option("spec_max16")) == lanes
    return ctx


def test_case_shapes_are_ragged():
    """The cases hold what the header promises (a change of the bounds kernel must not empty this file silently)."""
    from pbr.renderutils import ops
    seen_empty_window = seen_single = False
    for res, rough in CASES:
        _, bounds, tables = level(ops, res, rough)
        n, empty = window_counts(bounds)
        assert int(n.sum()) == tables[1].numel()
        assert (6 * res * res) % 8 != 0 and (6 * res * res) % 4 != 0
        assert empty.max() >= 1, "windows with empty faces"
        for lanes in LANES:
            assert (n % (lanes * K_U) != 0).any(), "candidate counts that are no multiple of kLanes kU"
        seen_empty_window |= bool((n == 0).any())
        seen_single |= bool((n == 1).any())
    assert seen_empty_window and seen_single
    n, _ = window_counts(level(ops, 7, 0.4)[1])
    assert (n == 8 * K_U).any() and (n == 8 * K_U + 1).any()  # a full batch of the 8-lane groups, and one more
    n, _ = window_counts(level(ops, 5, 1.0)[1])
    assert (n == 16 * K_U + 1).any()


@pytest.mark.parametrize("lanes", sorted(LANES))
@pytest.mark.parametrize("res,rough", CASES)
def test_table_path_matches_table_free_kernels(res, rough, lanes, monkeypatch):
    from pbr.renderutils import ops
    rng = np.random.default_rng(1000 * res + lanes)
    cm = rng.uniform(0, 1, size=(6, res, res, 3)).astype(np.float32)
    g4 = rng.normal(size=(6, res, res, 4)).astype(np.float32)
    cc, bounds, tables = level(ops, res, rough)
    n, _ = window_counts(bounds)
    avg = ops._avg_window(tables, res)
    full = tt((n > 0).reshape(6, res, res, 1).astype(np.float32))  # a window without candidates normalises to 0 / 0

    # reference: the table-free kernels, rgb and weight sum in four channels, then the public rgb / w
    x0 = tt(cm, grad=True)
    ref4 = ops._specular_cubemap.apply(x0, rough, cc, bounds, None)
    (ref4 * tt(g4)).sum().backward()
    with under(lanes, avg):
        # 1. four-channel kernels (specular_apply_kernel<., false, kLanes>)
        x1 = tt(cm, grad=True)
        out4 = ops._specular_cubemap.apply(x1, rough, cc, bounds, tables)
        (out4 * tt(g4)).sum().backward()
        np.testing.assert_allclose(out4.detach().cpu().numpy(), ref4.detach().cpu().numpy(), rtol=2e-5, atol=2e-6)
        assert rel_peak(x1.grad.cpu().numpy(), x0.grad.cpu().numpy()) < 2e-5
        # 2. normalised kernels (<., true, kLanes>) through the public entry point
        x2 = tt(cm, grad=True)
        out3 = ops.specular_cubemap(x2, rough)
        (torch.where(full > 0, out3, torch.zeros_like(out3)) * tt(g4[..., :3])).sum().backward()
        # 3. the same level through the one-launch-per-chain kernels (specular_apply_multi_kernel)
        x3 = tt(cm, grad=True)
        (lv,) = ops.specular_cubemap_levels([x3], [rough])
        (torch.where(full > 0, lv, torch.zeros_like(lv)) * tt(g4[..., :3])).sum().backward()
    fallback(ops, monkeypatch)
    xr = tt(cm, grad=True)
    ref3 = ops.specular_cubemap(xr, rough)
    assert ops._weight_tables(res, rough, 0.99, torch.device(DEV)) is None
    (torch.where(full > 0, ref3, torch.zeros_like(ref3)) * tt(g4[..., :3])).sum().backward()
    keep = (n > 0).reshape(6, res, res)
    for got, gx in ((out3, x2), (lv, x3)):
        a, b = got.detach().cpu().numpy(), ref3.detach().cpu().numpy()
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_array_equal(np.isnan(a).any(-1), ~keep)
        np.testing.assert_allclose(a[keep], b[keep], rtol=2e-5, atol=2e-6)
        # An empty window has the weight sum 0, and its texel is a candidate of its neighbours' windows: their gradient
        # is 0 / 0 in the table-free path (rgb / w through autograd) and 0 * (w / 0) with the pre-divided table -- NaN at
        # the same texels, finite and equal elsewhere.
        ga, gb = gx.grad.cpu().numpy(), xr.grad.cpu().numpy()
        np.testing.assert_array_equal(np.isnan(ga), np.isnan(gb))
        assert not np.isnan(gb).all() and (np.isnan(gb).any() <= (not keep.all()))  # NaN only where windows are empty
        fin = ~np.isnan(gb)
        assert rel_peak(ga[fin], gb[fin]) < 2e-5


@pytest.mark.parametrize("lanes", sorted(LANES))
@pytest.mark.parametrize("res,rough", [(9, 0.5), (7, 0.4)])
def test_rejected_candidates_never_touch_an_accumulator(res, rough, lanes):
    """Inf and NaN texels: a window that holds them only at rejected candidates (weight -1: inside the bounding
    rectangle, outside the cone) stays finite, and the non-finite pattern equals the table-free kernels', forward and
    backward (the backward gathers the incoming gradient through the same windows)."""
    from pbr.renderutils import ops
    rng = np.random.default_rng(7 * res + lanes)
    cc, bounds, tables = level(ops, res, rough)
    n, _ = window_counts(bounds)
    total = 6 * res * res
    bad = rng.choice(total, size=3, replace=False)
    vals = [np.inf, np.nan, -np.inf]

    def poisoned(ch):
        a = rng.uniform(0.1, 1, size=(total, ch)).astype(np.float32)
        for i, v in zip(bad, vals):
            a[i, i % 3] = v
        return a.reshape(6, res, res, ch)

    cm, g4 = poisoned(3), poisoned(4)
    # which windows hold a poisoned texel as an ACCEPTED candidate: those whose weight on it is positive, read off the
    # table-free forward of an indicator map (its kernels skip rejected candidates with a branch)
    ind = np.zeros((total, 3), np.float32)
    ind[bad, 0] = 1.0
    touched = ops._specular_cubemap.apply(tt(ind.reshape(6, res, res, 3)), rough, cc, bounds, None)[..., 0].cpu().numpy() > 0
    inside = np.zeros(total, bool)  # ... and which hold one inside a face rectangle at all
    b = bounds.cpu().numpy().reshape(total, 6, 4)
    for i in bad:
        s, y, x = i // (res * res), (i // res) % res, i % res
        inside |= (b[:, s, 0] <= x) & (x <= b[:, s, 1]) & (b[:, s, 2] <= y) & (y <= b[:, s, 3])
    rejected_only = inside & ~touched.reshape(-1)
    assert rejected_only.any(), "some window must hold a non-finite texel at rejected candidates only"

    x0 = tt(cm, grad=True)
    ref = ops._specular_cubemap.apply(x0, rough, cc, bounds, None)
    ref.backward(tt(g4))
    with under(lanes, ops._avg_window(tables, res)):
        x1 = tt(cm, grad=True)
        out = ops._specular_cubemap.apply(x1, rough, cc, bounds, tables)
        out.backward(tt(g4))
        # the pre-divided backward table and the normalising forward of the chain kernels
        x2 = tt(cm, grad=True)
        (lv,) = ops.specular_cubemap_levels([x2], [rough])
        lv.backward(tt(g4[..., :3]))
    for a, r in ((out, ref), (x1.grad, x0.grad)):
        a, r = a.detach().cpu().numpy(), r.detach().cpu().numpy()
        np.testing.assert_array_equal(np.isfinite(a), np.isfinite(r))
        np.testing.assert_array_equal(np.isnan(a), np.isnan(r))
        fin = np.isfinite(r)
        if a.shape[-1] == 4:
            np.testing.assert_allclose(a[fin], r[fin], rtol=2e-5, atol=2e-6)
        else:
            assert rel_peak(a[fin], r[fin]) < 2e-5
    o = out.detach().cpu().numpy().reshape(total, 4)
    assert np.isfinite(o[rejected_only]).all()
    assert not np.isfinite(o[touched.reshape(-1)]).all()
    # chain kernels: rgb / wsum of the same sums, and the gather of g / wsum
    want = ref.detach()[..., :3] / ref.detach()[..., 3:]
    a, r = lv.detach().cpu().numpy(), want.cpu().numpy()
    np.testing.assert_array_equal(np.isfinite(a), np.isfinite(r))
    assert np.isfinite(a.reshape(total, 3)[rejected_only & (n > 0)]).all()
    gw = ops._specular_cubemap.apply(tt(cm), rough, cc, bounds, None)[..., 3:]
    gref = torch.autograd.grad(ops._specular_cubemap.apply(x0, rough, cc, bounds, None),
                               x0, torch.cat([tt(g4[..., :3]) / gw, torch.zeros_like(gw)], -1))[0]
    np.testing.assert_array_equal(np.isfinite(x2.grad.cpu().numpy()), np.isfinite(gref.cpu().numpy()))
