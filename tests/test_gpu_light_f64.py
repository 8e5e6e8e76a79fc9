"""Per-texel float64 checks of the cubemap light filters on the device (cases, reference, metric and bounds:
tests/light_cases.py; the bounds are BOUND_FACTOR x the C oracle's recorded error, tests/golden/light_f64_bounds.json).

Every path is held to the same float64 values and the same bounds: the bounds kernel (bit-equal to the oracle's), the
table-free kernels, the table path (raw rgbw) under 8-, 16- and 64-lane groups, the normalised path through autograd
(pre-divided table) and the one-launch chain, the sparse backward entry (narrow scatter, tile gather, the fall-back of a level
over its capacity; each case reads the path taken and the count from `state`), the listed sparse forward, the diffuse filter and
cubemap_mip.  The backward reference is the TRANSPOSE of the forward; at the levels whose accepted set is not symmetric
((16, 0.22), (9, 0.3), (7, 0.4), (9, 0.5)) a gather over the texel's own window fails these tests by 0.02 ... 1.1 per texel.

The float64 reference of a level is built once per process (light_cases.level; 3 s at (32, 0.5), the largest) and every
forward is checked on every texel.  Result buffers of the direct C calls start as NaN (the table-free kernels, the scatter entry, the sparse
entries); the autograd paths allocate their own, so a NaN block of the same size is handed back to the caching allocator right
before them, and `poison_allocator` asserts that the next allocation of that size does receive it.  Every test prints
its worst error beside its bound and the share of texels widened for undecided pairs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import light_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LANES = {8: dict(spec_max8=1 << 30, spec_max16=1 << 30), 16: dict(spec_max8=0, spec_max16=1 << 30),
         64: dict(spec_max8=0, spec_max16=0)}
ALL = list(lc.LEVELS)


@pytest.fixture(scope="module")
def doc():
    return lc.load_bounds()


@pytest.fixture(autouse=True)
def _fresh_tables():
    from pbr.renderutils import ops
    ops._weightTables.clear()
    yield
    ops._weightTables.clear()


def tt(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)
    return t.requires_grad_(True) if grad else t


def nan_buffer(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def poison_allocator(*shape):
    """Leaves a NaN block of this size in the caching allocator for the next torch.empty of the same size."""
    t = nan_buffer(*shape)
    torch.cuda.synchronize()
    del t
    # freeing a block restores the allocator's state, so the next request of this size is served like this one
    probe = torch.empty(shape, dtype=torch.float32, device=DEV)
    assert bool(torch.isnan(probe).all()), "the allocator did not hand the NaN block back"
    del probe


def stream():
    return torch.cuda.current_stream().cuda_stream


def device_level(lv):
    from pbr.renderutils import ops
    cc, bounds = ops._ndf_bounds(lv.res, lv.rough_arg, lc.CUTOFF, torch.device(DEV))
    assert float(np.float32(cc)) == lv.cc, "the library's cutoff and the oracle's restatement round to one float32"
    return cc, bounds


def check(doc, lv, tensor, inp, got, what, section="levels"):
    """Asserts `got` against the float64 reference of (tensor, input) under the recorded bound; prints the figures."""
    x = lc.inputs(lv)[(tensor, inp)] if section == "levels" else lc.zero_undecided_outputs(lv, lc.sparse_grad(lv))
    ref, slack = _reference(lv, tensor, inp, x)
    b = lc.bound(doc, lv.name, tensor, inp, section)
    plain, over, excess = lc.judge(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, ref, slack, b)
    print(f"{lv.name} {what} {tensor}/{inp}: worst {plain:.3e} bound {b:.3e}; widened texels {(slack > 0).mean():.4f}")
    assert over == 0, (lv.name, what, tensor, inp, f"{over} texels over their bound, worst excess {excess:.3e}", plain, b)
    return plain


_refs = {}


def _reference(lv, tensor, inp, x):
    key = (lv.name, tensor, inp)
    if key not in _refs:
        _refs[key] = lc.reference(lv, tensor, x)
    return _refs[key]


# ---- bounds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + list(lc.SPARSE_ONLY))
def test_bounds_bit_equal_to_the_oracle(orc, name):
    lv = lc.level(orc, name)
    _, bounds = device_level(lv)
    np.testing.assert_array_equal(bounds.cpu().numpy().reshape(-1).view(np.uint32), lv.bounds32.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("name", ALL)
def test_symmetry_verdict_matches_the_structure(orc, name):
    import gigs_lib
    lv = lc.level(orc, name)
    got = gigs_lib.check(gigs_lib.lib().gigs_specular_window_symmetric(lv.res, lv.cc, stream()), "specular_window_symmetric")
    assert bool(got) == (not lc.LEVELS[name][2]["asym"])


# ---- table-free kernels (direct C calls, NaN-filled results) ---------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_table_free_kernels(orc, doc, name):
    import gigs_lib
    lib = gigs_lib.lib()
    lv = lc.level(orc, name)
    cc, bounds = device_level(lv)
    for (tensor, inp), x in lc.inputs(lv).items():
        if tensor == "fwd":
            out = nan_buffer(lv.T, 4)
            gigs_lib.check(lib.gigs_specular_cubemap_fwd(lv.res, tt(x).data_ptr(), bounds.data_ptr(), lv.rough_arg, cc,
                                                         out.data_ptr(), stream()), "specular_cubemap_fwd")
            check(doc, lv, tensor, inp, out, "table-free")
        elif tensor == "bwd":
            g4 = np.concatenate([x, np.full((lv.T, 1), 0.5, np.float32)], 1)  # the gradient of wsum does not reach the map
            out = nan_buffer(lv.T, 3)
            gigs_lib.check(lib.gigs_specular_cubemap_bwd(lv.res, bounds.data_ptr(), tt(g4).data_ptr(), lv.rough_arg, cc,
                                                         out.data_ptr(), stream()), "specular_cubemap_bwd")
            check(doc, lv, tensor, inp, out, "table-free")


# ---- table path, raw rgbw, per lane width ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", sorted(LANES))
@pytest.mark.parametrize("name", ALL)
def test_table_path_raw(orc, doc, name, lanes):
    import gigs_lib
    from pbr.renderutils import ops
    lv = lc.level(orc, name)
    cc, bounds = device_level(lv)
    tables = ops._weight_tables(lv.res, lv.rough_arg, lc.CUTOFF, torch.device(DEV))
    assert tables is not None and tables.symmetric == (not lc.LEVELS[name][2]["asym"])
    shp = (6, lv.res, lv.res)
    ins = lc.inputs(lv)
    with gigs_lib.options(**LANES[lanes]):
        for (tensor, inp), x in ins.items():
            if tensor != "fwd" or inp not in ("hdr", "onehot0", "onehot3"):
                continue
            x = tt(x.reshape(*shp, 3))
            poison_allocator(*shp, 4)
            out = ops._specular_cubemap.apply(x, lv.rough_arg, cc, bounds, tables)
            check(doc, lv, "fwd", inp, out.reshape(lv.T, 4), f"table {lanes} lanes")
        for inp in ("dense", "sparse"):
            g = ins[("bwd", inp)]
            x = tt(ins[("fwd", "hdr")].reshape(*shp, 3), grad=True)
            out = ops._specular_cubemap.apply(x, lv.rough_arg, cc, bounds, tables)
            g4 = np.concatenate([g, np.full((lv.T, 1), 0.5, np.float32)], 1)
            g4 = tt(g4.reshape(*shp, 4))
            poison_allocator(*shp, 3)
            out.backward(g4)
            check(doc, lv, "bwd", inp, x.grad.reshape(lv.T, 3), f"table {lanes} lanes")


# ---- normalised path through autograd (pre-divided table) ----------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_normalised_path_through_autograd(orc, doc, name):
    from pbr.renderutils import ops
    lv = lc.level(orc, name)
    shp = (6, lv.res, lv.res, 3)
    ins = lc.inputs(lv)
    for (tensor, inp), x in ins.items():
        if tensor == "fwd_norm":
            x = tt(x.reshape(shp))
            poison_allocator(*shp)
            out = ops.specular_cubemap(x, lv.rough_arg)
            check(doc, lv, tensor, inp, out.reshape(lv.T, 3), "normalised")
    tables = ops._weight_tables(lv.res, lv.rough_arg, lc.CUTOFF, torch.device(DEV))
    assert tables.bwd_scaled is not None, "the pre-divided table is what this test is about"
    for inp in ("dense", "sparse"):
        x = tt(ins[("fwd_norm", "hdr")].reshape(shp), grad=True)
        out = ops.specular_cubemap(x, lv.rough_arg)
        g = tt(ins[("bwd_norm", inp)].reshape(shp))
        poison_allocator(*shp)
        out.backward(g)
        check(doc, lv, "bwd_norm", inp, x.grad.reshape(lv.T, 3), "normalised")


@pytest.mark.parametrize("chain", [("64_0.22", "32_0.5", "16_1.0"), ("32_0.22", "16_0.22", "9_0.3"), ("7_0.4",)])
def test_chain_in_one_launch(orc, doc, chain):
    """specular_cubemap_levels: the standard-shaped chain, a chain that mixes symmetric and asymmetric levels (the latter leave
    the shared launch for the scatter), and a chain of one asymmetric level."""
    from pbr.renderutils import ops
    lvs = [lc.level(orc, n) for n in chain]
    for inp in ("dense", "sparse"):
        xs = [tt(lc.inputs(lv)[("fwd_norm", "hdr")].reshape(6, lv.res, lv.res, 3), grad=True) for lv in lvs]
        for lv in lvs[::-1]:
            poison_allocator(6, lv.res, lv.res, 3)
        outs = ops.specular_cubemap_levels(xs, [lv.rough_arg for lv in lvs])
        assert outs is not None
        gs = [tt(lc.inputs(lv)[("bwd_norm", inp)].reshape(6, lv.res, lv.res, 3)) for lv in lvs]
        for lv in lvs[::-1]:
            poison_allocator(6, lv.res, lv.res, 3)
        torch.autograd.backward(outs, gs)
        for lv, o, x in zip(lvs, outs, xs):
            if inp == "dense":
                check(doc, lv, "fwd_norm", "hdr", o.reshape(lv.T, 3), "chain")
            check(doc, lv, "bwd_norm", inp, x.grad.reshape(lv.T, 3), "chain")


# ---- the scatter entry, called directly into NaN buffers ---------------------------------------------------------------------
@pytest.mark.parametrize("name", lc.ASYMMETRIC + ["16_0.08", "32_0.22"])
def test_scatter_entry_direct(orc, doc, name):
    """gigs_specular_cubemap_bwd_scatter_w is the transpose at ANY level: the asymmetric ones, a level of mostly empty windows
    (every texel still has to be written: the entry clears the buffer) and a symmetric one.  Raw (no wsum, four-channel
    gradient) and normalised (wsum, three channels)."""
    import gigs_lib
    from pbr.renderutils import ops
    lib = gigs_lib.lib()
    lv = lc.level(orc, name)
    _, bounds = device_level(lv)
    t = ops._weight_tables(lv.res, lv.rough_arg, lc.CUTOFF, torch.device(DEV))
    ins = lc.inputs(lv)
    for inp in ("dense", "sparse"):
        g4 = tt(np.concatenate([ins[("bwd", inp)], np.full((lv.T, 1), 0.5, np.float32)], 1))
        out = nan_buffer(lv.T, 3)
        gigs_lib.check(lib.gigs_specular_cubemap_bwd_scatter_w(lv.res, bounds.data_ptr(), t.offsets.data_ptr(), t.fwd.data_ptr(), None,
                                                               g4.data_ptr(), 0, out.data_ptr(), stream()), "bwd_scatter_w")
        check(doc, lv, "bwd", inp, out, "scatter entry")
        g3 = tt(ins[("bwd_norm", inp)])
        out = nan_buffer(lv.T, 3)
        gigs_lib.check(lib.gigs_specular_cubemap_bwd_scatter_w(lv.res, bounds.data_ptr(), t.offsets.data_ptr(), t.fwd.data_ptr(),
                                                               t.wsum.data_ptr(), g3.data_ptr(), 1, out.data_ptr(), stream()),
                       "bwd_scatter_w")
        check(doc, lv, "bwd_norm", inp, out, "scatter entry")


# ---- sparse backward entry ---------------------------------------------------------------------------------------------
# (level, capacity in permille, path expected: True = a sparse path).  avg window <= 256: narrow scatter; else tile gather
SPARSE_CASES = [("32_0.22", 100, True), ("64_0.22", 100, True), ("64_0.08", 100, True),     # scatter, narrow
                ("16_1.0", 100, True), ("32_0.5", 100, True), ("64_0.36", 100, True),       # tile gather: 1, 4, 16 tiles a face
                ("32_0.22", 1, False), ("64_0.36", 1, False)]                                # over the capacity: falls back


@pytest.mark.parametrize("name,permille,sparse", SPARSE_CASES)
def test_sparse_backward_entry(orc, doc, name, permille, sparse):
    import test_gpu_spec_sparse as sps
    lv = lc.level(orc, name)
    g = lc.zero_undecided_outputs(lv, lc.sparse_grad(lv))
    count = int((g != 0).any(1).sum())
    dl = sps.level(lv.res, lv.rough_arg)
    np.testing.assert_array_equal(dl["bounds"].cpu().numpy().reshape(-1), lv.bounds32.reshape(-1))
    (got,), ((took_sparse, n),) = sps.run([dl], [g], sparse=True, permille=permille)
    cap = 6 * lv.res ** 2 * permille // 1000
    narrow = dl["avg"] <= 256
    print(f"{name}: count {n} capacity {cap} sparse {took_sparse} ({'scatter' if narrow else 'tile gather'}, mean window {dl['avg']})")
    assert n == count and took_sparse == sparse and (count <= cap) == sparse
    check(doc, lv, "bwd_norm", "sparse", got, "sparse entry", "sparse" if name in lc.SPARSE_ONLY else "levels")


def test_sparse_cases_take_both_sparse_paths():
    import test_gpu_spec_sparse as sps
    kinds = {(sps.level(*(lc.LEVELS.get(n) or lc.SPARSE_ONLY[n])[:2])["avg"] <= 256) for n, _, s in SPARSE_CASES if s}
    assert kinds == {True, False}


# ---- listed sparse forward ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [("64_0.22", "32_0.5"), ("32_0.22", "16_1.0")])
def test_listed_sparse_forward(orc, doc, names):
    """gigs_specular_cubemap_multi_fwd_sparse with the probe texels marked: listed texels against float64, the others still
    hold the poison."""
    import gigs_lib
    from pbr.renderutils import ops
    lib = gigs_lib.lib()
    lvs = [lc.level(orc, n) for n in names]
    n = len(lvs)
    POISON = -12345.0
    arr = (gigs_lib.SpecLevel * n)()
    needed, caps, keep, outs = (C.c_void_p * n)(), (C.c_int * n)(), [], []
    for i, lv in enumerate(lvs):
        _, bounds = device_level(lv)
        t = ops._weight_tables(lv.res, lv.rough_arg, lc.CUTOFF, torch.device(DEV))
        src = tt(lc.inputs(lv)[("fwd_norm", "hdr")])
        out, ws = torch.full((lv.T, 3), POISON, device=DEV), torch.full((lv.T,), POISON, device=DEV)
        mark = torch.zeros((lv.T, 3), device=DEV)
        mark[torch.from_numpy(lc.probes(lv.res)).to(DEV), 1] = 1.0
        arr[i] = gigs_lib.SpecLevel(lv.res, ops._avg_window(t, lv.res), src.data_ptr(), bounds.data_ptr(), t.offsets.data_ptr(),
                                    t.fwd.data_ptr(), out.data_ptr(), ws.data_ptr())
        needed[i], caps[i] = mark.data_ptr(), lv.T // 4
        keep += [src, ws, mark, t]
        outs.append(out)
    state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=DEV)
    lists = torch.empty(sum(caps), dtype=torch.int32, device=DEV)
    gigs_lib.check(lib.gigs_specular_cubemap_multi_fwd_sparse(gigs_lib.ctx_ptr(), n, C.cast(arr, C.c_void_p), needed, caps,
                                                              state.data_ptr(), lists.data_ptr(), stream()),
                   "specular_cubemap_multi_fwd_sparse")
    torch.cuda.synchronize()
    st = state.cpu().tolist()
    for i, (lv, out) in enumerate(zip(lvs, outs)):
        pr = lc.probes(lv.res)
        assert st[8 + i] == 1 and st[16 + i] == pr.size, st
        got = out.cpu().numpy()
        listed = np.zeros(lv.T, bool)
        listed[pr] = True
        assert (got[~listed] == POISON).all(), "a texel that is not listed was written"
        ref, slack = _reference(lv, "fwd_norm", "hdr", lc.inputs(lv)[("fwd_norm", "hdr")])
        full = np.where(listed[:, None], got, ref)  # judged on the listed rows; the others are the reference itself
        b = lc.bound(doc, lv.name, "fwd_norm", "hdr")
        plain, over, excess = lc.judge(full, ref, slack, b)
        print(f"{lv.name} listed forward: {pr.size} texels, worst {plain:.3e} bound {b:.3e}")
        assert over == 0, (over, excess)


# ---- diffuse filter and mip ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", lc.DIFFUSE_RES)
def test_diffuse_filter(doc, res):
    from pbr.renderutils import ops
    tex, f64, g, b64 = lc.diffuse_reference(res)
    x = tt(tex, grad=True)
    poison_allocator(6, res, res, 3)
    y = ops.diffuse_cubemap(x)
    g = tt(g)
    poison_allocator(6, res, res, 3)
    y.backward(g)
    for what, got, ref in (("fwd", y, f64), ("bwd", x.grad, b64)):
        e = lc.row_errors(got.detach().cpu().numpy().reshape(-1, 3), ref).max()
        b = lc.BOUND_FACTOR * max(doc["small"][f"diffuse{res}"][what], lc.ROUND_OFF)
        print(f"diffuse {res} {what}: worst {e:.3e} bound {b:.3e}")
        assert e <= b


@pytest.mark.parametrize("res", lc.MIP_RES)
def test_cubemap_mip(doc, res):
    from pbr.light import cubemap_mip
    tex, f64, g, b64 = lc.mip_reference(res)
    x, g = tt(tex, grad=True), tt(g)
    poison_allocator(6, res // 2, res // 2, 3)
    y = cubemap_mip.apply(x)
    poison_allocator(6, res, res, 3)
    y.backward(g)
    for what, got, ref in (("fwd", y, f64), ("bwd", x.grad, b64)):
        e = lc.row_errors(got.detach().cpu().numpy().reshape(-1, 3), ref).max()
        b = lc.BOUND_FACTOR * max(doc["small"][f"mip{res}"][what], lc.ROUND_OFF)
        print(f"mip {res} {what}: worst {e:.3e} bound {b:.3e}")
        assert e <= b
