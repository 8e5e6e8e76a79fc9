"""The sparse GGX backward (gigs_specular_cubemap_multi_bwd_sparse in csrc/light_filter.hip): census of the nonzero gradient
texels, a sparse path for the levels whose list fits its capacity, gather of the others.

The level API is driven directly, one level per call at res 16 and 32 with roughness 0.08, 0.22 and 1.0 (8-, 16- and
64-lane gathers, windows over one to six faces), plus one two-level chain whose levels take different paths.  Every
case reads the path taken and the count from the state buffer, so none can pass without entering a sparse path.
There are two sparse paths, chosen per level on the host: a level whose mean window holds at most 256 candidates is
SCATTERED, one wave per listed texel adding into memory with float atomics; a level with wider windows is summed on chip
by the workgroups that own 16 x 16-texel tiles of the destination (the tile gather, tests/test_gpu_spec_tile_gather.py).
Res 64 at roughness 0.08, 0.28 and 0.36 adds what res 16 and 32 cannot show: windows of several waves' worth of candidates
(0.28) and faces of more than one tile (0.36).  (scatter_plan below restates an earlier host rule, 32 x 32 LDS tiles; it
only serves test_levels_cover_the_three_lane_classes, which asks the levels for narrow and wide windows.)

Accuracy: the reference is formed in float64 from the forward table and the forward's weight sums (the float32 quotient
w / wsum, as both paths use it, times the gradient) -- sums formed from the library's own tables: the float64 check of
these paths against independent values is tests/test_gpu_light_f64.py.  The sparse result's largest deviation from it
may be at most 4x the gather's on the same input (floor: one ulp of the largest output magnitude): the scatter's additions
arrive in any order, the gather's order is fixed.  This reference is the TRANSPOSE of the forward; the gather is one only
where the level's accepted set is symmetric.  (16, 0.22) is not such a level (the bounds' tile cull drops in-cone
texels): there the gather's own deviation from this reference is of the order of the values, so the 4x rule holds the
scatter to nothing at that level -- pbr.renderutils.ops never gathers it (WeightTables.symmetric), and the float64
suite checks what it does instead.  A gradient over the capacity must give the bits of gigs_options.spec_sparse = 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LEVELS = [(16, 0.08), (16, 0.22), (16, 1.0), (32, 0.08), (32, 0.22), (32, 1.0), (64, 0.08), (64, 0.28), (64, 0.36)]
PERMILLE = 100  # capacity of the tests: a tenth of a level's texels
_cache = {}


def spec_lanes_for(avg_window, max8=128, max16=1500):
    """spec_lanes_for of csrc/light_filter.hip at the default thresholds."""
    return 8 if 0 < avg_window <= max8 else 16 if 0 < avg_window <= max16 else 64


def scatter_plan(res, avg_window):
    """(wide, chunks, tiles per face) as gigs_specular_cubemap_multi_bwd_sparse of csrc/light_filter.hip chooses them."""
    wide = avg_window * 16 >= 6 * res * res
    return wide, min(32, max(1, (max(1, avg_window) + 255) // 256)), ((res + 31) // 32) ** 2


def candidates(lv, o):
    """The candidate texel indices of texel o's window in table order: face rectangles in face order, row-major."""
    res, idx = lv["res"], []
    for s in range(6):
        x0, x1, y0, y1 = lv["b"][o, s]
        if x0 > x1 or y0 > y1:
            continue
        yy, xx = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        idx.append(((s * res + yy) * res + xx).reshape(-1))
    return np.concatenate(idx) if idx else np.zeros(0, np.int64)


def level(res, rough):
    """Device tables of a level plus host copies of its bounds, offsets, forward table and weight sums."""
    key = (res, rough)
    if key not in _cache:
        from pbr.renderutils import ops
        ops._weightTables.pop((res, rough, 0.99, DEV), None)
        _, bounds = ops._ndf_bounds(res, rough, 0.99, torch.device(DEV))
        tables = ops._weight_tables(res, rough, 0.99, torch.device(DEV))
        assert tables is not None and tables[3] is not None and tables[4] is not None
        b = bounds.cpu().numpy().reshape(-1, 6, 4).astype(np.int64)
        _cache[key] = dict(res=res, rough=rough, bounds=bounds, tables=tables, b=b,
                           off=tables[0].cpu().numpy().astype(np.int64).reshape(-1, 6)[:, 0],
                           wf=tables[1].cpu().numpy(), wsum=tables[4].cpu().numpy().reshape(-1),
                           avg=ops._avg_window(tables, res))
    return _cache[key]


def reference(lv, g):
    """float64 sum of float32(w / wsum[o]) * g[o] over the accepted candidates of every texel o with a nonzero gradient."""
    total = 6 * lv["res"] ** 2
    g = g.reshape(total, 3)
    where, terms = [np.zeros(0, np.int64)], [np.zeros((0, 3), np.float64)]
    with np.errstate(all="ignore"):
        for o in np.flatnonzero((g != 0).any(1)):
            c = candidates(lv, o)
            w = lv["wf"][lv["off"][o]:lv["off"][o] + len(c)]
            ok = w >= 0
            q = (w[ok] / np.float32(lv["wsum"][o])).astype(np.float32)  # the float32 quotient of the pre-divided table
            where.append(c[ok])
            terms.append(q.astype(np.float64)[:, None] * g[o].astype(np.float64)[None, :])
        where, terms = np.concatenate(where), np.concatenate(terms)
        return np.stack([np.bincount(where, terms[:, ch], minlength=total) for ch in range(3)], 1)


def run(lvs, grads, sparse, permille=PERMILLE):
    """One call of the entry point on the chain `lvs`; returns ([dst per level], [(scattered, count) per level])."""
    import gigs_lib
    from pbr.renderutils import ops
    lib = gigs_lib.lib()
    n = len(lvs)
    arr = (gigs_lib.SpecLevel * n)()
    wf, ws = (C.c_void_p * n)(), (C.c_void_p * n)()
    srcs = [torch.from_numpy(np.ascontiguousarray(g, np.float32)).to(DEV) for g in grads]
    dsts = [torch.full((6 * lv["res"] ** 2, 3), 7.0, device=DEV) for lv in lvs]  # the census must clear what is there
    for i, (lv, s, d) in enumerate(zip(lvs, srcs, dsts)):
        t = lv["tables"]
        arr[i] = gigs_lib.SpecLevel(lv["res"], lv["avg"], s.data_ptr(), lv["bounds"].data_ptr(), t[0].data_ptr(),
                                    t[3].data_ptr(), d.data_ptr(), None)
        wf[i], ws[i] = t[1].data_ptr(), t[4].data_ptr()
    with gigs_lib.options(spec_sparse=int(sparse), spec_sparse_permille=permille):
        caps = [lib.gigs_spec_sparse_capacity(gigs_lib.ctx_ptr(), lv["res"]) for lv in lvs]
        assert caps == [6 * lv["res"] ** 2 * permille // 1000 for lv in lvs]
        state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=DEV)
        lists = torch.full((max(1, sum(caps)),), -1, dtype=torch.int32, device=DEV)
        for _ in range(2):  # twice: the second call relies on the counters the first one cleared
            gigs_lib.check(lib.gigs_specular_cubemap_multi_bwd_sparse(
                gigs_lib.ctx_ptr(), n, C.cast(arr, C.c_void_p), wf, ws, state.data_ptr(), lists.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "specular_cubemap_multi_bwd_sparse")
        torch.cuda.synchronize()
    st = state.cpu().tolist()
    if sparse:
        assert st[:8] == [0] * 8, "the working counters are cleared for the next call"
    return [d.cpu().numpy() for d in dsts], [(bool(st[8 + i]), st[16 + i]) for i in range(n)]


def texel(res, face, y, x):
    return (face * res + y) * res + x


def gradients(res, rng, cap):
    """name -> ([total, 3] gradient, expected count of nonzero texels)."""
    total = 6 * res * res
    out = {}

    def at(idx, vals=None):
        g = np.zeros((total, 3), np.float32)
        g[idx] = rng.normal(size=(len(idx), 3)).astype(np.float32) if vals is None else vals
        return g

    out["zero"] = at([])
    out["face_centre"] = at([texel(res, 2, res // 2, res // 2)])
    out["face_edge"] = at([texel(res, 1, res // 2, res - 1)])
    out["cube_corner"] = at([texel(res, 4, 0, 0)])
    out["face_row"] = at([texel(res, 3, 5, x) for x in range(res)])
    out["random_5pct"] = at(rng.choice(total, size=total // 20, replace=False))
    out["capacity"] = at(rng.choice(total, size=cap, replace=False))
    g = at([texel(res, 0, 3, 4)])
    g[texel(res, 0, 3, 4)] = (0.0, -0.0, 1.5)  # one channel only
    g[texel(res, 5, 7, 7)] = (-0.0, -0.0, -0.0)  # -0 is not nonzero
    g[texel(res, 2, 1, 1)] = (-0.0, 0.0, -0.0)
    out["minus_zero"] = g
    g = at(rng.choice(total, size=9, replace=False))
    g[texel(res, 1, 2, 3)] = (np.nan, 0.0, 0.0)
    g[texel(res, 4, res - 1, res - 1)] = (0.0, np.inf, -1.0)
    out["nan_inf"] = g
    return {k: (v, int((v != 0).any(1).sum())) for k, v in out.items()}


def deviation(a, ref, gather=False):
    """Largest |a - ref| over the finite entries; the scatter's non-finite entries must agree in kind with the reference's.
    The gather may hold further NaNs: the bounds kernel's tile test is not conservative where a direction component peaks
    inside a 16-texel tile (res 16: the face centre), so a texel's window can be empty, its weight sum 0, while it is a
    candidate of its neighbours -- 0 * (w / 0) in the pre-divided table.  Those entries are left out of its deviation."""
    fin = np.isfinite(ref)
    if gather:
        fin &= np.isfinite(a)
    else:
        np.testing.assert_array_equal(np.isnan(a), np.isnan(ref))
        np.testing.assert_array_equal(np.isposinf(a), np.isposinf(ref))
        np.testing.assert_array_equal(np.isneginf(a), np.isneginf(ref))
    return float(np.abs(a.astype(np.float64)[fin] - ref[fin]).max()) if fin.any() else 0.0


def test_levels_cover_the_three_lane_classes():
    assert {spec_lanes_for(level(r, a)["avg"]) for r, a in LEVELS} == {8, 16, 64}
    plans = {(r, a): scatter_plan(r, level(r, a)["avg"]) for r, a in LEVELS}
    print("scatter plans (wide, chunks, tiles):", plans)
    narrow = [p for p in plans.values() if not p[0]]
    wide = [p for p in plans.values() if p[0]]
    assert any(p[1] == 1 for p in narrow) and any(p[1] > 1 for p in narrow), plans  # one wave per window, and several
    assert any(p[2] == 1 for p in wide) and any(p[2] > 1 for p in wide), plans  # one tile per face, and several
    faces = set()
    for r, a in LEVELS:
        lv = level(r, a)
        b = lv["bounds"].cpu().numpy().reshape(-1, 6, 4)
        faces |= set(((b[..., 0] <= b[..., 1]) & (b[..., 2] <= b[..., 3])).sum(1).tolist())
    assert {1, 6} <= faces, faces


@pytest.mark.parametrize("res,rough", LEVELS)
def test_scatter_matches_float64_reference(res, rough):
    lv = level(res, rough)
    total = 6 * res * res
    cap = total * PERMILLE // 1000
    rng = np.random.default_rng(100 * res + int(100 * rough))
    for name, (g, count) in gradients(res, rng, cap).items():
        (sp,), ((scattered, n),) = run([lv], [g], sparse=True)
        assert scattered and n == count, (name, scattered, n, count)
        (de,), _ = run([lv], [g], sparse=False)
        ref = reference(lv, g)
        dev_s, dev_d = deviation(sp, ref), deviation(de, ref, gather=True)
        peak = float(np.abs(ref[np.isfinite(ref)]).max()) if np.isfinite(ref).any() else 0.0
        floor = float(np.spacing(np.float32(peak)))
        print(f"res {res} roughness {rough} {name}: count {n} peak {peak:.3e} sparse dev {dev_s:.3e} dense dev {dev_d:.3e} "
              f"floor {floor:.3e}")
        assert dev_s <= 4.0 * max(dev_d, floor), (name, dev_s, dev_d, floor)
        if name == "zero":
            assert not sp.any()


@pytest.mark.parametrize("res,rough", LEVELS)
def test_over_capacity_takes_the_gather_bit_for_bit(res, rough):
    lv = level(res, rough)
    total = 6 * res * res
    cap = total * PERMILLE // 1000
    rng = np.random.default_rng(res + 7)
    for count in (cap + 1, total):
        g = np.zeros((total, 3), np.float32)
        idx = rng.choice(total, size=count, replace=False)
        g[idx] = rng.normal(size=(count, 3)).astype(np.float32)
        g[idx, 0] += 4.0  # no texel rounds to all-zero
        (sp,), ((scattered, n),) = run([lv], [g], sparse=True)
        assert not scattered and n == count
        (de,), _ = run([lv], [g], sparse=False)
        np.testing.assert_array_equal(sp.view(np.uint32), de.view(np.uint32))


def test_chain_with_mixed_paths():
    """Two levels in one call: the first over its capacity (gathered), the second sparse (scattered), and the reverse."""
    lvs = [level(32, 0.22), level(16, 1.0)]
    rng = np.random.default_rng(5)
    dense = [rng.normal(size=(6 * lv["res"] ** 2, 3)).astype(np.float32) + 3.0 for lv in lvs]
    sparse = []
    for lv in lvs:
        g = np.zeros((6 * lv["res"] ** 2, 3), np.float32)
        g[rng.choice(len(g), size=11, replace=False)] = rng.normal(size=(11, 3)).astype(np.float32)
        sparse.append(g)
    for grads, want in (([dense[0], sparse[1]], [False, True]), ([sparse[0], dense[1]], [True, False])):
        got, rep = run(lvs, grads, sparse=True)
        ref, _ = run(lvs, grads, sparse=False)
        assert [r[0] for r in rep] == want and [r[1] for r in rep] == [int((g != 0).any(1).sum()) for g in grads]
        for i, lv in enumerate(lvs):
            if want[i]:
                r64 = reference(lv, grads[i])
                dev_s, dev_d = deviation(got[i], r64), deviation(ref[i], r64, gather=True)
                assert dev_s <= 4.0 * max(dev_d, float(np.spacing(np.float32(np.abs(r64).max())))), (dev_s, dev_d)
            else:
                np.testing.assert_array_equal(got[i].view(np.uint32), ref[i].view(np.uint32))


def test_graph_replay_switches_paths():
    """Captured once with a sparse gradient; replayed with a dense one, then with a sparse one again: every replay equals
    the eager result of its own path, and the state buffer reports that path."""
    import gigs_lib
    lib = gigs_lib.lib()
    lv = level(32, 0.22)
    total = 6 * 32 * 32
    rng = np.random.default_rng(11)
    g_sparse = np.zeros((total, 3), np.float32)
    g_sparse[rng.choice(total, size=40, replace=False)] = rng.normal(size=(40, 3)).astype(np.float32)
    g_dense = rng.normal(size=(total, 3)).astype(np.float32) + 3.0
    eager = {"sparse": run([lv], [g_sparse], sparse=True)[0][0], "dense": run([lv], [g_dense], sparse=True)[0][0]}
    r64 = reference(lv, g_sparse)
    bound = 4.0 * max(deviation(run([lv], [g_sparse], sparse=False)[0][0], r64, gather=True), float(np.spacing(np.float32(np.abs(r64).max()))))

    t = lv["tables"]
    src = torch.from_numpy(g_sparse).to(DEV)
    dst = torch.empty((total, 3), device=DEV)
    arr = (gigs_lib.SpecLevel * 1)()
    arr[0] = gigs_lib.SpecLevel(32, lv["avg"], src.data_ptr(), lv["bounds"].data_ptr(), t[0].data_ptr(), t[3].data_ptr(),
                                dst.data_ptr(), None)
    wf, ws = (C.c_void_p * 1)(t[1].data_ptr()), (C.c_void_p * 1)(t[4].data_ptr())
    with gigs_lib.options(spec_sparse=1, spec_sparse_permille=PERMILLE):
        state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=DEV)
        lists = torch.empty(lib.gigs_spec_sparse_capacity(gigs_lib.ctx_ptr(), 32), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                gigs_lib.check(lib.gigs_specular_cubemap_multi_bwd_sparse(
                    gigs_lib.ctx_ptr(), 1, C.cast(arr, C.c_void_p), wf, ws, state.data_ptr(), lists.data_ptr(),
                    torch.cuda.current_stream().cuda_stream), "specular_cubemap_multi_bwd_sparse")
        torch.cuda.current_stream().wait_stream(side)
    for kind, g in (("dense", g_dense), ("sparse", g_sparse)):
        src.copy_(torch.from_numpy(g))
        graph.replay()
        torch.cuda.synchronize()
        st = state.cpu().tolist()
        assert st[8] == (1 if kind == "sparse" else 0) and st[16] == int((g != 0).any(1).sum()) and st[0] == 0
        got = dst.cpu().numpy()
        if kind == "dense":
            np.testing.assert_array_equal(got.view(np.uint32), eager["dense"].view(np.uint32))
        else:
            assert deviation(got, r64) <= bound
            assert deviation(eager["sparse"], r64) <= bound


def test_stage2_step_sparse_against_gather():
    """A small Stage2Step with spec_sparse = 1 against 0, the capacity at a tenth of a level.  The materials are rough but
    for a few Gaussians, so the light's finest level (64^2) receives its gradient from those and from the silhouettes
    (blended roughness below 0.5) only: about 7 % of its texels, scattered (asserted, with a count above 0), while the
    coarse levels are gathered.  The loss and the rendered image never see the GGX backward and are bit-identical.  The
    per-Gaussian gradients (albedo, roughness, metallic) come out of the rasterizer's backward, which sums with float
    atomics: two runs of the gather differ in them by an ulp, so for a key whose two gather runs differ the sparse run is held
    to that run-to-run deviation instead (the keys are printed).  Only the light's gradient passes through the GGX backward: it stays within 4x the
    gather's own run-to-run deviation (the shade backward feeds it through float atomics; floor: one ulp of the largest
    magnitude), every other output is bit-identical."""
    import gigs_lib
    import pbr
    import pipeline
    import scenes
    from helpers import GAUSS_KEYS
    from pbr.renderutils import ops

    def tt(a, grad=False):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        return t.requires_grad_(True) if grad else t

    sc = dict(scenes.surface_scene(P=4000, sh_degree=2, seed=21, scale_mu=0.03))
    rough = np.full_like(sc["roughness"], 0.9)
    rough[::500] = 0.1
    sc["roughness"] = rough
    H = W = 128
    cam = scenes.orbit_camera(0, 6, W, H, radius=3.5)
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    torch.manual_seed(3)
    gt = torch.rand(3, H, W, device=DEV) * 0.5
    lut = pbr.get_brdf_lut().to(DEV)
    vd = pipeline.view_dirs_for(camt, pipeline.canonical_rays(cam, DEV), DEV)

    def step(sparse):
        torch.manual_seed(6)
        light = pbr.CubemapLight(base_res=64, device=DEV)
        g = {k: tt(sc[k], grad=True) for k in GAUSS_KEYS}
        with gigs_lib.options(spec_sparse=int(sparse), spec_sparse_permille=PERMILLE):
            st = pipeline.Stage2Step(light, lut, scenes.GI_DEFAULTS, 2, fused=True, graphs=False)
            o = st(camt, g, gt, vd)
            torch.cuda.synchronize()
            shapes = [int(s.shape[1]) for s in light.specular]
            rep = ops.spec_sparse_report(shapes, torch.device(DEV)) if sparse else None
        outs = {k: g[k].grad.clone() for k in GAUSS_KEYS if g[k].grad is not None}
        outs["loss"], outs["render_rgb"] = torch.tensor([float(o["loss"])], dtype=torch.float64), o["render_rgb"].clone()
        return outs, light.base.grad.cpu().numpy().astype(np.float64), rep

    d1, l1, _ = step(False)
    d2, l2, _ = step(False)
    s1, ls, rep = step(True)
    print("levels (scattered, nonzero texels):", rep)
    assert rep is not None and rep[0][0] and rep[0][1] > 0 and not rep[-1][0], rep
    for k in d1:
        a, b, c = (x[k].cpu().numpy() for x in (s1, d1, d2))
        if k in ("loss", "render_rgb") or np.array_equal(b.view(np.uint32), c.view(np.uint32)):
            # the forward never sees the GGX backward: bit identity whatever the gather's own runs do
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32), err_msg=k)
        else:
            # the rasterizer's backward sums these with float atomics: two runs of the gather differ themselves, so bit
            # identity cannot be asked of them; the sparse run stays within that run-to-run deviation (same 4x margin)
            noise_k, dev_k = float(np.abs(b - c).max()), float(np.abs(a - b).max())
            print(f"{k}: not reproducible run to run (gather-gather {noise_k:.3e}), sparse-gather {dev_k:.3e}")
            assert dev_k <= 4.0 * noise_k, (k, dev_k, noise_k)
    noise = float(np.abs(l2 - l1).max())
    floor = float(np.spacing(np.float32(np.abs(l1).max())))
    dev = float(np.abs(ls - l1).max())
    print(f"light gradient: peak {np.abs(l1).max():.3e} sparse-gather {dev:.3e} gather-gather {noise:.3e} floor {floor:.3e}")
    assert dev <= 4.0 * max(noise, floor), (dev, noise, floor)
