"""GPU tests: the deferred shade's kernels (csrc/shade.hip shade_fwd_kernel, shade_bwd_kernel<kTiles>, cube_taps and the
scatter helpers wave_dedup_add / run_add3, through gigs_shade_fwd_ex, gigs_shade_bwd_ex, pbr.pbr_shading and gigs_cube_taps)
against the float64 restatement (oracle/torch_pbr_ref.py), per pixel and per light texel, on the cases of
tests/shade_cases.py that enter every branch on purpose: cube seams and corners at every level in either role of the blend,
both sides of every mip knot, the LUT's clamped rows, the tone / clamp / sRGB-knee combinations per channel, degenerate
geometry, masked, ragged and one-pixel images, and the NULL / given matrix of the optional arguments.

Bound: per case and tensor, shade_cases.BOUND_FACTOR x the worst per-row error of an fp32 CPU evaluation of the same formulae
(tests/golden/shade_f64_bounds.json; the C oracle for the forward, the float32 restatement for the gradients) -- the kernel
differs from those by summation order, FMA contraction and (1 / |c|) * 0.5 against 0.5 / |c|, a few ulps each, while a wrong
or missing branch is O(0.1 - 1) on its rows (tests/test_shade_f64_cpu.py shows that for ten of them).  No row is left out.
Where float64 is an exact zero the result must be one.  Per-pixel outputs start as NaN: every pixel is written.  The
backward runs under three contexts -- the default (32 x 32 tiles, wave deduplication), shade_bwd_rows = 1, and
shade_lds_floats = 0 (every level scattered globally, the coarse ones included) -- against the same reference and bounds,
and its per-pixel outputs are bit-identical across the three."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import shade_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CONTEXTS = (("default", {}), ("rows", dict(shade_bwd_rows=1)), ("no_lds", dict(shade_lds_floats=0)))


@pytest.fixture(scope="module")
def references():
    """name -> (case, float64 reference): one reference evaluation per case, shared by every test and context"""
    memo = {}

    def get(name):
        if name not in memo:
            case = sc.build(name)
            ref = sc.reference(case)
            sc.check_populations(case, ref)
            memo[name] = (case, ref)
        return memo[name]

    return get


@pytest.fixture(scope="module")
def recorded():
    return sc.load_bounds()


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


def _rgb(a, planar):
    """a [H,W,3] numpy plane on the device in the case's layout"""
    return None if a is None else tt(a.transpose(2, 0, 1) if planar else a)


def _hwc(t, planar):
    a = t.cpu().numpy()
    return np.ascontiguousarray(a.transpose(1, 2, 0)) if planar else a


def _inputs(case):
    g = case.g
    x = dict(normals=_rgb(g["normals"], case.planar), view_dirs=tt(g["view_dirs"]), albedo=_rgb(g["albedo"], case.planar),
             roughness=tt(g["roughness"]), mask=tt(g["mask"].astype(np.uint8)),
             occlusion=None if g.get("occlusion") is None else tt(g["occlusion"]),
             metallic=None if g.get("metallic") is None else tt(g["metallic"]),
             diffuse=tt(case.diffuse), spec=[tt(s) for s in case.spec], lut=tt(sc.lut_np()))
    x["spec_res"] = (C.c_int * len(case.spec))(*[int(s.shape[1]) for s in case.spec])
    return x


def hip_forward(case):
    import gigs_lib
    from pbr.shade import _ptr_array
    H, W, pl = case.H, case.W, case.planar
    x = _inputs(case)
    shape = (3, H, W) if pl else (H, W, 3)
    nan = lambda s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out = {k: nan(shape) for k in sc.FORWARD}
    bg = _rgb(case.background, pl)
    ext, keep = None, None
    if case.ext:
        out.update(F0=nan(shape), linear=nan(shape), roughness_out=nan((H, W)))
        keep = gigs_lib.ShadeExt(planar=int(pl), rough_scale=case.ext["rough_scale"], rough_bias=case.ext["rough_bias"],
                                 out_F0=_p(out["F0"]), out_linear=_p(out["linear"]), out_roughness=_p(out["roughness_out"]))
        ext = C.addressof(keep)
    else:
        assert not pl
    gigs_lib.check(gigs_lib.lib().gigs_shade_fwd_ex(
        gigs_lib.current().ptr, H, W, _p(x["normals"]), _p(x["view_dirs"]), _p(x["albedo"]), _p(x["roughness"]), _p(x["mask"]),
        _p(x["occlusion"]), _p(x["metallic"]), _p(bg), _p(x["diffuse"]), int(x["diffuse"].shape[1]), len(x["spec"]),
        _ptr_array(x["spec"]), x["spec_res"], _p(x["lut"]), 256, 256, int(case.tone), int(case.gamma), _p(out["render_rgb"]),
        _p(out["diffuse_rgb"]), _p(out["specular_rgb"]), _p(out["diffuse_light"]), ext, torch.cuda.current_stream().cuda_stream),
        "shade_fwd_ex")
    torch.cuda.synchronize()
    res = {k: (_hwc(v, pl) if v.dim() == 3 else v.cpu().numpy().reshape(H, W, 1)) for k, v in out.items()}
    return res


def hip_backward(case, **ctx_options):
    """one gigs_shade_bwd_ex call -> the gradient tensors by shade_cases' names (HWC), numpy"""
    import gigs_lib
    from pbr.shade import _ptr_array
    H, W, pl = case.H, case.W, case.planar
    x = _inputs(case)
    shape = (3, H, W) if pl else (H, W, 3)
    gr = {k: _rgb(v, pl) for k, v in case.grads.items()}
    names = case.gradient_names
    d_alb = torch.full(shape, float("nan"), device=DEV)
    d_rgh = torch.full((H, W, 1), float("nan"), device=DEV)
    d_met = torch.full((H, W, 1), float("nan"), device=DEV) if "metallic" in names else None
    d_dif = torch.zeros_like(x["diffuse"]) if "diffuse" in names else None
    d_sp = [torch.zeros_like(s) if "spec%d" % r in names else None for s, r in zip(x["spec"], case.spec_res)]
    ext, keep, held = None, None, []
    if case.ext:
        e = case.ext
        dev = lambda a, rgb=False: None if a is None else (_rgb(a, pl) if rgb else tt(a))  # noqa: E731
        held = [dev(e.get("mul_a"), True), dev(e.get("mul_b"), True), dev(e.get("add_r")), dev(e.get("add_m")),
                None if "g_scale" not in e else tt(np.array([e["g_scale"]], np.float32)), dev(e.get("lamb_mask")),
                None if "lamb_cnt" not in e else tt(np.array([0, 0, 0, e["lamb_cnt"]], np.float32))]
        keep = gigs_lib.ShadeExt(planar=int(pl), rough_scale=e["rough_scale"], rough_bias=e["rough_bias"],
                                 g_albedo_mul_a=_p(held[0]), g_albedo_mul_b=_p(held[1]), g_roughness_add=_p(held[2]),
                                 g_metallic_add=_p(held[3]), g_scale=_p(held[4]), lamb_mask=_p(held[5]), lamb_acc4=_p(held[6]))
        ext = C.addressof(keep)
    else:
        assert not pl
    ctx = gigs_lib.current().derive(**ctx_options)
    gigs_lib.check(gigs_lib.lib().gigs_shade_bwd_ex(
        ctx.ptr, H, W, _p(x["normals"]), _p(x["view_dirs"]), _p(x["albedo"]), _p(x["roughness"]), _p(x["mask"]),
        _p(x["occlusion"]), _p(x["metallic"]), _p(x["diffuse"]), int(x["diffuse"].shape[1]), len(x["spec"]),
        _ptr_array(x["spec"]), x["spec_res"], _p(x["lut"]), 256, 256, int(case.tone), int(case.gamma), _p(gr.get("g_render")),
        _p(gr.get("g_diffuse_rgb")), _p(gr.get("g_specular_rgb")), _p(gr.get("g_diffuse_light")), _p(d_alb), _p(d_rgh),
        _p(d_met), _p(d_dif), _ptr_array(d_sp), ext, torch.cuda.current_stream().cuda_stream), "shade_bwd_ex")
    torch.cuda.synchronize()
    del held
    got = dict(albedo=_hwc(d_alb, pl), roughness=d_rgh.cpu().numpy())
    if d_met is not None:
        got["metallic"] = d_met.cpu().numpy()
    if d_dif is not None:
        got["diffuse"] = d_dif.cpu().numpy()
    got.update({"spec%d" % r: d.cpu().numpy() for r, d in zip(case.spec_res, d_sp) if d is not None})
    return got


def check(case, got, ref_tensors, recorded, tag):
    """every tensor written everywhere, exact zeros kept, worst row within the bound; prints the figures"""
    bounds = sc.hip_bounds(recorded, case.name)
    rec = recorded["cases"][case.name]["comparator_worst"]
    assert set(got) == set(ref_tensors), (set(got), set(ref_tensors))
    for k, v in got.items():
        assert np.isfinite(v).all(), f"{tag} {case.name}.{k}: {int((~np.isfinite(v)).sum())} elements not written or not finite"
    errs = sc.all_row_errors(got, ref_tensors)
    for k, e in errs.items():
        print(f"{tag} {case.name}.{k}: HIP worst e_i {e.max():.3e}, bound {bounds[k]:.3e} (comparator {rec[k]:.3e})")
    bad_zero = sc.exact_zero_violations(got, ref_tensors)
    assert not bad_zero, f"{tag} {case.name}: non-zero where float64 is an exact zero: {bad_zero}"
    worst = {k: (float(e.max()), int(np.argmax(e)), bounds[k]) for k, e in errs.items() if e.max() > bounds[k]}
    assert not worst, f"{tag} {case.name}: (worst e_i, its row, bound) {worst}"
    return errs


@pytest.mark.parametrize("name", sc.CASES + sc.FORWARD_ONLY_CASES)
def test_forward_matches_float64_per_pixel(references, recorded, name):
    case, ref = references(name)
    check(case, hip_forward(case), sc.forward_reference(case, ref), recorded, "forward")


@pytest.mark.parametrize("name", sc.CASES)
def test_backward_matches_float64_per_pixel_and_texel(references, recorded, name):
    case, ref = references(name)
    want = sc.gradient_tensors(case, ref)
    first = None
    for tag, options in CONTEXTS:
        got = hip_backward(case, **options)
        check(case, got, want, recorded, tag)
        if first is None:
            first = got
        for k in sc.PIXEL_GRADS:  # the pixel mapping and the scatter's formulation change no per-pixel bit
            if k in got:
                np.testing.assert_array_equal(got[k].view(np.uint32), first[k].view(np.uint32), err_msg=f"{tag} {k}")


@pytest.mark.parametrize("name", ["seams", "opt_no_metallic"])
def test_python_binding_hands_back_what_the_entry_wrote(references, recorded, name):
    """pbr.pbr_shading with autograd: the four planes and the gradients of albedo, roughness, metallic and the light are
    the C entry's -- per-pixel tensors bit for bit, the light gradients (float atomics: the order of two runs differs)
    within the bounds of float64."""
    from pbr.shade import pbr_shading
    case, ref = references(name)
    assert case.ext is None and not case.planar and not case.skip
    g = case.g
    leaf = lambda a: None if a is None else tt(a).requires_grad_(True)  # noqa: E731
    albedo, rough, metal = leaf(g["albedo"]), leaf(g["roughness"]), leaf(g.get("metallic"))
    light = types.SimpleNamespace(diffuse=leaf(case.diffuse), specular=[leaf(s) for s in case.spec])
    out = pbr_shading(light, tt(g["normals"]), tt(g["view_dirs"]), albedo, rough, tt(g["mask"]), tone=case.tone, gamma=case.gamma,
                      occlusion=None if g.get("occlusion") is None else tt(g["occlusion"]), metallic=metal,
                      brdf_lut=tt(sc.lut_np()[None]), background=None if case.background is None else tt(case.background))
    fwd = hip_forward(case)
    for k in sc.FORWARD:
        np.testing.assert_array_equal(out[k].detach().cpu().numpy(), fwd[k], err_msg=k)
    keys = dict(g_render="render_rgb", g_diffuse_rgb="diffuse_rgb", g_specular_rgb="specular_rgb", g_diffuse_light="diffuse_light")
    sum((out[keys[k]] * tt(v)).sum() for k, v in case.grads.items() if v is not None).backward()
    torch.cuda.synchronize()
    got = dict(albedo=albedo.grad, roughness=rough.grad, diffuse=light.diffuse.grad)
    if metal is not None:
        got["metallic"] = metal.grad
    got.update({"spec%d" % r: s.grad for r, s in zip(case.spec_res, light.specular)})
    got = {k: v.cpu().numpy() for k, v in got.items()}
    check(case, got, sc.gradient_tensors(case, ref), recorded, "autograd")
    entry = hip_backward(case)
    for k in sc.PIXEL_GRADS:
        if k in got:
            np.testing.assert_array_equal(got[k].view(np.uint32), entry[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("res", sc.SPEC_RES5)
def test_cube_taps_on_the_seam_directions(recorded, res):
    """gigs_cube_taps: float64's index set per direction (-1 exactly where float64 drops the corner tap), weights within
    the recorded bound, and the weights of a direction -- dropped corners included -- sum to 1 within 4 ulp."""
    import gigs_lib
    dirs, want = sc.seam_taps()[res]
    rec = recorded["cube_taps"][str(res)]
    n = dirs.shape[0]
    assert n == rec["directions"] and want["wrapped"] >= 24 and want["dropped"] >= 24
    d = tt(dirs)
    idx = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    w = torch.full((n, 4), float("nan"), device=DEV)
    gigs_lib.check(gigs_lib.lib().gigs_cube_taps(res, n, d.data_ptr(), idx.data_ptr(), w.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "cube_taps")
    torch.cuda.synchronize()
    idx, w = idx.cpu().numpy(), w.cpu().numpy()
    np.testing.assert_array_equal(idx, want["idx"])
    assert np.array_equal(idx < 0, want["idx"] < 0) and int((idx < 0).any(-1).sum()) == want["dropped"]
    assert not np.any(w[idx < 0])
    worst = np.abs(w.astype(np.float64) - want["w"]).max()
    bound = sc.BOUND_FACTOR * rec["weight_worst"]
    off_one = np.abs(w.astype(np.float64).sum(-1) - 1.0).max()
    print(f"cube_taps {res}: HIP worst weight difference {worst:.3e}, bound {bound:.3e} (comparator {rec['weight_worst']:.3e}); "
          f"worst |sum - 1| {off_one:.3e}")
    assert worst <= bound
    assert off_one <= 4 * 2.0 ** -23
