"""GPU tests: the HIP backward (blend_bwd_kernel + preprocess_bwd_kernel, through _RasterizeGaussians) against autograd of
the float64 restatement (oracle/torch_ref.py), per Gaussian row, on the cases of tests/backward_cases.py that enter every
branch of the two kernels on purpose.

Bound: per case and tensor, backward_cases.BOUND_FACTOR x the fp32 CPU oracle's own worst per-row error against float64
(tests/golden/backward_f64_bounds.json) -- both are fp32 evaluations of the same formulae; the kernel differs by the
summation order (64-lane tree + float atomics across quadrants and tiles), FMA contraction and its exp2-based exponential,
a few ulps each, while a wrong or missing branch is O(1) on its rows.  Where the reference is an exact zero (culled rows,
rows only behind terminated pixels, SH rows above the active degree, clamped channels, planes without a gradient) the
result must be one.  The gradients land in a NaN-filled grad_sink holding all twelve names: every element is written."""
import numpy as np
import pytest
import torch

import backward_cases as bc
import gigs_lib
from test_gpu_parity import DEV, _dgr, hip_raw_forward, scratch_views, settings, tt

pytestmark = pytest.mark.gpu

MATERIAL = ("albedo", "roughness", "metallic")


@pytest.fixture(scope="module")
def references(orc):
    """name -> (case, float64 reference, populations): one reference evaluation per case, shared by the switch variants."""
    memo = {}

    def get(name):
        if name not in memo:
            case = bc.build(name)
            r, _, ref = bc.reference(orc, case)
            pop = bc.check_populations(case, ref)
            np.testing.assert_array_equal(ref["n_contrib"].ravel(), r.state("n_contrib"))
            memo[name] = (case, ref, pop)
        return memo[name]

    return get


def hip_backward(case, **ctx_options):
    """-> (gradients by sink name as numpy, n_contrib of the forward, tensors autograd handed back by input name)."""
    dgr = _dgr()
    sc = case.scene
    P, M = sc["means3D"].shape[0], (0 if case.colors_precomp is not None else sc["shs"].shape[1])
    st = settings(dgr, case.cam, sc["sh_degree"], bg=case.bg, scale_modifier=case.scale_modifier)
    e = torch.Tensor([])
    t = {k: tt(sc[k], grad=True) for k in ("means3D", "opacities", "normal", "albedo", "roughness", "metallic")}
    t["shs"] = tt(sc["shs"], grad=True) if case.colors_precomp is None else e
    t["colors"] = e if case.colors_precomp is None else tt(case.colors_precomp, grad=True)
    t["scales"] = tt(sc["scales"], grad=True) if case.cov3D_precomp is None else e
    t["rotations"] = tt(sc["rotations"], grad=True) if case.cov3D_precomp is None else e
    t["cov3D"] = e if case.cov3D_precomp is None else tt(case.cov3D_precomp, grad=True)
    m2d = torch.zeros((P, 3), device=DEV, requires_grad=True)
    shapes = dict(means3D=(P, 3), means2D=(P, 3), opacity=(P, 1), normal=(P, 3), albedo=(P, 3), roughness=(P, 1),
                  metallic=(P, 1), sh=(P, M, 3), scales=(P, 3), rotations=(P, 4), colors=(P, 3), cov3D=(P, 6))
    sink = {k: torch.full(s, float("nan"), device=DEV) for k, s in shapes.items()}
    with gigs_lib.use(gigs_lib.current().derive(**ctx_options)), dgr.grad_sink(sink):
        outs = dgr._RasterizeGaussians.apply(t["means3D"], m2d, t["opacities"], t["normal"], t["albedo"], t["roughness"],
                                             t["metallic"], t["shs"], t["colors"], t["scales"], t["rotations"], t["cov3D"], st)
        # the per-pixel state the backward walks from: the same forward once more through the raw entry point
        raw = hip_raw_forward(dgr, sc, case.cam, bg=case.bg, colors_precomp=case.colors_precomp,
                              cov3D_precomp=case.cov3D_precomp, scale_modifier=case.scale_modifier)
        n_contrib = scratch_views(dgr, raw, P, bc.W, bc.H)["n_contrib"].reshape(bc.H, bc.W).copy()
    color, radii, opacity, depth, normal, albedo, rough, metal, nview, pos = outs
    pg = case.planes
    used = {k: v for k, v in (("color", color), ("opacity", opacity), ("depth", depth), ("normal", normal), ("albedo", albedo),
                              ("roughness", rough), ("metallic", metal)) if np.any(pg[k] != 0)}
    loss = sum((v * tt(pg[k])).sum() for k, v in used.items())  # a plane without a gradient is not part of the loss
    loss.backward()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in sink.items()}
    back = {k: (None if v.grad is None else v.grad.cpu().numpy()) for k, v in t.items() if v.requires_grad}
    back["means2D"] = m2d.grad.cpu().numpy()
    return got, n_contrib, back, radii.cpu().numpy()


def check_against_float64(case, ref, got, n_contrib, radii, bounds, names=tuple(bc.TENSORS), tag=""):
    np.testing.assert_array_equal(radii, ref["radii"])
    np.testing.assert_array_equal(n_contrib, ref["n_contrib"])
    got = {k: got[k] for k in names}
    for k, v in got.items():
        assert not np.isnan(v).any(), f"{tag}{case.name}.{k}: {int(np.isnan(v).sum())} elements were not written"
    errs = bc.all_row_errors(got, ref)
    for k, e in errs.items():
        print(f"{tag}{case.name}.{k}: HIP worst e_i {e.max():.3e}, bound {bounds[k]:.3e}")
    bad_zero = bc.exact_zero_violations(got, ref)
    assert not bad_zero, f"{tag}{case.name}: non-zero where the reference is an exact zero: {bad_zero}"
    assert all(errs[k].max() <= bounds[k] for k in errs), "\n" + bc.report(case, ref, errs, bounds)
    return errs


@pytest.mark.parametrize("name", bc.CASES)
def test_hip_backward_matches_float64_per_gaussian(references, name):
    case, ref, _ = references(name)
    got, n_contrib, back, radii = hip_backward(case)
    check_against_float64(case, ref, got, n_contrib, radii, bc.hip_bounds(bc.load_bounds(), name))
    # what autograd hands back for an input is what the sink received
    pairs = dict(means3D="means3D", opacities="opacity", normal="normal", albedo="albedo", roughness="roughness",
                 metallic="metallic", shs="sh", colors="colors", scales="scales", rotations="rotations", cov3D="cov3D",
                 means2D="means2D")
    for k, v in back.items():
        assert v is not None, k
        np.testing.assert_array_equal(v, got[pairs[k]], err_msg=k)


@pytest.mark.parametrize("option", ["pre_bwd_sh_skip", "blend_cull"])
def test_hip_backward_switch_variants(references, option):
    """The geometry-rich case with the preprocess backward evaluating every visible Gaussian (pre_bwd_sh_skip=0) and with
    the blend's quadrant cull off (blend_cull=0): same reference, same bounds."""
    case, ref, _ = references(bc.GEOMETRY_RICH)
    got, n_contrib, _, radii = hip_backward(case, **{option: 0})
    check_against_float64(case, ref, got, n_contrib, radii, bc.hip_bounds(bc.load_bounds(), case.name), tag=f"{option}=0 ")


def test_hip_backward_declared_materials_only(references):
    """The materials-only case under gigs_ctx_set_materials_only: the three material gradients as the complete backward
    computes them (and as float64 does), nothing else materialised, no violation counted."""
    case, ref, _ = references("matonly")
    bounds = bc.hip_bounds(bc.load_bounds(), case.name)
    full, n_full, _, radii = hip_backward(case)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    got, n_contrib, back, _ = hip_backward(case, materials_only=counter)
    assert int(counter.item()) == 0
    check_against_float64(case, ref, got, n_contrib, radii, bounds, names=MATERIAL, tag="declared ")
    np.testing.assert_array_equal(n_contrib, n_full)
    for k in MATERIAL:
        assert np.abs(ref[bc.TENSORS[k]]).max() > 0
        np.testing.assert_array_equal(back[k], got[k])
        # two runs of the same kernels: the float atomics' order is all that differs
        e = bc.row_errors(got[k], full[k].astype(np.float64))
        assert e.max() <= 1e-5, (k, e.max())
    for k in ("means3D", "opacities", "normal", "shs", "scales", "rotations"):
        assert back[k] is None, k  # not materialised ...
    for k in ("means3D", "opacity", "normal", "sh", "scales", "rotations", "colors", "cov3D"):
        assert np.isnan(got[k]).all(), k  # ... and nothing written for them
        assert not np.any(full[k]), k     # exact zeros in the complete backward
    assert not np.any(got["means2D"])
