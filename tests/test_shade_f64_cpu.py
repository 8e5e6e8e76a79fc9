"""CPU tests (no GPU) of the net the deferred shade's kernels are checked with (tests/shade_cases.py): every case enters its
branches with every decision MIN_MARGIN from its threshold; the two independently written fp32 restatements -- the C oracle's
forward and the float32 evaluation of oracle/torch_pbr_ref.py -- agree with float64 per pixel and per texel within the
recorded figures, no row left out, with float64's tap sets, levels and LUT cells on every pixel; the committed figures are
what the generator produces; and the comparison has teeth: each deliberate error of the backward is at least ten times the
bound the HIP kernel is held to, on the case that owns its branch and on every tensor it changes."""
import os
import sys

import numpy as np
import pytest
import torch

import shade_cases as sc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_shade_f64_bounds as gen  # noqa: E402

ALL = sc.CASES + sc.FORWARD_ONLY_CASES


@pytest.fixture(scope="module")
def fresh(orc):
    """one run of the generator (one thread, as recorded), shared by the tests; the thread count is put back afterwards"""
    orc.set_threads(1)
    doc = gen.generate(orc)
    yield doc
    orc.set_threads(min(8, orc.max_threads()))


@pytest.fixture(scope="module")
def recorded():
    return sc.load_bounds()


@pytest.fixture(scope="module")
def references():
    memo = {}

    def get(name):
        if name not in memo:
            case = sc.build(name)
            memo[name] = (case, sc.reference(case))
        return memo[name]

    return get


def test_case_list_covers_the_argument_matrix():
    """every optional pointer of the two entry points is NULL in one case and given in another"""
    cases = [sc.build(n) for n in sc.CASES]
    for what, pred in (("metallic", lambda c: c.g.get("metallic") is None), ("occlusion", lambda c: c.g.get("occlusion") is None),
                       ("background", lambda c: c.background is None), ("ext", lambda c: c.ext is None),
                       ("planar", lambda c: not c.planar), ("d_metallic", lambda c: "metallic" in c.skip),
                       ("d_diffuse", lambda c: "diffuse" in c.skip), ("d_spec", lambda c: any(s.startswith("spec") for s in c.skip)),
                       ("ext extras", lambda c: not (c.ext and "mul_a" in c.ext)), ("tone", lambda c: not c.tone),
                       ("gamma", lambda c: not c.gamma)):
        hits = [pred(c) for c in cases]
        assert any(hits) and not all(hits), what
    for k in ("g_render", "g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light"):
        hits = [c.grads.get(k) is None for c in cases]
        assert any(hits) and not all(hits), k


@pytest.mark.parametrize("name", ALL)
def test_populations_margins_and_comparators(orc, references, recorded, name):
    """the case's branches are entered at a safe margin; the C oracle's forward and the float32 evaluation's gradients are
    within the recorded figures of float64 on EVERY row, with float64's decisions on every pixel (asserted inside
    comparator_worst), and the recorded figure is not a stale, looser one"""
    case, ref = references(name)
    pop = sc.check_populations(case, ref)
    orc.set_threads(1)
    try:
        worst = sc.comparator_worst(orc, case, ref)
    finally:
        orc.set_threads(min(8, orc.max_threads()))
    rec = recorded["cases"][name]["comparator_worst"]
    assert set(worst) == set(rec) == set(case.forward_names + ([] if case.forward_only else case.gradient_names))
    print(name, f"{case.H} x {case.W}, margin {pop['margin']:.2e}")
    for k, v in worst.items():
        print(f"  {name}.{k}: comparator worst e_i {v:.3e} (recorded {rec[k]:.3e})")
        # within the recorded figure: exactly for the C oracle (one thread, one summation order); the float32 evaluation
        # runs through torch's CPU kernels, whose last digits may differ between vector units
        assert v <= (rec[k] if k in case.forward_names else 1.02 * rec[k]), (name, k, v, rec[k])
        assert v >= 0.5 * rec[k], f"{name}.{k}: recorded {rec[k]:.3e}, measured {v:.3e}: regenerate the bounds"
    if not case.forward_only:  # NaN / inf nowhere, and gradient reaches every tensor the case asks for
        for k, t in sc.gradient_tensors(case, ref).items():
            assert np.isfinite(t).all(), k
            assert np.any(t) or name in ("all_masked", "one_pixel"), k  # (one pixel reaches two levels only)


def test_committed_bounds_are_the_generators(fresh, recorded):
    assert set(fresh["cases"]) == set(recorded["cases"]) == set(ALL)
    for k in ("factor", "min_margin", "metric"):
        assert fresh[k] == recorded[k], k
    for name in ALL:
        f, r = fresh["cases"][name], recorded["cases"][name]
        assert (f["H"], f["W"]) == (r["H"], r["W"]) and set(f["comparator_worst"]) == set(r["comparator_worst"]), name
        assert {k: v for k, v in f["populations"].items() if k != "margin"} == \
            {k: v for k, v in r["populations"].items() if k != "margin"}, name
        for k, v in f["comparator_worst"].items():
            rk = r["comparator_worst"][k]
            if k in sc.FORWARD:  # the C oracle on one thread: the same figure, digit for digit
                assert v == rk, (name, k, v, rk)
            else:  # torch's (gradients) and numpy's (ext outputs) CPU kernels: up to the last digits another vector unit gives
                assert abs(v - rk) <= 0.02 * rk, (name, k, v, rk)
    assert set(fresh["cube_taps"]) == set(recorded["cube_taps"]) == {str(r) for r in sc.SPEC_RES5}
    for res, f in fresh["cube_taps"].items():
        r = recorded["cube_taps"][res]
        assert {k: f[k] for k in ("directions", "wrapped", "dropped")} == {k: r[k] for k in ("directions", "wrapped", "dropped")}
        assert abs(f["weight_worst"] - r["weight_worst"]) <= 0.02 * r["weight_worst"], res


def test_no_bound_is_loose(recorded):
    """bounds of a per-row relative error: none is anywhere near the O(0.1) a wrong branch gives"""
    for name in ALL:
        for k, b in sc.hip_bounds(recorded, name).items():
            assert 0.0 <= b <= 4e-3, (name, k, b)
            assert b == sc.BOUND_FACTOR * recorded["cases"][name]["comparator_worst"][k]  # the plain rule, nothing added


def test_float32_evaluation_follows_its_inputs(references):
    """the restatement runs in the dtype it is given: float32 in, float32 through every lookup and out"""
    case, _ = references("seams")
    t = lambda a: sc.tp.as_dtype(a, torch.float32)  # noqa: E731
    g = sc.tp.restate_inputs(case.g)
    det = {}
    outs = sc.tp.shade(t(g["normals"]), t(g["view_dirs"]), t(g["albedo"]), t(g["roughness"]), torch.from_numpy(g["mask"]),
                       t(g["occlusion"]), t(g["metallic"]), None, t(case.diffuse), [t(s) for s in case.spec], t(sc.lut_np()),
                       gamma=True, details=det)
    assert all(o.dtype == torch.float32 for o in outs)
    assert det["pre_clamp"].dtype == torch.float32 and det["spec"][0]["w"].dtype == torch.float32


# mutation of the float64 backward -> (the case that owns its branch, the tensors it must change)
def _spec(case_res):
    return tuple("spec%d" % r for r in case_res)


TEETH = [
    ("wrapped_taps_0.9", "seams", ("diffuse",) + _spec(sc.SPEC_RES5)),
    ("wrapped_taps_0.9", "seams3", ("diffuse",) + _spec(sc.SPEC_RES3)),
    ("corner_renormalisation_lost", "seams", ("diffuse",) + _spec(sc.SPEC_RES5)),
    ("corner_renormalisation_lost", "seams3", ("diffuse",) + _spec(sc.SPEC_RES3)),
    ("srgb_slope_below_knee_halved", "tck_t0g1", ("albedo", "roughness", "metallic", "diffuse") + _spec(sc.SPEC_RES5)),
    ("srgb_slope_below_knee_halved", "tck_t1g1", ("albedo", "roughness", "metallic", "diffuse") + _spec(sc.SPEC_RES5)),
    ("mip_slope_below_min_kept", "levels", ("roughness",)),
    ("mip_slope_below_min_kept", "levels_ext", ("roughness",)),
    ("mip_slope_high_branch_1.25", "levels", ("roughness",)),
    ("mip_slope_high_branch_1.25", "levels3", ("roughness",)),
    ("clamp_passes_gradient", "tck_t0g0", ("albedo", "roughness", "metallic", "diffuse") + _spec(sc.SPEC_RES5)),
    ("clamp_passes_gradient", "tck_t1g1", ("albedo", "roughness", "metallic", "diffuse") + _spec(sc.SPEC_RES5)),
    ("lut_slope_in_clamped_rows", "levels", ("roughness",)),
    ("lut_slope_in_clamped_rows", "levels_ext", ("roughness",)),
    ("metallic_gradient_full_albedo", "levels", ("metallic",)),
    ("occlusion_missing_in_scatter", "seams", ("diffuse",)),
    ("level_weights_exchanged", "levels", _spec(sc.SPEC_RES5)),
    ("level_weights_exchanged", "levels3", _spec(sc.SPEC_RES3)),
]


@pytest.mark.parametrize("mutation,name,changes", TEETH)
def test_wrong_backward_is_told_apart(references, recorded, mutation, name, changes):
    """The net has teeth: a backward with one deliberate error (values untouched) is, on the case that owns the branch,
    more than ten times the HIP kernel's bound away from float64 on some row of EVERY tensor it changes -- and it changes
    exactly the tensors its branch feeds."""
    case, ref = references(name)
    wrong = sc.reference(case, mut=(mutation,))
    for k in sc.FORWARD:
        np.testing.assert_array_equal(wrong[k], ref[k], err_msg=k)  # a mutation of the gradient only
    bounds = sc.hip_bounds(recorded, name)
    good, bad = sc.gradient_tensors(case, ref), sc.gradient_tensors(case, wrong)
    errs = sc.all_row_errors(bad, good)
    changed = tuple(k for k in good if errs[k].max() > 1e-12)  # beyond float64 rounding of a rearranged expression
    assert set(changed) == set(changes), (mutation, name, changed)
    for k in changed:
        print(f"{mutation} on {name}: {k} worst e_i {errs[k].max():.3e} on {int((errs[k] > bounds[k]).sum())} rows, bound {bounds[k]:.3e}")
        assert errs[k].max() >= 10.0 * bounds[k], (mutation, name, k, errs[k].max(), bounds[k])
