"""CPU tests (no GPU): the oracle's backward against autograd of the float64 restatement (oracle/torch_ref.py), per Gaussian
row and on cases that enter every branch of the backward on purpose (tests/backward_cases.py) -- the clamped projection,
the 0.99 alpha cap, terminated pixels, clamped SH channels, precomputed colours / covariances, culled rows -- and a test
that the comparison has teeth: with one encoded deviation of the reference switched off, the restatement is a WRONG
reference and the oracle must be far from it on the rows of that branch."""
import numpy as np
import pytest

import backward_cases as bc


@pytest.fixture(scope="module")
def evaluated(orc):
    """name -> (case, oracle rasterizer, float64 reference, oracle gradients): computed once per case, on one thread (a fixed
    summation order, as the bounds were recorded); the session's thread count is put back afterwards."""
    orc.set_threads(1)
    memo = {}

    def get(name):
        if name not in memo:
            case = bc.build(name)
            r, _, ref = bc.reference(orc, case)
            memo[name] = (case, r, ref, bc.oracle_backward(r, case))
        return memo[name]

    yield get
    orc.set_threads(min(8, orc.max_threads()))


@pytest.fixture(scope="module")
def recorded():
    return bc.load_bounds()


@pytest.mark.parametrize("name", bc.CASES)
def test_oracle_backward_matches_float64_per_gaussian(evaluated, recorded, name):
    case, r, ref, got = evaluated(name)
    pop = bc.check_populations(case, ref)  # the branches are entered, no decision sits on its threshold
    np.testing.assert_array_equal(ref["n_contrib"].ravel(), r.state("n_contrib"))
    assert not bc.exact_zero_violations(got, ref)
    errs = bc.all_row_errors(got, ref)
    rec = recorded["cases"][name]["oracle_worst"]
    print(name, {k: pop[k] for k in ("R", "longest_list", "margin")}, "reference %.2f s" % ref["seconds"])
    for k, e in errs.items():
        print(f"  {k}: oracle worst e_i {e.max():.3e} (recorded {rec[k]:.3e})")
    for k, e in errs.items():
        # not above the recorded figure, and the recorded figure is not a stale, looser one
        assert e.max() <= rec[k], bc.report(case, ref, errs, rec)
        assert e.max() >= 0.5 * rec[k], f"{name}.{k}: recorded {rec[k]:.3e}, measured {e.max():.3e}: regenerate the bounds"
    assert ref["seconds"] < 5.0


def test_recorded_bounds_are_well_formed(recorded):
    assert set(recorded["cases"]) == set(bc.CASES) and recorded["factor"] == bc.BOUND_FACTOR
    for name in bc.CASES:
        b = bc.hip_bounds(recorded, name)
        assert set(b) == set(bc.TENSORS)
        for k, raised in recorded.get("raised", {}).get(name, {}).items():
            assert raised["factor"] > bc.BOUND_FACTOR and raised["reason"] and raised["observed"] > 0
            assert b[k] <= bc.BOUND_CAP


# deviation switched off -> (case, tensor the branch shows in, mask of the targeted rows, tensors that must stay within
# the bound on every row OUTSIDE the mask; None = every tensor)
def _targets(case, ref):
    bk = ref["book"]
    nonunit = np.abs(np.linalg.norm(case.scene["rotations"].astype(np.float64), axis=1) - 1.0) > 0.05
    material = ("normal", "albedo", "roughness", "metallic")
    return dict(
        sh_clamp=("sh", bk["sh_clamped"].any(axis=1), None),
        fov_clamp=("means3D", bk["fov_clamped_x"] | bk["fov_clamped_y"], None),
        detach_weights=("opacity", bk["contributes"], material),
        depth_surrogate=("means3D", bk["contributes"], material),
        border_normal=("normal", bk["on_border"], None),
        raw_quaternion=("rotations", bk["contributes"] & nonunit, ()),
        alpha_cap=("opacity", bk["capped"] | (case.tags == "undercap"), ()),
        cap_passes_grad=("opacity", bk["capped"], None),
        scale_modifier_grad=("scales", bk["contributes"], tuple(k for k in bc.TENSORS if k != "scales")),
    )


def _subgroups(switch, ref):
    bk = ref["book"]
    if switch == "fov_clamp":
        cx, cy = bk["fov_clamped_x"], bk["fov_clamped_y"]
        return [("x only", cx & ~cy), ("y only", cy & ~cx), ("x and y", cx & cy)]
    if switch == "sh_clamp":
        n = bk["sh_clamped"].sum(axis=1)
        return [(f"{k} channel(s)", n == k) for k in (1, 2, 3)]
    return []


@pytest.mark.parametrize("switch,name", [("sh_clamp", "lists"), ("sh_clamp", "rich"), ("fov_clamp", "rich"),
                                         ("detach_weights", "rich"), ("depth_surrogate", "rich"), ("border_normal", "lists"),
                                         ("border_normal", "quadrants"), ("raw_quaternion", "rich"), ("alpha_cap", "rich"),
                                         ("cap_passes_grad", "rich"), ("scale_modifier_grad", "rich")])
def test_wrong_reference_is_told_apart(orc, evaluated, recorded, switch, name):
    """The net has teeth: against the restatement WITHOUT one of the reference's deviations, the oracle's per-row error
    exceeds ten times the bound the HIP kernel is held to on some row of that branch -- and, where the deviation is local
    to its rows, stays within the bound everywhere else."""
    from oracle import torch_ref
    case, r, ref, got = evaluated(name)
    wrong = torch_ref.render_with_grads(case.scene, case.cam, np.asarray(case.bg), r.state("point_list"), r.state("ranges"),
                                        ref["radii"] > 0, case.planes, scale_modifier=case.scale_modifier,
                                        colors_precomp=case.colors_precomp, cov3D_precomp=case.cov3D_precomp, off=(switch,))
    bounds = bc.hip_bounds(recorded, name)
    errs = bc.all_row_errors(got, wrong)
    tensor, mask, quiet = _targets(case, ref)[switch]
    for label, sub in [("all", mask)] + _subgroups(switch, ref):  # every flavour of the branch on its own, too
        assert sub.sum() > 0, f"{name} has no row in the branch of {switch} ({label})"
        worst = errs[tensor][sub].max()
        print(f"{switch} on {name} ({label}): worst e_i of {tensor} on {int(sub.sum())} targeted rows {worst:.3e}, "
              f"bound {bounds[tensor]:.3e}")
        assert worst >= 10.0 * bounds[tensor], (switch, label, tensor, worst, bounds[tensor])
    for k in (bc.TENSORS if quiet is None else quiet):
        outside = errs[k][~mask] if quiet is None else errs[k]
        if quiet is not None and k == tensor:
            continue
        if outside.size:
            assert outside.max() <= bounds[k], f"{switch} moved {k} outside its branch: {outside.max():.3e} > {bounds[k]:.3e}"
