"""Generates tests/golden/backward_f64_bounds.json.

For every case of tests/backward_cases.py: the CPU oracle's backward (one thread: a fixed summation order) against
autograd of the float64 restatement (oracle/torch_ref.py), by the per-row metric of backward_cases.row_errors.  The worst
e_i per tensor is what two fp32 evaluations of the same formulae may differ from float64 by on that case; the HIP kernel is
allowed backward_cases.BOUND_FACTOR times as much (tests/test_gpu_backward_f64.py).  Values are rounded UP to three
significant digits.  The branch populations, the decision margin and the reference's CPU time are stored for the record.
An entry under "raised" (a factor above BOUND_FACTOR for one tensor of one case, with the observed figure and the reason)
is written by hand and survives regeneration.

    python tests/golden/make_backward_f64_bounds.py
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gi-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def round_up(x, digits=3):
    if x == 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(x)) - digits + 1)
    return float(f"{math.ceil(x / q) * q:.{digits - 1}e}")


def main():
    import backward_cases as bc
    from oracle import oracle as orc
    orc.build()
    orc.set_threads(1)
    old = {}
    if os.path.exists(bc.BOUNDS_JSON):
        old = bc.load_bounds()
    doc = dict(metric="e_i = |got_i - ref_i|_inf / (|ref_i|_inf + median_j |ref_j|_inf), worst row per tensor",
               factor=bc.BOUND_FACTOR, cap_for_raised=bc.BOUND_CAP, cases={}, raised=old.get("raised", {}))
    for name in bc.CASES:
        case = bc.build(name)
        r, _, ref = bc.reference(orc, case)
        pop = bc.check_populations(case, ref)
        assert (ref["n_contrib"].ravel() == r.state("n_contrib")).all(), name
        got = bc.oracle_backward(r, case)
        assert not bc.exact_zero_violations(got, ref), name
        errs = bc.all_row_errors(got, ref)
        doc["cases"][name] = dict(oracle_worst={k: round_up(float(e.max())) for k, e in errs.items()}, populations=pop,
                                  P=len(case.tags))
        print(name, "reference %.2f s" % ref["seconds"], doc["cases"][name])
    with open(bc.BOUNDS_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
