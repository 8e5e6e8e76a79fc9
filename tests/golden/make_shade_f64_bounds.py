"""Generates tests/golden/shade_f64_bounds.json.

For every case of tests/shade_cases.py: the fp32 CPU comparators against the float64 restatement of the deferred shade
(oracle/torch_pbr_ref.py), by the per-row metric of backward_cases.row_errors -- the C oracle (oracle/pbr_oracle.cpp, one
thread) for the forward planes, the float32 evaluation of the restatement itself for the gradients.  The worst e_i per
tensor is what an fp32 evaluation of these formulae may differ from float64 by on that case; the HIP kernels are allowed
shade_cases.BOUND_FACTOR times as much (tests/test_gpu_shade_f64.py).  "cube_taps" holds, per resolution, the worst
absolute difference of a bilinear weight between the float32 and the float64 evaluation on the seam directions.  Values are
rounded UP to three significant digits.  The branch populations and the decision margin are stored for the record.

    python tests/golden/make_shade_f64_bounds.py
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


def generate(orc, verbose=False):
    import shade_cases as sc
    doc = dict(metric="e_i = |got_i - ref_i|_inf / (|ref_i|_inf + median_j |ref_j|_inf), worst row per tensor; rows are "
                      "pixels, or texels for the light gradients",
               factor=sc.BOUND_FACTOR, min_margin=sc.MIN_MARGIN, cases={}, cube_taps={})
    for name in sc.CASES + sc.FORWARD_ONLY_CASES:
        case = sc.build(name)
        ref = sc.reference(case)
        pop = sc.check_populations(case, ref)
        worst = sc.comparator_worst(orc, case, ref)
        doc["cases"][name] = dict(comparator_worst={k: round_up(v) for k, v in worst.items()}, H=case.H, W=case.W,
                                  populations={k: (pop[k] if k != "margin" else round_up(pop[k])) for k in sorted(set(case.needs) | {"margin"})})
        if verbose:
            print(name, doc["cases"][name])
    for res, (_, tap) in sc.seam_taps().items():
        doc["cube_taps"][str(res)] = dict(weight_worst=round_up(tap["weight_worst"]), directions=tap["directions"],
                                          wrapped=tap["wrapped"], dropped=tap["dropped"])
    return doc


def main():
    import shade_cases as sc
    from oracle import oracle as orc
    orc.build()
    orc.set_threads(1)
    doc = generate(orc, verbose=True)
    with open(sc.BOUNDS_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
