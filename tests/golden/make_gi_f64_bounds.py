"""Generates tests/golden/gi_f64_bounds.json.

For every march case of tests/gi_cases.py: the C oracle (oracle/gigs_oracle.cpp orc_ssao / orc_ssr, one thread) against the
float64 restatement oracle/gi_ref.py -- its worst per-pixel error per plane, absolute and as a share of the pixel's a-priori
summation bound (which is derived, not recorded: gi_cases.bounds) -- with the branch populations and the share of undecided
rays, for the record.  For the A6 / median / bilateral cases: the C oracle's worst per-pixel error against float64 per tensor;
the HIP kernels are allowed gi_cases.BOUND_FACTOR times as much (tests/test_gpu_gi_f64.py).  Values are rounded UP to three
significant digits.

The section "device" is a record of a run on the GPU (tests/golden/record_gi_f64_device.py, per case and mode: how many
undecided rays the kernel decided differently from float64 and the largest margin among them); this script carries it over
unchanged.

    python tests/golden/make_gi_f64_bounds.py
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

POP_KEYS = ("hit", "miss", "hit_first", "hit_last", "left_first", "front_then_hit", "passed_behind", "den_nonpos", "hit_hole",
            "hole_missed", "self_hit_all", "all_missing", "dead_hits_nonfinite", "dead_only_nan", "nan_normal", "degenerate_frame", "hole_pixels",
            "ndv_clamped", "arg_clamped", "metallic_0", "metallic_1", "metallic_mid", "grazing_pixels", "left_x_low",
            "left_x_high", "left_y_low", "left_y_high", "pairs", "undecided")


def round_up(x, digits=3):
    if x == 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(x)) - digits + 1)
    return float(f"{math.ceil(x / q) * q:.{digits - 1}e}")


def march_record(orc, gc, name):
    case, m = gc.build(name)
    ref = gc.reference(case, m)
    pop = gc.check_populations(case, ref)
    occ, col, abd = gc.oracle_march(orc, case)
    rec = dict(W=case.W, H=case.H, rays=gc.gr.ray_table(case.gi["delta"])["n"], gi=case.gi,
               populations={k: pop[k] for k in POP_KEYS}, undecided_share=round_up(pop["undecided_share"]),
               undecided_weight_worst=round_up(pop["undecided_weight_worst"]), hit_share=round_up(pop["hit_share"]),
               oracle_worst_abs={}, oracle_worst_over_bound={})
    for k, got, b in (("occlusion", occ, "occ"), ("color", col, "color"), ("abd", abd, "abd")):
        e = gc.plane_errors(got, ref[b], ref[b + "_bound"])
        rec["oracle_worst_abs"][k] = round_up(e["worst_abs"])
        rec["oracle_worst_over_bound"][k] = round_up(e["worst_ratio"])
    return rec


def normal_record(orc, gc, c):
    import numpy as np
    n64, p64, early, _ = gc.gr.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], c["depth"])
    n32, p32 = orc.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], c["depth"])
    zero = np.zeros_like(n64)
    worst = dict(normal=round_up(gc.plane_errors(n32, n64, zero)["worst_abs"]),
                 depth_pos=round_up(gc.plane_errors(p32, p64, zero)["worst_abs"]))
    if min(c["W"], c["H"]) >= 2:  # the chain of the rasterizer's forward: median -> A6 -> bilateral, median of the positions
        cn64, cp64 = gc.normal_chain(gc.gr, c, np.float64)
        cn32, cp32 = gc.normal_chain(orc, c, np.float32)
        worst["chain_normal"] = round_up(gc.plane_errors(cn32, cn64, zero)["worst_abs"])
        worst["chain_pos"] = round_up(gc.plane_errors(cp32, cp64, zero)["worst_abs"])
    return dict(W=c["W"], H=c["H"], early={k: int((early == i).sum()) for i, k in enumerate(gc.gr.EARLY)}, comparator_worst=worst)


def filter_record(orc, gc, x):
    import numpy as np
    med, _, _ = gc.gr.median3x3(x)
    rec = dict(shape=list(x.shape), comparator_worst=dict(median=round_up(gc.plane_errors(orc.median3x3(x), med, np.zeros_like(med))["worst_abs"])))
    if min(x.shape[1:]) >= 2 and not np.isnan(x).any():
        b64 = gc.gr.bilateral3x3(x)
        rec["comparator_worst"]["bilateral"] = round_up(gc.plane_errors(orc.bilateral3x3(x), b64, np.zeros_like(b64))["worst_abs"])
    return rec


def generate(orc, verbose=False, device=None):
    import gi_cases as gc
    doc = dict(rule="decided: pixel margin > 2^-19 max(W, H), depth and denominator margins > 2^-19 max|z| (derived, not measured "
                    "on a device); summation bound (n + 8) 2^-24 sum|t_i| per pixel and plane (+ the tails' roundings, "
                    "gi_cases.bounds); A6 / median / bilateral: factor x the C oracle's worst per-pixel error",
               factor=gc.BOUND_FACTOR, cap_rays=gc.CAP_RAYS, cap_weight=gc.CAP_WEIGHT, march={}, normal={}, filters={},
               device=device if device is not None else {})
    for name in gc.MARCH_CASES:
        doc["march"][name] = march_record(orc, gc, name)
        if verbose:
            print(name, doc["march"][name])
    for name, c in gc.normal_cases().items():
        doc["normal"][name] = normal_record(orc, gc, c)
        if verbose:
            print(name, doc["normal"][name])
    for name, x in gc.filter_cases().items():
        doc["filters"][name] = filter_record(orc, gc, x)
        if verbose:
            print(name, doc["filters"][name])
    return doc


def main():
    import gi_cases as gc
    from oracle import oracle as orc
    orc.build()
    orc.set_threads(1)
    device = None
    if os.path.exists(gc.BOUNDS_JSON):
        with open(gc.BOUNDS_JSON) as f:
            device = json.load(f).get("device")
    doc = generate(orc, verbose=True, device=device)
    with open(gc.BOUNDS_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
