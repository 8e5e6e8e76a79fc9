"""Generates tests/golden/light_f64_bounds.json.

For every level of tests/light_cases.py, every tensor (fwd, fwd_norm, bwd, bwd_norm) and every input: the worst per-texel
error (backward_cases.row_errors) of the fp32 comparator -- the C oracle, oracle/pbr_oracle.cpp orc_specular_cubemap_fwd /
_bwd, whose backward scatters like the reference -- against the windowed float64 reference, over the texels without undecided
pairs, together with the level's populations and its share of texels with undecided pairs.  The same for the diffuse filter
and cubemap_mip.  The HIP kernels are allowed light_cases.BOUND_FACTOR times as much (tests/test_gpu_light_f64.py).  No figure
here comes from the library.  Values are rounded UP to three significant digits.

    python tests/golden/make_light_f64_bounds.py
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


def level_record(orc, lc, name):
    lv = lc.level(orc, name)
    rec = dict(res=lv.res, roughness=lv.rough_arg, cos_cutoff=lv.cc, populations=lc.check_populations(lv, lc.LEVELS[name][2]),
               comparator_worst={}, widened_share={})
    for (tensor, inp), x in lc.inputs(lv).items():
        ref, slack = lc.reference(lv, tensor, x)
        rec["widened_share"][f"{tensor}/{inp}"] = round_up(float((slack > 0).mean()))
        plain, over, _ = lc.judge(lc.comparator(orc, lv, tensor, x), ref, slack, float("inf"))
        rec["comparator_worst"][f"{tensor}/{inp}"] = round_up(plain)
    return rec


def sparse_record(orc, lc, name):
    lv = lc.level(orc, name)
    x = lc.zero_undecided_outputs(lv, lc.sparse_grad(lv))
    ref, slack = lc.reference(lv, "bwd_norm", x)
    plain, _, _ = lc.judge(lc.comparator(orc, lv, "bwd_norm", x), ref, slack, float("inf"))
    return dict(res=lv.res, roughness=lv.rough_arg, cos_cutoff=lv.cc, undecided=int(lv.und.sum()),
                comparator_worst={"bwd_norm/sparse": round_up(plain)})


def small_records(orc, lc):
    import numpy as np
    out = {}
    for res in lc.DIFFUSE_RES:
        tex, f64, g, b64 = lc.diffuse_reference(res)
        out[f"diffuse{res}"] = dict(fwd=round_up(float(lc.row_errors(orc.diffuse_cubemap_fwd(tex).reshape(-1, 3), f64).max())),
                                    bwd=round_up(float(lc.row_errors(orc.diffuse_cubemap_bwd(g).reshape(-1, 3), b64).max())))
    for res in lc.MIP_RES:
        tex, f64, g, b64 = lc.mip_reference(res)
        out[f"mip{res}"] = dict(fwd=round_up(float(lc.row_errors(orc.cubemap_mip_fwd(tex).reshape(-1, 3), f64).max())),
                                bwd=round_up(float(lc.row_errors(orc.cubemap_mip_bwd(g).reshape(-1, 3), b64).max())))
    return out


def generate(orc, verbose=False):
    import light_cases as lc
    doc = dict(rule="bound = factor x the C oracle's worst per-texel row error against float64 on the same input, over the texels "
                    "without undecided pairs (|L.V - cutoff| <= 1e-6); a texel with such pairs is widened by their summed magnitude",
               factor=lc.BOUND_FACTOR, undecided=lc.UNDECIDED, cap_undecided=lc.CAP_UNDECIDED, levels={}, sparse={}, small={})
    for name in lc.LEVELS:
        doc["levels"][name] = level_record(orc, lc, name)
        if verbose:
            print(name, doc["levels"][name], flush=True)
    for name in lc.SPARSE_ONLY:
        doc["sparse"][name] = sparse_record(orc, lc, name)
    doc["small"] = small_records(orc, lc)
    if verbose:
        print(doc["sparse"], doc["small"])
    return doc


def main():
    import light_cases as lc
    from oracle import oracle as orc
    orc.build()
    orc.set_threads(1)
    doc = generate(orc, verbose=True)
    with open(lc.BOUNDS_JSON, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
