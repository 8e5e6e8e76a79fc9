"""Writes the "device" section of tests/golden/gi_f64_bounds.json from a run on the GPU: per march case and per (gi_cert,
gi_interleave, gi_zero_rays), over all tile shapes, how many undecided rays the default march decided differently from float64
and the largest margin among them as a share of the rule's (decided rays: none may).  For the record; nothing is bounded by it.

    python tests/golden/record_gi_f64_device.py OUT.json
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gi-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gi_cases as gc  # noqa: E402
import test_gpu_gi_f64 as T  # noqa: E402


def record_device(path):
    """the bounds file with a fresh "device" section: per march case, over all modes, how many undecided rays the default march
    decided differently from float64 and the largest margin among them, as a share of the rule's (decided rays: none may)"""
    import gigs_lib
    lib = gigs_lib.lib()
    doc = gc.load_bounds()
    doc["device"] = {}
    for name in gc.MARCH_CASES:
        case, ref, g, dev = T.get_ref(name)
        if case.gi["step"] - case.gi["start"] > 60:
            continue
        per = {}
        for mode in T.MODES:
            with gigs_lib.options(**mode) as cx:
                _, _, offsets, entries = T.record_hits(lib, cx.ptr, case, g)
            marched = T.marched_rays(case, mode["gi_zero_rays"])
            n_bad, n_und, worst, _ = T.compare_decisions(case, dev, T.decode(case, offsets, entries, marched), marched)
            key = "cert%d_il%d_zero%d" % (mode["gi_cert"], mode["gi_interleave"], mode["gi_zero_rays"])
            cur = per.setdefault(key, dict(decided_differ=0, undecided_differ=0, largest_margin=0.0))
            cur["decided_differ"] = max(cur["decided_differ"], n_bad)
            cur["undecided_differ"] = max(cur["undecided_differ"], n_und)
            cur["largest_margin"] = max(cur["largest_margin"], float("%.3g" % worst))
        doc["device"][name] = per
        print(name, per)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record_device(sys.argv[1])
