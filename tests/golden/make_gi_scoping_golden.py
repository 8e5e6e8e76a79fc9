"""Generates tests/golden/gi_scoping.npz on a GPU, from the build of the commit BEFORE the one whose kernels
tests/test_gpu_gi_scoping.py checks (the recorded arrays are that build's outputs; running this with a later build only
re-records what the test then trivially passes).  Inputs and runners are the test module's; only outputs are stored.

    GIGS_LIB=<libgigs_hip.so built from COMMIT> python tests/golden/make_gi_scoping_golden.py COMMIT [OUT.npz]

The committed file was recorded from the build of 75cb5dc ("GGX pre-filter forward: filter only the texels the step's shade
reads"), the parent of the commit that rebuilt the SSR finish's inputs; COMMIT goes into the file's "provenance" entry, which the
test checks.  Without a march (start >= step) the outputs do not depend on delta: one array per case is stored and both deltas
must give it.

Refuses to write a vacuous fixture: rays must hit in every marched case, certification on and off must agree, the NaN frames
must finish with zero sums and the NaN radiance must show in the outputs of pixels outside its rows.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "gi-gs_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_gi_scoping as T  # noqa: E402


def both_certs(run, what):
    on, off = run(gi_cert=1), run(gi_cert=0)
    for k in on:
        T.same_bits(on[k], off[k], (what, k, "certification on / off"))
    return on


def main(commit, path):
    out = {"provenance": np.array("recorded from the build of commit %s" % commit)}
    for geom in T.GEOMS:
        r = T.Runner(geom)
        band = np.zeros((r.H, r.W), bool)
        if geom != "ragged":
            band[0:8, 0:20] = True
        for m, d, st, sp in T.ssr_settings():
            got = both_certs(lambda **o: r.ssr(m, d, st, sp, **o), (geom, m, d, st))
            for name, a in got.items():
                k = T.key("ssr", geom, m, T.stored_delta(d, st, sp), st, name)
                if k in out:
                    T.same_bits(a, out[k], (k, "both deltas"))
                out[k] = a
            nan = np.isnan(got["abd"]).any(0)
            # a NaN frame takes no hits, and the finish's fmaxf(N.V, 1e-7) drops the NaN normal: zero sums, finite planes
            assert (got["abd"][:, band] == 0).all(), "the zero-normal band must finish with zero sums"
            if geom != "nanrad" or st >= sp:
                assert not nan.any()
            else:
                rows = np.zeros_like(band)
                rows[12:15] = True
                assert nan[~band & ~rows].any(), "no ray outside the rows hits the NaN radiance"
            if st < sp:
                if m == 0:
                    assert (np.nan_to_num(got["abd"], nan=0.0, posinf=1.0) != 0).any(0)[~band].mean() > 0.05, "hardly a ray hits"
                    assert (np.nan_to_num(got["color"], nan=0.0, posinf=1.0) != 0).any(0)[~band].mean() > 0.05
            else:
                assert (got["abd"][:, ~band] == 0).all()
        if geom == "nanrad":
            continue
        for d in T.DELTAS:
            for st, sp in T.MARCHES:
                occ = both_certs(lambda **o: r.ssao(d, st, sp, **o), (geom, d, st))["occlusion"]
                k = T.key("ssao", geom, 0, T.stored_delta(d, st, sp), st, "occlusion")
                if k in out:
                    T.same_bits(occ, out[k], (k, "both deltas"))
                out[k] = occ
                assert (occ[0][band] == 1).all()
                assert ((occ < 1).mean() > 0.05) if st < sp else (occ == 1).all()
    for name, a in both_certs(lambda **o: T.runner("nanrad").ssr_multi(0, 0.125, 8, 16, **o), "multi").items():
        out[T.key("multi", "nanrad", 0, 0.125, 8, name)] = a
    assert not np.array_equal(np.isnan(out[T.key("multi", "nanrad", 0, 0.125, 8, "abd")][0]), np.isnan(out[T.key("multi", "nanrad", 0, 0.125, 8, "abd")][1]))
    for name, a in both_certs(lambda **o: T.runner("ragged").ssr_hits(0, 0.125, 8, 16, **o), "hits").items():
        out[T.key("hits", "ragged", 0, 0.125, 8, name)] = a
    rb = T.runner("band")
    for st, sp in ((8, 16), (5, 12)):
        for name, a in rb.ssr(0, 0.125, st, sp, gi_march="exact").items():
            out[T.key("exact%d" % sp, "band", 0, 0.125, st, name)] = a
        occ = rb.ssao(0.125, st, sp, gi_march="exact")["occlusion"]
        assert (occ < 1).mean() > 0.05
        out[T.key("exact%d" % sp, "band", 0, 0.125, st, "occlusion")] = occ
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes (%d entries in the hit list)" % (
        path, len(out), os.path.getsize(path), len(out[T.key("hits", "ragged", 0, 0.125, 8, "entries")])))


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN)
