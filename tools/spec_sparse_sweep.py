"""Sparse path against gather in the sparse GGX backward (gigs_specular_cubemap_multi_bwd_sparse), one level per call.

    python tools/spec_sparse_sweep.py [--reps 20]

Per level (256^2 at roughness 0.08, 128^2 at 0.22: the two fine levels of the 256..16 chain), per pattern and per density
of nonzero gradient texels it times three forms with events, median of --reps calls after 3 warm-up calls:
  gather   gigs_options.spec_sparse = 0: the one launch of gigs_specular_cubemap_multi_w
  dense    spec_sparse = 1 with capacity 0: census + gather -- what a level over its capacity costs
  sparse   spec_sparse = 1 with the capacity at the swept density (the sparse path's grid is sized by the capacity):
           census + the level's tile workgroups, its gather workgroups returning at entry
Patterns: `disc`, a filled disc around a face centre holding the swept share of the level's texels (past a sixth it fills
whole faces and continues on the next) -- what a training step produces, highlights cluster; and `uniform`, texels drawn
without replacement -- the worst case for the number of tiles a listed texel's neighbours touch.
The break-even density is where `sparse` crosses `dense` (linear interpolation between the swept points).  One capacity
serves every level, so gigs_options.spec_sparse_permille follows the smallest break-even over levels and patterns: the
tool prints it and half of it (the margin the default kept while one kernel served both levels; DESIGN section 5 has the
reasoning for the shipped value).
A last block times the whole chain with an all-nonzero gradient, gather against dense: the cost of the census.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gi-gs_amd"))
import gigs_lib  # noqa: E402
from pbr.renderutils import ops  # noqa: E402

DEV = torch.device("cuda:0")
CHAIN = [(256, 0.08), (128, 0.22), (64, 0.36), (32, 0.5), (16, 1.0)]


def call(levels, grads, reps, **opts):
    lib = gigs_lib.lib()
    n = len(levels)
    arr = (gigs_lib.SpecLevel * n)()
    wf, ws = (C.c_void_p * n)(), (C.c_void_p * n)()
    keep = []
    for i, ((res, rough), g) in enumerate(zip(levels, grads)):
        _, bounds = ops._ndf_bounds(res, rough, 0.99, DEV)
        t = ops._weight_tables(res, rough, 0.99, DEV)
        dst = torch.empty_like(g)
        keep += [dst]
        arr[i] = gigs_lib.SpecLevel(res, ops._avg_window(t, res), g.data_ptr(), bounds.data_ptr(), t[0].data_ptr(),
                                    t[3].data_ptr(), dst.data_ptr(), None)
        wf[i], ws[i] = t[1].data_ptr(), t[4].data_ptr()
    with gigs_lib.options(**opts):
        caps = sum(lib.gigs_spec_sparse_capacity(gigs_lib.ctx_ptr(), r) for r, _ in levels)
        state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=DEV)
        lists = torch.empty(max(1, caps), dtype=torch.int32, device=DEV)
        times = []
        for rep in range(reps + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            gigs_lib.check(lib.gigs_specular_cubemap_multi_bwd_sparse(
                gigs_lib.ctx_ptr(), n, C.cast(arr, C.c_void_p), wf, ws, state.data_ptr(), lists.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "specular_cubemap_multi_bwd_sparse")
            b.record()
            torch.cuda.synchronize()
            if rep >= 3:
                times.append(a.elapsed_time(b) * 1e3)
    return float(np.median(times)), state.cpu().tolist()


def pick(res, n, pattern, rng):
    """Indices of n nonzero texels of a res^2 level."""
    total = 6 * res * res
    if pattern == "uniform":
        return rng.choice(total, size=n, replace=False)
    yy, xx = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    d2 = ((yy - res / 2 + 0.5) ** 2 + (xx - res / 2 + 0.5) ** 2).reshape(-1)
    order = np.argsort(d2, kind="stable")  # a face's texels, nearest to its centre first
    return np.concatenate([f * res * res + order for f in range(6)])[:n]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    reps = ap.parse_args().reps
    rng = np.random.default_rng(0)
    print(f"median of {reps} calls, us (events around the call: launch gaps of the three kernels included)")
    evens = []
    for res, rough in CHAIN[:2]:
        total = 6 * res * res
        for pattern in ("disc", "uniform"):
            rows = []
            for pct in (0, 1, 2, 5, 10, 20, 40):
                g = np.zeros((total, 3), np.float32)
                idx = pick(res, total * pct // 100, pattern, rng)
                g[idx] = rng.normal(size=(len(idx), 3)).astype(np.float32) + 3.0
                gt = torch.from_numpy(g).to(DEV)
                t_g, _ = call([(res, rough)], [gt], reps, spec_sparse=0)
                t_d, st = call([(res, rough)], [gt], reps, spec_sparse=1, spec_sparse_permille=0)
                assert st[8] == (1 if pct == 0 else 0) and st[16] == len(idx)
                t_s, st = call([(res, rough)], [gt], reps, spec_sparse=1, spec_sparse_permille=max(1, 10 * pct))
                assert st[8] == 1 and st[16] == len(idx)
                rows.append((pct, t_g, t_d, t_s))
                print(f"{res}^2 roughness {rough} {pattern:7s}: {pct:3d} % nonzero ({len(idx):6d} texels)  gather {t_g:7.1f}  "
                      f"dense {t_d:7.1f}  sparse {t_s:7.1f}", flush=True)
            even = None
            for (p0, _, d0, s0), (p1, _, d1, s1) in zip(rows, rows[1:]):
                if s0 <= d0 and s1 > d1:
                    f = (d0 - s0) / ((d0 - s0) + (s1 - d1))
                    even = p0 + f * (p1 - p0)
            if even is not None:
                evens.append(even)
            print(f"{res}^2 {pattern}: sparse = dense at " + (f"{even:.1f} %" if even is not None else "no swept density"))
    if evens:
        print(f"smallest break-even {min(evens):.1f} % = {int(10 * min(evens))} permille; half of it {int(round(5 * min(evens)))} permille")
    grads = [torch.from_numpy(rng.normal(size=(6 * r * r, 3)).astype(np.float32) + 3.0).to(DEV) for r, _ in CHAIN]
    t_g, _ = call(CHAIN, grads, reps, spec_sparse=0)
    t_d, st = call(CHAIN, grads, reps, spec_sparse=1)
    assert st[8:13] == [0] * 5
    print(f"whole chain, all-nonzero gradient: gather {t_g:.1f}  census + gather {t_d:.1f}  (+{t_d - t_g:.1f})")
    zeros = [torch.zeros_like(g) for g in grads]
    t_z, st = call(CHAIN, zeros, reps, spec_sparse=1)
    assert st[8:13] == [1] * 5
    print(f"whole chain, all-zero gradient: {t_z:.1f}")


if __name__ == "__main__":
    main()
