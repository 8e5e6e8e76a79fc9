"""Sparse against dense GGX forward (gigs_specular_cubemap_multi_fwd_sparse against gigs_specular_cubemap_multi_w), one
level per call, ALONE on the device: the 256^2 and the 128^2 level of the 256..16 chain at needed fractions of 1, 5, 10,
25 and 50 % of the level's texels, marked as a filled disc (what a view reads: clustered) and as uniform noise.

    python tools/spec_fwd_sweep.py [--reps 30] > profiles/rNN/spec_fwd_sweep.txt

The sparse figure is the entry point's three launches (list census, listed texels + returning dense workgroups, finish) for
marks written beforehand; the tap census that writes them in a step is a pass over the pixels, timed in the step's trace.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gi-gs_amd")]
import gigs_lib  # noqa: E402
from pbr.renderutils import ops  # noqa: E402

DEV = torch.device("cuda:0")
LEVELS = [(256, 0.08), (128, 0.08 + 0.42 / 3.0)]  # (resolution, roughness) of the two fine levels of the 256..16 chain
FRACTIONS = [0.01, 0.05, 0.10, 0.25, 0.50]


def timed(fn, reps):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = sorted(1e3 * a.elapsed_time(b) for a, b in ev)
    return t[len(t) // 2], t[0], t[-1]


def marks(res, frac, kind, rng):
    total = 6 * res * res
    n = max(1, int(round(frac * total)))
    if kind == "uniform":
        return torch.from_numpy(rng.choice(total, n, replace=False)).to(DEV)
    y, x = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")  # a disc around one direction, nearest texels first
    a, b = 2.0 * (x + 0.5) / res - 1.0, 2.0 * (y + 0.5) / res - 1.0
    one = np.ones_like(a)
    faces = ((one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one))
    dirs = np.stack([np.stack(v, -1) for v in faces], 0)  # [6,res,res,3]
    dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
    axis = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    order = np.argsort(-(dirs.reshape(-1, 3) @ axis), kind="stable")
    return torch.from_numpy(order[:n].copy()).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    lib = gigs_lib.lib()
    rng = np.random.default_rng(28)
    print("GGX forward of one level alone on the device, us: median (min .. max) of %d calls" % args.reps)
    for res, rough in LEVELS:
        total = 6 * res * res
        _, bounds = ops._ndf_bounds(res, rough, 0.99, DEV)
        tables = ops._weight_tables(res, rough, 0.99, DEV)
        src = torch.rand((6, res, res, 3), device=DEV)
        dst, wsum = torch.empty((6, res, res, 3), device=DEV), torch.empty((6, res, res, 1), device=DEV)
        needed = torch.zeros((6, res, res, 3), device=DEV)
        state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=DEV)
        lists = torch.empty(total, dtype=torch.int32, device=DEV)
        arr = (gigs_lib.SpecLevel * 1)(gigs_lib.SpecLevel(res, ops._avg_window(tables, res), src.data_ptr(), bounds.data_ptr(),
                                                          tables.offsets.data_ptr(), tables.fwd.data_ptr(), dst.data_ptr(),
                                                          wsum.data_ptr()))
        need = (C.c_void_p * 1)(needed.data_ptr())
        caps = (C.c_int * 1)(total)
        s = torch.cuda.current_stream().cuda_stream

        def dense():
            gigs_lib.check(lib.gigs_specular_cubemap_multi_w(gigs_lib.ctx_ptr(), 1, C.cast(arr, C.c_void_p), 0, s), "dense")

        def sparse():
            gigs_lib.check(lib.gigs_specular_cubemap_multi_fwd_sparse(gigs_lib.ctx_ptr(), 1, C.cast(arr, C.c_void_p), need, caps,
                                                                      state.data_ptr(), lists.data_ptr(), s), "sparse")

        d_med, d_min, d_max = timed(dense, args.reps)
        print("level %d^2 (%d texels, %.0f candidates per window): dense %.1f (%.1f .. %.1f), spread %.1f"
              % (res, total, tables.fwd.numel() / total, d_med, d_min, d_max, d_max - d_min))
        for kind in ("disc", "uniform"):
            for frac in FRACTIONS:
                idx = marks(res, frac, kind, rng)
                flat = needed.view(-1, 3)

                def once():
                    flat[idx, 0] = 1.0  # the marks, written outside the timed stretch

                # the marks are consumed by every call: write them before each timed call, time the call alone
                ts = []
                for i in range(args.reps + 3):
                    once()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    sparse()
                    b.record()
                    torch.cuda.synchronize()
                    if i >= 3:
                        ts.append(1e3 * a.elapsed_time(b))
                ts.sort()
                listed = int(state.cpu()[16])
                print("  %-7s %4.0f %%: %6d listed, sparse %.1f (%.1f .. %.1f)  %s dense - spread"
                      % (kind, 100 * frac, listed, ts[len(ts) // 2], ts[0], ts[-1],
                         "below" if ts[len(ts) // 2] < d_med - (d_max - d_min) else "ABOVE"))


if __name__ == "__main__":
    main()
