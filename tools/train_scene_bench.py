#!/usr/bin/env python
"""End-to-end trainer throughput ("End-to-end training"): gi-gs_amd/trainer.py on the synthetic dataset of
gi-gs_amd/synthetic_dataset.py (the GPU tests' dataset) at C2-like size (800x800 images, 100 k initial points), with a
compressed schedule that has all three phases -- stage 1 inside the densify window, stage 1 after it, stage 2 -- once
graphed and once with the steppers' eager formulation (the comparison row).  Prints one JSON line: it/s per phase (each
phase timed between device synchronisations at its ends, reports and checkpoints excluded; the loss is read back every 10
iterations as train.py does), graph re-captures, peak memory.

    python tools/train_scene_bench.py [--iterations 1500] [--size 800] [--points 100000]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
importlib.import_module("gi-gs_amd")
import torch  # noqa: E402

import trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=1500)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--points", type=int, default=100_000)
    a = ap.parse_args()
    import synthetic_dataset
    root = tempfile.mkdtemp()
    src = synthetic_dataset.write_synthetic_dataset(os.path.join(root, "scene"), size=a.size, points=60_000)
    rows = []
    # one short run of each formulation first: kernel code objects, tables and allocator pools of the process settle, so
    # neither measured row pays them
    for graphs, n in ((True, 200), (False, 200), (True, a.iterations), (False, a.iterations)):
        pbr = int(n * 0.6)
        out_dir = os.path.join(root, "out_graphs" if graphs else "out_eager")
        args = trainer.parse_args(["-s", src, "-m", out_dir, "--eval", "--indirect", "--metallic",
                                   "--start", "64", "--init_points", str(a.points), "--iterations", str(n),
                                   "--pbr_iteration", str(pbr), "--densify_from_iter", "100", "--densify_until_iter", str(pbr // 2),
                                   "--densification_interval", "100", "--opacity_reset_interval", str(pbr // 4),
                                   "--sh_up_interval", str(max(1, n // 4)), "--test_iterations", str(n),
                                   "--save_iterations", str(n), "--checkpoint_iterations", str(n)])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        r = trainer.train_scene(args, graphs=graphs)
        phases = {k: dict(v, it_per_s=round(v["iterations"] / v["seconds"], 1) if v["seconds"] else None)
                  for k, v in r.timings.items() if isinstance(v, dict)}
        if n != a.iterations:
            continue
        rows.append({"formulation": "graphed (3 hipGraphs per iteration, statistics inside the backward)" if graphs else
                     "eager steppers (GaussianRasterizer op by op, eager statistics / densify / Adam)",
                     "phases": phases, "recaptures": r.recaptures, "total_s": r.timings["total_s"], "P_final": r.points[-1][1],
                     "peak_memory_MiB": torch.cuda.max_memory_allocated() >> 20,
                     "test_psnr": r.final_metrics["test"]["psnr"]})
    print(json.dumps({"size": a.size, "init_points": a.points, "iterations": a.iterations, "rows": rows}))

if __name__ == "__main__":
    main()
