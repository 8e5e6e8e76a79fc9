"""Times the novel-view evaluator (gi-gs_amd/evaluate.py: render.py's pbr branch plus the per-view PSNR / SSIM) at
BASELINE config C3 size, one view replayed from a hipGraph against the fused launches without a graph and against the
op-by-op formulation.

    python tools/eval_bench.py [--size 800] [--P 300000] [--light 256] [--views 30]

Prints one JSON line: views/s per mode (graphed, fused, unfused) and the metric launches alone (ms per view).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import evaluate  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--light", type=int, default=256)
    ap.add_argument("--views", type=int, default=30)
    args = ap.parse_args()
    dev = "cuda:0"
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    W = H = args.size
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: tt(sc[k]) for k in pipeline.RASTER_KEYS}
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=args.light)
    rng = np.random.default_rng(0)
    gt = tt(rng.uniform(size=(3, H, W)).astype(np.float32))
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.475 * W) ** 2).astype(np.float32)[None])
    views = []
    for i in range(8):
        cam = scenes.orbit_camera(i, 8, W, H, radius=3.5)
        ct = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        views.append((ct, pipeline.view_dirs_for(ct, pipeline.canonical_rays(cam, dev), dev)))
    res = dict(size=args.size, P=args.P, light=args.light, views=args.views)
    for mode in ("graphed", "fused", "unfused"):
        ev = evaluate.NovelViewEvaluator(light, scenes.GI_DEFAULTS, 2, graphs=(mode == "graphed"), fused=(mode != "unfused"))
        for i in range(3):
            ev(*views[i % len(views)][:1], g, views[i % len(views)][1], gt, alpha)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(args.views):
            cam, vd = views[i % len(views)]
            ev(cam, g, vd, gt, alpha)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.views
        res[mode] = dict(ms_per_view=round(ms, 4), views_per_s=round(1000.0 / ms, 1), psnr_avg=ev.results()["psnr_avg"])
        ev.close()
        del ev
    # the metric launches alone (gigs_image_metrics: SSIM + MSE partials and the finish kernel)
    pred = gt.flip(1).contiguous()
    scratch = torch.empty(int(evaluate._lib.gigs_image_metrics_scratch_bytes(3, H, W)), dtype=torch.uint8, device=dev)
    out = torch.empty(7, dtype=torch.float64, device=dev)
    for _ in range(5):
        evaluate.image_metrics(pred, gt, scratch=scratch, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(100):
        evaluate.image_metrics(pred, gt, scratch=scratch, out=out)
    t1.record()
    torch.cuda.synchronize()
    res["metrics_ms"] = round(t0.elapsed_time(t1) / 100, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
