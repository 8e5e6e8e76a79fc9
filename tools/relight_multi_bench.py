"""Times relighting one view under K environment maps at BASELINE config C3 size (800x800, 300k Gaussians, 256^2 lights,
whole view replayed from a hipGraph): relight.MultiRelighter (one G-buffer, SSAO and march for all K lights) against K
sequential relight.Relighter calls.  The two are alternated in the same process over several repeated blocks, so drift
affects both alike; per K and mode the median ms per view over the blocks and the spread (min, max) are reported.

    python tools/relight_multi_bench.py [--ks 1,3,5] [--blocks 5] [--views 20] [--size 800] [--P 300000] [--light 256]

Prints one JSON line.
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
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,3,5")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--views", type=int, default=20)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--light", type=int, default=256)
    args = ap.parse_args()
    dev = "cuda:0"
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    W = H = args.size
    ks = [int(k) for k in args.ks.split(",")]
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: tt(sc[k]) for k in pipeline.RASTER_KEYS}
    lights = [relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1 + i)), res=args.light) for i in range(max(ks))]
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.475 * W) ** 2).astype(np.float32)[None])
    views = []
    for i in range(8):
        cam = scenes.orbit_camera(i, 8, W, H, radius=3.5)
        ct = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        views.append((ct, pipeline.view_dirs_for(ct, pipeline.canonical_rays(cam, dev), dev)))
    gi = scenes.GI_DEFAULTS
    singles = [relight.Relighter(l, gi, 2, graphs=True) for l in lights]
    multis = {k: relight.MultiRelighter(lights[:k], gi, 2, graphs=True) for k in ks}

    def run_multi(k, i):
        ct, vd = views[i % len(views)]
        multis[k](ct, g, vd, alpha_mask=alpha)

    def run_seq(k, i):
        ct, vd = views[i % len(views)]
        for r in singles[:k]:
            r(ct, g, vd, alpha_mask=alpha)

    def timed(fn, k):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(args.views):
            fn(k, i)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / args.views

    for k in ks:  # capture and warm every graph
        for i in range(3):
            run_multi(k, i)
            run_seq(k, i)
    samples = {(k, m): [] for k in ks for m in ("multi", "sequential")}
    for b in range(args.blocks):
        for k in ks:
            order = (("multi", run_multi), ("sequential", run_seq))
            for m, fn in (order if b % 2 == 0 else order[::-1]):
                samples[(k, m)].append(timed(fn, k))
    res = dict(size=args.size, P=args.P, light=args.light, views=args.views, blocks=args.blocks, ms_per_view={})
    for k in ks:
        row = {}
        for m in ("multi", "sequential"):
            v = sorted(samples[(k, m)])
            row[m] = dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))
        row["speedup"] = round(row["sequential"]["median"] / row["multi"]["median"], 3)
        res["ms_per_view"][str(k)] = row
    if 1 in ks and len(ks) > 1:
        base = res["ms_per_view"]["1"]["multi"]["median"]
        kmax = max(ks)
        res["multi_ms_per_extra_light"] = round((res["ms_per_view"][str(kmax)]["multi"]["median"] - base) / (kmax - 1), 4)
    for r in [*singles, *multis.values()]:
        r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
