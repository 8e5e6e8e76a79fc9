"""Times LPIPS-VGG (lpips.LPIPS on gigs_lpips_vgg) per image pair at 400x400 and 800x800, the same network on
torch.nn.functional.conv2d (MIOpen) with the same weights as a yardstick, and NovelViewEvaluator per view at BASELINE
config C3 size (800x800, 300k Gaussians, 256^2 light, graphed) with and without LPIPS.  Random weights: He-initialised
convolutions, non-negative lin vectors.  Each figure is the median over --blocks timed blocks of --reps calls after a
warm-up, timed with device events; the spread is (min, max) over the blocks.  Effective TF/s uses the VGG16 FLOP count
2 * 305856 * H * W per image, two images per pair.

    python tools/lpips_bench.py [--sizes 400,800] [--blocks 5] [--reps 10] [--no-eval]

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import lpips  # noqa: E402

FLOP_PER_PIXEL = 2 * 305856  # sum over the 13 convs of 9 * Cin * Cout / (4 ** pool level), two FLOP per MAC


def random_state_dict(seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, (co, ci) in zip(lpips.VGG_CONV_INDICES, lpips.VGG_CHANNELS):
        sd[f"features.{idx}.weight"] = torch.randn((co, ci, 3, 3), generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f"features.{idx}.bias"] = torch.randn((co,), generator=g) * 0.05
    for k, c in enumerate(lpips.TAP_CHANNELS):
        sd[f"lin{k}.model.1.weight"] = (torch.rand((c,), generator=g) * 2.0 / c).reshape(1, c, 1, 1)
    return sd


def torch_lpips(ws, bs, lin, shift, scale, a, b, head_dtype=torch.float32):
    """The same network with torch ops (conv2d -> MIOpen), float32: the yardstick.  head_dtype=float64 evaluates the
    heads and the sums in double (the untimed cross-check against gigs_lpips_vgg's double record)."""
    h = (torch.cat([a, b]) - shift) / scale
    n = a.shape[0]
    val, layer = 0, 0
    for t, nl in enumerate((2, 2, 3, 3, 3)):
        if t:
            h = F.max_pool2d(h, 2, 2)
        for _ in range(nl):
            h = F.relu(F.conv2d(h, ws[layer], bs[layer], padding=1))
            layer += 1
        x = h.to(head_dtype)
        f = x / (torch.sqrt((x * x).sum(dim=1, keepdim=True)) + 1e-10)
        val = val + ((f[:n] - f[n:]) ** 2 * lin[t].to(head_dtype)[None, :, None, None]).sum(dim=1).mean(dim=(1, 2))
    return val


def timed(fn, blocks, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return float(np.median(ms)), (float(min(ms)), float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="400,800")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-eval", action="store_true", help="skip the NovelViewEvaluator timing")
    ap.add_argument("--no-torch", action="store_true", help="skip the conv2d yardstick")
    args = ap.parse_args()
    dev = "cuda:0"
    fn = lpips.LPIPS(net="vgg", state_dict=random_state_dict()).to(dev)
    ws, bs, lin = (
        [t.to(dev) for t in x] for x in fn.weights())
    shift = torch.tensor([-0.030, -0.088, -0.188], device=dev)[None, :, None, None]  # outside the timed calls
    scale = torch.tensor([0.458, 0.448, 0.450], device=dev)[None, :, None, None]
    res = {"metric": "lpips_vgg", "blocks": args.blocks, "reps": args.reps}
    g = torch.Generator().manual_seed(1)
    for s in (int(x) for x in args.sizes.split(",")):
        a = torch.rand((1, 3, s, s), generator=g).to(dev)
        b = torch.rand((1, 3, s, s), generator=g).to(dev)
        flop = 2 * FLOP_PER_PIXEL * s * s
        ms, spread = timed(lambda: fn(a, b), args.blocks, args.reps)
        row = {"ms_per_pair": round(ms, 3), "spread_ms": [round(x, 3) for x in spread], "tflops": round(flop / ms / 1e9, 1)}
        if not args.no_torch:
            with torch.no_grad():
                tms, tspread = timed(lambda: torch_lpips(ws, bs, lin, shift, scale, a, b), args.blocks, args.reps)
                ref = float(torch_lpips(ws, bs, lin, shift, scale, a, b, head_dtype=torch.float64)[0])
            got = float(fn.record(a, b)[0, 0])  # the double record, before the float32 rounding of the output
            row.update(conv2d_ms_per_pair=round(tms, 3), conv2d_spread_ms=[round(x, 3) for x in tspread],
                       conv2d_tflops=round(flop / tms / 1e9, 1), speedup_vs_conv2d=round(tms / ms, 2),
                       rel_diff_vs_conv2d=abs(got - ref) / abs(ref))
        res[f"{s}x{s}"] = row
    if not args.no_eval:
        res["novel_view_c3"] = eval_c3(fn, args.blocks)
    print(json.dumps(res))


def eval_c3(fn, blocks, views_per_block=10):
    import evaluate
    import pipeline
    import relight
    import scenes
    dev = "cuda:0"
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    W = H = 800
    sc = scenes.surface_scene(P=300_000, sh_degree=2, seed=0)
    g = {k: tt(sc[k]) for k in pipeline.RASTER_KEYS}
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=256)
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.475 * W) ** 2).astype(np.float32)[None])
    gt = tt(np.random.default_rng(2).uniform(size=(3, H, W)).astype(np.float32))
    views = []
    for i in range(8):
        cam = scenes.orbit_camera(i, 8, W, H, radius=3.5)
        ct = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        views.append((ct, pipeline.view_dirs_for(ct, pipeline.canonical_rays(cam, dev), dev)))
    evs = {"without": evaluate.NovelViewEvaluator(light, scenes.GI_DEFAULTS, 2, graphs=True, capacity=4096),
           "with_lpips": evaluate.NovelViewEvaluator(light, scenes.GI_DEFAULTS, 2, graphs=True, capacity=4096, lpips=fn)}
    ctr = {"i": 0}

    def run(ev):
        ct, vd = views[ctr["i"] % len(views)]
        ctr["i"] += 1
        ev(ct, g, vd, gt, alpha)

    for ev in evs.values():  # capture
        for _ in range(3):
            run(ev)
    torch.cuda.synchronize()
    ms = {m: [] for m in evs}
    for _ in range(blocks):  # alternate the two, so drift affects both alike
        for m, ev in evs.items():
            t, _ = timed(lambda: run(ev), 1, views_per_block, warmup=1)
            ms[m].append(t)
    out = {m: {"ms_per_view": round(float(np.median(v)), 3), "spread_ms": [round(min(v), 3), round(max(v), 3)]}
           for m, v in ms.items()}
    out["lpips_avg"] = evs["with_lpips"].results()["lpips_avg"]
    for ev in evs.values():
        ev.close()
    return out


if __name__ == "__main__":
    main()
