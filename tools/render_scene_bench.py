"""Times render_scene's per-view loop (evaluator + image_writer.ImageWriter) against writing the same images the way the
package allowed before the writer existed, at BASELINE config C3 size: 800 x 800, 300k Gaussians, 13 PNGs per view.

    python tools/render_scene_bench.py [--size 800] [--P 300000] [--views 64] [--blocks 3] [--workers 12] [--out DIR]
    python tools/render_scene_bench.py --kernels [--repeats 20]      (the two device launches alone, for a kernel trace)

Rows (views/s, wall clock from the first view to the last file on disk; median [min, max] over the blocks, the two
writers alternating block by block after one short warm-up block each):
    writer     the evaluator's planes -> ImageWriter.submit (gigs_pack_images + gigs_png_filter, threads deflate and write)
    pil        the comparison row: the same planes, per image x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) (depth
               normalised, brdf concatenated with torch) -> .cpu() -> PIL.Image.save(path) in the calling thread
    evaluator  the planes discarded: the ceiling
`submit_blocked_s` is the time the main thread waited for a free staging slot: when it is most of a block, the host
stage bounds the writer row, otherwise the GPU (or the main thread's own launch work) does.  File sizes are the sums over
one block's PNGs.  --kernels prints the algorithmic bytes of the two launches for one view's 13 images, computed from the
shapes (pack: 4 C read + 3 written per pixel and plane; filter: 3 read + 3 + 1/W written per pixel), and their time
by device events; run it under `rocprofv3 --kernel-trace --stats` for the per-kernel figures.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import evaluate  # noqa: E402
import image_writer  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import render_scene  # noqa: E402
import scenes  # noqa: E402


def algorithmic_bytes(images):
    """(pack bytes, filter bytes) of one batch of image_writer.Image objects."""
    pack = sum((4 * int(t.shape[0]) + 3) * int(t.shape[1]) * int(t.shape[2]) for im in images for t in im.planes)
    filt = sum(im.H * (3 * im.W + 3 * im.W + 1) for im in images)
    return pack, filt


def pil_write(paths, planes):
    """What a caller of the package wrote before image_writer: torch quantisation, a copy per image, PIL in this thread."""
    from PIL import Image
    q = lambda x, b=0.5: x.mul(255).add_(b).clamp_(0, 255).to(torch.uint8)  # noqa: E731
    rgb = lambda x: (x.expand(3, -1, -1) if x.shape[0] == 1 else x).permute(1, 2, 0)  # noqa: E731
    n = 0
    for key, path in paths.items():
        if key == "depth":
            d = planes["depth"]
            img = rgb(q((d - d.min()) / (d.max() - d.min())))
        elif key in ("normal", "from_depth"):
            img = rgb(q(planes[key]))
        else:
            src = render_scene.PBR_PLANES[key]
            if isinstance(src, tuple):
                img = torch.cat([rgb(q(planes[s])) for s in src], dim=1)
            else:
                img = rgb(q(planes[src], 0.0 if key == "_occlusion" else 0.5))
        Image.fromarray(img.contiguous().cpu().numpy(), "RGB").save(path)
        n += os.path.getsize(path)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--light", type=int, default=256)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup_views", type=int, default=4)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "bench_out", "render_scene"))
    ap.add_argument("--keep", action="store_true", help="keep the written images")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--repeats", type=int, default=20)
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
    ev = evaluate.NovelViewEvaluator(light, scenes.GI_DEFAULTS, 2, extra_planes=True)
    res = dict(size=args.size, P=args.P, views=args.views, blocks=args.blocks, workers=args.workers, slots=args.slots)

    def planes_of(i):
        cam, vd = views[i % len(views)]
        return ev(cam, g, vd, gt, alpha)

    def paths_of(mode, i):
        return render_scene.view_paths(os.path.join(args.out, mode), "test", 0, i, "v%03d" % i)

    for mode in ("writer", "pil"):
        for p in paths_of(mode, 0).values():
            os.makedirs(os.path.dirname(p), exist_ok=True)

    if args.kernels:
        images = render_scene.view_images(paths_of("writer", 0), planes_of(0))
        pack_b, filt_b = algorithmic_bytes(images)
        for _ in range(3):
            image_writer.encode(images)
        lay = image_writer._Layout(images)
        import gigs_lib
        bufs = [torch.empty(n, dtype=torch.uint8, device=dev) for n in (lay.sheet_bytes, lay.stream_bytes, lay.table_bytes)]
        lohi = torch.empty(2 * max(1, lay.n_norm), device=dev)
        scratch = torch.empty(gigs_lib.MINMAX_SCRATCH_FLOATS, device=dev)
        th = torch.empty(lay.table_bytes, dtype=torch.uint8).pin_memory()
        s = torch.cuda.current_stream().cuda_stream
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(args.repeats):
            image_writer._launch(lay, bufs[0], bufs[1], lohi, scratch, th, bufs[2], s)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.repeats
        res.update(mode="kernels", images=len(images), pack_bytes=pack_b, filter_bytes=filt_b, stream_bytes=lay.stream_bytes,
                   float_bytes=sum(4 * t.numel() for im in images for t in im.planes), launches_ms_per_view=round(ms, 4))
        print(json.dumps(res))
        ev.close()
        return

    def block(mode, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = {}
        if mode == "writer":
            with image_writer.ImageWriter(workers=args.workers, slots=args.slots) as wr:
                for i in range(n):
                    wr.submit(render_scene.view_images(paths_of(mode, i), planes_of(i)))
            info = dict(submit_blocked_s=round(wr.blocked_s, 3), png_bytes=wr.bytes_written)
        elif mode == "pil":
            info = dict(png_bytes=sum(pil_write(paths_of(mode, i), planes_of(i)) for i in range(n)))
        else:
            for i in range(n):
                planes_of(i)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dict(info, seconds=round(dt, 3), views_per_s=round(n / dt, 2))

    for mode in ("evaluator", "writer", "pil"):
        block(mode, args.warmup_views)
    rows = {"writer": [], "pil": [], "evaluator": []}
    for _ in range(args.blocks):
        for mode in ("writer", "pil", "evaluator"):
            rows[mode].append(block(mode, args.views))
    for mode, rs in rows.items():
        v = [r["views_per_s"] for r in rs]
        res[mode] = dict(views_per_s=[statistics.median(v), min(v), max(v)], blocks=rs)
    res["writer_not_slower_in_any_block"] = all(a["views_per_s"] >= b["views_per_s"] for a, b in zip(rows["writer"], rows["pil"]))
    res["writer_over_pil"] = round(res["writer"]["views_per_s"][0] / res["pil"]["views_per_s"][0], 2)
    res["png_bytes_writer_over_pil"] = round(rows["writer"][-1]["png_bytes"] / rows["pil"][-1]["png_bytes"], 4)
    # the two writers' files hold the same pixels
    from PIL import Image
    for key in ("", "_brdf", "depth", "_occlusion"):
        a, b = (np.asarray(Image.open(paths_of(m, args.views - 1)[key])) for m in ("writer", "pil"))
        assert np.array_equal(a, b), key
    res["same_pixels"] = True
    ev.close()
    if not args.keep:
        shutil.rmtree(args.out, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
