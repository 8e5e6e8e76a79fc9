"""Times a turntable -- one view under N yaw rotations of one environment map -- at BASELINE config C3 size (800x800, 300k
Gaussians, 256^2 lights) along three paths, alternated block by block in one process so that drift affects all alike:

    turntable    relight.TurntableRelighter: one G-buffer, one recorded march, then shade + gather per 16 lights
    multi16      the same lights through relight.MultiRelighter in chunks of 16 (a G-buffer, SSAO and ceil(K/4) marches per
                 chunk): relight_scene's path before TurntableRelighter, eager and replayed from hipGraphs
    relighter    N x relight.Relighter (eager)

Reported: median [min, max] ms per rotation over the blocks, per N.  Separately, what a turntable pays once and not per
view: the rotated conversion (one launch for all N) and build_mips per rotated light.

    python tools/turntable_bench.py [--ns 16,64] [--blocks 5] [--views 4] [--size 800] [--P 300000] [--light 256]

--gather runs only the hit-list gathers of one view, K = 16 planes: 16 x gigs_ssr_apply against one gigs_ssr_apply_multi,
timed with events and meant to be read from a kernel trace in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/turntable_bench.py --gather

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
import gigs_lib  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402

DEV = "cuda:0"


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stats(v):
    v = sorted(v)
    return dict(median=round(float(np.median(v)), 4), min=round(v[0], 4), max=round(v[-1], 4))


def timed(fn, n):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(n):
        fn(i)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / n


def gather_only(args, g, views):
    """One C3 view's hit list, then K = 16 planes through 16 single gathers and through one multi gather."""
    from diff_gaussian_rasterization import _gi_scratch
    lib = gigs_lib.lib()
    W = H = args.size
    gi = scenes.GI_DEFAULTS
    ct, _ = views[0]
    b = relight.SplatGBuffer(gi, 2)(ct, g)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = (W, H, float(W / (2.0 * ct["tanfovx"])), float(H / (2.0 * ct["tanfovy"])), float(gi["radius"]), float(gi["bias"]),
         float(gi["thick"]), float(gi["delta"]), int(gi["step"]), int(gi["start"]))
    s = torch.cuda.current_stream().cuda_stream
    scratch = _gi_scratch(W, H, DEV)
    n = W * H
    counts = torch.zeros(4 * n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(4 * n + 1, dtype=torch.int32, device=DEV)
    c0, a0 = torch.empty(3, H, W, device=DEV), torch.empty(3, H, W, device=DEV)
    planes = (p(b["onv"]), p(b["depth_pos"]), p(b["albedo_map"]), p(b["albedo_map"]), p(b["roughness_map"]),
              p(b["metallic_in"]), p(b["F0"]), p(c0), p(a0))
    gigs_lib.check(lib.gigs_ssr_hits(gigs_lib.ctx_ptr(), *a, *planes, 1, p(counts), None, None, 0, p(scratch), s), "count")
    torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
    total = int(offsets[-1])
    entries = torch.empty((max(total, 1), 2), dtype=torch.int32, device=DEV)
    gigs_lib.check(lib.gigs_ssr_hits(gigs_lib.ctx_ptr(), *a, *planes, 2, None, p(offsets), p(entries), total, p(scratch), s),
                   "fill")
    K = 16
    rgb = torch.rand((K, 3, H, W), device=DEV)
    color, abd = torch.empty((K, 3, H, W), device=DEV), torch.empty((K, 3, H, W), device=DEV)
    tail = (p(b["albedo_map"]), p(b["metallic_in"]), p(b["F0"]))

    def single(_):
        for k in range(K):
            gigs_lib.check(lib.gigs_ssr_apply(W, H, float(gi["delta"]), p(offsets), p(entries), p(b["onv"]), p(b["depth_pos"]),
                                              p(rgb[k]), *tail, p(color[k]), p(abd[k]), s), "ssr_apply")

    packed = torch.empty(int(lib.gigs_ssr_apply_multi_scratch_bytes(K, W, H)), dtype=torch.uint8, device=DEV)

    def multi(_):
        gigs_lib.check(lib.gigs_ssr_apply_multi(K, W, H, float(gi["delta"]), p(offsets), p(entries), p(b["onv"]),
                                                p(b["depth_pos"]), p(rgb), *tail, p(color), p(abd), p(packed), s),
                       "ssr_apply_multi")

    def march(_):
        gigs_lib.check(lib.gigs_ssr_multi(gigs_lib.ctx_ptr(), K, *a, p(b["onv"]), p(b["depth_pos"]), p(rgb), p(b["albedo_map"]),
                                          p(b["roughness_map"]), p(b["metallic_in"]), p(b["F0"]), p(color), p(abd), p(scratch),
                                          s), "ssr_multi")

    fns = dict(apply_single_x16=single, apply_multi_16=multi, march_multi_16=march)
    for fn in fns.values():
        fn(0)
    samples = {k: [] for k in fns}
    for blk in range(args.blocks):
        order = list(fns.items())
        for name, fn in (order if blk % 2 == 0 else order[::-1]):
            samples[name].append(timed(fn, args.views))
    return dict(mode="gather", size=args.size, hits=total, hits_per_pixel=round(total / n, 3), planes=K,
                lib=os.path.basename(gigs_lib.LIB_PATH), ms_per_16_planes={k: stats(v) for k, v in samples.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="16,64")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--light", type=int, default=256)
    ap.add_argument("--gather", action="store_true")
    args = ap.parse_args()
    W = H = args.size
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: tt(sc[k]) for k in pipeline.RASTER_KEYS}
    views = []
    for i in range(8):
        cam = scenes.orbit_camera(i, 8, W, H, radius=3.5)
        ct = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        views.append((ct, pipeline.view_dirs_for(ct, pipeline.canonical_rays(cam, DEV), DEV)))
    if args.gather:
        with torch.no_grad():
            print(json.dumps(gather_only(args, g, views)))
        return
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - W / 2) ** 2 + (yy - H / 2) ** 2) < (0.475 * W) ** 2).astype(np.float32)[None])
    gi = scenes.GI_DEFAULTS
    env = tt(scenes.synthetic_envmap(512, 1024, seed=1))
    res = dict(size=args.size, P=args.P, light=args.light, views=args.views, blocks=args.blocks, ms_per_rotation={}, once={})
    for n in [int(x) for x in args.ns.split(",")]:
        turns = relight.yaw_rotations(n)
        convert = [timed(lambda _: relight.latlong_to_cubemap_rot(env, [args.light, args.light], turns), 3) for _ in range(3)]
        lights = relight.rotated_lights(env, turns, res=args.light)
        with torch.no_grad():
            lights[0].build_mips()
            mips = [timed(lambda i: lights[i % n].build_mips(), n) for _ in range(3)]
        res["once"][str(n)] = dict(convert_all_ms=stats(convert), build_mips_ms_per_light=stats(mips))
        tr = relight.TurntableRelighter(lights, gi, 2)
        chunks = [lights[i:i + relight.MAX_LIGHTS] for i in range(0, n, relight.MAX_LIGHTS)]
        eager = [relight.MultiRelighter(c, gi, 2) for c in chunks]
        graphed = [relight.MultiRelighter(c, gi, 2, graphs=True) for c in chunks]
        singles = [relight.Relighter(l, gi, 2) for l in lights]

        def view(i):
            return views[i % len(views)]

        def run_turntable(i):
            tr(view(i)[0], g, view(i)[1], alpha_mask=alpha)

        def run_eager(i):
            for m in eager:
                m(view(i)[0], g, view(i)[1], alpha_mask=alpha)

        def run_graphed(i):
            for m in graphed:
                m(view(i)[0], g, view(i)[1], alpha_mask=alpha)

        def run_singles(i):
            for r in singles:
                r(view(i)[0], g, view(i)[1], alpha_mask=alpha)

        fns = dict(turntable=run_turntable, multi16_eager=run_eager, multi16_graphs=run_graphed, relighter=run_singles)
        for fn in fns.values():  # warm up; capture the graphs
            for i in range(2):
                fn(i)
        samples = {k: [] for k in fns}
        for blk in range(args.blocks):
            order = list(fns.items())
            for name, fn in (order if blk % 2 == 0 else order[::-1]):
                samples[name].append(timed(fn, args.views) / n)
        row = {k: stats(v) for k, v in samples.items()}
        row["hits_per_pixel"] = round(tr.last_hits / (W * H), 3) if tr.last_hits else None
        res["ms_per_rotation"][str(n)] = row
        for r in [tr, *eager, *graphed, *singles]:
            r.close()
        del tr, eager, graphed, singles, lights
        pipeline._collect_idle()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
