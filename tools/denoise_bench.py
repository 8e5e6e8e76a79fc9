"""Times the a-trous denoiser (gi-gs_amd/denoise.py: atrous) on the covered pixels of one view of an extracted mesh, beside the
trace it filters (mesh.gather_points at 64 rays) in the same session, and measures what it buys: the RMSE of the raw and of the
filtered planes against a 1024-ray trace of the same view.

    python tools/denoise_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--rays 64]
                                  [--more_rays 256] [--reference_rays 1024] [--sky_res 32] [--repeats 7]

The mesh, the view and the points are tools/mesh_gather_bench.py's: the C2 stand-in scene fused from --fuse_views orbit views,
extracted at --grid and simplified by --ratio, rasterized once at --size x --size from the first orbit camera.  By device
events after three warm-up calls, the median (and the least and the largest) of --repeats:
    gather_ms          mesh.gather_points at --rays with the sky and the radiosity of one bounce
    atrous_ms[C][n]    denoise.atrous of C = 7 channels (occlusion, irradiance, indirect: groups 1, 3, 3) and of C = 11 (those
                       and four further single channels, as four shadow planes would be), n = 1 .. 5 iterations, the whole call:
                       pack, variance, n steps, unpack, the read-back of the live count
and, over the covered pixels, rmse[plane] = {raw at --rays, filtered at --rays (shipped defaults), raw at --more_rays} against
the trace at --reference_rays, for occlusion and irradiance.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import denoise  # noqa: E402
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402


def spread_ms(fn, repeats, warmup=3):
    """-> dict(median, least, largest) in ms by device events."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return dict(median=round(statistics.median(times), 4), least=round(min(times), 4), largest=round(max(times), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--rays", type=int, default=64)
    ap.add_argument("--more_rays", type=int, default=256)
    ap.add_argument("--reference_rays", type=int, default=1024)
    ap.add_argument("--sky_res", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = H = args.size
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in pipeline.RASTER_KEYS}
    fuse = [scenes.orbit_camera(i, args.fuse_views, W, H, radius=3.5, elevation=0.5 if i % 2 == 0 else 0.9)
            for i in range(args.fuse_views)]
    lo, hi = mesh.auto_bounds(g)
    voxel, dims = mesh.grid_for_bounds(lo, hi, args.grid)
    vol = mesh.TSDFVolume(lo, voxel, dims, 4 * voxel, device=dev)
    mesh.fuse_views(g, 2, fuse, scenes.GI_DEFAULTS, vol)
    raw = vol.extract(2)
    origin = vol.lo
    del vol
    pipeline._collect_idle()
    m, _ = mesh.simplify(raw, args.ratio * voxel, origin=origin)
    del raw
    base = relight.latlong_to_cubemap(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(dev), [256, 256])
    sky = mesh.sky_cube(base, args.sky_res)
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in fuse[0].items()}
    rho = (m.albedo * (1.0 - m.metallic)[:, None]).contiguous()
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, vertices=int(m.vertices.shape[0]),
               faces=int(m.faces.shape[0]), rays=args.rays)
    with mesh_render.MeshRasterizer(m, device=dev) as rast, \
            mesh_render.RaytracedLight(m, rays=args.rays, cube=sky, bounces=1, reflectance=rho, device=dev) as tracer:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        view = (o["pos"], o["normal"], cam["viewmatrix"], cover)
        t = tracer.planes(*view)
        res.update(pixels=int(cover.numel()), pixels_covered=int(cover.sum()), plane_distance=tracer.plane_distance())
        res["gather_ms"] = spread_ms(lambda: tracer.planes(*view), args.repeats)
        signal7 = torch.cat([t["occlusion"], t["irradiance"], t["indirect"]], 0)
        signal11 = torch.cat([signal7, t["occlusion"].expand(4, H, W) * torch.rand((4, 1, 1), device=dev)], 0).contiguous()
        res["atrous_ms"] = {}
        for signal, groups in ((signal7, [1, 3, 3]), (signal11, [1, 3, 3, 1, 1, 1, 1])):
            rows = {}
            for n in range(1, denoise.MAX_ITERATIONS + 1):
                rows[n] = spread_ms(lambda: denoise.atrous(signal, t["points"], t["normals"], t["mask"], groups, n,
                                                           plane_distance=tracer.plane_distance()), args.repeats)
            res["atrous_ms"][int(signal.shape[0])] = rows
            print(json.dumps({"channels": int(signal.shape[0]), "atrous_ms": rows}), flush=True)
        d = tracer.denoise(t)
        more = tracer.planes(*view, rays=args.more_rays)
        ref = tracer.planes(*view, rays=args.reference_rays)
        rmse = lambda x, y: float(((x.double() - y.double()).pow(2) * cover).sum().div(cover.sum() * x.shape[0]).sqrt())  # noqa: E731
        res["denoise_report"] = d["denoise_report"]
        res["rmse"] = {k: {"raw_%d" % args.rays: rmse(t[k], ref[k]), "filtered_%d" % args.rays: rmse(d[k], ref[k]),
                           "raw_%d" % args.more_rays: rmse(more[k], ref[k])} for k in ("occlusion", "irradiance")}
        res["reference_rays"] = args.reference_rays
    print(json.dumps(res))


if __name__ == "__main__":
    main()
