"""Times rendering and relighting an exported mesh (gi-gs_amd/mesh_render.py) beside the Gaussians it came from.

    python tools/mesh_render_bench.py [--grid 256] [--size 800] [--P 300000] [--views 32] [--fuse_views 64]
                                      [--small_max 16 64 256]
    python tools/mesh_render_bench.py --kernels   (few views, for `rocprofv3 --kernel-trace --stats` in a run of its own)

The C2 stand-in scene (scenes.surface_scene) is fused from --fuse_views orbit views and extracted at --grid
(mesh.fuse_views, TSDFVolume.extract).  Then, at --size squared and by device events over --views orbit views after a
warm-up pass over the same views:
    raster        gigs_mesh_project + the clear of the key plane + gigs_mesh_raster + gigs_mesh_resolve, per --small_max
    mesh relight  the full MeshRelighter view (raster, derived normals, SSAO, G-buffer post, shade, SSR, finish)
    splat raster  pipeline.rasterize(inference=True) of the Gaussians (with its derived normals and SSAO)
    splat relight Relighter(fused=True, graphs=False) of the Gaussians
The bytes the raster algorithm needs per view: the key plane cleared and read once (8 B written + 8 B read per pixel),
68 B of planes written per pixel, the vertex array read and the projected arrays written and read back once
(12 + 2 x 21 B per vertex), the face array read twice (raster and, for the winners, resolve: 2 x 12 B per face).  Atomic
traffic on the key plane is not counted: it depends on the depth complexity.  `bytes / time` is set against the 6.3 TB/s
copy rate: the floor of a rasterizer that did nothing but move those bytes.
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
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402

COPY_RATE = 6.3e12  # bytes / s, the measured HBM copy rate


def raster_bytes(V, F, W, H):
    return (8 + 8 + 68) * W * H + (12 + 2 * 21) * V + 2 * 12 * F


def events_ms(fn, cams):
    """Mean time per view of fn(cam) over `cams`, after one warm-up pass over the same views."""
    for c in cams:
        fn(c)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for c in cams:
        fn(c)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / len(cams)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--small_max", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = H = args.size
    n_views = 2 if args.kernels else args.views
    gi = scenes.GI_DEFAULTS
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in pipeline.RASTER_KEYS}
    fuse = [scenes.orbit_camera(i, args.fuse_views, W, H, radius=3.5, elevation=0.5 if i % 2 == 0 else 0.9)
            for i in range(args.fuse_views)]
    lo, hi = mesh.auto_bounds(g)
    voxel, dims = mesh.grid_for_bounds(lo, hi, args.grid)
    vol = mesh.TSDFVolume(lo, voxel, dims, 4 * voxel, device=dev)
    mesh.fuse_views(g, 2, fuse, gi, vol)
    m = vol.extract(2)
    del vol
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cams = []
    for i in range(n_views):
        c = scenes.orbit_camera(i, n_views, W, H, radius=3.5, elevation=0.6)
        cams.append({k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    rays = pipeline.canonical_rays(cams[0], dev)
    vds = {id(c): pipeline.view_dirs_for(c, rays, dev) for c in cams}
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=256)
    bg = torch.zeros(3, device=dev)
    rast = mesh_render.MeshRasterizer(m, device=dev)
    V, F = rast.V, rast.F
    b = raster_bytes(V, F, W, H)
    res = dict(size=args.size, P=args.P, grid=args.grid, views=n_views, vertices=V, faces=F, raster_bytes_per_view=b,
               copy_floor_ms=round(b / COPY_RATE * 1e3, 4), raster=[])
    with torch.no_grad():
        o = rast(cams[0])
        res["covered_share"] = round(float((o["tri_id"] >= 0).float().mean()), 4)
        boxes = rast._screen[rast._mesh["faces"].long().clamp(0, max(V - 1, 0))]  # [F,3,2]
        ext = ((boxes.max(1).values >> 8) - ((boxes.min(1).values + 255) >> 8) + 1).clamp(min=0).prod(1)
        res["box_pixels"] = dict(median=float(ext.float().median()), p99=float(ext.float().quantile(0.99)), max=int(ext.max()))
        for sm in args.small_max:
            ms = events_ms(lambda c, sm=sm: rast(c, small_max=sm), cams)
            res["raster"].append(dict(small_max=sm, ms_per_view=round(ms, 4), tb_per_s=round(b / (ms * 1e-3) / 1e12, 3),
                                      of_copy_rate=round(b / (ms * 1e-3) / COPY_RATE, 3)))
        mrl = mesh_render.MeshRelighter(light, gi)
        res["mesh_relight_ms"] = round(events_ms(lambda c: mrl(c, rast, vds[id(c)]), cams), 4)
        res["splat_raster_ms"] = round(events_ms(lambda c: pipeline.rasterize(c, g, 2, bg, gi, inference=True), cams), 4)
        srl = relight.Relighter(light, gi, 2, fused=True, graphs=False)
        res["splat_relight_ms"] = round(events_ms(lambda c: srl(c, g, vds[id(c)]), cams), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
