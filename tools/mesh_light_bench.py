"""Times baking light into an extracted mesh (gi-gs_amd/mesh.py: trace_hemispheres, gather_light) and records what the bake
says about the mesh.

    python tools/mesh_light_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--rays 64 256]
                                     [--bounces 4] [--sky_res 32] [--repeats 15] [--slow_ms 3000]

The mesh is tools/mesh_bake_bench.py's: the C2 stand-in scene fused from --fuse_views orbit views and extracted at --grid,
and its --ratio simplification.  The sky is scenes.synthetic_envmap as a 256^2 cube pooled to --sky_res (mesh.sky_cube).  Per
mesh and per --rays, by device events after three warm-up calls, the median of --repeats:
    trace_ms          mesh.trace_hemispheres (no distance limit), the whole call
    occlusion_ms      mesh.bake_occlusion with the same rays, bias and NO distance limit either: the same traversals with a
                      count in place of the records, so the difference is what the records cost
    gather_ms         one pass of gigs_mesh_gather_light on the call's own arrays, pass 0 (sky only) and pass 1 (with the
                      previous radiosity); bytes = the 12 V R of the records plus the 24 V of the two outputs, and
                      share_of_copy = bytes / time over the 6.3 TB/s copy rate DESIGN.md uses
    mean_irradiance   of the passes 0 .. --bounces, and the counters of the trace
A timed call whose first warm-up takes more than --slow_ms is timed with three repeats.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402
from mesh_bake_bench import events_ms  # noqa: E402

COPY_RATE = 6.3e12  # bytes / s: the copy rate DESIGN.md sets memory-bound kernels beside


def light_rows(m, grid, sky, args):
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    rows = []
    for R in args.rays:
        hits, report = mesh.trace_hemispheres(m, rays=R, grid=grid)
        passes, _, gathered = mesh._gather_light(m, hits, sky, bounces=args.bounces)
        row = dict(rays=R, trace=report, mean_irradiance=gathered["mean_irradiance"])
        row["trace_ms"], row["repeats"] = events_ms(lambda: mesh.trace_hemispheres(m, rays=R, grid=grid), args.repeats, args.slow_ms)
        far = 1e30  # bake_occlusion takes a finite distance: one no ray of the scene reaches
        row["occlusion_ms"], _ = events_ms(lambda: mesh.bake_occlusion(m, rays=R, grid=grid, max_distance=far, bias=report["bias"]),
                                           args.repeats, args.slow_ms)
        table = torch.from_numpy(hits.directions).to(dev)
        rho = (m.albedo * (1.0 - m.metallic)[:, None]).contiguous()
        out, rad, prev = (torch.zeros((V, 3), device=dev) for _ in range(3))
        prev.copy_(rho * passes[0])
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream().cuda_stream
        nbytes = 12 * V * R + 24 * V
        for name, previous in (("pass0", None), ("pass1", prev)):
            def launch():
                gigs_lib.check(gigs_lib.lib().gigs_mesh_gather_light(
                    V, F, m.vertices.data_ptr(), m.normals.data_ptr(), m.faces.data_ptr(), table.data_ptr(), R, hits.rotations,
                    hits.seed, hits.face.data_ptr(), hits.bary.data_ptr(), int(sky.shape[1]), sky.data_ptr(), rho.data_ptr(),
                    previous.data_ptr() if previous is not None else None, out.data_ptr(), rad.data_ptr(), overflow.data_ptr(), s),
                    "gather")
            ms, _ = events_ms(launch, args.repeats, args.slow_ms)
            assert int(overflow.item()) == 0 and torch.equal(out, passes[0 if previous is None else 1])
            row["gather_%s_ms" % name] = ms
            row["gather_%s_share_of_copy" % name] = round(nbytes / (ms * 1e-3) / COPY_RATE, 4)
        row["gather_bytes"] = nbytes
        rows.append(row)
        del hits, passes
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--sky_res", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--slow_ms", type=float, default=3000.0)
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
    simple, _ = mesh.simplify(raw, args.ratio * voxel, origin=origin)
    sky = mesh.sky_cube(relight.latlong_to_cubemap(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(dev), [256, 256]), args.sky_res)
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, sky_res=args.sky_res, meshes=[])
    for name, m in (("raw", raw), ("simplified", simple)):
        grid = mesh.triangle_grid(m)
        row = dict(name=name, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]),
                   grid=dict(cell=grid.cell, dims=list(grid.dims), pairs=int(grid.pairs.shape[0])))
        row["light"] = light_rows(m, grid, sky, args)
        res["meshes"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
