"""Times baking a texture atlas over a simplified mesh from the extracted one (gi-gs_amd/mesh.py: bake_atlas), stage by stage,
against the closest-point search alone, and records what the atlas buys: the material error of the atlas and of the light
mesh's own vertices against the heavy mesh.

    python tools/mesh_atlas_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratios 2 4] [--block 8]
                                     [--repeats 15] [--samples 100000] [--ao_rays 64]

The meshes are tools/mesh_bake_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit views
and extracted at --grid (the source), and per --ratios its simplification with cells of that many voxels from the volume's
corner (the target).  The source's occlusion is mesh.bake_occlusion with --ao_rays rays.  Per ratio, by device events after
three warm-up calls, the median of --repeats:
    bake_atlas        the whole call with the source's grid passed in (allocations, the one read-back and the host's sort of
                      the queries by cell included)
    points            gigs_mesh_atlas_points alone, on buffers of its own
    search            mesh._closest on the texel points (the host's sort by cell and gigs_mesh_closest)
    transfer          gigs_mesh_transfer alone, nine channels, on the search's faces
    closest_point     the reference: mesh.closest_point of the same texel points, the search as it was before this tool's
                      kernels existed
    triangle_grid     mesh.triangle_grid(source), which bake_atlas runs when no grid is passed
and, with --samples N, texture_mesh.material_error: per channel group the RMS difference to the source of the atlas lookup
and of the target's own per-vertex attributes at N surface samples of the target.  These are times of this tool's calls; no
hardware rate is derived from them.
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
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import pipeline  # noqa: E402
import scenes  # noqa: E402
import texture_mesh  # noqa: E402


def events_ms(fn, repeats, warmup=3):
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
    return round(statistics.median(times), 4)


def atlas_row(dst, src, occlusion, grid, args):
    dev = src.vertices.device
    atlas, report = mesh.bake_atlas(dst, src, block=args.block, occlusion=occlusion, grid=grid)
    lay = atlas.layout
    row = dict(faces=int(dst.faces.shape[0]), vertices=int(dst.vertices.shape[0]), report=report,
               queries=lay.n_blocks * lay.block * (lay.block + 1))
    row["bake_atlas_ms"] = events_ms(lambda: mesh.bake_atlas(dst, src, block=args.block, occlusion=occlusion, grid=grid), args.repeats)
    row["points_ms"] = events_ms(lambda: mesh._atlas_points(dst, lay), args.repeats)
    points, _, _, dest, _ = mesh._atlas_points(dst, lay)
    row["search_ms"] = events_ms(lambda: mesh._closest(points, src, grid, None), args.repeats)
    _, face, _ = mesh._closest(points, src, grid, None)
    values = torch.cat((src.albedo, occlusion[:, None], src.roughness[:, None], src.metallic[:, None], src.normals), 1).contiguous()
    # the launch alone: the outputs are allocated and cleared once, outside the timed region
    N, plane = int(points.shape[0]), lay.width * lay.height
    out = torch.zeros((9, plane), dtype=torch.float32, device=dev)
    coverage = torch.zeros(plane, dtype=torch.uint8, device=dev)
    bary = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    def launch():
        gigs_lib.check(gigs_lib.lib().gigs_mesh_transfer(
            int(src.vertices.shape[0]), int(src.faces.shape[0]), src.vertices.data_ptr(), src.faces.data_ptr(), 9, values.data_ptr(),
            N, points.data_ptr(), face.data_ptr(), dest.data_ptr(), plane, out.data_ptr(), coverage.data_ptr(), bary.data_ptr(),
            counts.data_ptr(), counts[2:].data_ptr(), s), "transfer")

    row["transfer_ms"] = events_ms(launch, args.repeats)
    assert torch.equal(out.view(9, lay.height, lay.width)[0:3], atlas.albedo) and int(counts[2]) == 0
    row["transfer_call_ms"] = events_ms(lambda: mesh._transfer(points, face, src, values, dest, plane), args.repeats)
    row["closest_point_ms"] = events_ms(lambda: mesh.closest_point(points, src, grid=grid), args.repeats)
    if args.samples > 0:
        dst_occ = mesh.transfer_attributes(dst.vertices, src, occlusion, grid=grid)[0][:, 0].contiguous()
        row["material_error"] = texture_mesh.material_error(dst, dst_occ, src, occlusion, atlas, args.samples, grid=grid)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratios", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--ao_rays", type=int, default=64)
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
    grid = mesh.triangle_grid(raw)
    occlusion, _ = mesh.bake_occlusion(raw, rays=args.ao_rays, grid=grid)
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, block=args.block,
               source=dict(vertices=int(raw.vertices.shape[0]), faces=int(raw.faces.shape[0]), cell=grid.cell, dims=list(grid.dims),
                           pairs=int(grid.pairs.shape[0])),
               triangle_grid_ms=events_ms(lambda: mesh.triangle_grid(raw), args.repeats), targets=[])
    for ratio in args.ratios:
        simple, _ = mesh.simplify(raw, ratio * voxel, origin=origin)
        row = dict(ratio=ratio, **atlas_row(simple, raw, occlusion, grid, args))
        res["targets"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
