"""Times ray casting against an extracted mesh and baking its ambient occlusion (gi-gs_amd/mesh.py: raycast,
bake_occlusion), and records what the bake says about the mesh.

    python tools/mesh_bake_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--rays 64 256]
                                    [--casts 100000 1000000] [--repeats 15] [--host_rays 2000] [--slow_ms 3000]

The mesh is tools/mesh_simplify_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit
views and extracted at --grid, and its --ratio simplification (cell = ratio voxels from the volume's corner).  Per mesh:
    bake              mesh.bake_occlusion per --rays by device events, after three warm-up calls, the median of --repeats;
                      the launch alone (gigs_mesh_bake_occlusion on the call's own arrays), with the vertices in cell order
                      and in their own; the outcome: mean, a ten-bin histogram of the baked values, no_normal, hits_total
    raycast           per --casts N: N rays from hash-random origins in a box of twice the mesh's extent towards surface
                      samples of the mesh; mesh.raycast, and the launch alone with and without the host's sort by entry cell
    brute             the launch on a one-cell grid (every face for every ray: the GPU's own brute force), the smallest
                      --casts, one timed call, the simplified mesh only (the raw mesh has four times the faces), and whether
                      its bits are the grid's
    host              the numpy restatement (tests/mesh_raycast_ref.py) on --host_rays of the same rays, grid construction
                      apart (wall clock): whether face, t and bary bits agree, and the mean cells and faces visited per ray
A timed call whose first warm-up takes more than --slow_ms is timed with three repeats; `repeats` says which.  These are
times of this tool's calls; no hardware rate is derived from them.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import mesh_raycast_ref  # noqa: E402
import pipeline  # noqa: E402
import scenes  # noqa: E402


def events_ms(fn, repeats, slow_ms, warmup=3):
    """-> (median ms, repeats used)."""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    if (time.perf_counter() - t0) * 1e3 > slow_ms:
        repeats = min(repeats, 3)
    else:
        for _ in range(warmup - 1):
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
    return round(statistics.median(times), 4), repeats


def bake_rows(m, grid, rays, args):
    rows = []
    for R in rays:
        occ, hits, report = mesh._bake_occlusion(m, rays=R, grid=grid)
        row = dict(rays=R, report=report, mean=float(occ.double().mean().item()),
                   histogram=[int(x) for x in torch.histc(occ, bins=10, min=0.0, max=1.0).cpu().tolist()])
        row["call_ms"], row["repeats"] = events_ms(lambda: mesh.bake_occlusion(m, rays=R, grid=grid), args.repeats, args.slow_ms)
        # the launch alone: everything the call does before it is hoisted by keeping the order and the table
        for name, sort in (("launch_ms", True), ("launch_unsorted_ms", False)):
            order = mesh._cell_order(m.vertices.double(), grid) if sort else None
            table = torch.from_numpy(mesh.occlusion_directions(R, 16)).to(m.vertices.device)
            V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
            out, h = torch.empty(V, device=m.vertices.device), torch.empty(V, dtype=torch.int32, device=m.vertices.device)
            counts = torch.zeros(3, dtype=torch.int64, device=m.vertices.device)
            c_lo, c_dims = mesh._c_grid(grid.lo, grid.dims)
            s = torch.cuda.current_stream().cuda_stream

            def launch():
                gigs_lib.check(gigs_lib.lib().gigs_mesh_bake_occlusion(
                    V, F, m.vertices.data_ptr(), m.normals.data_ptr(), m.faces.data_ptr(), c_lo, grid.cell, c_dims,
                    grid.cell_start.data_ptr(), grid.pairs.data_ptr(), int(grid.pairs.shape[0]), mesh._scale(grid),
                    order.data_ptr() if order is not None else None, table.data_ptr(), R, 16, 0, report["max_distance"],
                    report["bias"], out.data_ptr(), h.data_ptr(), counts.data_ptr(), counts[2:].data_ptr(), s), "bake")

            row[name], _ = events_ms(launch, args.repeats, args.slow_ms)
            assert torch.equal(h, hits) and int(counts[2]) == 0
        rows.append(row)
    return rows


def make_rays(m, grid, n, seed=0):
    dev = m.vertices.device
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    lo = torch.from_numpy(grid.lo.astype(np.float32)).to(dev)
    ext = torch.tensor(grid.dims, dtype=torch.float32, device=dev) * float(grid.cell)
    o = lo + 0.5 * ext + (torch.rand((n, 3), generator=gen, device=dev) - 0.5) * 2.0 * ext
    target = mesh.sample_surface(m, n, seed)[0]
    return o.contiguous(), (target - o).contiguous()


def raycast_rows(m, grid, casts, args, brute, host):
    rows = []
    for k, n in enumerate(sorted(casts)):
        o, d = make_rays(m, grid, n)
        t, face, bary, report = mesh.raycast(o, d, m, grid=grid)
        row = dict(rays=n, report=report)
        row["call_ms"], row["repeats"] = events_ms(lambda: mesh.raycast(o, d, m, grid=grid), args.repeats, args.slow_ms)
        row["sort_ms"], _ = events_ms(lambda: mesh._entry_order(o, d, grid), args.repeats, args.slow_ms)
        for name, sort in (("launch_ms", True), ("launch_unsorted_ms", False)):
            # _raycast allocates its outputs and sorts; the sort is timed apart above
            ms, _ = events_ms(lambda: mesh._raycast(o, d, m, grid, None, sort=sort), args.repeats, args.slow_ms)
            row[name] = round(ms - (row["sort_ms"] if sort else 0.0), 4)
        if k == 0 and brute:
            one = mesh.triangle_grid(m, cell=1e6 * grid.cell)
            assert one.dims == (1, 1, 1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            tb, fb, bb, _ = mesh.raycast(o, d, m, grid=one)
            t1.record()
            torch.cuda.synchronize()
            row["brute_ms"] = round(t0.elapsed_time(t1), 3)
            row["brute_equal"] = bool(torch.equal(fb, face) and torch.equal(tb.view(torch.int32), t.view(torch.int32))
                                      and torch.equal(bb.view(torch.int32), bary.view(torch.int32)))
        if k == 0 and host:
            hq = min(args.host_rays, n)
            hv, hf = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
            t0 = time.perf_counter()
            hg = mesh_raycast_ref.build_grid(hv, hf, cell=grid.cell)
            tg = time.perf_counter()
            want = mesh_raycast_ref.raycast(o[:hq].cpu().numpy(), d[:hq].cpu().numpy(), hv, hf, grid=hg)
            bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
            row["host"] = dict(rays=hq, grid_s=round(tg - t0, 2), raycast_ms=round((time.perf_counter() - tg) * 1e3, 1),
                               same_grid=bool(list(hg["G"]) == list(grid.dims)),
                               faces_equal=bool(np.array_equal(face[:hq].cpu().numpy(), want["face"])),
                               t_bits_equal=bool(np.array_equal(bits(t[:hq].cpu().numpy()), bits(want["t"]))),
                               bary_bits_equal=bool(np.array_equal(bits(bary[:hq].cpu().numpy()), bits(want["bary"]))),
                               slabs_per_ray=round(want["slabs"] / hq, 2), cells_per_ray=round(want["cells"] / hq, 2),
                               faces_per_ray=round(want["tests"] / hq, 2), hits=want["hits"])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--rays", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--casts", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host_rays", type=int, default=2000)
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
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, meshes=[])
    for name, m in (("raw", raw), ("simplified", simple)):
        tg, _ = events_ms(lambda: mesh.triangle_grid(m), args.repeats, args.slow_ms)
        grid = mesh.triangle_grid(m)
        row = dict(name=name, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]), triangle_grid_ms=tg,
                   grid=dict(cell=grid.cell, dims=list(grid.dims), pairs=int(grid.pairs.shape[0]), faces_skipped=grid.faces_skipped))
        row["bake"] = bake_rows(m, grid, args.rays, args)
        row["raycast"] = raycast_rows(m, grid, args.casts, args, brute=name == "simplified", host=True)
        res["meshes"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
