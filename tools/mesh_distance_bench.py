"""Times comparing an extracted mesh with its simplifications (gi-gs_amd/mesh.py: distance) and records what the comparison
says about them.

    python tools/mesh_distance_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratios 2 3]
                                        [--samples 100000 1000000] [--repeats 15] [--host_queries 2000]

The mesh is tools/mesh_simplify_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit
views and extracted at --grid.  Per ratio R (cell = R voxels from the volume's corner, as extract_mesh.py --simplify R) and
per sample count N:
    report            mesh.distance(raw, simplified, N): Chamfer, Hausdorff, the one-sided statistics, both grids
    distance          that call by device events, after three warm-up calls, the median of --repeats
    launches          each native launch of one direction (raw samples against the simplified mesh, and the reverse) issued
                      alone through the C ABI on the call's own intermediate arrays, by device events: face_areas,
                      sample_surface, grid_count, grid_pairs, closest; distance minus their sum over both directions is the
                      sorts, scans, reductions, read-backs and the torch calls around them
    brute             gigs_mesh_closest on a one-cell grid (every face for every query: the GPU's own brute force), N =
                      the smallest --samples only, once, with the largest difference to the grid search (expected 0)
    host              the numpy restatement (tests/mesh_distance_ref.py) on --host_queries of the same samples, grid
                      construction apart (wall clock), and whether its faces and distances agree
"""
import argparse
import ctypes as C
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
import mesh_distance_ref  # noqa: E402
import pipeline  # noqa: E402
import scenes  # noqa: E402


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
    return statistics.median(times)


def launches_ms(src, dst, n, seed, repeats):
    """The native launches of one direction of mesh.distance one by one, on the arrays the call itself makes."""
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    dev = src.vertices.device
    p = lambda t: t.data_ptr()  # noqa: E731
    out = {}
    Vs, Fs = int(src.vertices.shape[0]), int(src.faces.shape[0])
    Vd, Fd = int(dst.vertices.shape[0]), int(dst.faces.shape[0])
    areas, skipped = torch.empty(Fs, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    out["face_areas"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_face_areas(
        Vs, Fs, p(src.vertices), p(src.faces), p(areas), p(skipped), s), "areas"), repeats)
    cum = torch.cumsum(areas, 0)
    pts, face, bary = (torch.empty((n, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                       torch.empty((n, 2), device=dev))
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out["sample_surface"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_sample_surface(
        Vs, Fs, p(src.vertices), p(src.faces), p(cum), n, seed, p(pts), p(face), p(bary), p(flag), s), "sample"), repeats)
    grid = mesh.triangle_grid(dst)
    c_lo, c_dims = mesh._c_grid(grid.lo, grid.dims)
    d_areas = mesh._face_areas(dst).areas
    counts = torch.empty(Fd, dtype=torch.int32, device=dev)
    out["grid_count"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_grid_count(
        Vd, Fd, p(dst.vertices), p(dst.faces), p(d_areas), c_lo, grid.cell, c_dims, p(counts), s), "count"), repeats)
    offsets = torch.cumsum(counts, 0, dtype=torch.int64) - counts
    total = int(grid.pairs.shape[0])
    pairs = torch.empty(total, dtype=torch.int64, device=dev)
    out["grid_pairs"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_grid_pairs(
        Vd, Fd, p(dst.vertices), p(dst.faces), p(d_areas), c_lo, grid.cell, c_dims, p(offsets), total, p(pairs), p(flag), s),
        "pairs"), repeats)
    lo = torch.from_numpy(grid.lo.astype(np.float64)).to(dev)
    G = torch.tensor(grid.dims, dtype=torch.float64, device=dev)
    c = ((pts.double() - lo) / grid.cell).floor().clamp_(min=0).minimum(G - 1).long()
    order = torch.sort((c[:, 2] * grid.dims[1] + c[:, 1]) * grid.dims[0] + c[:, 0]).indices
    dist, cf, cnt = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)

    def closest(g, order_ptr):
        lo_, dims_ = mesh._c_grid(g.lo, g.dims)
        gigs_lib.check(lib.gigs_mesh_closest(Vd, Fd, p(dst.vertices), p(dst.faces), lo_, g.cell, dims_, p(g.cell_start), p(g.pairs),
                                             int(g.pairs.shape[0]), n, p(pts), order_ptr, float("inf"), p(dist), p(cf), p(cnt),
                                             p(flag), s), "closest")

    out["closest"] = events_ms(lambda: closest(grid, p(order)), repeats)
    out["closest_unsorted"] = events_ms(lambda: closest(grid, None), repeats)
    assert int(flag) == 0
    info = dict(cell=grid.cell, dims=list(grid.dims), pairs=total, cells=int(grid.cell_start.shape[0]) - 1)
    return {k: round(v, 4) for k, v in out.items()}, info, (pts, dist.clone(), cf.clone(), grid, closest)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratios", type=float, nargs="+", default=[2.0, 3.0])
    ap.add_argument("--samples", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--host_queries", type=int, default=2000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = H = args.size
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
    origin = vol.lo
    del vol
    pipeline._collect_idle()
    res = dict(grid=args.grid, size=args.size, P=args.P, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]),
               voxel=voxel, repeats=args.repeats, median_edge=mesh.median_edge(m), ratios=[])
    for R in args.ratios:
        simple, srep = mesh.simplify(m, R * voxel, origin=origin)
        row = dict(ratio=R, cell=R * voxel, vertices=srep["vertices"], faces=srep["faces"], runs=[])
        for k, n in enumerate(sorted(args.samples)):
            run = dict(samples=n, report=mesh.distance(m, simple, samples=n))
            run["distance_ms"] = round(events_ms(lambda: mesh.distance(m, simple, samples=n), args.repeats), 4)
            total = 0.0
            for name, src, dst in (("raw_to_simple", m, simple), ("simple_to_raw", simple, m)):
                ms, info, (pts, dist, face, grid, closest) = launches_ms(src, dst, n, 0, args.repeats)
                run[name] = dict(launches_ms=ms, grid=info)
                total += sum(v for key, v in ms.items() if key != "closest_unsorted")
                if k == 0:
                    one = mesh.triangle_grid(dst, cell=1e6 * grid.cell)
                    assert one.dims == (1, 1, 1)
                    d1, f1, _ = mesh.closest_point(pts, dst, grid=one)  # also the warm-up
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    d1, f1, _ = mesh.closest_point(pts, dst, grid=one)
                    t1.record()
                    torch.cuda.synchronize()
                    run[name]["brute_ms"] = round(t0.elapsed_time(t1), 3)
                    run[name]["brute_equal"] = bool(torch.equal(d1, dist) and torch.equal(f1, face))
                    hq = min(args.host_queries, n)
                    hp = pts[:hq].cpu().numpy()
                    hv, hf = dst.vertices.cpu().numpy(), dst.faces.cpu().numpy()
                    t0 = time.perf_counter()
                    hg = mesh_distance_ref.build_grid(hv, hf)
                    tg = time.perf_counter()
                    want = mesh_distance_ref.closest(hp, hv, hf, grid=hg)
                    run[name]["host"] = dict(queries=hq, grid_s=round(tg - t0, 2), closest_ms=round((time.perf_counter() - tg) * 1e3, 1),
                                             faces_equal=bool(np.array_equal(face[:hq].cpu().numpy(), want["face"])),
                                             distance_bits_equal=bool(np.array_equal(dist[:hq].cpu().numpy().view(np.uint32),
                                                                                     want["distance"].view(np.uint32))),
                                             open_ties=int(want["tie"].sum()), tests_per_query=round(want["tests"] / hq, 1),
                                             shells=want["shells"])
            run["launches_sum_ms"] = round(total, 4)
            row["runs"].append(run)
        res["ratios"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
