"""Times the mesh export (gi-gs_amd/mesh.py): TSDF integration and surface nets, and the whole route for 64 views.

    python tools/mesh_bench.py [--grids 256 512] [--size 800] [--P 300000] [--repeats 10] [--views 64] [--grid 256]
    python tools/mesh_bench.py --kernels      (the launches alone, for `rocprofv3 --kernel-trace --stats` in a run of its own)

Integration: one rendered view of the C2 stand-in scene (scenes.surface_scene) at --size, integrated into a cube of G^3
samples around the scene, 1 view and 8 views per launch, by device events over --repeats launches after a warm-up.  The
bytes the algorithm needs are computed from the volume after the launches, per launch of n views:
    hot    8 B read per sample + 8 B written per sample a view touched (tsdf, weight)
    cold   36 B read + 36 B written per sample with attributes (attr_weight + 8 attributes)
    planes 8 B (opacity, depth) per touched sample and view at most, 32 B more with attributes; the planes themselves are
           40 B per pixel and view and stay in cache, so they are counted once per launch: 40 W H n
`bytes / time` is set against the 6.3 TB/s copy rate.  Extraction: count, two scans, one read-back, write, for the fused
volume of the whole route.  The whole route: 64 orbit views rendered and fused (mesh.fuse_views), extracted, written as a
PLY: what extract_mesh.py does after loading the checkpoint.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import mesh  # noqa: E402
import pipeline  # noqa: E402
import scene_io  # noqa: E402
import scenes  # noqa: E402

COPY_RATE = 6.3e12  # bytes / s, the measured HBM copy rate


def algorithmic_bytes(vol, n_views, W, H):
    """Bytes one launch of n_views equal views needs, from the volume's state after it (see the module docstring)."""
    G = vol.n_samples
    touched = int((vol.weight > 0).sum())
    cold = int((vol.attr_weight > 0).sum())
    return 8 * G + 8 * touched + 72 * cold + 40 * W * H * n_views


def events_ms(fn, repeats):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(repeats):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--grid", type=int, default=256, help="grid of the whole route")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    W = H = args.size
    sc = scenes.surface_scene(P=args.P, sh_degree=2, seed=0)
    g = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev) for k in pipeline.RASTER_KEYS}
    bg = torch.zeros(3, device=dev)
    cams = [scenes.orbit_camera(i, 8, W, H, radius=3.5) for i in range(8)]
    with torch.no_grad():
        planes = [mesh.view_planes(pipeline.rasterize(c, g, 2, bg, scenes.GI_DEFAULTS, inference=True)[0]) for c in cams]
    res = dict(size=args.size, P=args.P, repeats=args.repeats, integrate=[])
    for G in args.grids:
        voxel = 3.4 / (G - 1)
        for n in (1, 8):
            vol = mesh.TSDFVolume((-1.7, -1.7, -1.7), voxel, (G, G, G), 4 * voxel, device=dev)
            run = lambda: vol.integrate(cams[:n], planes[:n])  # noqa: E731
            run()
            ms = events_ms(run, 2 if args.kernels else args.repeats)
            b = algorithmic_bytes(vol, n, W, H)
            res["integrate"].append(dict(grid=G, views_per_launch=n, ms_per_launch=round(ms, 4), ms_per_view=round(ms / n, 4),
                                         bytes_per_launch=b, tb_per_s=round(b / (ms * 1e-3) / 1e12, 3),
                                         of_copy_rate=round(b / (ms * 1e-3) / COPY_RATE, 3),
                                         hot_pair_mb=round(8 * vol.n_samples / 1e6, 1)))
            del vol
    # the whole route
    cams64 = [scenes.orbit_camera(i, args.views, W, H, radius=3.5, elevation=0.5 if i % 2 == 0 else 0.9) for i in range(args.views)]
    lo, hi = mesh.auto_bounds(g)
    voxel, dims = mesh.grid_for_bounds(lo, hi, args.grid)

    def route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vol = mesh.TSDFVolume(lo, voxel, dims, 4 * voxel, device=dev)
        mesh.fuse_views(g, 2, cams64, scenes.GI_DEFAULTS, vol)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m = vol.extract(2)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        with tempfile.TemporaryDirectory() as d:
            scene_io.save_mesh_ply(os.path.join(d, "mesh.ply"), *m)
            size = os.path.getsize(os.path.join(d, "mesh.ply"))
        t3 = time.perf_counter()
        return vol, m, dict(fuse_s=round(t1 - t0, 4), extract_s=round(t2 - t1, 4), write_s=round(t3 - t2, 4),
                            total_s=round(t3 - t0, 4), ply_bytes=size)

    route()
    vol, m, times = route()
    res["route"] = dict(times, views=args.views, dims=list(dims), samples=vol.n_samples, vertices=int(m.vertices.shape[0]),
                        faces=int(m.faces.shape[0]))
    res["extract_ms"] = round(events_ms(lambda: vol.extract(2), 2 if args.kernels else args.repeats), 4)
    # not a timing: how far the vertices lie from the scene's spheres and plane, in voxels
    v = m.vertices.cpu().numpy().astype(np.float64)
    centers = np.array([[0.0, 0.0, 0.0], [0.9, 0.5, -0.3], [-0.8, -0.6, -0.35], [0.1, -1.0, -0.45]])
    radii = np.array([0.6, 0.35, 0.3, 0.2])
    dist = np.abs(np.linalg.norm(v[:, None, :] - centers[None], axis=2) - radii[None]).min(axis=1)
    dist = np.minimum(dist, np.abs(v[:, 2] + 0.65))
    res["route"]["median_distance_h"] = round(float(np.median(dist)) / voxel, 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
