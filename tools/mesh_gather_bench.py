"""Times ray-traced light per pixel (gi-gs_amd/mesh.py: gather_points; mesh_render.RaytracedLight) for the covered pixels of
one view of an extracted mesh, beside the per-vertex trace of the same session.

    python tools/mesh_gather_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--rays 64 256]
                                      [--sky_res 32] [--repeats 7] [--slow_ms 3000] [--spread 3]

The meshes are tools/mesh_light_bench.py's: the C2 stand-in scene fused from --fuse_views orbit views and extracted at --grid,
and its --ratio simplification; the sky is the same 256^2 cube pooled to --sky_res.  Each mesh is rasterized once at --size x
--size from the first orbit camera (mesh_render.MeshRasterizer), and its covered pixels, with the position and normal planes
of that view, are the points.  Per mesh and per --rays, by device events after three warm-up calls, the median of --repeats:
    occlusion_ms      mesh.gather_points(cube=None): the rays stop at ao_distance (the default, 0.1 of the grid's longest axis)
    light_ms          mesh.gather_points with the sky and the radiosity of one bounce: the rays run without a limit
    trace_ms          mesh.trace_hemispheres on the mesh's vertices with the same rays: the per-vertex trace
and each as rays per second (points or vertices with rays x rays / time).  --spread repeats the whole light_ms and trace_ms
measurement that many times and reports min and max of the medians: the run-to-run spread the two rates are read against.
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
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import scenes  # noqa: E402
from mesh_bake_bench import events_ms  # noqa: E402


def gather_rows(m, grid, sky, cam, args):
    dev = m.vertices.device
    rho = (m.albedo * (1.0 - m.metallic)[:, None]).contiguous()
    with mesh_render.MeshRasterizer(m, device=dev) as rast, mesh_render.RaytracedLight(m, device=dev) as prep:
        o = rast(cam)
        points, normals, mask = prep.prepare(o["pos"], o["normal"], cam["viewmatrix"], o["tri_id"] >= 0)
    rows = []
    for R in args.rays:
        hits, traced = mesh.trace_hemispheres(m, rays=R, grid=grid)
        _, radiosity, _ = mesh._gather_light(m, hits, sky, 0, rho)
        del hits
        common = dict(rays=R, bias=traced["bias"], mask=mask, grid=grid)
        _, occ = mesh.gather_points(points, normals, m, **common)
        _, lit = mesh.gather_points(points, normals, m, sky, radiosity[0], **common)
        n_rays = R * (lit["n"] - lit["masked"] - lit["no_normal"])
        v_rays = R * (traced["n"] - traced["no_normal"])
        row = dict(rays=R, pixels=lit["n"], pixels_traced=n_rays // R, occlusion=occ, light=lit, trace=traced)
        timed = dict(occlusion=lambda: mesh.gather_points(points, normals, m, **common),
                     light=lambda: mesh.gather_points(points, normals, m, sky, radiosity[0], **common),
                     trace=lambda: mesh.trace_hemispheres(m, rays=R, grid=grid))
        for name, fn in timed.items():
            ms = [events_ms(fn, args.repeats, args.slow_ms)[0] for _ in range(1 if name == "occlusion" else args.spread)]
            rays_all = v_rays if name == "trace" else n_rays
            row[name + "_ms"] = sorted(ms)[len(ms) // 2]
            row[name + "_ms_min_max"] = [min(ms), max(ms)]
            row[name + "_mrays_per_s"] = round(rays_all / (row[name + "_ms"] * 1e-3) / 1e6, 2)
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
    ap.add_argument("--sky_res", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slow_ms", type=float, default=3000.0)
    ap.add_argument("--spread", type=int, default=3)
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
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in fuse[0].items()}
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, spread=args.spread, sky_res=args.sky_res,
               meshes=[])
    for name, m in (("raw", raw), ("simplified", simple)):
        grid = mesh.triangle_grid(m)
        row = dict(name=name, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]),
                   grid=dict(cell=grid.cell, dims=list(grid.dims), pairs=int(grid.pairs.shape[0])))
        row["gather"] = gather_rows(m, grid, sky, cam, args)
        res["meshes"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
