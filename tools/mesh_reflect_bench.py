"""Times ray-traced reflections per pixel (gi-gs_amd/mesh.py: reflect_points) for the covered pixels of one view of an
extracted mesh, beside the diffuse gather (mesh.gather_points) at the same ray count in the same session.

    python tools/mesh_reflect_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--rays 64]
                                       [--levels 16] [--roughness 0.1 0.5 0.9] [--sky_res 32] [--reflection_sky_res 128]
                                       [--repeats 7] [--slow_ms 3000]

The meshes, the view and the points are tools/mesh_gather_bench.py's: the C2 stand-in scene fused from --fuse_views orbit views
and extracted at --grid, and its --ratio simplification, rasterized once at --size x --size from the first orbit camera; the
views are mesh_render.prepare_views of that camera.  Per mesh and per --rays, by device events after three warm-up calls, the
median of --repeats:
    gather_ms         mesh.gather_points with the sky (--sky_res) and the radiosity of one bounce: the diffuse final gather
    reflect_ms        mesh.reflect_points with the sky pooled to --reflection_sky_res and the same radiosity, every pixel at
                      one --roughness; a row per value
    visibility_ms     the same without a cube: specular occlusion alone
and each as rays per second (the rays actually CAST: a reflection ray below the horizon is not).  A timed call whose first
warm-up takes more than --slow_ms is timed with three repeats.
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


def reflect_rows(m, grid, sky, glossy_sky, cam, args):
    dev = m.vertices.device
    rho = (m.albedo * (1.0 - m.metallic)[:, None]).contiguous()
    with mesh_render.MeshRasterizer(m, device=dev) as rast, mesh_render.RaytracedLight(m, device=dev) as prep:
        o = rast(cam)
        points, normals, mask = prep.prepare(o["pos"], o["normal"], cam["viewmatrix"], o["tri_id"] >= 0)
    views = mesh_render.prepare_views(points, cam["campos"])
    rows = []
    for R in args.rays:
        hits, traced = mesh.trace_hemispheres(m, rays=R, grid=grid)
        _, radiosity, _ = mesh._gather_light(m, hits, sky, 0, rho)
        del hits
        common = dict(rays=R, bias=traced["bias"], mask=mask, grid=grid)
        _, lit = mesh.gather_points(points, normals, m, sky, radiosity[0], **common)
        ms = events_ms(lambda: mesh.gather_points(points, normals, m, sky, radiosity[0], **common), args.repeats, args.slow_ms)[0]
        n_rays = R * (lit["n"] - lit["masked"] - lit["no_normal"])
        row = dict(rays=R, levels=args.levels, pixels=lit["n"], pixels_traced=n_rays // R, gather_ms=ms,
                   gather_mrays_per_s=round(n_rays / (ms * 1e-3) / 1e6, 2), reflect=[])
        table = mesh.ggx_directions(R, 16, args.levels)
        for r in args.roughness:
            rough = torch.full((int(points.shape[0]),), float(r), dtype=torch.float32, device=dev)
            spec = dict(directions=table, bias=traced["bias"], mask=mask, grid=grid)
            _, rep = mesh.reflect_points(points, normals, views, rough, m, glossy_sky, radiosity[0], **spec)
            cast = rep["misses"] + rep["front_hits"] + rep["back_hits"]
            one = dict(roughness=r, report=rep, rays_cast=cast)
            for name, fn in (("reflect", lambda: mesh.reflect_points(points, normals, views, rough, m, glossy_sky, radiosity[0], **spec)),
                             ("visibility", lambda: mesh.reflect_points(points, normals, views, rough, m, **spec))):
                ms = events_ms(fn, args.repeats, args.slow_ms)[0]
                one[name + "_ms"] = ms
                one[name + "_mrays_per_s"] = round(cast / (ms * 1e-3) / 1e6, 2)
            row["reflect"].append(one)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--rays", type=int, nargs="+", default=[64])
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--roughness", type=float, nargs="+", default=[0.1, 0.5, 0.9])
    ap.add_argument("--sky_res", type=int, default=32)
    ap.add_argument("--reflection_sky_res", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
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
    base = relight.latlong_to_cubemap(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(dev), [256, 256])
    sky, glossy_sky = mesh.sky_cube(base, args.sky_res), mesh.sky_cube(base, args.reflection_sky_res)
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in fuse[0].items()}
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, sky_res=args.sky_res,
               reflection_sky_res=args.reflection_sky_res, meshes=[])
    for name, m in (("raw", raw), ("simplified", simple)):
        grid = mesh.triangle_grid(m)
        row = dict(name=name, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]),
                   grid=dict(cell=grid.cell, dims=list(grid.dims), pairs=int(grid.pairs.shape[0])))
        row["reflect"] = reflect_rows(m, grid, sky, glossy_sky, cam, args)
        res["meshes"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
