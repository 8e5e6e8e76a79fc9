"""Times the shadows of analytic lights (gi-gs_amd/mesh.py: shadow_points) and their shade (analytic_lights.shade_lights) for
the covered pixels of one view of an extracted mesh, beside the SAME rays through the nearest-hit kernel (mesh.raycast).

    python tools/mesh_shadow_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratio 2] [--lights 1 4]
                                      [--samples 1 16] [--repeats 7] [--slow_ms 3000] [--spread 3] [--out FILE.json]

The meshes and the view are tools/mesh_gather_bench.py's: the C2 stand-in scene fused from --fuse_views orbit views and
extracted at --grid, and its --ratio simplification, rasterized once at --size x --size from the first orbit camera; the
covered pixels with the position and normal planes of that view are the points.  The lights: a point light above the scene
(radius 0.05 of its extent); with 4, a second point light beside it and two directional ones (half-angles 1 and 3 degrees).
Per mesh, per --lights L and per --samples S, by device events around the WHOLE call after three warm-up calls, the median of
--repeats:
    shadow_ms     mesh.shadow_points: the cell sort of the points, the any-hit kernel, the read-back of the counters
    raycast_ms    mesh.raycast on the rays shadow_points casts -- origin point + bias normal and direction formed in float64
                  as the kernel forms them, rounded to float32, the samples below the horizon left out -- with the same
                  t_max: one call for the point lights' rays (t_max = 1), one for the directional lights' (no limit).
                  Each call sorts its rays by entry cell and reads its counters back.  This is the only way to the answer
                  without the any-hit kernel; forming the rays is not timed.
    blocked / raycast_hits: the two answers (equal but for rays whose float32 rounding crosses an edge)
    shade_ms      analytic_lights.shade_lights with the visibility, alone
--spread repeats every measurement that many times and reports min and max of the medians: the run-to-run spread the ratio
raycast_ms / shadow_ms is read against.
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
import analytic_lights  # noqa: E402
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import pipeline  # noqa: E402
import scenes  # noqa: E402
from mesh_bake_bench import events_ms  # noqa: E402


def bench_lights(m, L):
    lo, hi = m.vertices.min(0).values.cpu().numpy().astype(np.float64), m.vertices.max(0).values.cpu().numpy().astype(np.float64)
    centre, extent = 0.5 * (lo + hi), float((hi - lo).max())
    at = lambda x, y, z: [float(c) for c in centre + np.array([x, y, z]) * extent]  # noqa: E731
    entries = [dict(kind="point", position=at(0.2, -0.1, 1.2), radius=0.05 * extent),
               dict(kind="directional", direction=[-0.3, 0.2, -1.0], angle=1.0),
               dict(kind="point", position=at(-1.0, 0.6, 0.5), radius=0.05 * extent),
               dict(kind="directional", direction=[0.5, 0.4, -0.6], angle=3.0)]
    return analytic_lights.parse_lights(entries[:L])


def shadow_rays(points, normals, mask, rows, offsets, seed, bias):
    """The rays shadow_points casts, in torch float64 rounded to float32 -> [(origins, directions, t_max)], one entry for the
    point lights and one for the directional ones."""
    dev = points.device
    K, S = offsets.shape[:2]
    n = normals.double()
    n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    good = (mask != 0) & torch.isfinite(points).all(1) & (n2 >= 1.0 - 2.0 ** -10) & (n2 <= 1.0 + 2.0 ** -10)
    q = torch.nonzero(good)[:, 0]
    with np.errstate(over="ignore"):
        k = (mesh._mix64((np.uint64(seed) << np.uint64(32)) + q.cpu().numpy().astype(np.uint64)) % np.uint64(K)).astype(np.int64)
    u = torch.from_numpy(offsets.astype(np.float64)).to(dev)[torch.from_numpy(k).to(dev)]  # [n,S,3]
    n, o = n[q], points.double()[q] + bias * n[q]
    r = torch.from_numpy(rows.astype(np.float64)).to(dev)
    groups = {0: ([], []), 1: ([], [])}
    for l in range(len(rows)):
        kind = int(rows[l, 0])
        d = (r[l, 1:4] + r[l, 4] * u) - o[:, None, :] if kind == 0 else (-r[l, 1:4]) + r[l, 4] * u
        cast = ((d[..., 0] * n[:, None, 0] + d[..., 1] * n[:, None, 1]) + d[..., 2] * n[:, None, 2]) > 0
        groups[kind][0].append(o[:, None, :].expand_as(d)[cast].float())
        groups[kind][1].append(d[cast].float())
    return [(torch.cat(oo).contiguous(), torch.cat(dd).contiguous(), 1.0 if kind == 0 else None)
            for kind, (oo, dd) in groups.items() if oo]


def shadow_rows(m, grid, cam, args):
    dev = m.vertices.device
    with mesh_render.MeshRasterizer(m, device=dev) as rast, mesh_render.RaytracedLight(m, device=dev) as prep:
        o = rast(cam)
        points, normals, mask = prep.prepare(o["pos"], o["normal"], cam["viewmatrix"], o["tri_id"] >= 0)
        albedo = o["albedo"].reshape(3, -1).t().contiguous()
        roughness, metallic = o["roughness"].reshape(-1).contiguous(), o["metallic"].reshape(-1).contiguous()
    campos = cam["campos"]
    rows = []
    for L in args.lights:
        lights = bench_lights(m, L)
        packed = analytic_lights.pack(lights)[0]
        for S in args.samples:
            common = dict(samples=S, mask=mask, grid=grid)
            vis, _, rep = mesh.shadow_points(points, normals, m, lights, **common)
            rays = shadow_rays(points, normals, mask, packed, analytic_lights.ball_offsets(S, 16), 0, rep["bias"])
            cast = lambda: [mesh.raycast(oo, dd, m, t_max=t, grid=grid)[3] for oo, dd, t in rays]  # noqa: E731
            found = cast()
            row = dict(lights=L, samples=S, pixels=rep["n"], report=rep, raycast_rays=sum(x["n"] for x in found),
                       raycast_hits=sum(x["hits"] for x in found))
            timed = dict(shadow=lambda: mesh.shadow_points(points, normals, m, lights, **common), raycast=cast,
                         shade=lambda: analytic_lights.shade_lights(points, normals, albedo, roughness, metallic, campos, lights, vis, mask))
            for name, fn in timed.items():
                ms = [events_ms(fn, args.repeats, args.slow_ms)[0] for _ in range(args.spread)]
                row[name + "_ms"] = sorted(ms)[len(ms) // 2]
                row[name + "_ms_min_max"] = [min(ms), max(ms)]
            row["shadow_mrays_per_s"] = round(rep["rays"] / (row["shadow_ms"] * 1e-3) / 1e6, 2)
            row["raycast_over_shadow"] = round(row["raycast_ms"] / row["shadow_ms"], 3)
            row["raycast_over_shadow_min_max"] = [round(row["raycast_ms_min_max"][0] / row["shadow_ms_min_max"][1], 3),
                                                  round(row["raycast_ms_min_max"][1] / row["shadow_ms_min_max"][0], 3)]
            rows.append(row)
            del rays
            print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratio", type=float, default=2.0)
    ap.add_argument("--lights", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--slow_ms", type=float, default=3000.0)
    ap.add_argument("--spread", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
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
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in fuse[0].items()}
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, spread=args.spread, meshes=[])
    for name, m in (("raw", raw), ("simplified", simple)):
        grid = mesh.triangle_grid(m)
        row = dict(name=name, vertices=int(m.vertices.shape[0]), faces=int(m.faces.shape[0]),
                   grid=dict(cell=grid.cell, dims=list(grid.dims), pairs=int(grid.pairs.shape[0])))
        row["shadows"] = shadow_rows(m, grid, cam, args)
        res["meshes"].append(row)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
