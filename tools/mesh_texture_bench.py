"""Times the textured resolve (gi-gs_amd/mesh_render.py: TexturedMeshRasterizer, gigs_mesh_resolve_textured) beside the
per-vertex one on the same key plane, and records what a textured light mesh looks like against the heavy mesh it was baked
from: render_mesh.py's mesh_vs_mesh figures.

    python tools/mesh_texture_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--ratios 2 4] [--block 8]
                                       [--repeats 15] [--views 8] [--ao_rays 64]

The meshes are tools/mesh_atlas_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit views
and extracted at --grid (the heavy mesh, occlusion by mesh.bake_occlusion), and per --ratios its simplification with cells
of that many voxels (the light mesh) with an atlas of --block texels a chart (mesh.bake_atlas).  Per ratio, at --size squared,
by device events after three warm-up calls, the median of --repeats, on one orbit view:
    resolve               gigs_mesh_resolve on the light mesh's per-vertex tables: the launch alone, on planes allocated once
    resolve_textured      gigs_mesh_resolve_textured on the same key plane and the atlas's float planes, likewise
    *_batch               the same launch 20 times back to back between one pair of events, per launch: what the kernel
                          costs once the launches overlap
    *_call_ms, *_host_us  MeshRasterizer.resolve / TexturedMeshRasterizer.resolve as called (ten allocations and the launch):
                          by events, and the host's time for the call by the wall clock without a synchronisation
    render, render_textured   the complete project + clear + raster + resolve of a view
and over --views orbit views, against the heavy mesh relit by the same MeshRelighter, render_mesh.mesh_vs_mesh of the light
mesh textured from the float atlas, from the 8-bit PNGs texture_mesh.py writes (read back by load_textured_mesh) and from its
own per-vertex attributes (SSAO throughout: the comparison is of materials).  These are times of this tool's calls; no
hardware rate is derived from them.
"""
import argparse
import json
import os
import statistics
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
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import pipeline  # noqa: E402
import relight  # noqa: E402
import render_mesh  # noqa: E402
import scenes  # noqa: E402
import texture_mesh  # noqa: E402

BATCH = 20


def events_ms(fn, repeats, warmup=3, batch=1):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(batch):
            fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1) / batch)
    return round(statistics.median(times), 5)


def host_us(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    return round(statistics.median(times), 2)


def launches(plain, textured, cam, W, H):
    """The two C-ABI calls alone, on planes allocated once and the key plane `plain` has just rastered."""
    dev = plain.device
    lib, s = gigs_lib.lib(), torch.cuda.current_stream().cuda_stream
    vm = plain._viewmatrix(cam, dev)
    out = {k: torch.empty((c, H, W), dtype=torch.float32, device=dev) for k, c in mesh_render.TEXTURED_PLANES.items()}
    tri_id = torch.empty((H, W), dtype=torch.int32, device=dev)
    vis, m, t = plain._vis, plain._mesh, textured._mesh
    Wt, Ht = textured.texture_size

    def resolve():
        gigs_lib.check(lib.gigs_mesh_resolve(
            plain.V, plain.F, m["faces"].data_ptr(), plain._view_pos.data_ptr(), plain._screen.data_ptr(), plain._flags.data_ptr(),
            m["normals"].data_ptr(), m["albedo"].data_ptr(), m["roughness"].data_ptr(), m["metallic"].data_ptr(), vm.data_ptr(), W, H,
            vis.data_ptr(), *(out[k].data_ptr() for k in mesh_render.PLANES), tri_id.data_ptr(), s), "mesh_resolve")

    def resolve_textured():
        gigs_lib.check(lib.gigs_mesh_resolve_textured(
            plain.V, plain.F, m["faces"].data_ptr(), plain._view_pos.data_ptr(), plain._screen.data_ptr(), plain._flags.data_ptr(),
            t["uvs"].data_ptr(), None, Wt, Ht, t["tex_albedo"].data_ptr(), t["tex_orm"].data_ptr(), t["tex_normal"].data_ptr(),
            vm.data_ptr(), W, H, vis.data_ptr(), *(out[k].data_ptr() for k in mesh_render.TEXTURED_PLANES), tri_id.data_ptr(), s),
            "mesh_resolve_textured")

    return resolve, resolve_textured


def compare(rast, heavy, light, gi, cams, vds):
    """render_mesh.mesh_vs_mesh of `rast` against the heavy mesh, averaged over the views."""
    rl, ref = mesh_render.MeshRelighter(light, gi), mesh_render.MeshRelighter(light, gi)
    rows = []
    for c in cams:
        v = render_mesh.mesh_vs_mesh(rl(c, rast, vds[id(c)]), ref(c, heavy, vds[id(c)]))
        rows.append({k: float(v[k]) for k in render_mesh.MESH_VS_MESH_KEYS} | {"relit_psnr": float(v["relit_psnr"][0])})
    return {k: round(sum(r[k] for r in rows) / len(rows), 4) for k in rows[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--ratios", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--block", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--ao_rays", type=int, default=64)
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
    raw = vol.extract(2)
    origin = vol.lo
    del vol, g
    pipeline._collect_idle()
    grid = mesh.triangle_grid(raw)
    occlusion, _ = mesh.bake_occlusion(raw, rays=args.ao_rays, grid=grid)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cams = []
    for i in range(args.views):
        c = scenes.orbit_camera(i, args.views, W, H, radius=3.5, elevation=0.6)
        cams.append({k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    rays = pipeline.canonical_rays(cams[0], dev)
    vds = {id(c): pipeline.view_dirs_for(c, rays, dev) for c in cams}
    light = relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1)), res=256)
    heavy = mesh_render.MeshRasterizer(raw, device=dev)
    res = dict(grid=args.grid, size=args.size, P=args.P, voxel=voxel, repeats=args.repeats, block=args.block, views=args.views,
               source=dict(vertices=heavy.V, faces=heavy.F), targets=[])
    cam = cams[0]
    with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
        for ratio in args.ratios:
            simple, _ = mesh.simplify(raw, ratio * voxel, origin=origin)
            atlas, report = mesh.bake_atlas(simple, raw, block=args.block, occlusion=occlusion, grid=grid)
            plain = mesh_render.MeshRasterizer(simple, device=dev)
            textured = mesh_render.TexturedMeshRasterizer.from_atlas(simple, atlas)
            obj = os.path.join(tmp, "light_%g.obj" % ratio)
            texture_mesh.save_textured_mesh(obj, simple, atlas)
            from_png = mesh_render.TexturedMeshRasterizer(**mesh_render.load_textured_mesh(obj), device=dev)
            row = dict(ratio=ratio, vertices=plain.V, faces=plain.F, atlas=[atlas.layout.width, atlas.layout.height],
                       covered_share=round(float((plain(cam)["tri_id"] >= 0).float().mean()), 4))
            plain.project(cam)
            plain.raster(W, H)
            resolve, resolve_textured = launches(plain, textured, cam, W, H)
            row["resolve_ms"] = events_ms(resolve, args.repeats)
            row["resolve_textured_ms"] = events_ms(resolve_textured, args.repeats)
            row["resolve_batch_ms"] = events_ms(resolve, args.repeats, batch=BATCH)
            row["resolve_textured_batch_ms"] = events_ms(resolve_textured, args.repeats, batch=BATCH)
            textured.project(cam)
            textured.raster(W, H)
            row["resolve_call_ms"] = events_ms(lambda: plain.resolve(cam), args.repeats)
            row["resolve_textured_call_ms"] = events_ms(lambda: textured.resolve(cam), args.repeats)
            row["resolve_host_us"] = host_us(lambda: plain.resolve(cam), args.repeats)
            row["resolve_textured_host_us"] = host_us(lambda: textured.resolve(cam), args.repeats)
            row["render_ms"] = events_ms(lambda: plain(cam), args.repeats)
            row["render_textured_ms"] = events_ms(lambda: textured(cam), args.repeats)
            row["render_host_us"] = host_us(lambda: plain(cam), args.repeats)
            row["render_textured_host_us"] = host_us(lambda: textured(cam), args.repeats)
            row["mesh_vs_mesh"] = dict(textured=compare(textured, heavy, light, gi, cams, vds),
                                       vertices=compare(plain, heavy, light, gi, cams, vds),
                                       textured_png=compare(from_png, heavy, light, gi, cams, vds))
            res["targets"].append(row)
            print(json.dumps(row), flush=True)
            for r in (plain, textured, from_png):
                r.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
