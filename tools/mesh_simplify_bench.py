"""Times simplifying an extracted mesh (gi-gs_amd/mesh.py: simplify) beside its numpy restatement on the host, and compares
the renders of the raw and the simplified meshes with the splat render.

    python tools/mesh_simplify_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--views 8]
                                        [--ratios 2 3] [--repeats 15]

The mesh is tools/mesh_render_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit
views and extracted at --grid.  Per ratio R (cell = R voxels from the volume's corner, as extract_mesh.py --simplify R):
    sizes             vertices, faces, clusters before and after, mesh.simplify's report
    simplify          mesh.simplify by device events, after three warm-up calls, the median of --repeats
    launches          each native launch of the call issued alone through the C ABI on mesh.simplify's own intermediate
                      arrays, by device events (cluster_keys, cluster_faces, cluster_solve, face_dedupe, mark, compact);
                      simplify minus their sum is the sorts, scans, read-backs and the torch calls around them
    host              the numpy restatement (tests/mesh_simplify_ref.py) on arrays already on the host (wall clock)
    compare           render_mesh.py --compare's albedo PSNR / SSIM and mean |depth difference| over the pixels both cover,
                      mesh G-buffer (mesh_render.MeshRasterizer) against the Gaussians' (pipeline.rasterize, inference),
                      averaged over --views orbit views, for the raw mesh and each simplified one
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
import evaluate  # noqa: E402
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import mesh_render  # noqa: E402
import mesh_simplify_ref  # noqa: E402
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


def launches_ms(m, cell, origin, repeats):
    """The native launches of mesh.simplify one by one, on the arrays the call itself makes."""
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    cl = mesh._cluster(m, cell, origin)
    Cn = cl.n
    org = (C.c_float * 3)(*(float(x) for x in cl.origin))
    keys = torch.empty(V, **i64)
    triples, pairs, counts = torch.empty((F, 3), **i32), torch.empty(3 * F, **i64), torch.empty(2, **i32)
    out = {}
    out["cluster_keys"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_cluster_keys(
        V, p(m.vertices), org, float(cl.inv), p(keys), s), "keys"), repeats)
    faces_call = lambda: gigs_lib.check(lib.gigs_mesh_cluster_faces(  # noqa: E731
        V, F, Cn, p(m.faces), p(cl.cluster_of), p(triples), p(pairs), p(counts), s), "faces")
    out["cluster_faces"] = events_ms(faces_call, repeats)
    spairs = torch.sort(pairs).values
    pair_start = torch.searchsorted(spairs, torch.arange(Cn + 1, **i64) << 32)
    cv = mesh._sized(dev, Cn, 0)
    flags = torch.zeros(2, **i32)
    out["cluster_solve"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_cluster_solve(
        V, F, Cn, p(m.vertices), p(m.normals), p(m.albedo), p(m.roughness), p(m.metallic), p(m.faces), p(cl.order),
        p(cl.member_start), p(spairs), p(pair_start), p(cl.keys), org, float(np.float32(cell)), 1e-3, p(cv.vertices),
        p(cv.normals), p(cv.albedo), p(cv.roughness), p(cv.metallic), p(flags), s), "solve"), repeats)
    t = triples.long()
    by_last = torch.sort(t[:, 2], stable=True).indices
    order = by_last[torch.sort(((t[:, 0] << 32) | t[:, 1])[by_last], stable=True).indices]
    faces = torch.empty((F, 3), **i32)
    out["face_dedupe"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_face_dedupe(
        F, p(triples), p(order), p(faces), p(flags[1:]), p(flags), s), "dedupe"), repeats)
    face_keep, vertex_keep = torch.empty(F, **i32), torch.empty(Cn, **i32)
    label, root_keep = torch.zeros(F, **i32), torch.ones(Cn, dtype=torch.uint8, device=dev)
    out["mark"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_mark(
        Cn, F, p(faces), p(label), p(root_keep), p(face_keep), p(vertex_keep), s), "mark"), repeats)
    v_incl, f_incl = torch.cumsum(vertex_keep, 0, dtype=torch.int32), torch.cumsum(face_keep, 0, dtype=torch.int32)
    V2, F2 = int(v_incl[-1]), int(f_incl[-1])
    v_off, f_off = v_incl - vertex_keep, f_incl - face_keep
    o = mesh._sized(dev, V2, F2)
    flag = torch.zeros(1, **i32)
    out["compact"] = events_ms(lambda: gigs_lib.check(lib.gigs_mesh_compact(
        Cn, F, p(cv.vertices), p(cv.normals), p(cv.albedo), p(cv.roughness), p(cv.metallic), p(faces), p(vertex_keep), p(v_off),
        p(face_keep), p(f_off), V2, F2, p(o.vertices), p(o.normals), p(o.albedo), p(o.roughness), p(o.metallic), p(o.faces),
        p(flag), s), "compact"), repeats)
    assert int(flags[0]) == 0 and int(flag) == 0
    return {k: round(v, 4) for k, v in out.items()}, o


def compare(m, g, cams, gi):
    """render_mesh.py --compare's albedo and depth figures, averaged over `cams`."""
    bg = torch.zeros(3, device=m.vertices.device)
    psnr, ssim, depth = [], [], []
    with mesh_render.MeshRasterizer(m, device=m.vertices.device) as rast, torch.no_grad():
        for c in cams:
            o = rast(c)
            s = pipeline.rasterize(c, g, 2, bg, gi, inference=True)[0]
            rec = evaluate.image_metrics(o["albedo"], s[7]).cpu()
            both = (o["tri_id"] >= 0) & (s[3][0] > 0)
            depth.append(float(((o["depth"][0] - s[3][0]).abs() * both).sum() / both.sum().clamp(min=1)))
            psnr.append(float(rec[3]))
            ssim.append(float(rec[4]))
    return dict(albedo_psnr=round(statistics.mean(psnr), 3), albedo_ssim=round(statistics.mean(ssim), 4),
                depth_abs_diff=round(statistics.mean(depth), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--ratios", type=float, nargs="+", default=[2.0, 3.0])
    ap.add_argument("--repeats", type=int, default=15)
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
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    cams = []
    for i in range(args.views):
        c = scenes.orbit_camera(i, args.views, W, H, radius=3.5, elevation=0.6)
        cams.append({k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()})
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    res = dict(grid=args.grid, size=args.size, P=args.P, vertices=V, faces=F, voxel=voxel, repeats=args.repeats, views=args.views,
               raw_compare=compare(m, g, cams, gi), ratios=[])
    host = {k: t.cpu().numpy() for k, t in zip(mesh.Mesh._fields, m)}
    for R in args.ratios:
        cell = R * voxel
        out, report = mesh.simplify(m, cell, origin=origin)
        row = dict(ratio=R, report=report)
        row["simplify_ms"] = round(events_ms(lambda: mesh.simplify(m, cell, origin=origin), args.repeats), 4)
        row["launches_ms"], replay = launches_ms(m, cell, origin, args.repeats)
        row["launches_sum_ms"] = round(sum(row["launches_ms"].values()), 4)
        row["replay_equal"] = bool(all(torch.equal(a, b) for a, b in zip(replay, out)))
        times = []
        for i in range(3):
            t0 = time.perf_counter()
            ref, ref_report, _ = mesh_simplify_ref.simplify(host, cell, origin)
            if i >= 1:
                times.append((time.perf_counter() - t0) * 1e3)
        row["host_ms"] = round(statistics.median(times), 2)
        got = {k: t.cpu().numpy() for k, t in zip(mesh.Mesh._fields, out)}
        row["host_faces_equal"] = bool(np.array_equal(got["faces"], ref["faces"]))
        row["host_report_equal"] = bool(all(report[k] == ref_report[k] for k in mesh_simplify_ref.REPORT_KEYS))
        tol = mesh_simplify_ref.position_tolerance(ref["vertices"], cell)
        row["position_diff_of_tolerance"] = float((np.abs(got["vertices"].astype(np.float64) - ref["vertices"]) / tol).max())
        row["normal_diff_of_tolerance"] = float(np.abs(got["normals"].astype(np.float64) - ref["normals"]).max()
                                                / mesh_simplify_ref.NORMAL_TOLERANCE)
        row["attributes_bit_equal"] = bool(all(np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32))
                                               for k in ("albedo", "roughness", "metallic")))
        row["compare"] = compare(out, g, cams, gi)
        res["ratios"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
