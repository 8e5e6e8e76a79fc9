"""Times cleaning an extracted mesh (gi-gs_amd/mesh.py: components, clean) beside the host route a user has without it.

    python tools/mesh_clean_bench.py [--grid 256] [--size 800] [--P 300000] [--fuse_views 64] [--repeats 15]

The mesh is tools/mesh_render_bench.py's: the C2 stand-in scene (scenes.surface_scene) fused from --fuse_views orbit
views and extracted at --grid.  By device events, after three warm-up calls, the median of --repeats:
    components        mesh.components: hook / flatten rounds with one int read back per round, the count pass, the roots
    clean             mesh.clean(keep_largest=1): the same labelling, the threshold (a device sort and its read-back), the
                      mark pass, two scans, the read-back of the sizes, the compaction
    label kernels     the same hook, flatten and count launches for the observed number of rounds issued back to back
                      through the C ABI with no read-back in between: what the labelling costs when nothing waits.
                      1 - label kernels / components is the share of `components` that is read-backs, their launch gaps
                      and the torch calls around them rather than kernels
    host              faces to the CPU, scipy.sparse.csgraph.connected_components over the face edges, numpy counts,
                      threshold and compaction, the result back on the device (wall clock with a synchronised device)
Also the rounds used and the histogram of component sizes.  Bytes the labelling needs, from the shapes: a hook pass
reads 12 B per face and at least 12 B of parents, a flatten pass reads and writes 4 B per vertex, the count pass reads
16 B and writes 4 B per face and clears 4 B per vertex: (24 F + 8 V) rounds + 20 F + 4 V.
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
sys.path.insert(0, ROOT)

import importlib  # noqa: E402

importlib.import_module("gi-gs_amd")
import gigs_lib  # noqa: E402
import mesh  # noqa: E402
import pipeline  # noqa: E402
import scenes  # noqa: E402


def label_bytes(V, F, rounds):
    return (24 * F + 8 * V) * rounds + 20 * F + 4 * V


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


def host_clean(m, keep_largest):
    """The route without this module: labels by scipy on the CPU, numpy compaction, the mesh back on the device."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    dev = m.vertices.device
    a = [t.cpu().numpy() for t in m]
    f = a[1].astype(np.int64)
    V = len(a[0])
    ok = ((f >= 0) & (f < V)).all(axis=1)
    g = f[ok]
    rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    _, lab = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
    count = np.bincount(lab[g[:, 0]], minlength=int(lab.max()) + 1 if V else 0)
    thr = mesh.keep_threshold(count[count > 0], keep_largest, 0)
    face_keep = ok.copy()
    face_keep[ok] = count[lab[g[:, 0]]] >= thr
    vertex_keep = np.zeros(V, bool)
    vertex_keep[f[face_keep].reshape(-1)] = True
    new_index = np.cumsum(vertex_keep) - 1
    out = [a[0][vertex_keep], new_index[f[face_keep]].astype(np.int32)] + [x[vertex_keep] for x in a[2:]]
    return mesh.Mesh(*(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--fuse_views", type=int, default=64)
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
    del vol, g
    pipeline._collect_idle()
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    cc = mesh.components(m)
    counts = cc.counts.cpu().numpy()
    edges = [1, 2, 10, 100, 1000, 10_000, 100_000, 1 << 31]
    hist = {"%d..%d" % (a, b - 1): int(((counts >= a) & (counts < b)).sum()) for a, b in zip(edges[:-1], edges[1:])}
    cleaned, report = mesh.clean(m, keep_largest=1)
    res = dict(grid=args.grid, size=args.size, P=args.P, vertices=V, faces=F, rounds=cc.rounds, round_cap=mesh.cc_round_cap(V),
               components=int(len(counts)), largest=int(counts.max()) if len(counts) else 0, invalid_faces=cc.invalid_faces,
               component_faces_histogram=hist, clean_report=report, vertices_kept=int(cleaned.vertices.shape[0]),
               faces_kept=int(cleaned.faces.shape[0]), label_bytes=label_bytes(V, F, cc.rounds), repeats=args.repeats)
    res["components_ms"] = round(events_ms(lambda: mesh.components(m), args.repeats), 4)
    res["clean_ms"] = round(events_ms(lambda: mesh.clean(m, keep_largest=1), args.repeats), 4)

    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    i32 = dict(dtype=torch.int32, device=dev)
    parent, face_label, count, flag = torch.empty(V, **i32), torch.empty(F, **i32), torch.empty(V, **i32), torch.zeros(2, **i32)
    ident = torch.arange(V, **i32)

    def kernels():
        parent.copy_(ident)
        for r in range(cc.rounds):
            gigs_lib.check(lib.gigs_mesh_cc_hook(V, F, m.faces.data_ptr(), parent.data_ptr(), flag.data_ptr(), s), "hook")
            if r + 1 < cc.rounds:
                gigs_lib.check(lib.gigs_mesh_cc_flatten(V, parent.data_ptr(), s), "flatten")
        gigs_lib.check(lib.gigs_mesh_cc_count(V, F, m.faces.data_ptr(), parent.data_ptr(), face_label.data_ptr(),
                                              count.data_ptr(), flag[1:].data_ptr(), s), "count")

    res["label_kernels_ms"] = round(events_ms(kernels, args.repeats), 4)
    res["label_kernels_equal"] = bool(torch.equal(parent, cc.labels) and torch.equal(face_label, cc.face_labels))
    res["readback_and_launch_share"] = round(1.0 - res["label_kernels_ms"] / res["components_ms"], 3)
    res["label_tb_per_s"] = round(res["label_bytes"] / (res["label_kernels_ms"] * 1e-3) / 1e12, 4)
    try:
        import scipy  # noqa: F401
    except ImportError:
        res["host_ms"] = None
    else:
        times = []
        for i in range(2 + min(args.repeats, 5)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = host_clean(m, 1)
            torch.cuda.synchronize()
            if i >= 2:
                times.append((time.perf_counter() - t0) * 1e3)
        res["host_ms"] = round(statistics.median(times), 3)
        res["host_equal"] = bool(all(torch.equal(a, b) for a, b in zip(ref, cleaned)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
