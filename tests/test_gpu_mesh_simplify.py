"""GPU: mesh simplification (csrc/mesh_simplify.hip through mesh.cluster_map / mesh.simplify, simplify_mesh.py,
extract_mesh.py --simplify) against its numpy restatement (tests/mesh_simplify_ref.py).  cluster_of, C, the faces, the
report and the mean attributes (as bit patterns) are compared by array_equal; positions within 2^-22 max(|coordinate|, cell)
and normals within 2^-22 per component: the float64 solve is conditioned at most 3 / reg + 1, so what separates two
implementations is a float64 sqrt that need not be correctly rounded and one float32 rounding that may fall either way."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as cr
import mesh_simplify_ref as sr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FLOAT_KEYS = ("vertices", "normals", "albedo", "roughness", "metallic")


def _to_mesh(d):
    import mesh
    return mesh.Mesh(*(torch.from_numpy(np.ascontiguousarray(d[k])).to(DEV) for k in mesh.Mesh._fields))


def _to_dict(m):
    import mesh
    return {k: t.cpu().numpy() for k, t in zip(mesh.Mesh._fields, m)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _close(got, want, cell, what):
    """Positions, normals within their tolerances; the mean attributes bit for bit.  got, want: dicts of arrays."""
    for k in FLOAT_KEYS:
        assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (what, k)
    for k in ("albedo", "roughness", "metallic"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (what, k)
    if len(want["vertices"]) == 0:
        return
    dp = np.abs(got["vertices"].astype(np.float64) - want["vertices"]) / sr.position_tolerance(want["vertices"], cell)
    dn = np.abs(got["normals"].astype(np.float64) - want["normals"]) / sr.NORMAL_TOLERANCE
    print("%s: largest position difference %.3f of its tolerance, normal %.3f (2^-22 = 1)" % (what, dp.max(), dn.max()))
    assert dp.max() <= 1.0, (what, "positions")
    assert dn.max() <= 1.0, (what, "normals")


def _check(d, cell, origin, what):
    import mesh
    m = _to_mesh(d)
    want, want_report, det = sr.simplify(d, cell, origin)
    cluster_of, n = mesh.cluster_map(m, cell, origin)
    assert cluster_of.dtype == torch.int32 and cluster_of.device == m.vertices.device and isinstance(n, int)
    cm = sr.cluster_map(d["vertices"], cell, origin) if len(d["vertices"]) else dict(C=0, cluster_of=np.zeros(0, np.int32))
    assert n == cm["C"] and np.array_equal(cluster_of.cpu().numpy(), cm["cluster_of"])
    if len(d["faces"]) and len(d["vertices"]):
        assert n == det["C"] and np.array_equal(cm["cluster_of"], det["cluster_of"])
    out, report = mesh.simplify(m, cell, origin)
    assert sorted(report) == sorted(sr.REPORT_KEYS) and json.loads(json.dumps(report)) == report
    for k in sr.REPORT_KEYS:
        assert report[k] == want_report[k], (what, k, report[k], want_report[k])
    g = _to_dict(out)
    V2, F2 = len(want["vertices"]), len(want["faces"])
    assert out.faces.dtype == torch.int32 and tuple(out.faces.shape) == (F2, 3) and tuple(out.vertices.shape) == (V2, 3)
    assert tuple(out.roughness.shape) == (V2,) and tuple(out.metallic.shape) == (V2,)
    assert np.array_equal(g["faces"], want["faces"])
    _close(g, want, cell, what)
    again, report2 = mesh.simplify(m, cell, origin)  # two calls, the same bits
    assert report2 == report and np.array_equal(again.faces.cpu().numpy(), g["faces"])
    for k, t in zip(FLOAT_KEYS, (again.vertices, again.normals, again.albedo, again.roughness, again.metallic)):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(g[k])), (what, k)
    return out, report, det


@functools.lru_cache(maxsize=None)
def _blob():
    """(the extracted blob mesh on the device, the same as a dict of arrays, h).  Read-only for the tests."""
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    return m, _to_dict(m), h


@pytest.mark.parametrize("name", ["cube", "plane", "identity", "debris", "sheets", "fan", "strip"])
def test_simplify_equals_the_restatement(name):
    d, cell, origin = sr.shared_cases()[name]
    out, report, det = _check(d, cell, origin, name)
    if name == "debris":
        assert report["faces_invalid"] == 3 and report["vertices_unclustered"] == 1
        _check(d, cell, (-0.6, -0.6, -0.6), "debris from an origin inside it")
    if name == "sheets":
        assert report["faces_duplicate"] == 8 and report["faces"] == 16
    if name == "fan":
        assert int(det["count"].max()) == 301
    if name == "strip":
        assert report["vertices_in"] == 8194 and report["clusters"] > 256
    if name == "identity":
        assert report["clusters"] == report["vertices_in"] == 98 and report["faces"] == 192


def test_clean_of_a_simplified_mesh_changes_nothing():
    """simplify() and clean() end in one compaction (mesh._compact): what it left has no invalid face and no vertex without
    a face, so clean(.., 0, 0) of it -- the labelling, then the same tail -- returns it bit for bit, for every shared case."""
    import mesh
    cases = sr.shared_cases()
    assert sorted(cases) == sorted(["cube", "plane", "identity", "debris", "sheets", "fan", "strip"])
    for name, (d, cell, origin) in cases.items():
        simple = mesh.simplify(_to_mesh(d), cell, origin)[0]
        again, report = mesh.clean(simple, 0, 0)
        assert (report["faces_removed"], report["vertices_removed"], report["invalid_faces"]) == (0, 0, 0), name
        want, got = _to_dict(simple), _to_dict(again)
        assert got["faces"].dtype == np.int32 and np.array_equal(got["faces"], want["faces"]), name
        for k in FLOAT_KEYS:
            assert got[k].dtype == np.float32 and got[k].shape == want[k].shape, (name, k)
            assert np.array_equal(_bits(got[k]), _bits(want[k])), (name, k)


@pytest.mark.parametrize("ratio,clusters,faces,vertices", [(2, 195, 376, 193), (3, 89, 166, 86)])
def test_blob_mesh(ratio, clusters, faces, vertices):
    m, d, h = _blob()
    assert (len(d["vertices"]), len(d["faces"])) == (980, 1944)
    out, report, _ = _check(d, np.float32(ratio) * h, None, "blob at %d h" % ratio)
    assert (report["clusters"], report["faces"], report["vertices"], report["faces_duplicate"]) == (clusters, faces, vertices, 0)


def test_empty_inputs_launch_nothing():
    import mesh
    _, d, h = _blob()
    empty = {k: np.asarray(v)[:0] for k, v in d.items()}
    for case, V, F in ((empty, 0, 0), (dict(d, faces=d["faces"][:0]), 980, 0), (dict(empty, faces=d["faces"]), 0, 1944)):
        out, report, _ = _check(case, 0.1, None, "empty %d %d" % (V, F))
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and report["clusters"] == 0
        assert report["vertices_in"] == V and report["faces_in"] == F
    nowhere = dict(d, vertices=np.full_like(d["vertices"], np.nan))  # no finite vertex: no cluster
    out, report, _ = _check(nowhere, 0.1, None, "no finite vertex")
    assert report["vertices_unclustered"] == 980 and report["faces_invalid"] == 1944 and tuple(out.faces.shape) == (0, 3)
    with pytest.raises(ValueError, match="2\\^21 cells"):
        mesh.simplify(_to_mesh(d), 1e-7)


def test_invalid_faces_touch_nothing_outside_the_arrays():
    """The debris mesh with its NaN vertex, its face on an index == V and its face on -1, through the C ABI with pads of -7
    around cluster_of, the keys, the triples, the pair keys and every output."""
    import gigs_lib
    import mesh
    d, cell, origin = sr.shared_cases()["debris"]
    _, want_report, det = sr.simplify(d, cell, origin)
    m = _to_mesh(d)
    V, F, Cn = 12, 11, det["C"]
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    pad = 64

    def padded(n, dtype, fill=-7):
        t = torch.full((n + 2 * pad,), fill, dtype=dtype, device=DEV)
        return t, t[pad:pad + n]

    def untouched(t, n, fill=-7):
        return bool((t[:pad] == fill).all()) and bool((t[pad + n:] == fill).all())

    org = (C.c_float * 3)(*det["origin"].tolist())
    keys_all, keys = padded(V, torch.int64)
    gigs_lib.check(lib.gigs_mesh_cluster_keys(V, m.vertices.data_ptr(), org, float(det["inv"]), keys.data_ptr(), s), "keys")
    want_keys, _ = sr.cluster_keys(d["vertices"], det["origin"], det["inv"])
    assert untouched(keys_all, V) and np.array_equal(keys.cpu().numpy(), want_keys) and want_keys[11] == -1
    of_all, of = padded(V, torch.int32)
    of.copy_(torch.from_numpy(det["cluster_of"]))
    tri_all, tri = padded(3 * F, torch.int32)
    pairs_all, pairs = padded(3 * F, torch.int64)
    counts_all, counts = padded(2, torch.int32)
    gigs_lib.check(lib.gigs_mesh_cluster_faces(V, F, Cn, m.faces.data_ptr(), of.data_ptr(), tri.data_ptr(), pairs.data_ptr(),
                                               counts.data_ptr(), s), "faces")
    cf = sr.cluster_faces(V, d["faces"], det["cluster_of"])
    assert untouched(of_all, V) and untouched(tri_all, 3 * F) and untouched(pairs_all, 3 * F) and untouched(counts_all, 2)
    assert np.array_equal(tri.cpu().numpy().reshape(F, 3), cf["triples"])
    assert counts.tolist() == [3, want_report["faces_collapsed"]] == [want_report["faces_invalid"], want_report["faces_collapsed"]]
    got_pairs = pairs.cpu().numpy().reshape(F, 3)
    assert (got_pairs[~cf["valid"]] == 2 ** 63 - 1).all() and (got_pairs[cf["valid"], 0] >> 32 == cf["clusters"][cf["valid"], 0]).all()
    assert ((got_pairs[cf["valid"], 0] & 0xffffffff) == np.nonzero(cf["valid"])[0]).all()
    # dedupe and solve on mesh.simplify's own intermediate arrays
    t = tri.reshape(F, 3).long()
    by_last = torch.sort(t[:, 2], stable=True).indices
    order = by_last[torch.sort(((t[:, 0] << 32) | t[:, 1])[by_last], stable=True).indices]
    out_all, out_faces = padded(3 * F, torch.int32)
    flags_all, flags = padded(2, torch.int32)
    flags.zero_()
    gigs_lib.check(lib.gigs_mesh_face_dedupe(F, tri.data_ptr(), order.data_ptr(), out_faces.data_ptr(), flags[1:].data_ptr(),
                                             flags.data_ptr(), s), "dedupe")
    assert untouched(out_all, 3 * F) and untouched(flags_all, 2) and flags.tolist() == [0, want_report["faces_duplicate"]]
    assert np.array_equal(out_faces.cpu().numpy().reshape(F, 3), det["faces"])
    cl = mesh._cluster(m, cell, origin)
    assert cl.n == Cn
    spairs = torch.sort(pairs).values
    pair_start = torch.searchsorted(spairs, torch.arange(Cn + 1, dtype=torch.int64, device=DEV) << 32)
    outs = [padded(3 * Cn, torch.float32, -7.0), padded(3 * Cn, torch.float32, -7.0), padded(3 * Cn, torch.float32, -7.0),
            padded(Cn, torch.float32, -7.0), padded(Cn, torch.float32, -7.0)]
    gigs_lib.check(lib.gigs_mesh_cluster_solve(
        V, F, Cn, m.vertices.data_ptr(), m.normals.data_ptr(), m.albedo.data_ptr(), m.roughness.data_ptr(), m.metallic.data_ptr(),
        m.faces.data_ptr(), cl.order.data_ptr(), cl.member_start.data_ptr(), spairs.data_ptr(), pair_start.data_ptr(),
        cl.keys.data_ptr(), org, float(np.float32(cell)), 1e-3, *(o[1].data_ptr() for o in outs), flags.data_ptr(), s), "solve")
    assert flags.tolist()[0] == 0 and untouched(flags_all, 2)
    got = {}
    for k, (whole, inner) in zip(FLOAT_KEYS, outs):
        assert untouched(whole, inner.numel(), -7.0), k
        got[k] = inner.cpu().numpy().reshape(det[k].shape)
    _close(got, det, cell, "debris through the C ABI")
    # an offset table that points outside its arrays raises the flag and nothing is stored
    broken = cl.member_start.clone()
    broken[-1] = V + 5
    for _, inner in outs:
        inner.fill_(-7.0)
    gigs_lib.check(lib.gigs_mesh_cluster_solve(
        V, F, Cn, m.vertices.data_ptr(), m.normals.data_ptr(), m.albedo.data_ptr(), m.roughness.data_ptr(), m.metallic.data_ptr(),
        m.faces.data_ptr(), cl.order.data_ptr(), broken.data_ptr(), spairs.data_ptr(), pair_start.data_ptr(),
        cl.keys.data_ptr(), org, float(np.float32(cell)), 1e-3, *(o[1].data_ptr() for o in outs), flags.data_ptr(), s), "solve")
    assert flags.tolist()[0] == 1 and bool((outs[3][1][Cn - 1] == -7.0).all()) and bool((outs[3][1][:Cn - 1] != -7.0).all())


def test_render_of_the_simplified_mesh_stays_within_the_cell_bound_of_the_raw_silhouette():
    """The clamp keeps every representative in the cell of its members, so corresponding points of the two surfaces are at
    most sqrt(3) cell apart: a pixel that exactly one of the two renders covers lies within ceil(sqrt(3) cell f / z_min) + 1
    pixels of the boundary of the raw silhouette (f: the focal length in pixels, z_min: the nearest vertex depth)."""
    import mesh
    import mesh_render
    import scenes
    m, d, h = _blob()
    cell = float(np.float32(2) * h)
    simple, report = mesh.simplify(m, cell)
    cam = scenes.look_at_camera((0.05, 0.02, 3.0), (0.0, 0.0, 0.0), 64, 64, 0.6911, up=(0.0, 1.0, 0.0))
    z = (np.concatenate([d["vertices"], np.ones((980, 1), np.float32)], 1).astype(np.float64) @ cam["viewmatrix"].astype(np.float64))[:, 2]
    focal = 64 / (2.0 * cam["tanfovx"])
    assert z.min() > 1.0
    reach = math.ceil(math.sqrt(3.0) * cell * focal / z.min()) + 1
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    with mesh_render.MeshRasterizer(m, device=DEV) as a, mesh_render.MeshRasterizer(simple, device=DEV) as b:
        raw = a(cam)["tri_id"].cpu().numpy() >= 0
        new = b(cam)["tri_id"].cpu().numpy() >= 0
    edge = np.zeros_like(raw)  # the pixels with a 4-neighbour on the other side of the raw silhouette
    edge[:-1] |= raw[:-1] != raw[1:]
    edge[1:] |= raw[:-1] != raw[1:]
    edge[:, :-1] |= raw[:, :-1] != raw[:, 1:]
    edge[:, 1:] |= raw[:, :-1] != raw[:, 1:]
    one = np.argwhere(raw != new)
    iou = (raw & new).sum() / max(int((raw | new).sum()), 1)
    far = 0.0
    if len(one):
        far = float(np.sqrt(((one[:, None, :] - np.argwhere(edge)[None, :, :]) ** 2).sum(-1)).min(axis=1).max())
    print("raw covers %d pixels, simplified %d (%d of %d faces), IoU %.4f; %d pixels in one only, the farthest %.2f pixels from "
          "the raw boundary, allowed %d" % (raw.sum(), new.sum(), report["faces"], report["faces_in"], iou, len(one), far, reach))
    assert raw.sum() > 200 and new.sum() > 200 and edge.any()
    assert far <= reach


def test_simplify_mesh_tool_and_extract_mesh_simplify(tmp_path):
    """simplify_mesh.py on a PLY of extract_mesh.py --grid 40 (test_gpu_mesh_clean.py's set-up), and extract_mesh.py
    --simplify."""
    from argparse import Namespace

    import densify
    import extract_mesh
    import mesh
    import optim
    import relight
    import scene_io
    import scenes
    import simplify_mesh
    import synthetic_dataset
    import train_iteration as ti
    src = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=6, size=64)
    out = str(tmp_path / "run")
    os.makedirs(out)
    raw = ti.raw_from_scene(scenes.surface_scene(P=4000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [raw[k]], "lr": 0.0, "name": k} for k in raw], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, raw, densify.DensifyState(raw["xyz"].shape[0], DEV), opt, 1.0),
                             light.state_dict(), {}, 7)
    with open(os.path.join(out, "cfg_args"), "w") as f:
        f.write(str(Namespace(sh_degree=3, source_path=src, model_path=out, images="images", resolution=-1,
                              white_background=False, data_device="cuda", eval=True)))
    assert extract_mesh.parse_args(["-m", out, "--checkpoint", ck]).simplify == 0
    base = ["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test"]
    r1 = extract_mesh.extract_mesh(base + ["-o", "raw1.ply"])
    r0 = extract_mesh.extract_mesh(base + ["--simplify", "0", "-o", "raw0.ply"])
    assert open(r1["path"], "rb").read() == open(r0["path"], "rb").read()
    today = ["path", "views", "samples", "dims", "voxel", "lo", "hi", "vertices", "faces", "load_s", "cameras_s", "fuse_s",
             "extract_s", "write_s"]
    assert sorted(r1) == sorted(today) and sorted(r0) == sorted(today)
    r2 = extract_mesh.extract_mesh(base + ["--simplify", "2", "-o", "simple.ply"])
    assert sorted(r2) == sorted(today + ["clusters", "faces_collapsed", "faces_duplicate", "simplify_s"])
    assert 0 < r2["faces"] < r1["faces"] and 0 < r2["vertices"] <= r2["clusters"] < r1["vertices"] and r2["simplify_s"] >= 0
    print("extract_mesh --simplify 2: %d -> %d vertices, %d -> %d faces, %d clusters" % (
        r1["vertices"], r2["vertices"], r1["faces"], r2["faces"], r2["clusters"]))
    # cells aligned with the voxels: mesh.simplify of the raw PLY's arrays with cell = 2 voxel from the volume's lo
    raw_ply = scene_io.read_mesh_ply(r1["path"])
    cell = 2.0 * r1["voxel"]
    want, want_report, _ = sr.simplify(raw_ply, cell, r1["lo"])
    assert (r2["clusters"], r2["faces"], r2["vertices"]) == (want_report["clusters"], want_report["faces"], want_report["vertices"])

    def same(path_a, path_b):
        a, b = scene_io.read_mesh_ply(path_a), scene_io.read_mesh_ply(path_b)
        for k in cr.MESH_KEYS:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
            assert np.array_equal(a[k] if k == "faces" else _bits(a[k]), b[k] if k == "faces" else _bits(b[k])), k

    # simplify_mesh.py on the file against mesh.simplify of its arrays, both written through the PLY's 8-bit albedo
    for flags, kw in ((["--cell", repr(cell)], dict(cell=cell)), (["--cell_edges", "2.5"], None)):
        rep = simplify_mesh.simplify_mesh([r1["path"], "-o", str(tmp_path / "tool.ply")] + flags)
        assert json.loads(json.dumps(rep)) == rep and rep["faces_in"] == r1["faces"] and rep["vertices_in"] == r1["vertices"]
        c = rep["cell"]
        if kw is None:
            assert abs(c - 2.5 * mesh.median_edge(_to_mesh(raw_ply))) <= 1e-6 * c and rep["median_edge"] > 0
        direct, report = mesh.simplify(_to_mesh(raw_ply), c)
        scene_io.save_mesh_ply(str(tmp_path / "direct.ply"), *direct)
        same(rep["path"], str(tmp_path / "direct.ply"))
        for k in sr.REPORT_KEYS:
            assert rep[k] == report[k], k
        assert 0 < rep["faces"] < rep["faces_in"]
    rep = simplify_mesh.simplify_mesh([r1["path"], "-o", str(tmp_path / "tool1.ply"), "--cell", repr(cell), "--keep_largest", "1"])
    direct, _ = mesh.clean(mesh.simplify(_to_mesh(raw_ply), cell)[0], keep_largest=1)
    assert rep["components_kept"] >= 1 and rep["faces"] == int(direct.faces.shape[0]) and "clean_s" in rep
