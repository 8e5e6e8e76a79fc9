"""GPU: mesh cleaning (csrc/mesh_clean.hip through mesh.components / mesh.clean, extract_mesh.py, clean_mesh.py) against
its numpy restatement (tests/mesh_clean_ref.py).  Labels, face labels, roots, counts and the cleaned mesh are integers that
do not depend on the order of execution: everything is compared by array_equal, floats as bit patterns."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_clean_ref as cr
import mesh_ref

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
    return np.ascontiguousarray(a).view(np.uint32)


def _same_mesh(got, want):
    """got: a mesh.Mesh, want: a dict of arrays.  Shapes, dtypes, integers and float bit patterns."""
    g = _to_dict(got)
    V, F = len(want["vertices"]), len(want["faces"])
    assert got.faces.dtype == torch.int32 and tuple(got.faces.shape) == (F, 3) and tuple(got.vertices.shape) == (V, 3)
    assert tuple(got.roughness.shape) == (V,) and tuple(got.metallic.shape) == (V,)
    assert np.array_equal(g["faces"], np.asarray(want["faces"]).reshape(-1, 3))
    for k in FLOAT_KEYS:
        assert g[k].dtype == np.float32 and np.array_equal(_bits(g[k]), _bits(np.asarray(want[k], np.float32))), k


def _check_components(V, faces, m=None):
    import mesh
    m = _to_mesh(cr.with_attributes(V, faces)) if m is None else m
    cc = mesh.components(m)
    ref = cr.components(V, faces)
    for k in ("labels", "face_labels", "roots", "counts"):
        t = getattr(cc, k)
        assert t.dtype == torch.int32 and t.device == m.vertices.device
        assert np.array_equal(t.cpu().numpy(), ref[k]), k
    assert cc.invalid_faces == ref["invalid_faces"]
    assert 1 <= cc.rounds <= mesh.cc_round_cap(V)
    return cc


def _check_clean(d, K, M):
    import mesh
    out, report = mesh.clean(_to_mesh(d), keep_largest=K, min_faces=M)
    want, want_report = cr.clean(d, K, M)
    _same_mesh(out, want)
    for k, v in want_report.items():
        assert report[k] == v, k
    return out, report


# ---- hand-made meshes -----------------------------------------------------------------------------------------------------
def test_debris_invalid_faces_and_unreferenced_vertices():
    V, faces = cr.hand_made()["debris"]
    cc = _check_components(V, faces)
    assert cc.invalid_faces == 2 and cc.face_labels[-2:].tolist() == [-1, -1]
    assert cc.labels.tolist() == [0, 1, 2, 2, 2, 2, 6, 7, 7, 7, 7] and cc.roots.tolist() == [2, 7] and cc.counts.tolist() == [4, 4]
    d = cr.with_attributes(V, faces, seed=3)
    out, report = _check_clean(d, 0, 0)  # removes the two invalid faces and the three unreferenced vertices, nothing else
    assert report["invalid_faces"] == 2 and report["faces_removed"] == 2 and report["vertices_removed"] == 3
    assert np.array_equal(out.faces.cpu().numpy(), np.concatenate([cr.TET, cr.TET + 4]))
    # the same faces through the C ABI with canaries around parent and count: nothing is touched through a bad index
    import gigs_lib
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    pad = 64
    parent = torch.full((V + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    parent[pad:pad + V] = torch.arange(V, dtype=torch.int32, device=DEV)
    count = torch.full((V + 2 * pad,), -7, dtype=torch.int32, device=DEV)
    f = torch.from_numpy(faces).to(DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    face_label = torch.empty(len(faces), dtype=torch.int32, device=DEV)
    pp = parent[pad:pad + V]
    for _ in range(3):
        gigs_lib.check(lib.gigs_mesh_cc_hook(V, len(faces), f.data_ptr(), pp.data_ptr(), flags.data_ptr(), s), "hook")
        gigs_lib.check(lib.gigs_mesh_cc_flatten(V, pp.data_ptr(), s), "flatten")
    gigs_lib.check(lib.gigs_mesh_cc_count(V, len(faces), f.data_ptr(), pp.data_ptr(), face_label.data_ptr(),
                                          count[pad:pad + V].data_ptr(), flags[1:].data_ptr(), s), "count")
    assert flags.tolist() == [0, 2]
    assert (parent[:pad] == -7).all() and (parent[pad + V:] == -7).all() and (count[:pad] == -7).all() and (count[pad + V:] == -7).all()
    assert pp.tolist() == cc.labels.tolist() and count[pad:pad + V].tolist() == [0, 0, 4, 0, 0, 0, 0, 4, 0, 0, 0]


def test_shells_sharing_one_vertex_are_one_component():
    V, faces = cr.hand_made()["kiss"]
    cc = _check_components(V, faces)
    assert cc.roots.tolist() == [0] and cc.counts.tolist() == [8] and cc.labels.tolist() == [0] * 7
    _check_clean(cr.with_attributes(V, faces), 1, 0)


def test_a_tie_at_the_kth_keeps_both():
    V, faces = cr.hand_made()["twins"]
    cc = _check_components(V, faces)
    assert cc.roots.tolist() == [0, 4] and cc.counts.tolist() == [4, 4]
    d = cr.with_attributes(V, faces)
    out, report = _check_clean(d, 1, 0)
    assert report["components_kept"] == 2 and report["faces_removed"] == 0 and report["threshold"] == 4
    _same_mesh(out, d)


def test_a_degenerate_face_connects():
    V, faces = cr.hand_made()["degenerate"]
    cc = _check_components(V, faces)
    assert cc.labels[5].item() == 0 and cc.roots.tolist() == [0, 8] and cc.counts.tolist() == [3, 1]
    out, report = _check_clean(cr.with_attributes(V, faces), 1, 0)
    assert out.faces.tolist() == [[0, 1, 2], [3, 3, 2], [3, 4, 5]] and report["vertices_removed"] == 5


# ---- strips: many workgroups, several rounds ------------------------------------------------------------------------------
@pytest.mark.parametrize("ordering", cr.STRIP_ORDERINGS)
def test_strip_is_one_component_within_the_round_cap(ordering):
    import mesh
    V, faces = cr.strip(ordering)
    assert (V, len(faces)) == (8194, 8192)
    cc = _check_components(V, faces)
    print("strip %s: %d rounds on the GPU, %d in the synchronous model, cap %d" % (ordering, cc.rounds, cr.sync_rounds(V, faces),
                                                                                  mesh.cc_round_cap(V)))
    assert cc.roots.tolist() == [0] and cc.counts.tolist() == [8192] and int(cc.labels.max()) == 0
    assert cc.rounds <= mesh.cc_round_cap(V)


def test_reaching_the_round_cap_raises_and_returns_no_labels(monkeypatch):
    import mesh
    V, faces = cr.strip("random")
    m = _to_mesh(cr.with_attributes(V, faces))
    monkeypatch.setattr(mesh, "cc_round_cap", lambda n: 3)  # this numbering needs 9 passes
    with pytest.raises(mesh.ComponentsNotConverged, match="3 hook passes"):
        mesh.components(m)
    with pytest.raises(mesh.ComponentsNotConverged):
        mesh.clean(m, keep_largest=1)
    monkeypatch.undo()
    assert mesh.components(m).roots.tolist() == [0]


# ---- the extracted blob field ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blob():
    """(the extracted mesh on the device, the same as a dict of arrays).  Read-only for the tests."""
    import mesh
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    vol = mesh.TSDFVolume(lo, h, cr.BLOB_DIMS, np.float32(3.0) * h, device=DEV)
    vol.load(tsdf, weight, attr_weight, attr)
    m = vol.extract(1)
    return m, _to_dict(m)


def test_blob_components():
    m, d = _blob()
    V, F = len(d["vertices"]), len(d["faces"])
    assert (V, F) == (980, 1944) and len(np.unique(d["faces"])) == V
    cc = _check_components(V, d["faces"], m)
    assert cc.counts.tolist() == [48, 1200, 652, 44] and cc.invalid_faces == 0


@pytest.mark.parametrize("K,M,faces_left,kept", [(2, 0, 1200 + 652, 2), (0, 46, 1944 - 44, 3), (3, 100, 1200 + 652, 2)])
def test_blob_clean(K, M, faces_left, kept):
    _, d = _blob()
    out, report = _check_clean(d, K, M)
    f = out.faces.cpu().numpy()
    V2 = out.vertices.shape[0]
    assert len(f) == faces_left and report["components_kept"] == kept and report["components"] == 4
    assert len(np.unique(f)) == V2 and f.min() >= 0 and f.max() < V2  # no kept vertex is unreferenced
    assert (mesh_ref.edge_counts(f)[1] == 2).all()  # the shells are closed: the remap preserved the topology


def test_identity_and_idempotence():
    import mesh
    m, d = _blob()
    out, report = mesh.clean(m)
    _same_mesh(out, d)
    assert report["faces_removed"] == 0 and report["vertices_removed"] == 0 and report["components_kept"] == 4
    once, _ = mesh.clean(m, keep_largest=2)
    twice, report = mesh.clean(once, keep_largest=2)
    _same_mesh(twice, _to_dict(once))
    assert report["components"] == 2 and report["faces_removed"] == 0


def test_empty_inputs():
    import mesh
    _, d = _blob()
    empty = {k: np.asarray(v)[:0] for k, v in d.items()}
    no_faces = dict(d, faces=d["faces"][:0])
    no_vertices = dict(empty, faces=d["faces"])
    for case, V, F in ((empty, 0, 0), (no_faces, 980, 0), (no_vertices, 0, 1944)):
        cc = mesh.components(_to_mesh(case))
        assert tuple(cc.labels.shape) == (V,) and tuple(cc.face_labels.shape) == (F,) and cc.labels.tolist() == list(range(V))
        assert tuple(cc.roots.shape) == (0,) and tuple(cc.counts.shape) == (0,) and cc.rounds == 0 and cc.invalid_faces == F
        assert bool((cc.face_labels == -1).all()) and cc.labels.dtype == torch.int32 and cc.roots.dtype == torch.int32
        out, report = _check_clean(case, 1, 0)
        assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.roughness.shape) == (0,)
    out, report = _check_clean(d, 0, 5000)  # min_faces above every count
    assert tuple(out.vertices.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.normals.shape) == (0, 3)
    assert tuple(out.albedo.shape) == (0, 3) and tuple(out.roughness.shape) == (0,) and tuple(out.metallic.shape) == (0,)
    assert out.faces.dtype == torch.int32 and report["components_kept"] == 0 and report["faces_removed"] == 1944


# ---- the overflow guard ---------------------------------------------------------------------------------------------------
def test_compact_sets_the_flag_and_stores_nothing_beyond_a_short_capacity():
    """Capacities one short of the need; a canary row lies behind each capacity.  The kernel must not store there."""
    import gigs_lib
    m, d = _blob()
    lib = gigs_lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    V, F = 980, 1944
    want, _ = cr.clean(d, 2, 0)
    V2, F2 = len(want["vertices"]), len(want["faces"])
    i32 = dict(dtype=torch.int32, device=DEV)
    cc = cr.components(V, d["faces"])
    root_keep = np.zeros(V, np.uint8)
    root_keep[cc["roots"][cc["counts"] >= 652]] = 1
    face_keep, vertex_keep = torch.empty(F, **i32), torch.empty(V, **i32)
    face_label, root_keep = torch.from_numpy(cc["face_labels"]).to(DEV), torch.from_numpy(root_keep).to(DEV)
    gigs_lib.check(lib.gigs_mesh_mark(V, F, m.faces.data_ptr(), face_label.data_ptr(), root_keep.data_ptr(), face_keep.data_ptr(),
                                      vertex_keep.data_ptr(), s), "mark")
    v_off = torch.cumsum(vertex_keep, 0, dtype=torch.int32) - vertex_keep
    f_off = torch.cumsum(face_keep, 0, dtype=torch.int32) - face_keep
    assert int(vertex_keep.sum()) == V2 and int(face_keep.sum()) == F2
    CAN_F, CAN_I = -123.5, -77

    def run(vcap, fcap):
        outs = [torch.full((V2, 3), CAN_F, device=DEV), torch.full((V2, 3), CAN_F, device=DEV), torch.full((V2, 3), CAN_F, device=DEV),
                torch.full((V2,), CAN_F, device=DEV), torch.full((V2,), CAN_F, device=DEV)]
        faces_out = torch.full((F2, 3), CAN_I, **i32)
        overflow = torch.zeros(1, **i32)
        gigs_lib.check(lib.gigs_mesh_compact(V, F, m.vertices.data_ptr(), m.normals.data_ptr(), m.albedo.data_ptr(),
                                             m.roughness.data_ptr(), m.metallic.data_ptr(), m.faces.data_ptr(),
                                             vertex_keep.data_ptr(), v_off.data_ptr(), face_keep.data_ptr(), f_off.data_ptr(),
                                             vcap, fcap, *(t.data_ptr() for t in outs), faces_out.data_ptr(),
                                             overflow.data_ptr(), s), "compact")
        return outs, faces_out, int(overflow.item())

    outs, faces_out, flag = run(V2, F2)  # exact capacities: no flag, the restatement's mesh
    assert flag == 0 and np.array_equal(faces_out.cpu().numpy(), want["faces"])
    outs, faces_out, flag = run(V2 - 1, F2)  # the last vertex row is the canary
    assert flag == 1
    for t, k in zip(outs, FLOAT_KEYS):
        assert bool((t[V2 - 1] == CAN_F).all()), k
        assert np.array_equal(_bits(t[:V2 - 1].cpu().numpy()), _bits(want[k][:V2 - 1])), k
    got = faces_out.cpu().numpy()
    uses_last = (want["faces"] == V2 - 1).any(axis=1)
    assert uses_last.any() and (got[uses_last] == CAN_I).all() and np.array_equal(got[~uses_last], want["faces"][~uses_last])
    outs, faces_out, flag = run(V2, F2 - 1)  # the last face row is the canary
    assert flag == 1 and bool((faces_out[F2 - 1] == CAN_I).all())
    assert np.array_equal(faces_out[:F2 - 1].cpu().numpy(), want["faces"][:F2 - 1])
    for t, k in zip(outs, FLOAT_KEYS):
        assert np.array_equal(_bits(t.cpu().numpy()), _bits(want[k])), k


# ---- rendering ------------------------------------------------------------------------------------------------------------
def test_render_of_the_cleaned_mesh_equals_the_raw_render_on_kept_faces():
    import mesh
    import mesh_render
    import scenes
    m, d = _blob()
    cleaned, _ = mesh.clean(m, keep_largest=2)
    cc = cr.components(980, d["faces"])
    face_keep = np.isin(cc["face_labels"], cc["roots"][cc["counts"] >= 652])
    rank = np.cumsum(face_keep) - 1
    cam = scenes.look_at_camera((0.05, 0.02, 3.0), (0.0, 0.0, 0.0), 64, 64, 0.6911, up=(0.0, 1.0, 0.0))
    cam = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    removed = dict(d, faces=d["faces"][~face_keep])
    with mesh_render.MeshRasterizer(m, device=DEV) as a, mesh_render.MeshRasterizer(cleaned, device=DEV) as b, \
            mesh_render.MeshRasterizer(removed, device=DEV) as c:
        raw = {k: v.cpu().numpy() for k, v in a(cam).items()}
        new = {k: v.cpu().numpy() for k, v in b(cam).items()}
        gone = c(cam)["tri_id"].cpu().numpy()
    tri = raw["tri_id"]
    covered = tri >= 0
    ok = covered & face_keep[np.where(covered, tri, 0)] & (gone < 0)  # a kept face won, and no removed face covers the pixel
    share = ok.sum() / max(int(covered.sum()), 1)
    print("covered %d pixels, qualifying %d (%.3f), removed faces cover %d" % (covered.sum(), ok.sum(), share, (gone >= 0).sum()))
    assert covered.sum() > 200 and share >= 0.5 and (gone >= 0).any()
    assert np.array_equal(new["tri_id"][ok], rank[tri[ok]])
    for k in mesh_render.PLANES:
        assert np.array_equal(_bits(raw[k])[:, ok], _bits(new[k])[:, ok]), k


# ---- tools ----------------------------------------------------------------------------------------------------------------
def test_extract_mesh_and_clean_mesh_tools(tmp_path):
    """extract_mesh.py on a scene folder and an output folder as trainer.py leaves them (test_gpu_mesh.py's set-up)."""
    from argparse import Namespace

    import clean_mesh
    import densify
    import extract_mesh
    import mesh
    import optim
    import relight
    import scene_io
    import scenes
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
    a = extract_mesh.parse_args(["-m", out, "--checkpoint", ck])
    assert (a.keep_largest, a.min_faces) == (0, 0)
    base = ["-m", out, "--checkpoint", ck, "--grid", "40", "--split", "test"]
    r1 = extract_mesh.extract_mesh(base + ["-o", "raw1.ply"])
    r2 = extract_mesh.extract_mesh(base + ["-o", "raw2.ply"])
    assert open(r1["path"], "rb").read() == open(r2["path"], "rb").read()
    for k in ("components", "components_kept", "faces_removed", "clean_s"):
        assert k not in r1
    assert sorted(r1) == sorted(["path", "views", "samples", "dims", "voxel", "lo", "hi", "vertices", "faces", "load_s",
                                 "cameras_s", "fuse_s", "extract_s", "write_s"])

    def same(path, want):  # albedo after the PLY's 8-bit quantisation, which both sides went through once
        got = scene_io.read_mesh_ply(path)
        for k in cr.MESH_KEYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
            assert np.array_equal(got[k] if k == "faces" else _bits(got[k]), want[k] if k == "faces" else _bits(want[k])), k

    # --keep_largest 1 on that folder, and --min_faces 3 on a noisier extraction (--min_weight 1 leaves border fragments)
    for extra, flags, K, M in (([], ["--keep_largest", "1"], 1, 0), (["--min_weight", "1"], ["--min_faces", "3"], 0, 3)):
        raw = r1 if not extra else extract_mesh.extract_mesh(base + extra + ["-o", "raw3.ply"])
        raw_ply = scene_io.read_mesh_ply(raw["path"])  # positions, normals, roughness and metallic bit for bit
        want, want_report = cr.clean(raw_ply, K, M)
        r3 = extract_mesh.extract_mesh(base + extra + flags + ["-o", "clean.ply"])
        assert r3["components"] == want_report["components"] and r3["components_kept"] == want_report["components_kept"]
        assert r3["faces_removed"] == want_report["faces_removed"] and r3["clean_s"] >= 0
        assert r3["faces"] == len(want["faces"]) and r3["vertices"] == len(want["vertices"])
        print("extract_mesh %s: %d components, %d kept, %d of %d faces removed" % (
            " ".join(extra + flags), r3["components"], r3["components_kept"], r3["faces_removed"], raw["faces"]))
        same(r3["path"], want)
        # the same through mesh.clean of the raw PLY's arrays, and through clean_mesh.py on the file
        direct, _ = mesh.clean(_to_mesh(raw_ply), keep_largest=K, min_faces=M)
        _same_mesh(direct, want)
        rep = clean_mesh.clean_mesh([raw["path"], "-o", str(tmp_path / "tool.ply")] + flags)
        assert rep["faces"] == len(want["faces"]) and rep["vertices"] == len(want["vertices"]) and rep["faces_in"] == raw["faces"]
        assert rep["components_kept"] == want_report["components_kept"] and json.loads(json.dumps(rep)) == rep
        same(rep["path"], want)
    assert want_report["components"] > want_report["components_kept"] >= 1 and want_report["faces_removed"] > 0
