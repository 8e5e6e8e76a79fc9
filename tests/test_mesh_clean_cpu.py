"""CPU: the restatement of mesh cleaning (tests/mesh_clean_ref.py) against a brute-force breadth-first search in plain
Python (and scipy's connected_components where scipy imports), and mesh.keep_threshold's cases."""
import numpy as np
import pytest

import mesh_clean_ref as cr
import mesh_ref


def _bfs_labels(V, faces):
    """label[v] = the smallest vertex of v's component, by breadth-first search over vertex adjacency through valid faces."""
    adj = [set() for _ in range(V)]
    for f in np.asarray(faces).reshape(-1, 3).tolist():
        if all(0 <= i < V for i in f):
            for i in f:
                adj[i].update(f)
    label = [-1] * V
    for s in range(V):  # ascending: the seed of a search is the smallest vertex of its component
        if label[s] >= 0:
            continue
        label[s], queue = s, [s]
        while queue:
            nxt = []
            for v in queue:
                for u in adj[v]:
                    if label[u] < 0:
                        label[u] = s
                        nxt.append(u)
            queue = nxt
    return np.array(label, np.int32).reshape(V)


def _check_against_bfs(V, faces):
    cc = cr.components(V, faces)
    labels = _bfs_labels(V, faces)
    assert np.array_equal(cc["labels"], labels)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = np.array([all(0 <= i < V for i in row) for row in f.tolist()], bool).reshape(len(f))
    assert cc["invalid_faces"] == int((~ok).sum())
    want = np.full(len(f), -1, np.int32)
    want[ok] = labels[f[ok, 0]]
    assert np.array_equal(cc["face_labels"], want)
    roots = sorted(set(want[ok].tolist()))
    assert cc["roots"].tolist() == roots
    assert cc["counts"].tolist() == [int((want == r).sum()) for r in roots]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return cc
    if V == 0:
        return cc
    g = f[ok]
    rows, cols = np.concatenate([g[:, 0], g[:, 1]]), np.concatenate([g[:, 1], g[:, 2]])
    n, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(V, V)), directed=False)
    first = np.full(n, V, np.int64)  # scipy numbers the components as it likes: name each by its smallest vertex
    np.minimum.at(first, lab, np.arange(V))
    assert np.array_equal(first[lab], labels)
    return cc


def test_restatement_matches_breadth_first_search_on_the_hand_made_meshes():
    meshes = cr.hand_made()
    cc = _check_against_bfs(*meshes["debris"])
    assert cc["invalid_faces"] == 2 and cc["roots"].tolist() == [2, 7] and cc["counts"].tolist() == [4, 4]
    assert cc["labels"].tolist() == [0, 1, 2, 2, 2, 2, 6, 7, 7, 7, 7] and cc["face_labels"][-2:].tolist() == [-1, -1]
    cc = _check_against_bfs(*meshes["kiss"])  # one shared vertex joins the shells
    assert cc["roots"].tolist() == [0] and cc["counts"].tolist() == [8]
    cc = _check_against_bfs(*meshes["twins"])
    assert cc["roots"].tolist() == [0, 4] and cc["counts"].tolist() == [4, 4]
    cc = _check_against_bfs(*meshes["degenerate"])  # (5, 5, 2) joins the triangles (0, 1, 2) and (5, 6, 7)
    assert cc["roots"].tolist() == [0, 8] and cc["counts"].tolist() == [3, 1] and cc["labels"][5] == 0
    for V, faces in ((0, np.zeros((0, 3), np.int32)), (5, np.zeros((0, 3), np.int32)), (0, np.array([[0, 1, 2]], np.int32))):
        cc = _check_against_bfs(V, faces)
        assert len(cc["roots"]) == 0 and cc["labels"].tolist() == list(range(V))


def test_restatement_matches_breadth_first_search_on_strips_and_the_blob_mesh():
    for ordering in cr.STRIP_ORDERINGS:
        V, faces = cr.strip(ordering, quads=300)
        cc = _check_against_bfs(V, faces)
        assert cc["roots"].tolist() == [0] and cc["counts"].tolist() == [600]
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    m = mesh_ref.surface_nets(tsdf, weight, attr_weight, attr, lo, h, 1)
    V = len(m["vertices"])
    cc = _check_against_bfs(V, m["faces"])
    assert (V, len(m["faces"])) == (980, 1944) and cc["counts"].tolist() == [48, 1200, 652, 44]
    assert len(np.unique(m["faces"])) == V  # no unreferenced vertex
    for K, M, faces_left, kept in ((2, 0, 1200 + 652, 2), (0, 46, 1944 - 44, 3), (3, 100, 1200 + 652, 2), (0, 0, 1944, 4)):
        out, report = cr.clean(m, K, M)
        assert len(out["faces"]) == faces_left and report["components_kept"] == kept and report["components"] == 4
        assert len(np.unique(out["faces"])) == len(out["vertices"]) and out["faces"].max() < len(out["vertices"])
        assert (mesh_ref.edge_counts(out["faces"])[1] == 2).all()  # closed shells stay closed: the remap kept the topology
        again, _ = cr.clean(out, K, M)
        assert all(np.array_equal(again[k], out[k]) for k in cr.MESH_KEYS)


def test_clean_restatement_drops_invalid_faces_and_unreferenced_vertices_only_at_zero():
    V, faces = cr.hand_made()["debris"]
    m = cr.with_attributes(V, faces)
    out, report = cr.clean(m)
    keep = [2, 3, 4, 5, 7, 8, 9, 10]
    assert report == dict(components=2, components_kept=2, faces_removed=2, vertices_removed=3, invalid_faces=2, threshold=1)
    assert np.array_equal(out["faces"], np.concatenate([cr.TET, cr.TET + 4]))
    for k in cr.MESH_KEYS:
        if k != "faces":
            assert np.array_equal(out[k].view(np.uint32), m[k][keep].view(np.uint32))


@pytest.mark.parametrize("which", ["mesh", "ref"])
def test_keep_threshold(which):
    if which == "mesh":
        import mesh
        thr = mesh.keep_threshold
    else:
        thr = cr.keep_threshold
    counts = [48, 1200, 652, 44]
    assert thr(counts, 0, 0) == 1                      # K = 0: everything with a face
    assert thr(counts, -3, 0) == 1
    assert thr(counts, 1, 0) == 1200                   # K = 1: the largest
    assert thr(counts, 2, 0) == 652
    assert thr(counts, 4, 0) == 44                     # K = the number of components: the smallest count
    assert thr(counts, 9, 0) == 44                     # K beyond it
    assert thr(counts, 0, 46) == 46 and thr(counts, 3, 100) == 100 and thr(counts, 2, 100) == 652
    assert thr(counts, 1, 5000) == 5000                # M above every count: nothing reaches it
    assert sum(c >= thr(counts, 1, 5000) for c in counts) == 0
    ties = [7, 4, 4, 4, 2]
    assert thr(ties, 2, 0) == 4 and sum(c >= thr(ties, 2, 0) for c in ties) == 4  # ties at the K-th are all kept
    assert thr([4, 4], 1, 0) == 4
    assert thr([], 3, 0) == 1 and thr([], 0, 7) == 7
    assert thr(np.array(counts, np.int32), 2, 0) == 652
    assert isinstance(thr(counts, 2, 0), int)


def test_round_cap_and_cpu_tensors_fail_loudly():
    import torch

    import mesh
    assert mesh.cc_round_cap(1) == 8 and mesh.cc_round_cap(2) == 10 and mesh.cc_round_cap(8194) == 2 * 14 + 8
    assert mesh.cc_round_cap(2 ** 31 - 1) == 70
    for ordering in cr.STRIP_ORDERINGS:  # the synchronous model stays far below the cap
        V, faces = cr.strip(ordering)
        assert cr.sync_rounds(V, faces) <= mesh.cc_round_cap(V)
    V, faces = cr.hand_made()["kiss"]
    m = mesh.Mesh(*(torch.from_numpy(cr.with_attributes(V, faces)[k]) for k in mesh.Mesh._fields))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.components(m)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.clean(m, keep_largest=1)
