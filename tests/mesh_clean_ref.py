"""CPU restatement of mesh cleaning (csrc/mesh_clean.hip through mesh.components / mesh.clean), as include/gigs_hip.h states
it: valid faces, vertex connectivity, labels = the smallest vertex index of a component, counts, the keep threshold and the
compaction.  All integers; floats are only copied.  Also the hand-made meshes and the fields the tests share."""
import numpy as np

import mesh_ref

MESH_KEYS = ("vertices", "faces", "normals", "albedo", "roughness", "metallic")


def valid_faces(V, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(axis=1)


def components(V, faces):
    """-> dict(labels [V], face_labels [F], roots [C], counts [C] (int32), invalid_faces).  Union-find whose root is the
    smaller index, so a root is the minimum of its set."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = valid_faces(V, f)
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b, c in f[ok].tolist():
        ra, rb, rc = find(a), find(b), find(c)
        m = min(ra, rb, rc)
        parent[ra] = parent[rb] = parent[rc] = m
    labels = np.array([find(v) for v in range(V)], np.int32).reshape(V)
    face_labels = np.full(len(f), -1, np.int32)
    face_labels[ok] = labels[f[ok, 0]]
    count = np.bincount(face_labels[ok], minlength=max(V, 1))[:V] if V else np.zeros(0, np.int64)
    roots = np.nonzero(count > 0)[0].astype(np.int32)
    return dict(labels=labels, face_labels=face_labels, roots=roots, counts=count[roots].astype(np.int32),
                invalid_faces=int((~ok).sum()))


def keep_threshold(counts, keep_largest=0, min_faces=0):
    c = sorted((int(x) for x in np.asarray(counts).reshape(-1)), reverse=True)
    c_k = 0
    if keep_largest > 0 and c:
        c_k = c[min(keep_largest, len(c)) - 1]
    return max(int(min_faces), c_k, 1)


def clean(mesh, keep_largest=0, min_faces=0):
    """mesh: a dict with MESH_KEYS (arrays) -> (the cleaned dict, report)."""
    V = len(mesh["vertices"])
    f = np.asarray(mesh["faces"], np.int32).reshape(-1, 3)
    cc = components(V, f)
    thr = keep_threshold(cc["counts"], keep_largest, min_faces)
    kept_roots = cc["roots"][cc["counts"] >= thr]
    face_keep = np.isin(cc["face_labels"], kept_roots) & (cc["face_labels"] >= 0)
    vertex_keep = np.zeros(V, bool)
    vertex_keep[f[face_keep].reshape(-1)] = True
    new_index = np.cumsum(vertex_keep) - 1
    out = {k: np.ascontiguousarray(np.asarray(mesh[k])[vertex_keep]) for k in MESH_KEYS if k != "faces"}
    out["faces"] = new_index[f[face_keep]].astype(np.int32).reshape(-1, 3)
    report = dict(components=len(cc["roots"]), components_kept=len(kept_roots), faces_removed=len(f) - int(face_keep.sum()),
                  vertices_removed=V - int(vertex_keep.sum()), invalid_faces=cc["invalid_faces"], threshold=thr)
    return out, report


# ---- the meshes the tests share -------------------------------------------------------------------------------------------
TET = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)


def with_attributes(V, faces, seed=0):
    """A mesh dict over `faces` with seeded random positions and attributes (float32)."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.uniform(-1.0, 1.0, size=s).astype(np.float32)  # noqa: E731
    return dict(vertices=r(V, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3), normals=r(V, 3), albedo=r(V, 3),
                roughness=r(V), metallic=r(V))


def hand_made():
    """name -> (V, faces).  `debris`: two tetrahedra (vertices 2..5 and 7..10), three unreferenced vertices (0, 1, 6), a face
    with an index == V and one with -1.  `kiss`: two tetrahedra sharing exactly vertex 3.  `twins`: two identical
    tetrahedra.  `degenerate`: a face (a, a, b) between two triangles that nothing else joins, and one far triangle."""
    debris = np.concatenate([TET + 2, TET + 7, [[2, 3, 11]], [[4, -1, 5]]]).astype(np.int32)
    kiss = np.concatenate([TET, np.array([[3, 4, 5], [3, 6, 4], [4, 6, 5], [5, 6, 3]])]).astype(np.int32)
    twins = np.concatenate([TET + 4, TET]).astype(np.int32)  # the larger indices first
    degenerate = np.array([[0, 1, 2], [5, 5, 2], [5, 6, 7], [8, 9, 10]], np.int32)
    return dict(debris=(11, debris), kiss=(7, kiss), twins=(8, twins), degenerate=(11, degenerate))


STRIP_QUADS = 4096
STRIP_ORDERINGS = ("ascending", "descending", "random", "alternating")


def strip(ordering, quads=STRIP_QUADS):
    """A strip of `quads` quads: columns i = 0..quads of two vertices, two triangles per quad; the geometric vertex g is
    numbered number[g].  -> (V, faces)."""
    n = 2 * (quads + 1)
    g = np.arange(n)
    if ordering == "ascending":
        number = g
    elif ordering == "descending":
        number = n - 1 - g
    elif ordering == "random":
        number = np.random.default_rng(4096).permutation(n)
    elif ordering == "alternating":  # even columns take the next two low numbers, odd columns the next two high ones
        low = (g // 4) * 2 + g % 2
        number = np.where((g // 2) % 2 == 0, low, n - 1 - low)
    else:
        raise ValueError(ordering)
    i = np.arange(quads)
    a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 3, 2 * i + 2  # the quad a-b-c-d
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)
    return n, number[faces].astype(np.int32)


def sync_rounds(V, faces):
    """Passes of a synchronous model of min-hooking (every face reads the roots of the flat forest the last pass left,
    every root takes the minimum offered to it, then the forest is flattened), counting the confirming pass."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(V, f)]
    parent = np.arange(V)
    rounds = 0
    while True:
        rounds += 1
        r = parent[f]
        m = r.min(axis=1, keepdims=True)
        if (r == m).all():
            return rounds
        np.minimum.at(parent, r.reshape(-1), np.broadcast_to(m, r.shape).reshape(-1))
        while True:  # flatten
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt


BLOB_DIMS = (33, 25, 21)
BLOBS = ((-0.45, 0.0, 0.0, 0.30), (0.35, 0.05, 0.0, 0.22), (0.75, -0.3, 0.2, 0.06), (0.0, 0.45, -0.3, 0.06))


def blob_field(seed=9):
    """(lo, h, tsdf, weight, attr_weight, attr) on mesh_ref.sphere_grid(BLOB_DIMS): clip(min_i(|s - c_i| - r_i) / (3h), -1,
    1) over BLOBS, weights all 1, random attributes."""
    lo, h = mesh_ref.sphere_grid(BLOB_DIMS)
    Gx, Gy, Gz = BLOB_DIMS
    x = lo[0].astype(np.float64) + np.arange(Gx) * float(h)
    y = lo[1].astype(np.float64) + np.arange(Gy) * float(h)
    z = lo[2].astype(np.float64) + np.arange(Gz) * float(h)
    d = np.full((Gz, Gy, Gx), np.inf)
    for cx, cy, cz, r in BLOBS:
        d = np.minimum(d, np.sqrt((x[None, None, :] - cx) ** 2 + (y[None, :, None] - cy) ** 2 + (z[:, None, None] - cz) ** 2) - r)
    tsdf = np.clip(d / (3.0 * float(h)), -1.0, 1.0).astype(np.float32)
    rng = np.random.default_rng(seed)
    attr = rng.uniform(-1.0, 1.0, size=tsdf.shape + (8,)).astype(np.float32)
    return lo, h, tsdf, np.ones_like(tsdf), np.ones_like(tsdf), attr
