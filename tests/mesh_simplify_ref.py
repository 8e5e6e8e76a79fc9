"""CPU restatement of mesh simplification (csrc/mesh_simplify.hip through mesh.cluster_map / mesh.simplify), as
include/gigs_hip.h states it under "Simplifying meshes": cells and keys in float32, clusters in ascending key order, the
rotated cluster triples of the surviving faces without their same-winding duplicates, the member means of the attributes,
the quadric placement in float64 local to the cell centre, and clean(.., 0, 0)'s compaction.  Every sum runs in the stated
order (np.add.at adds element after element), so the integers and the mean attributes are the kernel's bit for bit; the
positions and normals differ from it by a float64 sqrt and one float32 rounding at most.  Also the meshes the tests share."""
import numpy as np

import mesh_clean_ref as cr

CELL_AXIS = 1 << 21
REPORT_KEYS = ("clusters", "vertices", "faces", "faces_in", "vertices_in", "faces_collapsed", "faces_duplicate", "faces_invalid",
               "vertices_unclustered", "cell", "origin")


def cluster_grid(vertices, cell, origin=None):
    """-> (origin float32 [3], inv float32).  ValueError as mesh.cluster_grid."""
    cell32 = np.float32(cell)
    if not (np.isfinite(cell32) and cell32 > 0):
        raise ValueError("cell must be positive")
    with np.errstate(over="ignore"):
        inv = np.float32(1) / cell32
    if not np.isfinite(inv):
        raise ValueError("1 / cell is not finite")
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    v = v[np.isfinite(v).all(axis=1)]
    lo = None
    if len(v):
        lo, hi = v.min(axis=0), v.max(axis=0)
        with np.errstate(over="ignore"):
            top = np.floor((hi - lo) * inv)
        if not (top < CELL_AXIS).all():
            raise ValueError("the extent needs more than 2^21 cells on an axis")
    if origin is None:
        org = lo if lo is not None else np.zeros(3, np.float32)
    else:
        org = np.asarray(origin, np.float32).reshape(3)
        if not np.isfinite(org).all():
            raise ValueError("origin must be finite")
    return org.astype(np.float32), inv


def cluster_keys(vertices, origin, inv):
    """-> (keys [V] int64, -1 for an unclustered vertex; cells [V,3] int64)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.floor((v - origin.astype(np.float32)[None, :]) * np.float32(inv))  # float32 throughout
        assert t.dtype == np.float32
        ok = (np.isfinite(v) & (t >= 0) & (t < CELL_AXIS)).all(axis=1)
    c = np.where(ok[:, None], t, 0).astype(np.int64)
    keys = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
    return np.where(ok, keys, -1), c


def cluster_map(vertices, cell, origin=None):
    """-> dict(cluster_of [V] int32, C, keys [C] int64 ascending, cells [C,3], origin, inv)."""
    org, inv = cluster_grid(vertices, cell, origin)
    keys, _ = cluster_keys(vertices, org, inv)
    uniq = np.unique(keys[keys >= 0])
    cluster_of = np.full(len(keys), -1, np.int32)
    cluster_of[keys >= 0] = np.searchsorted(uniq, keys[keys >= 0]).astype(np.int32)
    cells = np.stack([uniq & (CELL_AXIS - 1), (uniq >> 21) & (CELL_AXIS - 1), (uniq >> 42) & (CELL_AXIS - 1)], axis=1)
    return dict(cluster_of=cluster_of, C=len(uniq), keys=uniq, cells=cells.reshape(-1, 3), origin=org, inv=inv)


def cluster_faces(V, faces, cluster_of):
    """-> dict(valid [F] bool, clusters [F,3] (-1 rows where invalid), survive [F] bool, triples [F,3] int32: the rotated
    triple of a surviving face, else -1)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = cr.valid_faces(V, f)
    cl = np.full(f.shape, -1, np.int64)
    cl[valid] = cluster_of[f[valid]]
    valid = valid & (cl >= 0).all(axis=1)
    cl[~valid] = -1
    survive = valid & (cl[:, 0] != cl[:, 1]) & (cl[:, 1] != cl[:, 2]) & (cl[:, 0] != cl[:, 2])
    shift = np.argmin(np.where(survive[:, None], cl, 0), axis=1)  # the smallest is unique on a surviving face
    rows = np.arange(len(f))
    rotated = np.stack([cl[rows, shift], cl[rows, (shift + 1) % 3], cl[rows, (shift + 2) % 3]], axis=1)
    triples = np.where(survive[:, None], rotated, -1).astype(np.int32)
    return dict(valid=valid, clusters=cl, survive=survive, triples=triples)


def dedupe(triples):
    """-> (faces [F,3] int32 with every repetition of an earlier row's triple set to -1, their number)."""
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    order = np.lexsort((np.arange(len(t)), t[:, 2], t[:, 1], t[:, 0]))
    s = t[order]
    dup_sorted = np.zeros(len(t), bool)
    dup_sorted[1:] = (s[1:] == s[:-1]).all(axis=1) & (s[1:, 0] >= 0)
    dup = np.zeros(len(t), bool)
    dup[order] = dup_sorted
    return np.where(dup[:, None], -1, t).astype(np.int32), int(dup.sum())


def solve3(A, r):
    """x with A x = r for stacks of symmetric 3x3 matrices, by cofactors (the kernel's closed form)."""
    m00, m01, m02, m11, m12, m22 = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2], A[:, 1, 1], A[:, 1, 2], A[:, 2, 2]
    c00, c01, c02 = m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11
    c11, c12, c22 = m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01
    det = m00 * c00 + m01 * c01 + m02 * c02
    return np.stack([(c00 * r[:, 0] + c01 * r[:, 1] + c02 * r[:, 2]) / det, (c01 * r[:, 0] + c11 * r[:, 1] + c12 * r[:, 2]) / det,
                     (c02 * r[:, 0] + c12 * r[:, 1] + c22 * r[:, 2]) / det], axis=1)


def quadrics(vertices, cf, centres, C):
    """-> (A [C,3,3], b [C,3]) float64: every valid face adds its area-weighted plane quadric, local to the cluster's cell
    centre, once to each distinct cluster among its three, in ascending face index."""
    p = np.asarray(vertices, np.float32).astype(np.float64)
    A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
    cl = cf["clusters"]
    parts = []
    for slot in range(3):  # a slot counts if no earlier slot of the face names its cluster
        first = cf["valid"].copy()
        for earlier in range(slot):
            first &= cl[:, slot] != cl[:, earlier]
        f = np.nonzero(first)[0]
        k = cl[f, slot]
        g = centres[k]
        face = cf["faces"][f]
        q0 = p[face[:, 0]] - g
        e1, e2 = (p[face[:, 1]] - g) - q0, (p[face[:, 2]] - g) - q0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        length = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        has = length > 0
        f, k, q0, n, length = f[has], k[has], q0[has], n[has], length[has]
        u = n / length[:, None]
        d = -(u[:, 0] * q0[:, 0] + u[:, 1] * q0[:, 1] + u[:, 2] * q0[:, 2])
        wu = (length * 0.5)[:, None] * u
        parts.append((f, k, wu[:, :, None] * u[:, None, :], wu * d[:, None]))
    # a cluster meets a face in one slot only, so sorting the contributions by face fixes every cluster's order
    order = np.argsort(np.concatenate([x[0] for x in parts]), kind="stable")
    k = np.concatenate([x[1] for x in parts])[order]
    np.add.at(A, k, np.concatenate([x[2] for x in parts])[order])
    np.add.at(b, k, np.concatenate([x[3] for x in parts])[order])
    return A, b


def place(mesh, cm, cf, cell, reg=1e-3):
    """The C cluster vertices before compaction -> dict(vertices, normals, albedo, roughness, metallic (float32), mean [C,3]
    float32: the member mean position, for comparison; A, b, m, lam, centres: the float64 system)."""
    C = cm["C"]
    cell64 = float(np.float32(cell))
    centres = cm["origin"].astype(np.float64)[None, :] + (cm["cells"].astype(np.float64) + 0.5) * cell64
    of = cm["cluster_of"]
    idx = np.nonzero(of >= 0)[0]  # ascending vertex index
    k = of[idx]
    count = np.bincount(k, minlength=C).astype(np.float64)

    def member_sum(values):
        a = np.asarray(values, np.float32).astype(np.float64).reshape(len(of), -1)
        s = np.zeros((C, a.shape[1]))
        np.add.at(s, k, a[idx])
        return s

    p = np.asarray(mesh["vertices"], np.float32).astype(np.float64)
    sp = np.zeros((C, 3))
    np.add.at(sp, k, p[idx] - centres[k])
    m = sp / count[:, None]
    A, b = quadrics(mesh["vertices"], cf, centres, C)
    lam = float(reg) * ((A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]) / 3.0
    x = m.copy()
    s = lam > 0
    if s.any():
        x[s] = solve3(A[s] + lam[s, None, None] * np.eye(3)[None], lam[s, None] * m[s] - b[s])
    half = 0.5 * cell64
    x = np.where(x < -half, -half, np.where(x > half, half, x))
    sn = member_sum(mesh["normals"])
    nl = np.sqrt(sn[:, 0] * sn[:, 0] + sn[:, 1] * sn[:, 1] + sn[:, 2] * sn[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        normals = np.where(nl[:, None] > 0, sn / nl[:, None], 0.0)
    return dict(vertices=(centres + x).astype(np.float32), normals=normals.astype(np.float32),
                albedo=(member_sum(mesh["albedo"]) / count[:, None]).astype(np.float32),
                roughness=(member_sum(mesh["roughness"])[:, 0] / count).astype(np.float32),
                metallic=(member_sum(mesh["metallic"])[:, 0] / count).astype(np.float32),
                mean=(centres + m).astype(np.float32), A=A, b=b, m=m, lam=lam, centres=centres, count=count)


def simplify(mesh, cell, origin=None, reg=1e-3):
    """mesh: a dict with cr.MESH_KEYS -> (the simplified dict, the report, detail: cluster_of, C, the cluster vertices of
    place() and `faces` [F,3], the rewritten faces before compaction)."""
    if not (float(cell) > 0):
        raise ValueError("cell must be positive")
    V = len(mesh["vertices"])
    f = np.asarray(mesh["faces"], np.int32).reshape(-1, 3)
    F = len(f)
    report = dict(clusters=0, vertices=0, faces=0, faces_in=F, vertices_in=V, faces_collapsed=0, faces_duplicate=0,
                  faces_invalid=0, vertices_unclustered=0, cell=float(np.float32(cell)))
    empty = {k: np.asarray(mesh[k])[:0] for k in cr.MESH_KEYS if k != "faces"}
    empty["faces"] = np.zeros((0, 3), np.int32)
    if V == 0 or F == 0:
        org = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3)
        report.update(origin=[float(x) for x in org], faces_invalid=F if V == 0 else 0)
        return empty, report, dict(cluster_of=np.full(V, -1, np.int32), C=0)
    cm = cluster_map(mesh["vertices"], cell, origin)
    report.update(origin=[float(x) for x in cm["origin"]], clusters=cm["C"], vertices_unclustered=int((cm["cluster_of"] < 0).sum()))
    if cm["C"] == 0:
        report.update(faces_invalid=F)
        return empty, report, dict(cluster_of=cm["cluster_of"], C=0)
    cf = cluster_faces(V, f, cm["cluster_of"])
    cf["faces"] = f.astype(np.int64)
    faces, n_dup = dedupe(cf["triples"])
    placed = place(mesh, cm, cf, cell, reg)
    out, _ = cr.clean(dict({k: placed[k] for k in cr.MESH_KEYS if k != "faces"}, faces=faces))
    report.update(vertices=len(out["vertices"]), faces=len(out["faces"]), faces_invalid=int((~cf["valid"]).sum()),
                  faces_collapsed=int((cf["valid"] & ~cf["survive"]).sum()), faces_duplicate=n_dup)
    return out, report, dict(placed, cluster_of=cm["cluster_of"], C=cm["C"], faces=faces, cells=cm["cells"], origin=cm["origin"],
                             inv=cm["inv"])


# ---- the meshes the tests share -------------------------------------------------------------------------------------------
def with_attributes(vertices, faces, seed=0):
    """A mesh dict over the given positions with seeded random attributes (float32)."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    d = cr.with_attributes(len(v), faces, seed)
    d["vertices"] = v
    return d


def cube(n=4):
    """The surface of the unit cube [0,1]^3, every side an n x n grid of quads cut into two triangles, outward winding;
    shared vertices merged: 6 n^2 + 2 vertices, 12 n^2 faces.  -> (vertices float32, faces int32)."""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, 1):
            for i in range(n):
                for j in range(n):
                    def corner(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side * n, i + di, j + dj
                        return vid(tuple(p))
                    a, b, c, d = corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)
                    quad = [(a, b, c), (a, c, d)] if side else [(a, c, b), (a, d, c)]  # e_u x e_w = +e_axis
                    faces.extend(quad)
    return (np.array(verts, np.float64) / n).astype(np.float32), np.array(faces, np.int32)


def plane_grid(n=9, seed=5, normal=(0.0, 0.0, 1.0), offset=0.25):
    """An n x n grid of vertices on the plane z = offset (before `normal` is made the axis), jittered within the plane by a
    third of the spacing.  -> (vertices, faces)."""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    xy = np.stack([i, j], -1).reshape(-1, 2) / (n - 1) + rng.uniform(-1, 1, size=(n * n, 2)) / (3.0 * (n - 1))
    v = np.concatenate([xy, np.full((n * n, 1), offset)], axis=1)
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
    return v.astype(np.float32), faces.astype(np.int32)


def sheets(cell=0.5):
    """Three 2 x 2-quad sheets over the same 3 x 3 cells: the second 0.1 cell above the first with the same winding, the
    third 0.2 cell above with the opposite winding.  Every vertex sits in the interior of its cell.  -> (vertices, faces)."""
    i, j = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    base = np.stack([(i + 0.5) * cell, (j + 0.5) * cell, np.full(i.shape, 0.3 * cell)], -1).reshape(-1, 3)
    q = (i[:-1, :-1] * 3 + j[:-1, :-1]).reshape(-1)
    quad = np.concatenate([np.stack([q, q + 3, q + 4], 1), np.stack([q, q + 4, q + 1], 1)])
    v = np.concatenate([base, base + [0, 0, 0.1 * cell], base + [0, 0, 0.2 * cell]])
    faces = np.concatenate([quad, quad + 9, (quad + 18)[:, ::-1]])
    return v.astype(np.float32), faces.astype(np.int32)


def fan(n=300, cell=1.0, seed=11):
    """A fan inside one cell: a hub and n rim vertices (radius 0.3 cell, wavy in z) around the centre of the cell (1, 1, 1),
    n faces hub-rim-rim, and an outer ring of 8 vertices in the neighbouring cells joined to every 38th rim vertex by
    two faces each.  -> (vertices, faces)."""
    rng = np.random.default_rng(seed)
    c = np.array([1.5, 1.5, 1.5]) * cell
    t = 2 * np.pi * np.arange(n) / n
    rim = c + np.stack([0.3 * cell * np.cos(t), 0.3 * cell * np.sin(t), 0.05 * cell * np.sin(5 * t)], 1)
    rim += rng.uniform(-0.01, 0.01, size=rim.shape) * cell
    hub = c + [0, 0, 0.1 * cell]
    t8 = 2 * np.pi * (np.arange(8) + 0.5) / 8
    ring = c + np.stack([1.1 * cell * np.cos(t8), 1.1 * cell * np.sin(t8), np.zeros(8)], 1)
    v = np.concatenate([hub[None], rim, ring])
    r = 1 + np.arange(n)
    faces = [np.stack([np.zeros(n, np.int64), r, 1 + (np.arange(n) + 1) % n], 1)]
    o = 1 + n + np.arange(8)
    inner = 1 + (np.arange(8) * (n // 8)) % n
    faces.append(np.stack([inner, o, 1 + n + (np.arange(8) + 1) % 8], 1))
    faces.append(np.stack([inner, 1 + n + (np.arange(8) + 1) % 8, 1 + (inner - 1 + n // 8) % n], 1))
    return v.astype(np.float32), np.concatenate(faces).astype(np.int32)


def debris_with_nan(seed=3):
    """mesh_clean_ref's `debris` (two tetrahedra, three unreferenced vertices, two invalid faces) plus vertex 11 = NaN and
    a face (7, 8, 11) on it.  -> the mesh dict."""
    V, faces = cr.hand_made()["debris"]
    d = cr.with_attributes(V + 1, np.concatenate([faces, [[7, 8, 11]]]).astype(np.int32), seed)
    d["vertices"][11, 1] = np.nan
    return d


def random_strip(seed=0):
    """mesh_clean_ref.strip("random") with its seeded random positions in [-1, 1]^3: 8194 vertices, 8192 faces."""
    V, faces = cr.strip("random")
    return cr.with_attributes(V, faces, seed)


def sphere_distance(points):
    """The distance of every point to the nearest sphere surface of mesh_clean_ref.BLOBS (float64)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d = np.full(len(p), np.inf)
    for cx, cy, cz, r in cr.BLOBS:
        sd = np.sqrt(((p - [cx, cy, cz]) ** 2).sum(axis=1)) - r
        d = np.where(np.abs(sd) < np.abs(d), sd, d)
    return np.abs(d)


def position_tolerance(positions, cell):
    """2^-22 max(|coordinate|, cell) per component: the float64 system is conditioned at most 3 / reg + 1, so two
    implementations differ by about 1e-11 cell before the one float32 rounding, which may then fall either way."""
    return 2.0 ** -22 * np.maximum(np.abs(np.asarray(positions, np.float64)), float(cell))


NORMAL_TOLERANCE = 2.0 ** -22


def shared_cases():
    """name -> (mesh dict, cell, origin) for the meshes that need no extraction."""
    return dict(cube=(with_attributes(*cube(), seed=1), 0.5, (-0.25, -0.25, -0.25)),
                plane=(with_attributes(*plane_grid(), seed=2), 0.3, None),
                identity=(with_attributes(*cube(), seed=4), 0.1, None),
                debris=(debris_with_nan(), 0.5, None),
                sheets=(with_attributes(*sheets(0.5), seed=6), 0.5, (0.0, 0.0, 0.0)),
                fan=(with_attributes(*fan(300, 1.0), seed=7), 1.0, (0.0, 0.0, 0.0)),
                strip=(random_strip(), 0.25, None))
