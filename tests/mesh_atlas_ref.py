"""CPU restatement of mesh texturing (csrc/mesh_atlas.hip through mesh.atlas_layout / mesh.face_uvs / mesh.transfer_attributes
/ mesh.bake_atlas / mesh.sample_atlas), as include/gigs_hip.h states it under "Texturing meshes": the atlas of equal per-face
charts, the surface point of every texel, the closest point of a query on a given triangle as barycentric weights, and the
interpolation of per-vertex channels there.  Every float64 expression is written in the header's operation order and there is
no sqrt, so points, weights and channels are the kernels' bit for bit.  The search between the two kernels is
mesh_distance_ref.closest."""
import math

import numpy as np

import mesh_distance_ref as dr


# ---- the layout ------------------------------------------------------------------------------------------------------------
def atlas_layout(F, block=8, width=None):
    """-> dict(block, width, height, blocks_per_row, n_blocks)."""
    B, F = int(block), int(F)
    if B < 3:
        raise ValueError("block must be >= 3")
    n_blocks = (F + 1) // 2
    if width is None:
        width = 1
        while width < B + 1 or (width // (B + 1)) * (width // B) < n_blocks:
            width *= 2
    width = int(width)
    if width < B + 1:
        raise ValueError("width below one block")
    per_row = width // (B + 1)
    return dict(block=B, width=width, height=-(-n_blocks // per_row) * B, blocks_per_row=per_row, n_blocks=n_blocks)


def owner(B):
    """[B, B + 1] (row j, column i): the half that owns each texel of a block."""
    j, i = np.meshgrid(np.arange(B), np.arange(B + 1), indexing="ij")
    return (i + j > B - 1).astype(np.int64)


def corners(B):
    """[2, 3, 2]: the texel (i, j) at whose centre each corner of each half sits."""
    return np.array([[(0, 0), (B - 2, 0), (0, B - 2)], [(B, B - 1), (2, B - 1), (B, 1)]], np.int64)


def face_uvs(F, layout):
    """[F,3,2] float32: (X / W, 1 - Y / H) at the centres of the corner texels."""
    B, W, H, per_row = layout["block"], layout["width"], layout["height"], layout["blocks_per_row"]
    f = np.arange(int(F), dtype=np.int64)
    b, half = f // 2, f % 2
    c = corners(B)[half]  # [F,3,2]
    X = ((b % per_row) * (B + 1))[:, None] + c[..., 0] + 0.5
    Y = ((b // per_row) * B)[:, None] + c[..., 1] + 0.5
    if F == 0:
        return np.zeros((0, 3, 2), np.float32)
    return np.stack([X / float(W), 1.0 - Y / float(H)], -1).astype(np.float32)


def atlas_points(vertices, faces, layout):
    """-> dict(points [Q,3] float32, bary [Q,2] float32, texel_face [Q] int32, dest [Q] int64), block-major."""
    B, W, per_row, nb = layout["block"], layout["width"], layout["blocks_per_row"], layout["n_blocks"]
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    F = len(fc)
    q = np.arange(nb * B * (B + 1), dtype=np.int64)
    blk, r = q // (B * (B + 1)), q % (B * (B + 1))
    j, i = r // (B + 1), r % (B + 1)
    half = (i + j > B - 1).astype(np.int64)
    f = 2 * blk + half
    li, lj = np.where(half == 1, B - i, i), np.where(half == 1, B - 1 - j, j)
    w1, w2 = li.astype(np.float64) / float(B - 2), lj.astype(np.float64) / float(B - 2)
    w0 = (1.0 - w1) - w2
    slot = f < F
    idx = np.zeros((len(q), 3), np.int64)
    idx[slot] = fc[f[slot]]
    ok = slot & ((idx >= 0) & (idx < len(v))).all(axis=1)
    P = np.zeros((len(q), 3, 3))
    P[ok] = v[idx[ok]]
    ok = ok & np.isfinite(P).all(axis=(1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        pts = (w0[:, None] * P[:, 0] + w1[:, None] * P[:, 1]) + w2[:, None] * P[:, 2]
    pts = np.where(ok[:, None], pts, np.nan).astype(np.float32)
    x, y = (blk % per_row) * (B + 1) + i, (blk // per_row) * B + j
    return dict(points=pts, bary=np.stack([w1, w2], 1).astype(np.float32), texel_face=np.where(slot, f, -1).astype(np.int32),
                dest=np.where(ok, y * W + x, -1).astype(np.int64))


# ---- closest point on a given triangle ---------------------------------------------------------------------------------------
def _segment(p, a, b):
    """-> (d^2, s) of mesh_distance_ref._segment_d2, the parameter kept."""
    ab, ap = b - a, p - a
    t, den = dr._dot(ap, ab), dr._dot(ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = t / den
    s = np.where(t <= 0, 0.0, np.where(t >= den, 1.0, s))
    q = ap - s[..., None] * ab
    bp = p - b
    return np.where(t <= 0, dr._dot(ap, ap), np.where(t >= den, dr._dot(bp, bp), dr._dot(q, q))), s


def triangle_weights(p, P, idx):
    """Points p [N,3] float64, triangles P [N,3,3] float64 with vertex indices idx [N,3] -> (w [N,3] float64, d2 [N])."""
    N = len(p)
    d2 = np.full(N, np.inf)
    w = np.zeros((N, 3))
    w[:, 0] = 1.0
    for j, k in ((0, 1), (1, 2), (2, 0)):
        swap = idx[:, j] > idx[:, k]
        a, b = np.where(swap[:, None], P[:, k], P[:, j]), np.where(swap[:, None], P[:, j], P[:, k])
        s2, s = _segment(p, a, b)
        wj, wk = np.where(swap, s, 1.0 - s), np.where(swap, 1.0 - s, s)
        win = s2 < d2
        cand = np.zeros((N, 3))
        cand[:, j], cand[:, k] = wj, wk
        w = np.where(win[:, None], cand, w)
        d2 = np.where(win, s2, d2)
    p0, p1, p2 = P[:, 0], P[:, 1], P[:, 2]
    n = dr._cross(p1 - p0, p2 - p0)
    f0 = dr._dot(dr._cross(p1 - p0, p - p0), n)
    f1 = dr._dot(dr._cross(p2 - p1, p - p1), n)
    f2 = dr._dot(dr._cross(p0 - p2, p - p2), n)
    h = dr._dot(p - p0, n)
    S = (f0 + f1) + f2
    with np.errstate(invalid="ignore", divide="ignore"):
        plane = h * h / dr._dot(n, n)
        inner = np.stack([f1 / S, f2 / S, f0 / S], 1)
    win = (f0 >= 0) & (f1 >= 0) & (f2 >= 0) & (plane < d2) & (S > 0)
    return np.where(win[:, None], inner, w), np.where(win, plane, d2)


def transfer(points, face, vertices, faces, values, dest=None, plane=0):
    """gigs_mesh_transfer.  -> dict(out ([N,C], or [C,plane] with dest; zero where nothing is stored), bary [N,2] float32,
    coverage [plane] uint8 (with dest), transferred, skipped, w [N,3] float64, done [N] bool)."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    fc = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.asarray(values, np.float32)
    a = a.reshape(len(v), -1).astype(np.float64)
    face = np.asarray(face, np.int64)
    N, C = len(p), a.shape[1]
    d = np.arange(N, dtype=np.int64) if dest is None else np.asarray(dest, np.int64)
    assert ((face >= -1) & (face < len(fc))).all() and (d >= -1).all()
    go = (face >= 0) & (d >= 0)
    idx = np.zeros((N, 3), np.int64)
    idx[go] = fc[face[go]]
    assert ((idx >= 0) & (idx < max(len(v), 1))).all()
    P = np.zeros((N, 3, 3))
    P[go] = v[idx[go]]
    go = go & np.isfinite(p).all(axis=1) & np.isfinite(P).all(axis=(1, 2))
    w = np.zeros((N, 3))
    w[go], _ = triangle_weights(p[go], P[go], idx[go])
    A = np.zeros((N, 3, C))
    A[go] = a[idx[go]]
    with np.errstate(invalid="ignore", over="ignore"):
        val = ((w[:, 0, None] * A[:, 0] + w[:, 1, None] * A[:, 1]) + w[:, 2, None] * A[:, 2]).astype(np.float32)
    bary = np.zeros((N, 2), np.float32)
    bary[go] = w[go][:, 1:].astype(np.float32)
    res = dict(bary=bary, transferred=int(go.sum()), skipped=int(N - go.sum()), w=w, done=go)
    if dest is None:
        out = np.zeros((N, C), np.float32)
        out[go] = val[go]
    else:
        out = np.zeros((C, int(plane)), np.float32)
        out[:, d[go]] = val[go].T
        cov = np.zeros(int(plane), np.uint8)
        cov[d[go]] = 1
        res["coverage"] = cov
    res["out"] = out
    return res


def channels(mesh, occlusion=None):
    """[V,9] float32: albedo, (occlusion, roughness, metallic), normal -- the channel table of mesh.bake_atlas."""
    V = len(mesh["vertices"])
    o = np.ones(V, np.float32) if occlusion is None else np.asarray(occlusion, np.float32).reshape(V)
    return np.concatenate([mesh["albedo"].reshape(V, 3), o[:, None], mesh["roughness"].reshape(V, 1),
                           mesh["metallic"].reshape(V, 1), mesh["normals"].reshape(V, 3)], axis=1).astype(np.float32)


def bake_atlas(dst, src, block=8, width=None, occlusion=None, max_distance=None, cell=None, stride=1):
    """mesh.bake_atlas on mesh dicts: the points restatement, mesh_distance_ref.closest, the transfer restatement.
    `stride` thins the texels that are searched (the others stay unbaked): -> dict(layout, planes [9,H,W], coverage [H,W],
    searched [Q] bool, dest, closest: mesh_distance_ref.closest's answer for the searched texels, transferred, skipped)."""
    lay = atlas_layout(len(dst["faces"]), block, width)
    pts = atlas_points(dst["vertices"], dst["faces"], lay)
    Q = len(pts["dest"])
    searched = np.zeros(Q, bool)
    searched[::stride] = True
    near = dr.closest(pts["points"][searched], src["vertices"], src["faces"], cell=cell, max_distance=max_distance)
    face = np.full(Q, -1, np.int64)
    face[searched] = near["face"]
    W, H = lay["width"], lay["height"]
    t = transfer(pts["points"], face, src["vertices"], src["faces"], channels(src, occlusion), dest=pts["dest"], plane=W * H)
    return dict(layout=lay, planes=t["out"].reshape(9, H, W), coverage=t["coverage"].reshape(H, W), searched=searched,
                dest=pts["dest"], closest=near, transferred=t["transferred"], skipped=t["skipped"], bary=t["bary"], face=face)


# ---- looking the atlas up ----------------------------------------------------------------------------------------------------
def sample_atlas(planes, layout, face, bary):
    """[N,C] float64: the bilinear lookup at uv = w0 uv0 + w1 uv1 + w2 uv2 (float64 on face_uvs' float32 corners); the texel
    coordinates are x = u W - 1/2, y = (1 - v) H - 1/2, taps clamped to the image."""
    planes = np.asarray(planes, np.float64)
    C, H, W = planes.shape
    face = np.asarray(face, np.int64)
    uv = face_uvs(int(face.max()) + 1 if len(face) else 0, layout).astype(np.float64)[face]
    b = np.asarray(bary, np.float32).astype(np.float64)
    w1, w2 = b[:, 0], b[:, 1]
    w0 = (1.0 - w1) - w2
    u = (w0 * uv[:, 0, 0] + w1 * uv[:, 1, 0]) + w2 * uv[:, 2, 0]
    v = (w0 * uv[:, 0, 1] + w1 * uv[:, 1, 1]) + w2 * uv[:, 2, 1]
    x, y = u * W - 0.5, (1.0 - v) * H - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xa, xb = np.clip(x0, 0, W - 1).astype(np.int64), np.clip(x0 + 1, 0, W - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, H - 1).astype(np.int64), np.clip(y0 + 1, 0, H - 1).astype(np.int64)
    top = (1.0 - fx) * planes[:, ya, xa] + fx * planes[:, ya, xb]
    bot = (1.0 - fx) * planes[:, yb, xa] + fx * planes[:, yb, xb]
    return ((1.0 - fy) * top + fy * bot).T


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------
BLOCKS = (3, 4, 8)


def voronoi_queries(P):
    """Points in every Voronoi region of the triangle P [3,3] (float64): beyond each vertex, beyond each edge, and over the
    interior on both sides of the plane; each also in the plane.  -> [n,3] float32."""
    p0, p1, p2 = P
    n = np.cross(p1 - p0, p2 - p0)
    scale = math.sqrt(max(float(np.dot(p1 - p0, p1 - p0)), float(np.dot(p2 - p0, p2 - p0))))
    nn = float(np.dot(n, n))
    up = n / math.sqrt(nn) * scale if nn > 0 else np.array([0.0, 0.0, scale])
    c = (p0 + p1 + p2) / 3.0
    pts = []
    for a, b, o in ((p0, p1, p2), (p1, p2, p0), (p2, p0, p1)):
        pts.append(a + 0.7 * (a - c))              # beyond the vertex a
        mid, e = 0.5 * (a + b), b - a
        out = (mid - o) - (np.dot(mid - o, e) / np.dot(e, e)) * e  # in the plane, square to the edge, away from o
        out = out / math.sqrt(float(np.dot(out, out))) * scale
        pts.append(mid + 0.6 * out)                # beyond the edge a b
        pts.append(0.25 * a + 0.75 * b + 0.01 * out)
    pts += [c, 0.6 * p0 + 0.3 * p1 + 0.1 * p2, 0.1 * p0 + 0.2 * p1 + 0.7 * p2, p0, p1, p2, 0.5 * (p0 + p1)]
    pts = np.array(pts)
    return np.concatenate([pts, pts + 0.4 * up, pts - 0.9 * up]).astype(np.float32)


TRIANGLES = {
    "right": ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [0, 1, 2]),
    "tilted": ([[0.2, -0.3, 0.1], [1.4, 0.5, 0.9], [-0.3, 1.1, 0.6]], [7, 3, 5]),   # the index order turns two edges round
    "obtuse": ([[0, 0, 0], [4, 0, 0], [3.5, 0.5, 0.25]], [2, 1, 0]),
    "sliver": ([[0, 0, 0], [1, 0, 0], [0.5, 1e-4, 0]], [0, 2, 1]),
}


def voronoi_mesh():
    """TRIANGLES as one mesh (each triangle moved to a place of its own, its vertex indices in the table's order) with the
    Voronoi queries of every triangle and the face each is meant for.  -> (vertices [32,3], faces [4,3], points, face)."""
    v = np.zeros((8 * len(TRIANGLES), 3), np.float32)
    faces, points, face = [], [], []
    for k, name in enumerate(sorted(TRIANGLES)):
        P, idx = TRIANGLES[name]
        P = (np.asarray(P, np.float64) + [10.0 * k, 0.0, 0.0]).astype(np.float32)
        idx = np.asarray(idx) + 8 * k
        v[idx] = P
        faces.append(idx)
        q = voronoi_queries(P.astype(np.float64))
        points.append(q)
        face.append(np.full(len(q), k))
    return v, np.asarray(faces, np.int32), np.concatenate(points), np.concatenate(face).astype(np.int32)
