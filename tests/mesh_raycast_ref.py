"""CPU restatement of ray casting and occlusion baking (csrc/mesh_raycast.hip through mesh.raycast / mesh.bake_occlusion), as
include/gigs_hip.h states them under "Baking occlusion": the edge functions walked from the lower vertex index, the inside
test, the grazing guard, t, the box test of the hit point, the (t, face) minimum, the slab traversal of the triangle grid
with its slack, the default direction table, the frame of Duff et al. and the per-vertex hit count.  Every float64
expression is written in the header's operation order and there is no sqrt or transcendental on the device side, so t,
bary and the hit counts are the kernel's bit for bit.  raycast() walks the grid the way the kernel does, brute_force()
tests every usable face: the CPU tests hold the two against each other."""
import math

import numpy as np

import mesh_distance_ref as dr
from mesh_distance_ref import _corners, _cross, _dot, build_grid, cell_of, mix64  # noqa: F401

GUARD = 2.0 ** -40   # a face is a candidate only if dn^2 > GUARD (d.d)(n.n)
SLACK = 2.0 ** -26   # sigma = SLACK (M + max |o_a|)
NORMAL_BAND = 2.0 ** -10


# ---- ray - triangle --------------------------------------------------------------------------------------------------------
def ray_triangle(o, d, sigma, tmax, P, idx):
    """Rays (o, d [...,3] float64, sigma [...]) against triangles P [...,3,3] with vertex indices idx [...,3].
    -> (accepted bool, t, w1, w2, sum), float64, broadcast."""
    a = [P[..., k, :] - o for k in range(3)]
    w = []
    for j, k in ((1, 2), (2, 0), (0, 1)):
        fwd = idx[..., j] < idx[..., k]
        lo, hi = np.where(fwd[..., None], a[j], a[k]), np.where(fwd[..., None], a[k], a[j])
        s = _dot(d, _cross(lo, hi))
        w.append(np.where(fwd, s, -s))
    pos = (w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)
    neg = (w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0)
    ok = (pos | neg) & ~(pos & neg)
    n = _cross(P[..., 1, :] - P[..., 0, :], P[..., 2, :] - P[..., 0, :])
    dn = _dot(d, n)
    dd = _dot(d, d)
    ok = ok & (dn * dn > GUARD * (dd * _dot(n, n)))
    with np.errstate(invalid="ignore", divide="ignore"):
        t = _dot(a[0], n) / dn
        ok = ok & (t >= 0) & (t <= tmax)
        x = o + t[..., None] * d
        inside = (x >= P.min(axis=-2) - sigma[..., None]) & (x <= P.max(axis=-2) + sigma[..., None])
    ok = ok & inside.all(axis=-1)
    return ok, t, w[1], w[2], (w[0] + w[1]) + w[2]


def mesh_scale(vertices, faces):
    """M: the largest |coordinate| of a corner of a usable face (0 without one)."""
    areas, _ = dr.face_areas(vertices, faces)
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    corners = v[f[areas > 0].reshape(-1)]
    return float(np.abs(corners.astype(np.float64)).max()) if len(corners) else 0.0


def _rays(origins, directions):
    """float64 [N,3] each, and the valid ones.  float32 arrays are the API's rays, float64 ones the bake's."""
    o, d = np.asarray(origins), np.asarray(directions)
    if o.dtype != np.float64:
        o = np.asarray(o, np.float32)
    if d.dtype != np.float64:
        d = np.asarray(d, np.float32)
    o, d = o.reshape(-1, 3).astype(np.float64), d.reshape(-1, 3).astype(np.float64)
    valid = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
    return o, d, valid


def _finish(N, valid, best_t, best_f, w1, w2, sm, **more):
    hit = best_f >= 0
    with np.errstate(invalid="ignore", divide="ignore"):
        bary = np.where(hit[:, None], np.stack([w1 / sm, w2 / sm], 1), 0.0)
    out = dict(t=np.where(hit, best_t, np.inf).astype(np.float32), t64=best_t, face=best_f.astype(np.int32),
               bary=bary.astype(np.float32), hits=int(hit.sum()), rays_invalid=int(N - valid.sum()))
    out.update(more)
    return out


def brute_force(origins, directions, vertices, faces, t_max=None):
    """Every usable face against every ray.  -> raycast()'s dict."""
    o, d, valid = _rays(origins, directions)
    N = len(o)
    tmax = np.inf if t_max is None else float(t_max)
    areas, _ = dr.face_areas(vertices, faces)
    use = np.nonzero(areas > 0)[0]
    best_t, best_f = np.full(N, np.inf), np.full(N, -1, np.int64)
    w1, w2, sm = np.zeros(N), np.zeros(N), np.ones(N)
    if len(use) and N:
        M = mesh_scale(vertices, faces)
        _, P = _corners(vertices, faces)
        idx = np.asarray(faces, np.int64).reshape(-1, 3)
        sigma = SLACK * (M + np.abs(o).max(axis=1))
        rows = np.nonzero(valid)[0]
        step = max(1, 1_000_000 // len(use))
        for s in range(0, len(rows), step):
            r = rows[s:s + step]
            ok, t, a, b, c = ray_triangle(o[r][:, None, :], d[r][:, None, :], sigma[r][:, None], tmax, P[use][None],
                                          idx[use][None])
            t = np.where(ok, t, np.inf)
            k = np.argmin(t, axis=1)  # the first of equal minima: the smallest face index
            j = np.arange(len(r))
            got = ok[j, k]
            rr = r[got]
            best_t[rr], best_f[rr] = t[j, k][got], use[k][got]
            w1[rr], w2[rr], sm[rr] = a[j, k][got], b[j, k][got], c[j, k][got]
    return _finish(N, valid, best_t, best_f, w1, w2, sm)


def raycast(origins, directions, vertices, faces, t_max=None, cell=None, grid=None):
    """The kernel's traversal.  -> dict(t float32, t64, face int32 (-1: a miss or an invalid ray), bary float32 [N,2], hits,
    rays_invalid, cells: cell headers read, tests: ray-triangle tests, slabs: slabs entered, grid)."""
    o, d, valid = _rays(origins, directions)
    N = len(o)
    tmax = np.inf if t_max is None else float(t_max)
    best_t, best_f = np.full(N, np.inf), np.full(N, -1, np.int64)
    w1, w2, sm = np.zeros(N), np.zeros(N), np.ones(N)
    g = build_grid(vertices, faces, cell) if grid is None else grid
    cells = tests = slabs = 0
    if g is not None and valid.any():
        lo, cell, G = g["lo"].astype(np.float64), g["cell"], np.asarray(g["G"], np.int64)
        M = mesh_scale(vertices, faces)
        _, P = _corners(vertices, faces)
        idx = np.asarray(faces, np.int64).reshape(-1, 3)
        q = np.nonzero(valid)[0]
        ad = np.abs(d[q])
        A = np.where((ad[:, 0] >= ad[:, 1]) & (ad[:, 0] >= ad[:, 2]), 0, np.where(ad[:, 1] >= ad[:, 2], 1, 2))
        U, W = np.where(A == 2, 0, A + 1), np.where(A == 0, 2, A - 1)
        row = np.arange(len(q))
        take = lambda x, ax: x[row, ax]  # noqa: E731
        oA, dA, oU, dU, oW, dW = take(o[q], A), take(d[q], A), take(o[q], U), take(d[q], U), take(o[q], W), take(d[q], W)
        stride = np.array([1, G[0], G[0] * G[1]], np.int64)
        sigma = SLACK * (M + np.abs(o[q]).max(axis=1))
        s2, s3 = 2.0 * sigma, 3.0 * sigma
        up = dA > 0
        step = np.where(up, 1, -1)
        cell_ax = lambda x, ax: np.where(ax == 0, cell_of(x, lo[0], cell, G[0]), np.where(  # noqa: E731
            ax == 1, cell_of(x, lo[1], cell, G[1]), cell_of(x, lo[2], cell, G[2])))
        k = cell_ax(np.where(up, oA - s3, oA + s3), A)
        live = np.ones(len(q), bool)
        for _ in range(int(G.max())):
            live &= (k >= 0) & (k < G[A])
            if not live.any():
                break
            ta = ((lo[A] + k.astype(np.float64) * cell - s2) - oA) / dA
            tb = ((lo[A] + (k + 1).astype(np.float64) * cell + s2) - oA) / dA
            tn, tf = np.minimum(ta, tb), np.maximum(ta, tb)
            behind = tf < 0
            live &= behind | ~((tn > tmax) | (best_t[q] < tn))
            now = np.nonzero(live & ~behind)[0]
            slabs += len(now)
            if len(now):
                tn_, tf_ = np.maximum(tn[now], 0.0), np.minimum(tf[now], tmax)
                un, uf = oU[now] + tn_ * dU[now], oU[now] + tf_ * dU[now]
                wn, wf = oW[now] + tn_ * dW[now], oW[now] + tf_ * dW[now]
                u0, u1 = cell_ax(np.minimum(un, uf) - s2[now], U[now]), cell_ax(np.maximum(un, uf) + s2[now], U[now])
                w0, w1_ = cell_ax(np.minimum(wn, wf) - s2[now], W[now]), cell_ax(np.maximum(wn, wf) + s2[now], W[now])
                cq, cc = [], []
                for dw in range(int((w1_ - w0).max()) + 1):
                    for du in range(int((u1 - u0).max()) + 1):
                        m = (u0 + du <= u1) & (w0 + dw <= w1_)
                        cq.append(now[m])
                        cc.append(k[now][m] * stride[A[now][m]] + (u0[m] + du) * stride[U[now][m]]
                                  + (w0[m] + dw) * stride[W[now][m]])
                cq, cc = np.concatenate(cq), np.concatenate(cc)
                cells += len(cc)
                start, n = g["cell_start"][cc], g["cell_start"][cc + 1] - g["cell_start"][cc]
                total = int(n.sum())
                if total:
                    rep = np.repeat(np.arange(len(cc)), n)
                    f = g["pair_face"][start[rep] + (np.arange(total) - np.repeat(np.cumsum(n) - n, n))]
                    r = cq[rep]  # rows of q
                    tests += total
                    ok, t, a, b, c = ray_triangle(o[q[r]], d[q[r]], sigma[r], tmax, P[f], idx[f])
                    r, f, t, a, b, c = r[ok], f[ok], t[ok], a[ok], b[ok], c[ok]
                    order = np.lexsort((f, t, r))
                    r, f, t, a, b, c = r[order], f[order], t[order], a[order], b[order], c[order]
                    first = np.ones(len(r), bool)
                    first[1:] = r[1:] != r[:-1]
                    r, f, t, a, b, c = r[first], f[first], t[first], a[first], b[first], c[first]
                    qq = q[r]
                    better = (t < best_t[qq]) | ((t == best_t[qq]) & (f < best_f[qq]))
                    qq = qq[better]
                    best_t[qq], best_f[qq] = t[better], f[better]
                    w1[qq], w2[qq], sm[qq] = a[better], b[better], c[better]
            k = k + step
    return _finish(N, valid, best_t, best_f, w1, w2, sm, cells=cells, tests=tests, slabs=slabs, grid=g)


# ---- the bake --------------------------------------------------------------------------------------------------------------
def direction_table(R, K):
    """[K,R,3] float32: a cosine-weighted spiral lattice of R points on the hemisphere z >= 0 (point i: u = (i + 1/2) / R,
    radius sqrt(u), azimuth i times the golden angle, z = sqrt(1 - u)), turned about z by 2 pi k / K."""
    i = np.arange(R, dtype=np.float64)
    u = (i + 0.5) / R
    r, z = np.sqrt(u), np.sqrt(1.0 - u)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    phi = i[None, :] * golden + (2.0 * math.pi * np.arange(K, dtype=np.float64) / K)[:, None]
    return np.stack([r[None] * np.cos(phi), r[None] * np.sin(phi), np.broadcast_to(z, phi.shape)], -1).astype(np.float32)


def frame(n):
    """The branch-free orthonormal basis of Duff et al. around n [...,3] float64 -> (T, B)."""
    sign = np.copysign(1.0, n[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        a = -1.0 / (sign + n[..., 2])
    b = (n[..., 0] * n[..., 1]) * a
    T = np.stack([1.0 + ((sign * n[..., 0]) * n[..., 0]) * a, sign * b, (-sign) * n[..., 0]], -1)
    B = np.stack([b, sign + (n[..., 1] * n[..., 1]) * a, -n[..., 1]], -1)
    return T, B


def rotation_of(seed, v, K):
    with np.errstate(over="ignore"):
        z = (np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) << np.uint64(32)) + np.asarray(v, np.uint64)
    return (mix64(z) % np.uint64(K)).astype(np.int64)


def bake_defaults(grid, max_distance=None, bias=None):
    """max_distance = 0.1 of the longest axis of the grid's box, bias = 1e-3 max_distance (conventions)."""
    if max_distance is None:
        max_distance = 0.1 * max(G * grid["cell"] for G in grid["G"]) if grid is not None else 0.0
    if bias is None:
        bias = 1e-3 * max_distance
    return float(max_distance), float(bias)


def bake(vertices, faces, normals, directions, max_distance=None, bias=None, seed=0, cell=None, grid=None, subset=None,
         brute=False):
    """-> dict(hits [V] int (-1 for a vertex outside `subset`), occlusion [V] float32, no_normal, hits_total, rotation [V],
    valid [V]).  `directions`: the [K,R,3] float32 table.  `brute`: brute_force() in place of the traversal."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    nrm = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    table = np.asarray(directions, np.float32).astype(np.float64)
    K, R = table.shape[:2]
    V = len(v)
    g = build_grid(vertices, faces, cell) if grid is None else grid
    max_distance, bias = bake_defaults(g, max_distance, bias)
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = _dot(nrm, nrm)
        valid = np.isfinite(v).all(axis=1) & (n2 >= 1.0 - NORMAL_BAND) & (n2 <= 1.0 + NORMAL_BAND)
    rot = rotation_of(seed, np.arange(V), K)
    rows = np.nonzero(valid)[0] if subset is None else np.asarray(subset)[valid[np.asarray(subset)]]
    hits = np.full(V, -1, np.int64)
    if subset is None:
        hits[~valid] = 0
    else:
        hits[np.asarray(subset)[~valid[np.asarray(subset)]]] = 0
    if len(rows):
        if g is None:
            hits[rows] = 0
        else:
            n = nrm[rows]
            T, B = frame(n)
            x, y, z = (table[rot[rows]][..., c] for c in range(3))  # [rows, R]
            d = (x[..., None] * T[:, None, :] + y[..., None] * B[:, None, :]) + z[..., None] * n[:, None, :]
            o = np.broadcast_to((v[rows] + bias * n)[:, None, :], d.shape)
            if brute:
                got = brute_force(o.reshape(-1, 3), d.reshape(-1, 3), vertices, faces, max_distance)
            else:
                got = raycast(o.reshape(-1, 3), d.reshape(-1, 3), vertices, faces, max_distance, grid=g)
            hits[rows] = (got["face"].reshape(len(rows), R) >= 0).sum(axis=1)
    occ = np.where(hits >= 0, (R - np.maximum(hits, 0)).astype(np.float64) / float(R), np.nan).astype(np.float32)
    return dict(hits=hits, occlusion=occ, no_normal=int((~valid).sum() if subset is None else (~valid[np.asarray(subset)]).sum()),
                hits_total=int(np.maximum(hits, 0).sum()), rotation=rot, valid=valid, max_distance=max_distance, bias=bias,
                grid=g)


# ---- the inputs the tests share --------------------------------------------------------------------------------------------
CELL_FACTORS = (0.5, 1.0, 3.0, 1e9)  # of the default cell; the last gives the one-cell grid: brute force through the traversal


def cell_sizes(vertices, faces):
    g = build_grid(vertices, faces)
    return [float(np.float32(g["cell"] * k)) for k in CELL_FACTORS]


def ray_sets(vertices, faces, grid, stride=None, n_random=1024):
    """name -> (origins, directions) [n,3] float32: hash-random rays in a box of twice the extent; rays from outside aimed
    at every vertex, edge midpoint and face centroid; axis-parallel rays; rays in cell planes and through cell corners; rays
    that start inside the grid, on its boundary and far outside; rays pointing away; invalid rays.  The aimed rays keep
    every stride-th target (mesh_distance_ref.default_stride)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if stride is None:
        stride = dr.default_stride(f)
    lo = grid["lo"].astype(np.float64)
    hi = lo + np.asarray(grid["G"]) * grid["cell"]
    centre, ext = 0.5 * (lo + hi), hi - lo
    ext = np.where(ext > 0, ext, ext.max())
    i = np.arange(n_random, dtype=np.uint64)
    ro = centre + (np.stack([dr.uniform(41, i, k) for k in range(3)], 1) - 0.5) * 2.0 * ext
    rd = np.stack([dr.uniform(42, i, k) for k in range(3)], 1) - 0.5
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    fv = f[ok]
    P = v.astype(np.float64)[fv] if len(fv) else np.zeros((0, 3, 3))
    fin = np.isfinite(P).all(axis=(1, 2))
    P = P[fin]
    targets = np.concatenate([v[np.isfinite(v).all(axis=1)].astype(np.float64), 0.5 * (P[:, 0] + P[:, 1]), 0.5 * (P[:, 1] + P[:, 2]),
                              0.5 * (P[:, 2] + P[:, 0]), P.mean(axis=1)])[::stride]
    j = np.arange(len(targets), dtype=np.uint64)
    away = np.stack([dr.uniform(43, j, k) for k in range(3)], 1) - 0.5
    away = away / np.abs(away).max(axis=1, keepdims=True)
    ao = centre + away * 1.5 * ext
    ad = targets - ao.astype(np.float32).astype(np.float64)
    axes = np.concatenate([np.eye(3), -np.eye(3)])
    xo = np.concatenate([np.repeat((centre + (np.stack([dr.uniform(44, np.arange(32, dtype=np.uint64), k) for k in range(3)], 1)
                                             - 0.5) * ext)[:, None, :], 6, 1).reshape(-1, 3)])
    xo = xo - np.tile(axes, (32, 1)) * 1.5 * ext
    xd = np.tile(axes, (32, 1))
    ks = [sorted({0, 1, G // 2, G}) for G in grid["G"]]
    corners = np.array([[lo[0] + kx * grid["cell"], lo[1] + ky * grid["cell"], lo[2] + kz * grid["cell"]]
                        for kx in ks[0] for ky in ks[1] for kz in ks[2]], np.float64)
    pd = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [0, 1, -1], [1, 1, 1], [-1, 1, 1], [1, -2, 0]], np.float64)
    po = np.repeat(corners, len(pd), 0) - np.tile(pd, (len(corners), 1)) * 0.75 * ext.max()
    pdd = np.tile(pd, (len(corners), 1))
    c8 = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    so = np.concatenate([np.repeat(centre[None], 8, 0), centre + 0.5 * ext * c8, centre + 50.0 * ext.max() * c8])
    sd = np.concatenate([c8 + np.array([0.25, -0.125, 0.0625]), -c8 + np.array([0.03125, 0.0625, -0.125]),
                         -c8 + np.array([0.001, -0.002, 0.003])])
    wo, wd = centre + 1.5 * ext * c8, c8 + np.array([0.125, 0.25, 0.0625])
    bo = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]) + centre
    bd = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0], [np.nan, 1, 0], [0, -np.inf, 1]], np.float64)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(random=(f32(ro), f32(rd)), aimed=(f32(ao), f32(ad)), axis=(f32(xo), f32(xd)), planes=(f32(po), f32(pdd)),
                starts=(f32(so), f32(sd)), away=(f32(wo), f32(wd)), bad=(f32(bo), f32(bd)))


def box_interior(n=4):
    """mesh_simplify_ref.cube(n) (closed, shared vertices merged) seen from inside: every vertex carries the normalised sum of
    the INWARD normals of the sides it lies on, so vertex + bias normal is strictly inside.  -> (vertices, faces, normals)."""
    import mesh_simplify_ref as sr
    v, f = sr.cube(n)
    v = np.asarray(v, np.float64)
    nrm = (v == 0).astype(np.float64) - (v == v.max()).astype(np.float64)
    nrm = nrm / np.sqrt((nrm ** 2).sum(axis=1, keepdims=True))
    return v.astype(np.float32), np.asarray(f, np.int32), nrm.astype(np.float32)


def crease(n=4, size=64.0):
    """Two quads of `size` at a right angle, n x n cells each: the floor z = 0 (x in [0, size], normal +z) and the wall x = 0
    (z in [0, size], normal +x).  The crease row x = z = 0 belongs to the floor (and a copy of it to the wall).  -> (vertices, faces, normals, crease rows)."""
    lin = np.linspace(0.0, size, n + 1)
    a, b = np.meshgrid(lin, lin, indexing="ij")
    floor = np.stack([a, b, np.zeros_like(a)], -1).reshape(-1, 3)     # x = a, y = b
    wall = np.stack([np.zeros_like(a), b, a], -1).reshape(-1, 3)      # z = a, y = b
    ij = np.arange(n)
    i, j = np.meshgrid(ij, ij, indexing="ij")
    c = (i * (n + 1) + j).reshape(-1)
    quad = np.concatenate([np.stack([c, c + n + 1, c + n + 2], 1), np.stack([c, c + n + 2, c + 1], 1)])
    v = np.concatenate([floor, wall]).astype(np.float32)
    f = np.concatenate([quad, quad + len(floor)]).astype(np.int32)
    nrm = np.concatenate([np.repeat([[0.0, 0.0, 1.0]], len(floor), 0), np.repeat([[1.0, 0.0, 0.0]], len(wall), 0)]).astype(np.float32)
    rows = np.arange(1, n)  # floor vertices with x = 0, y strictly inside
    # Their normal leans 0.01 rad away from the wall: with the floor's own normal the origin vertex + bias normal would lie
    # IN the wall's plane and every ray would meet the wall at t = 0, which 0 <= t accepts.
    nrm[rows] = np.array([math.sin(0.01), 0.0, math.cos(0.01)], np.float32)
    return v, f, nrm, rows
