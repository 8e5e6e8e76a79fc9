"""CPU restatement of mesh comparison (csrc/mesh_distance.hip through mesh.sample_surface / mesh.closest_point /
mesh.distance), as include/gigs_hip.h states it under "Comparing meshes": usable faces and their float64 areas, the counter
hash, the stratified area-weighted samples, the triangle grid with its conservative cell ranges, the float64 point-triangle
distance with its tie rule, and the expanding-shell search with its lower bound L(r).  Every float64 expression is written
in the header's operation order, so hash, barycentrics, sample points and d^2 are the kernel's bit for bit; the distance
differs from it by a float64 sqrt and one float32 rounding at most.  closest() searches the grid the way the kernel does,
brute_force() tests every usable face: the CPU tests hold the two against each other."""
import math

import numpy as np

AMBIGUOUS = 2.0 ** -40       # of A around a boundary of the cumulative areas
TIE = 2.0 ** -40             # relative gap of the two best d^2 below which the face is not compared
GRID_AXIS = 256
SHRINK = 1.0 - 2.0 ** -40    # the relative part of the slack on L(r)


# ---- usable faces, areas ---------------------------------------------------------------------------------------------------
def _corners(vertices, faces):
    """-> (in_range [F] bool, P [F,3,3] float64 with zeros where an index is out of range)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(axis=1)
    P = np.zeros((len(f), 3, 3))
    P[ok] = v[f[ok]]
    return ok, P


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def face_areas(vertices, faces):
    """-> (areas [F] float64, 0 for an unusable face; the number of unusable faces)."""
    ok, P = _corners(vertices, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = ok & np.isfinite(P).all(axis=(1, 2))
        n = _cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        length = np.sqrt(_dot(n, n))
        ok = ok & (length > 0)
    areas = np.where(ok, length * 0.5, 0.0)
    return areas, int((~ok).sum())


# ---- the counter hash ------------------------------------------------------------------------------------------------------
def mix64(z):
    """The splitmix64 finaliser on uint64 arrays."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def uniform(seed, i, k):
    """u(i, k) in [0, 1): mix64((seed 2^32 + i) 4 + k) >> 11, times 2^-53 (all modulo 2^64)."""
    with np.errstate(over="ignore"):
        x = ((np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) << np.uint64(32)) + np.asarray(i, np.uint64)) * np.uint64(4) + np.uint64(k)
    return (mix64(x) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


# ---- sampling --------------------------------------------------------------------------------------------------------------
def sample_surface(vertices, faces, n, seed=0):
    """-> dict(points [n,3] float32, face [n] int32, bary [n,2] float32, ambiguous: the indices of the samples whose t lies
    within 2^-40 A of a boundary of `cum` (a boundary that is exactly 0 is a sum of zeros in every order and is no such
    boundary), counts [F]: the samples per face, expected [F] = n area / A)."""
    areas, _ = face_areas(vertices, faces)
    cum = np.cumsum(areas)
    A = float(cum[-1]) if len(cum) else 0.0
    n = int(n)
    if not (A > 0) or n == 0:
        return dict(points=np.zeros((0, 3), np.float32), face=np.zeros(0, np.int32), bary=np.zeros((0, 2), np.float32),
                    ambiguous=np.zeros(0, np.int64), counts=np.zeros(len(areas), np.int64), expected=np.zeros(len(areas)))
    i = np.arange(n, dtype=np.uint64)
    t = (i.astype(np.float64) + uniform(seed, i, 0)) / float(n) * A
    f = np.searchsorted(cum, t, side="right")
    f = np.minimum(f, np.searchsorted(cum, A, side="left"))  # the face that brings cum to A: the last usable one
    near = np.zeros(n, bool)
    hi = np.searchsorted(cum, t, side="left")
    for j in (hi - 1, hi):
        inside = (j >= 0) & (j < len(cum))
        b = cum[np.clip(j, 0, len(cum) - 1)]
        near |= inside & (b != 0) & (np.abs(t - b) <= AMBIGUOUS * A)
    a, b = uniform(seed, i, 1), uniform(seed, i, 2)
    fold = a + b > 1.0
    a, b = np.where(fold, 1.0 - a, a), np.where(fold, 1.0 - b, b)
    _, P = _corners(vertices, faces)
    p0, p1, p2 = P[f, 0], P[f, 1], P[f, 2]
    pts = (p0 + a[:, None] * (p1 - p0)) + b[:, None] * (p2 - p0)
    return dict(points=pts.astype(np.float32), face=f.astype(np.int32), bary=np.stack([a, b], 1).astype(np.float32),
                ambiguous=np.nonzero(near)[0], counts=np.bincount(f, minlength=len(areas)), expected=n * areas / A)


# ---- point - triangle ------------------------------------------------------------------------------------------------------
def _segment_d2(p, a, b):
    ab, ap = b - a, p - a
    t, den = _dot(ap, ab), _dot(ab, ab)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = t / den
    q = ap - s[..., None] * ab
    bp = p - b
    return np.where(t <= 0, _dot(ap, ap), np.where(t >= den, _dot(bp, bp), _dot(q, q)))


def triangle_d2(p, P, idx):
    """d^2 (float64) of points p [...,3] to triangles P [...,3,3] whose vertex indices are idx [...,3]: the minimum of the
    three point-segment d^2, every segment walked from its lower vertex index, and of the plane d^2 where the three edge
    functions against n are >= 0."""
    shape = np.broadcast_shapes(p.shape[:-1], P.shape[:-2])
    d2 = np.full(shape, np.inf)
    for j, k in ((0, 1), (1, 2), (2, 0)):
        swap = (idx[..., j] > idx[..., k])[..., None]
        a, b = np.where(swap, P[..., k, :], P[..., j, :]), np.where(swap, P[..., j, :], P[..., k, :])
        s = _segment_d2(p, a, b)
        d2 = np.where(s < d2, s, d2)
    p0, p1, p2 = P[..., 0, :], P[..., 1, :], P[..., 2, :]
    n = _cross(p1 - p0, p2 - p0)
    inside = np.ones(shape, bool)
    for a, b in ((p0, p1), (p1, p2), (p2, p0)):
        inside = inside & (_dot(_cross(b - a, p - a), n) >= 0)
    h = _dot(p - p0, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        plane = h * h / _dot(n, n)
    return np.where(inside & (plane < d2), plane, d2)


# ---- the grid --------------------------------------------------------------------------------------------------------------
def median_edge(vertices, faces):
    """mesh.median_edge: the lower median of the finite edge lengths of the faces with indices in range."""
    ok, P = _corners(vertices, faces)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.sqrt(((P[ok] - np.roll(P[ok], -1, axis=1)) ** 2).sum(axis=2)).reshape(-1)
    e = np.sort(e[np.isfinite(e)])
    return float(e[(len(e) - 1) // 2]) if len(e) else 0.0


def grid_dims(lo, hi, cell):
    """-> (cell, G): cell as a float32 value, raised so that no axis needs more than 256 cells; G = clamp(ceil(extent /
    cell), 1, 256)."""
    ext = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    cell = float(np.float32(cell))
    need = float(ext.max()) / GRID_AXIS
    if cell < need:
        cell = float(np.nextafter(np.float32(need), np.float32(np.inf)))
    G = [int(min(max(math.ceil(e / cell), 1), GRID_AXIS)) for e in ext]
    return cell, G


def cell_of(x, lo, cell, G):
    """The clamped cell coordinate of x on one axis (float64 arrays)."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.floor((np.asarray(x, np.float64) - lo) / cell)
    return np.where(t >= 0, np.minimum(t, G - 1), 0).astype(np.int64)  # a NaN goes to 0


def build_grid(vertices, faces, cell=None):
    """-> dict(lo float32 [3], cell, G, cell_start [cells + 1], pair_face [pairs] (each cell's faces ascending), pairs,
    faces_skipped, usable), or None when no face is usable."""
    areas, skipped = face_areas(vertices, faces)
    usable = areas > 0
    if not usable.any():
        return None
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    corners = v[f[usable].reshape(-1)]
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    if cell is None:
        cell = 2.0 * median_edge(vertices, faces)
    if not (cell > 0 and np.isfinite(cell)):
        cell = float((hi.astype(np.float64) - lo).max())
    F = len(f)
    _, P = _corners(vertices, faces)
    while True:
        cell, G = grid_dims(lo, hi, cell)
        c0 = np.stack([cell_of(P[:, :, a].min(axis=1), float(lo[a]), cell, G[a]) for a in range(3)], 1)
        c1 = np.stack([cell_of(P[:, :, a].max(axis=1), float(lo[a]), cell, G[a]) for a in range(3)], 1)
        count = np.where(usable, (c1 - c0 + 1).prod(axis=1), 0)
        if count.sum() <= 8 * F + 4096:
            break
        cell = 2.0 * cell
    keys = []
    for face in np.nonzero(usable)[0]:
        z, y, x = np.meshgrid(*(np.arange(c0[face, a], c1[face, a] + 1) for a in (2, 1, 0)), indexing="ij")
        keys.append((((z * G[1] + y) * G[0] + x).reshape(-1) << 32) | face)
    keys = np.sort(np.concatenate(keys))
    cells = G[0] * G[1] * G[2]
    cell_start = np.searchsorted(keys, np.arange(cells + 1, dtype=np.int64) << 32)
    return dict(lo=lo, cell=cell, G=G, cell_start=cell_start, pair_face=keys & 0xFFFFFFFF, pairs=len(keys),
                faces_skipped=skipped, usable=usable)


def slack(lo, cell, G):
    """The absolute part of the slack on L(r): 2^-45 of the largest |coordinate| of a cell plane."""
    m = max(max(abs(float(lo[a])), abs(float(lo[a]) + G[a] * cell)) for a in range(3))
    return 2.0 ** -45 * m


# ---- closest point ---------------------------------------------------------------------------------------------------------
def _shell(r):
    o = np.arange(-r, r + 1)
    z, y, x = np.meshgrid(o, o, o, indexing="ij")
    off = np.stack([x, y, z], -1).reshape(-1, 3)
    return off[np.abs(off).max(axis=1) == r]


def _take(state, q, d2, f):
    """Fold the candidates (query q, d^2, face f) into state = [best2, bestf, second2, secondf]: per query the two best
    DIFFERENT faces by (d^2, face index)."""
    if len(q) == 0:
        return
    first = np.ones(len(q), bool)  # the candidates of a query are consecutive
    first[1:] = q[1:] != q[:-1]
    start = np.nonzero(first)[0]
    seg = np.cumsum(first) - 1
    big = np.iinfo(np.int64).max

    def best_of(d):
        m = np.minimum.reduceat(d, start)
        face = np.minimum.reduceat(np.where(d == m[seg], f, big), start)
        return m, face

    m1, f1 = best_of(d2)
    m2, f2 = best_of(np.where(f == f1[seg], np.inf, d2))  # a face that several cells list gives the same d^2 every time
    f2 = np.where(np.isinf(m2), -1, f2)
    rows = q[first]
    D = np.full((len(rows), 4), np.inf)
    Fc = np.full((len(rows), 4), -1, np.int64)
    best2, bestf, second2, secondf = state
    D[:, 0], Fc[:, 0], D[:, 1], Fc[:, 1] = best2[rows], bestf[rows], second2[rows], secondf[rows]
    D[:, 2], Fc[:, 2], D[:, 3], Fc[:, 3] = m1, f1, m2, f2
    for j in (2, 3):  # a face seen in an earlier shell comes with the same d^2 again
        again = (Fc[:, j] == Fc[:, 0]) | (Fc[:, j] == Fc[:, 1])
        D[again, j], Fc[again, j] = np.inf, -1
    key = np.where(Fc < 0, np.iinfo(np.int64).max, Fc)
    rid = np.broadcast_to(np.arange(len(rows))[:, None], D.shape)
    o = np.lexsort((key.ravel(), D.ravel(), rid.ravel())).reshape(len(rows), 4)
    D, Fc = np.take_along_axis(D, o % 4, axis=1), np.take_along_axis(Fc, o % 4, axis=1)
    best2[rows], bestf[rows], second2[rows], secondf[rows] = D[:, 0], Fc[:, 0], D[:, 1], Fc[:, 1]


def _finish(points, best2, bestf, second2, valid, max_distance):
    N = len(points)
    md = np.inf if max_distance is None else float(max_distance)
    far = valid & ((bestf < 0) | (best2 > md * md))
    with np.errstate(invalid="ignore"):
        d = np.sqrt(best2)
    d = np.where(far, md, d)
    d = np.where(valid, d, np.inf)
    face = np.where(far | ~valid, -1, bestf).astype(np.int32)
    with np.errstate(invalid="ignore"):
        # an exact tie is decided by the face index; only a gap that two float64 evaluations could close is left open
        tie = valid & ~far & (second2 > best2) & (second2 - best2 < TIE * best2)
    return dict(distance=d.astype(np.float32), d=d, face=face, d2=best2, second2=second2, far=int(far.sum()),
                queries_invalid=int(N - valid.sum()), tie=tie)


def brute_force(points, vertices, faces, max_distance=None):
    """Every usable face against every query.  -> closest()'s dict."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    N = len(p)
    valid = np.isfinite(p).all(axis=1)
    areas, _ = face_areas(vertices, faces)
    use = np.nonzero(areas > 0)[0]
    _, P = _corners(vertices, faces)
    idx = np.asarray(faces, np.int64).reshape(-1, 3)
    best2, bestf, second2 = np.full(N, np.inf), np.full(N, -1, np.int64), np.full(N, np.inf)
    rows = np.nonzero(valid)[0]
    step = max(1, 2_000_000 // max(len(use), 1))
    for s in range(0, len(rows), step):
        r = rows[s:s + step]
        if len(use) == 0:
            break
        d2 = triangle_d2(p[r][:, None, :], P[use][None], idx[use][None])  # [r, use]
        k = np.argmin(d2, axis=1)  # the first of equal minima: the smallest face index
        best2[r], bestf[r] = d2[np.arange(len(r)), k], use[k]
        d2[np.arange(len(r)), k] = np.inf
        second2[r] = d2.min(axis=1) if len(use) > 1 else np.inf
    return _finish(p, best2, bestf, second2, valid, max_distance)


def closest(points, vertices, faces, cell=None, max_distance=None, grid=None):
    """The kernel's search.  -> dict(distance float32, d float64, face int32 (-1: far or invalid), d2, second2: the best d^2
    of another face among those visited, far, queries_invalid, tie [N] bool, shells: the largest number of rounds of a
    query, tests: point-triangle tests in all)."""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    N = len(p)
    valid = np.isfinite(p).all(axis=1)
    best2, bestf, second2 = np.full(N, np.inf), np.full(N, -1, np.int64), np.full(N, np.inf)
    state = [best2, bestf, second2, np.full(N, -1, np.int64)]
    g = build_grid(vertices, faces, cell) if grid is None else grid
    shells = tests = 0
    if g is not None and N:
        lo, cell, G = g["lo"].astype(np.float64), g["cell"], np.asarray(g["G"])
        md = np.inf if max_distance is None else float(max_distance)
        eps = slack(lo, cell, G)
        _, P = _corners(vertices, faces)
        idx = np.asarray(faces, np.int64).reshape(-1, 3)
        c0 = np.stack([cell_of(np.where(valid, p[:, a], 0.0), lo[a], cell, G[a]) for a in range(3)], 1)
        active = np.nonzero(valid)[0]
        for r in range(int(G.max())):
            if len(active) == 0:
                break
            shells = r + 1
            off = _shell(r)
            step = max(1, 400_000 // len(off))
            for s in range(0, len(active), step):
                q = active[s:s + step]
                c = c0[q][:, None, :] + off[None]
                inside = ((c >= 0) & (c < G[None, None, :])).all(axis=2)
                lin = ((c[..., 2] * G[1] + c[..., 1]) * G[0] + c[..., 0])[inside]
                qq = np.broadcast_to(q[:, None], inside.shape)[inside]
                start, n = g["cell_start"][lin], g["cell_start"][lin + 1] - g["cell_start"][lin]
                total = int(n.sum())
                if total == 0:
                    continue
                rep = np.repeat(np.arange(len(lin)), n)
                pos = start[rep] + (np.arange(total) - np.repeat(np.cumsum(n) - n, n))
                f = g["pair_face"][pos]
                tests += total
                _take(state, qq[rep], triangle_d2(p[qq[rep]], P[f], idx[f]), f)
            # L(r): the nearest face of the visited block that has cells behind it
            L = np.full(len(active), np.inf)
            for a in range(3):
                below, above = c0[active, a] - r > 0, c0[active, a] + r < G[a] - 1
                d_lo = p[active, a] - (lo[a] + (c0[active, a] - r).astype(np.float64) * cell)
                d_hi = (lo[a] + (c0[active, a] + r + 1).astype(np.float64) * cell) - p[active, a]
                L = np.where(below, np.minimum(L, np.maximum(d_lo, 0.0)), L)
                L = np.where(above, np.minimum(L, np.maximum(d_hi, 0.0)), L)
            Ls = (L - eps) * SHRINK
            done = np.isinf(L) | ((Ls > 0) & (best2[active] <= Ls * Ls)) | (Ls > md)
            active = active[~done]
    out = _finish(p, best2, bestf, second2, valid, max_distance)
    out.update(shells=shells, tests=tests, grid=g)
    return out


def distance_tolerance(d, cell):
    """2^-22 max(d, cell): one float32 rounding falling either way after a float64 sqrt that need not be correctly rounded."""
    return 2.0 ** -22 * np.maximum(np.asarray(d, np.float64), float(cell))


# ---- the inputs the tests share --------------------------------------------------------------------------------------------
B_CASES = ("cube", "plane", "debris", "sheets", "fan", "strip")
SAMPLE_SIZES = (1, 63, 4097)
SAMPLE_SEEDS = (0, 7)
LARGE = 4000  # faces from which a case's queries are thinned (see queries())


def b_meshes():
    """name -> (vertices, faces): mesh_simplify_ref.shared_cases() as data, and the blob mesh by the numpy surface nets."""
    import mesh_clean_ref as cr
    import mesh_ref
    import mesh_simplify_ref as sr
    cases = sr.shared_cases()
    out = {k: (cases[k][0]["vertices"], cases[k][0]["faces"]) for k in B_CASES}
    lo, h, tsdf, weight, attr_weight, attr = cr.blob_field()
    blob = mesh_ref.surface_nets(tsdf, weight, attr_weight, attr, lo, h, 1)
    out["blob"] = (blob["vertices"], blob["faces"])
    return out


def default_stride(faces):
    """Keeps the restatement's work on a case at a few million point-triangle tests."""
    return 64 if len(faces) >= LARGE else 4 if len(faces) >= 1000 else 1


def queries(vertices, faces, grid, stride=None):
    """name -> points [n,3] float32 around the mesh: its own vertices; 4096 samples of a second mesh (the unit cube's
    surface stretched to 1.1 times the mesh's box); 4096 hash-random points in a box of twice the extent; 8 points 50
    extents away; points on the grid's cell planes; three non-finite points.  The first three kinds keep every stride-th
    point (default_stride()): a mesh of LARGE or more random faces has a one-cell grid at every cell size, so the
    restatement tests every face for every query, and the queries far from a mesh of a thousand faces walk many shells."""
    import mesh_simplify_ref as sr
    v = np.asarray(vertices, np.float32).reshape(-1, 3)
    if stride is None:
        stride = default_stride(faces)
    lo = grid["lo"].astype(np.float64)
    hi = lo + np.asarray(grid["G"]) * grid["cell"]
    fin = v[np.isfinite(v).all(axis=1)].astype(np.float64)
    lo, hi = np.minimum(lo, fin.min(axis=0)), np.maximum(hi, fin.max(axis=0))
    centre, ext = 0.5 * (lo + hi), hi - lo
    cv, cf = sr.cube()
    second = centre + (sample_surface(cv, cf, 4096, 3)["points"].astype(np.float64) - 0.5) * 1.1 * ext
    i = np.arange(4096, dtype=np.uint64)
    rand = centre + (np.stack([uniform(99, i, k) for k in range(3)], 1) - 0.5) * 2.0 * ext
    corners = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    far = centre + 50.0 * float(ext.max()) * corners
    ks = [sorted({0, 1, G // 2, G}) for G in grid["G"]]
    planes = np.array([[grid["lo"][0] + kx * grid["cell"], grid["lo"][1] + ky * grid["cell"], grid["lo"][2] + kz * grid["cell"]]
                       for kx in ks[0] for ky in ks[1] for kz in ks[2]], np.float64)
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]])
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    return dict(vertices=f32(v[::stride]), second=f32(second[::stride]), random=f32(rand[::stride]), far=f32(far),
                planes=f32(planes), bad=f32(bad))
