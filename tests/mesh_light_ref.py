"""CPU restatement of light baking (csrc/mesh_light.hip through mesh.trace_hemispheres / mesh.gather_light), as
include/gigs_hip.h states it under "Baking light": the records of every ray of every vertex's hemisphere (the face, the side
it was hit on, the float32 weights), the nearest sky texel of a direction, the contribution of a miss and of a front hit,
the per-lane sums in ascending chunk order and their butterfly, irradiance and radiosity.  The rays, the traversal, the frame,
the rotation and the table are mesh_raycast_ref.py's; every float64 expression is written in the header's operation order,
so records, irradiance and radiosity are the kernels' bit for bit."""
import numpy as np

import mesh_raycast_ref as rr
from mesh_raycast_ref import _corners, _cross, _dot, build_grid

WAVE = 64


# ---- the rays ----------------------------------------------------------------------------------------------------------------
def hemispheres(vertices, normals, directions, seed):
    """-> (v [V,3] float64, n [V,3] float64, valid [V] (the no_normal rule), rotation [V], d [V,R,3] float64 world directions;
    rows of an invalid vertex are whatever the expressions give and are not used)."""
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    n = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    table = np.asarray(directions, np.float32).astype(np.float64)
    K = table.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        n2 = _dot(n, n)
        valid = np.isfinite(v).all(axis=1) & (n2 >= 1.0 - rr.NORMAL_BAND) & (n2 <= 1.0 + rr.NORMAL_BAND)
    rot = rr.rotation_of(seed, np.arange(len(v)), K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        T, B = rr.frame(n)
        x, y, z = (table[rot][..., c] for c in range(3))  # [V,R]
        d = (x[..., None] * T[:, None, :] + y[..., None] * B[:, None, :]) + z[..., None] * n[:, None, :]
    return v, n, valid, rot, d


def default_bias(grid):
    """bake_occlusion's: 1e-3 of 0.1 of the longest axis of the grid's box."""
    return rr.bake_defaults(grid)[1]


# ---- the trace ---------------------------------------------------------------------------------------------------------------
def trace(vertices, faces, normals, directions, max_distance=None, bias=None, seed=0, cell=None, grid=None, subset=None,
          brute=False):
    """-> dict(face [V,R] int32, bary [V,R,2] float32, rows: the vertices traced (all the valid ones, or those of `subset`),
    misses, front_hits, back_hits, no_normal (over `subset` if given), valid, bias, grid).  Records of a vertex outside
    `subset` stay -1 / 0.  `brute`: brute_force() over all usable faces in place of the traversal."""
    table = np.asarray(directions, np.float32)
    R = table.shape[1]
    v, n, valid, _, d = hemispheres(vertices, normals, table, seed)
    V = len(v)
    g = build_grid(vertices, faces, cell) if grid is None else grid
    if bias is None:
        bias = default_bias(g)
    chosen = np.arange(V) if subset is None else np.asarray(subset)
    rows = chosen[valid[chosen]]
    face = np.full((V, R), -1, np.int32)
    bary = np.zeros((V, R, 2), np.float32)
    front = back = 0
    if len(rows) and g is not None:
        dd = d[rows].reshape(-1, 3)
        o = np.broadcast_to((v[rows] + bias * n[rows])[:, None, :], d[rows].shape).reshape(-1, 3)
        cast = rr.brute_force if brute else (lambda *a: rr.raycast(*a, grid=g))
        got = cast(o, dd, vertices, faces, max_distance)
        f = got["face"].astype(np.int64)
        hit = f >= 0
        _, P = _corners(vertices, faces)
        Pf = P[np.maximum(f, 0)]
        s = _dot(dd, _cross(Pf[:, 1] - Pf[:, 0], Pf[:, 2] - Pf[:, 0]))
        is_front = hit & (s < 0)
        record = np.where(hit, np.where(is_front, f, -2 - f), -1)
        face[rows] = record.reshape(len(rows), R).astype(np.int32)
        bary[rows] = got["bary"].reshape(len(rows), R, 2)
        front, back = int(is_front.sum()), int((hit & ~is_front).sum())
    return dict(face=face, bary=bary, rows=rows, misses=len(rows) * R - front - back, front_hits=front, back_hits=back,
                no_normal=int((~valid[chosen]).sum()), valid=valid, bias=float(bias), grid=g)


# ---- the sky -----------------------------------------------------------------------------------------------------------------
def _texel_of(u, n):
    with np.errstate(invalid="ignore"):
        t = np.floor(u * float(n))
        return np.where(~(t >= 0.0), 0.0, np.where(t > float(n - 1), float(n - 1), t)).astype(np.int64)  # a NaN goes to 0


def sky_texel(d, n):
    """d [...,3] float64 -> (face, iy, ix): cube_face_uv's selection and signs in float64, the nearest texel."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    is_z = az > np.maximum(ax, ay)
    is_y = ~is_z & (ay > ax)
    idx = np.where(is_z, 4, np.where(is_y, 2, 0))
    c = np.where(is_z, z, np.where(is_y, y, x))
    a = np.where(is_z | is_y, x, z)
    b = np.where(is_y, z, y)
    idx = idx + (c < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = 0.5 / np.abs(c)
        m0 = np.where((idx == 0) | (idx == 5), -m, m)
        m1 = np.where(idx != 2, -m, m)
        u = np.fmin(np.fmax(a * m0 + 0.5, 0.0), 1.0)
        w = np.fmin(np.fmax(b * m1 + 0.5, 0.0), 1.0)
    return idx, _texel_of(w, n), _texel_of(u, n)


# ---- the gather --------------------------------------------------------------------------------------------------------------
def gather(vertices, faces, normals, directions, seed, face, bary, sky, reflectance, previous=None, rows=None):
    """One pass.  -> (irradiance [V,3] float32, radiosity [V,3] float32); a vertex outside `rows` (default: all) keeps 0."""
    table = np.asarray(directions, np.float32)
    R = table.shape[1]
    v, n, valid, _, d = hemispheres(vertices, normals, table, seed)
    V = len(v)
    sky = np.asarray(sky, np.float32)
    rho = np.asarray(reflectance, np.float32).reshape(V, 3).astype(np.float64)
    idx = np.asarray(faces, np.int64).reshape(-1, 3)
    chosen = np.arange(V) if rows is None else np.asarray(rows)
    rows = chosen[valid[chosen]]
    irradiance, radiosity = np.zeros((V, 3), np.float32), np.zeros((V, 3), np.float32)
    if len(rows) == 0:
        return irradiance, radiosity
    rec = np.asarray(face, np.int32)[rows].astype(np.int64)  # [n,R]
    miss, front = rec == -1, rec >= 0
    c = np.zeros(rec.shape + (3,), np.float64)
    cf, iy, ix = sky_texel(d[rows], sky.shape[1])
    c[miss] = sky[cf[miss], iy[miss], ix[miss]].astype(np.float64)
    if previous is not None and front.any():
        Q = np.asarray(previous, np.float32).reshape(V, 3).astype(np.float64)
        tri = idx[rec[front]]
        b = np.asarray(bary, np.float32)[rows][front].astype(np.float64)
        b1, b2 = b[:, 0:1], b[:, 1:2]
        b0 = np.maximum(0.0, (1.0 - b1) - b2)
        c[front] = (b0 * Q[tri[:, 0]] + b1 * Q[tri[:, 1]]) + b2 * Q[tri[:, 2]]
    S = np.zeros((len(rows), WAVE, 3), np.float64)
    for j in range(0, R, WAVE):  # lane l adds its chunks in ascending order, from 0.0
        S = S + c[:, j:j + WAVE]
    lane = np.arange(WAVE)
    for s in (32, 16, 8, 4, 2, 1):  # the butterfly: all lanes at once
        S = S + S[:, lane ^ s]
    assert (S == S[:, :1]).all() or np.isnan(S).any()
    irradiance[rows] = (S[:, 0] / float(R)).astype(np.float32)
    radiosity[rows] = (rho[rows] * irradiance[rows].astype(np.float64)).astype(np.float32)
    return irradiance, radiosity


def light(vertices, faces, normals, directions, seed, face, bary, sky, reflectance, bounces=1, rows=None):
    """-> (irradiance [bounces + 1, V, 3] float32, radiosity likewise): every pass.  With `rows`, the previous radiosity of the
    OTHER vertices is 0, so rows must be all vertices (None) when bounces >= 1 and the result is to match the kernel."""
    I, Q, prev = [], [], None
    for _ in range(bounces + 1):
        irr, prev = gather(vertices, faces, normals, directions, seed, face, bary, sky, reflectance, prev, rows)
        I.append(irr)
        Q.append(prev)
    return np.stack(I), np.stack(Q)


# ---- the inputs the tests share ----------------------------------------------------------------------------------------------
def open_box(n=4):
    """mesh_raycast_ref.box_interior(n) with the side z = max removed and the winding of the other five turned, so that the
    faces FRONT the interior: light enters through the opening and bounces between the walls.  The vertices that lay
    strictly inside the removed side stay, free-standing, with their normal (0, 0, -1).  -> (vertices, faces, normals)."""
    v, f, nrm = rr.box_interior(n)
    top = (v[f][..., 2] == v.max()).all(axis=1)
    f = f[~top][:, [0, 2, 1]]
    return v, np.ascontiguousarray(f, np.int32), nrm


def face_colour_sky(n=4):
    """[6,n,n,3] float32: six distinct constant face colours."""
    colours = np.array([[1, 0.5, 0.25], [0.125, 2, 0.75], [3, 0.0625, 1.5], [0.375, 0.875, 4], [5, 6, 0.5], [0.25, 7, 8]], np.float32)
    return np.ascontiguousarray(np.broadcast_to(colours[:, None, None, :], (6, n, n, 3)))


def hash_sky(n=8, top=1e4, seed=11):
    """[6,n,n,3] float32: hash-random values in [0, top)."""
    import mesh_distance_ref as dr
    i = np.arange(6 * n * n * 3, dtype=np.uint64)
    return (dr.uniform(seed, i, 0) * top).astype(np.float32).reshape(6, n, n, 3)


def texel_centres(n):
    """[6,n,n,3] float64: the direction of every texel centre with its major component +-1, by the inverse of sky_texel's
    mapping (checked against it)."""
    t = (np.arange(n, dtype=np.float64) + 0.5) / n
    v_, u_ = np.meshgrid(t, t, indexing="ij")  # [iy, ix]
    p, q = 2.0 * u_ - 1.0, 2.0 * v_ - 1.0
    one = np.ones_like(p)
    dirs = np.stack([np.stack([one, -q, -p], -1), np.stack([-one, -q, p], -1), np.stack([p, one, q], -1),
                     np.stack([p, -one, -q], -1), np.stack([p, -q, one], -1), np.stack([-p, -q, -one], -1)])
    cf, iy, ix = sky_texel(dirs, n)
    want = np.broadcast_to(np.arange(6)[:, None, None], cf.shape), np.broadcast_to(np.arange(n)[None, :, None], cf.shape), \
        np.broadcast_to(np.arange(n)[None, None, :], cf.shape)
    assert all(np.array_equal(g, w) for g, w in zip((cf, iy, ix), want)), "texel_centres and sky_texel disagree"
    return dirs


def linear_sky(a, b, n=256):
    """[6,n,n,3] float32: L(d) = a + b . d^ per channel (a [3], b [3 channels, 3 axes]) at the texel centres."""
    dirs = texel_centres(n)
    unit = dirs / np.sqrt((dirs ** 2).sum(-1, keepdims=True))
    return (np.asarray(a, np.float64) + unit @ np.asarray(b, np.float64).T).astype(np.float32)


def vertex_normals(vertices, faces):
    """Area-weighted vertex normals of the usable faces, float32; zero where a vertex has none."""
    import mesh_distance_ref as dr
    v64 = np.asarray(vertices, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    use = dr.face_areas(vertices, f)[0] > 0
    n = np.zeros_like(v64)
    fn = np.cross(v64[f[use, 1]] - v64[f[use, 0]], v64[f[use, 2]] - v64[f[use, 0]])
    for k in range(3):
        np.add.at(n, f[use, k], fn)
    ln = np.sqrt((n ** 2).sum(axis=1, keepdims=True))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ln > 0, n / ln, 0.0).astype(np.float32)


ANALYTIC_A = np.ones(3)
ANALYTIC_B = np.stack([np.roll(np.array([0.5, -0.3, 0.2]), -k) for k in range(3)])  # one permutation of b per channel


def analytic_normals():
    """[9,3] float32: the six axis normals and three oblique ones, of unit length."""
    n = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1], [1, 2, 2], [-2, 3, 6]], np.float64)
    return (n / np.sqrt((n ** 2).sum(axis=1, keepdims=True))).astype(np.float32)


def analytic_irradiance(normals):
    """-> (expected [V,3] float64, bound [3]) under linear_sky(ANALYTIC_A, ANALYTIC_B, 256) with R = 1024, K = 16 and nothing to
    hit: the cosine-weighted mean of a + b . d over the hemisphere about n is a + (2/3) b . n.  The bound is derived, not
    measured: (|b_x| + |b_y| + |b_z|) 5.2e-4, the lattice's first-moment error (the worst rotation of the R = 1024, K = 16
    table has a mean within 5.2e-4 of (0, 0, 2/3) in x and y and within 1.9e-6 in z), plus |b|_2 sqrt(2) / 256, the
    nearest texel's half-diagonal."""
    want = ANALYTIC_A + (2.0 / 3.0) * np.asarray(normals, np.float32).astype(np.float64) @ ANALYTIC_B.T
    bound = np.abs(ANALYTIC_B).sum(axis=1) * 5.2e-4 + np.sqrt((ANALYTIC_B ** 2).sum(axis=1)) * np.sqrt(2.0) / 256.0
    return want, bound
