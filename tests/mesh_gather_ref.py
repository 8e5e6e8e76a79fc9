"""CPU restatement of ray-traced light per point (csrc/mesh_gather.hip through mesh.gather_points), as include/gigs_hip.h states
it under "Ray-traced light per point": the masked and no_normal rules, the rays of a point (mesh_light_ref.hemispheres with the
points in the vertices' place), the traversal (mesh_raycast_ref.raycast), the classification, the hit count within
ao_distance, the contribution of a miss (mesh_light_ref.sky_texel) and of a front hit with the weights rounded to float32,
the two per-lane sums in ascending chunk order and their butterfly.  Every float64 expression is written in the header's
operation order, so all four outputs are the kernel's bit for bit."""
import numpy as np

import mesh_light_ref as lr
import mesh_raycast_ref as rr
from mesh_raycast_ref import _corners, _cross, _dot, build_grid

WAVE = 64


def _butterfly(c, R):
    """c [n,R,3] float64 -> [n,3]: lane l adds its chunks in ascending order from 0.0, then S <- S + S[lane xor s]."""
    S = np.zeros((c.shape[0], WAVE, 3), np.float64)
    for j in range(0, R, WAVE):
        S = S + c[:, j:j + WAVE]
    lane = np.arange(WAVE)
    for s in (32, 16, 8, 4, 2, 1):
        S = S + S[:, lane ^ s]
    assert (S == S[:, :1]).all() or np.isnan(S).any()
    return S[:, 0]


def gather_points(points, normals, vertices, faces, directions, sky=None, radiosity=None, ao_distance=None, max_distance=None,
                  bias=None, seed=0, mask=None, cell=None, grid=None):
    """-> dict(hits [N] int32, occlusion [N] float32, irradiance, indirect [N,3] float32 or None (no sky), misses, front_hits,
    back_hits, no_normal, masked, ao_distance, bias, grid).  ao_distance and bias default as mesh_raycast_ref.bake_defaults;
    max_distance None is no limit."""
    table = np.asarray(directions, np.float32)
    R = table.shape[1]
    p, n, valid, _, d = lr.hemispheres(points, normals, table, seed)
    N = len(p)
    live = np.ones(N, bool) if mask is None else np.asarray(mask).reshape(N) != 0
    g = build_grid(vertices, faces, cell) if grid is None else grid
    ao_distance, bias = rr.bake_defaults(g, ao_distance, bias)
    tmax = np.inf if max_distance is None else float(max_distance)
    if sky is None:
        tmax = min(ao_distance, tmax)
    rows = np.nonzero(live & valid)[0]
    hits = np.zeros(N, np.int32)
    occlusion = np.ones(N, np.float32)
    irradiance = indirect = None
    if sky is not None:
        sky = np.asarray(sky, np.float32)
        irradiance, indirect = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    front_n = back_n = 0
    if len(rows) and g is not None:
        dd = d[rows].reshape(-1, 3)
        o = np.broadcast_to((p[rows] + bias * n[rows])[:, None, :], d[rows].shape).reshape(-1, 3)
        got = rr.raycast(o, dd, vertices, faces, tmax, grid=g)
        f = got["face"].astype(np.int64)
        hit = f >= 0
        idx, P = _corners(vertices, faces)
        Pf = P[np.maximum(f, 0)]
        s = _dot(dd, _cross(Pf[:, 1] - Pf[:, 0], Pf[:, 2] - Pf[:, 0]))
        front = hit & (s < 0)
        front_n, back_n = int(front.sum()), int((hit & ~front).sum())
        near = (hit & (got["t64"] <= ao_distance)).reshape(len(rows), R)
        hits[rows] = near.sum(axis=1)
        occlusion[rows] = ((R - hits[rows]).astype(np.float64) / float(R)).astype(np.float32)
        if sky is not None:
            c = np.zeros((len(dd), 3), np.float64)
            cf, iy, ix = lr.sky_texel(dd, sky.shape[1])
            miss = ~hit
            c[miss] = sky[cf[miss], iy[miss], ix[miss]].astype(np.float64)
            if radiosity is not None and front.any():
                Q = np.asarray(radiosity, np.float32).reshape(-1, 3).astype(np.float64)
                tri = np.asarray(faces, np.int64).reshape(-1, 3)[f[front]]
                b = got["bary"][front].astype(np.float64)  # float32(w1 / W), float32(w2 / W): the records' rounding
                b1, b2 = b[:, 0:1], b[:, 1:2]
                b0 = np.maximum(0.0, (1.0 - b1) - b2)
                c[front] = (b0 * Q[tri[:, 0]] + b1 * Q[tri[:, 1]]) + b2 * Q[tri[:, 2]]
            c = c.reshape(len(rows), R, 3)
            ci = np.where(front.reshape(len(rows), R, 1), c, 0.0)
            # the kernel adds nothing to S_ind off a front hit; adding +0.0 to a sum that started at +0.0 gives the same bits
            irradiance[rows] = (_butterfly(c, R) / float(R)).astype(np.float32)
            indirect[rows] = (_butterfly(ci, R) / float(R)).astype(np.float32)
    traced = len(rows) if g is not None else 0
    return dict(hits=hits, occlusion=occlusion, irradiance=irradiance, indirect=indirect,
                misses=traced * R - front_n - back_n, front_hits=front_n, back_hits=back_n, no_normal=int((live & ~valid).sum()),
                masked=int((~live).sum()), ao_distance=float(ao_distance), bias=float(bias), grid=g)


COUNTERS = ("misses", "front_hits", "back_hits", "no_normal", "masked")


def counters(report):
    return tuple(report[k] for k in COUNTERS)


def face_points(vertices, faces, every=1):
    """(points [n,3], normals [n,3]) float32: the centroids of every `every`-th usable face and their unit geometric normals."""
    import mesh_distance_ref as dr
    v = np.asarray(vertices, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[dr.face_areas(vertices, f)[0] > 0][::every]
    P = v[f]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm = nrm / np.sqrt((nrm ** 2).sum(axis=1, keepdims=True))
    return P.mean(axis=1).astype(np.float32), nrm.astype(np.float32)


def hash_radiosity(V, seed=17, top=50.0):
    """[V,3] float32 in [0, top): a hash-random vertex radiosity."""
    import mesh_distance_ref as dr
    return (dr.uniform(seed, np.arange(3 * V, dtype=np.uint64), 2) * top).astype(np.float32).reshape(V, 3)


def prepare(pos_view, normal, viewmatrix, normal_space="world"):
    """RaytracedLight.prepare's transform in numpy float64 -> (points [H W,3], normals [H W,3]) float64, NOT rounded."""
    M = np.asarray(viewmatrix, np.float32).astype(np.float64).reshape(4, 4)
    Rm, t = M[:3, :3], M[3, :3]
    p = np.asarray(pos_view, np.float32).astype(np.float64).reshape(3, -1)
    v = np.asarray(normal, np.float32).astype(np.float64).reshape(3, -1)
    d = [p[j] - t[j] for j in range(3)]
    points = np.stack([(d[0] * Rm[i, 0] + d[1] * Rm[i, 1]) + d[2] * Rm[i, 2] for i in range(3)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if normal_space == "view":
            w = [-((v[0] * Rm[i, 0] + v[1] * Rm[i, 1]) + v[2] * Rm[i, 2]) for i in range(3)]
        else:
            w = [v[0], v[1], v[2]]
        length = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
        normals = np.stack([w[i] / length for i in range(3)], 1)
    return points, normals
