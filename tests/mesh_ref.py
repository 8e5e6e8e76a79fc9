"""CPU restatement of csrc/mesh.hip in numpy float32, in the operation order include/gigs_hip.h states: TSDF integration
of one view at a time, and naive surface nets.  Every array operation below rounds once per element in float32, as the
kernels do under -ffp-contract=off; divisions are IEEE.  Fields are [Gz,Gy,Gx] arrays (x fastest), attributes
[Gz,Gy,Gx,8].  Also the mesh checks the tests share (edges, Euler characteristic, orientation, volume)."""
import numpy as np

F = np.float32
NEAR = F(0.2)

# the 12 edges of a cell in their fixed order: (dx, dy, dz of the first corner, axis)
EDGES = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 1, 1, 0),
         (0, 0, 0, 1), (1, 0, 0, 1), (0, 0, 1, 1), (1, 0, 1, 1),
         (0, 0, 0, 2), (1, 0, 0, 2), (0, 1, 0, 2), (1, 1, 0, 2)]


class Volume:
    def __init__(self, lo, voxel, dims, trunc, opacity_min=0.5, carve=True):
        self.lo = np.asarray(lo, dtype=F)
        self.h, self.trunc, self.opacity_min, self.carve = F(voxel), F(trunc), F(opacity_min), bool(carve)
        self.dims = tuple(int(d) for d in dims)
        Gx, Gy, Gz = self.dims
        self.tsdf = np.ones((Gz, Gy, Gx), F)
        self.weight = np.zeros((Gz, Gy, Gx), F)
        self.attr_weight = np.zeros((Gz, Gy, Gx), F)
        self.attr = np.zeros((Gz, Gy, Gx, 8), F)

    def samples(self):
        """x, y, z of every sample, each [Gz,Gy,Gx]: lo + index * h, two roundings."""
        Gx, Gy, Gz = self.dims
        x = self.lo[0] + np.arange(Gx, dtype=F) * self.h
        y = self.lo[1] + np.arange(Gy, dtype=F) * self.h
        z = self.lo[2] + np.arange(Gz, dtype=F) * self.h
        return np.broadcast_arrays(x[None, None, :], y[None, :, None], z[:, None, None])

    def integrate(self, cam, planes, tol=1e-4):
        """One view.  planes: opacity, depth, roughness, metallic [H,W] or [1,H,W], normal, albedo [3,H,W] (arrays).  Returns
        masks [Gz,Gy,Gx]: `behind` (p.z <= 0.2), `outside` (the pixel is not in the image; only where not behind) and
        `fragile` (u + 0.5 or v + 0.5 within tol of an integer, or sdf within tol * trunc of -trunc or +trunc)."""
        m = np.asarray(cam["viewmatrix"], dtype=F).reshape(16)
        W, H = int(cam["image_width"]), int(cam["image_height"])
        fx = F(W) / (F(2.0) * F(cam["tanfovx"]))
        fy = F(H) / (F(2.0) * F(cam["tanfovy"]))
        cx, cy = F(W - 1) / F(2.0), F(H - 1) / F(2.0)
        pl = {k: np.asarray(v, dtype=F).reshape(-1, H, W) for k, v in planes.items()}
        x, y, z = self.samples()
        with np.errstate(all="ignore"):
            px = m[0] * x + m[4] * y + m[8] * z + m[12]
            py = m[1] * x + m[5] * y + m[9] * z + m[13]
            pz = m[2] * x + m[6] * y + m[10] * z + m[14]
            behind = ~(pz > NEAR)
            u = px / pz * fx + cx
            v = py / pz * fy + cy
            fu, fv = np.floor(u + F(0.5)), np.floor(v + F(0.5))
            inside = (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
            live = ~behind & inside
            ix = np.where(live, fu, 0).astype(np.int64)
            iy = np.where(live, fv, 0).astype(np.int64)
            O, D = pl["opacity"][0][iy, ix], pl["depth"][0][iy, ix]
            bg = O < self.opacity_min
            sdf = D - pz
            near = sdf >= -self.trunc
            d = np.where(bg, F(1.0), np.fmin(F(1.0), sdf / self.trunc)).astype(F)
            upd = live & np.where(bg, self.carve, near)
            t_new = (self.tsdf * self.weight + d) / (self.weight + F(1.0))
            self.tsdf = np.where(upd, t_new, self.tsdf).astype(F)
            self.weight = np.where(upd, self.weight + F(1.0), self.weight).astype(F)
            upd_a = live & ~bg & near & (sdf <= self.trunc)
            vals = np.stack([pl["normal"][0], pl["normal"][1], pl["normal"][2], pl["albedo"][0], pl["albedo"][1],
                             pl["albedo"][2], pl["roughness"][0], pl["metallic"][0]], axis=-1)[iy, ix]  # [Gz,Gy,Gx,8]
            aw = self.attr_weight[..., None]
            a_new = (self.attr * aw + vals) / (aw + F(1.0))
            self.attr = np.where(upd_a[..., None], a_new, self.attr).astype(F)
            self.attr_weight = np.where(upd_a, self.attr_weight + F(1.0), self.attr_weight).astype(F)
            # fragile: a decision of this view turns on the last bits
            u5, v5 = (u + F(0.5)).astype(np.float64), (v + F(0.5)).astype(np.float64)
            frag_pix = (np.abs(u5 - np.round(u5)) < tol) | (np.abs(v5 - np.round(v5)) < tol)
            tr = float(self.trunc)
            frag_sdf = (np.abs(sdf.astype(np.float64) + tr) < tol * tr) | (np.abs(sdf.astype(np.float64) - tr) < tol * tr)
            fragile = ~behind & (frag_pix | (inside & ~bg & frag_sdf))
        return dict(behind=behind, outside=~behind & ~inside, fragile=fragile)

    def extract(self, min_weight=1):
        return surface_nets(self.tsdf, self.weight, self.attr_weight, self.attr, self.lo, self.h, min_weight)


def _corner(a, dx, dy, dz):
    """a[k + dz, j + dy, i + dx] for every cell (i,j,k)."""
    Gz, Gy, Gx = a.shape[:3]
    return a[dz:Gz - 1 + dz, dy:Gy - 1 + dy, dx:Gx - 1 + dx]


def surface_nets(tsdf, weight, attr_weight, attr, lo, h, min_weight=1):
    """-> dict(vertices [V,3], faces [F,3] int32, normals, albedo [V,3], roughness, metallic [V])."""
    tsdf, weight, attr_weight, attr = (np.asarray(a, dtype=F) for a in (tsdf, weight, attr_weight, attr))
    lo, h = np.asarray(lo, dtype=F), F(h)
    Gz, Gy, Gx = tsdf.shape
    empty = dict(vertices=np.zeros((0, 3), F), faces=np.zeros((0, 3), np.int32), normals=np.zeros((0, 3), F),
                 albedo=np.zeros((0, 3), F), roughness=np.zeros(0, F), metallic=np.zeros(0, F))
    if min(Gx, Gy, Gz) < 2:
        return empty
    inside = tsdf < 0
    ok = weight >= F(min_weight)
    valid = np.ones((Gz - 1, Gy - 1, Gx - 1), bool)
    n_in = np.zeros((Gz - 1, Gy - 1, Gx - 1), np.int32)
    for c in range(8):
        off = (c & 1, (c >> 1) & 1, c >> 2)
        valid &= _corner(ok, *off)
        n_in += _corner(inside, *off)
    active = valid & (n_in != 0) & (n_in != 8)
    V = int(active.sum())
    if V == 0:
        return empty
    vid = (np.cumsum(active.reshape(-1)) - 1).reshape(active.shape)  # vertex of an active cell, ascending cell index
    kk, jj, ii = np.nonzero(active)  # C order = ascending cell index
    # ---- vertices
    sx, sy, sz, sw = (np.zeros(V, F) for _ in range(4))
    sa = np.zeros((V, 8), F)
    n = np.zeros(V, np.int32)
    with np.errstate(all="ignore"):
        for dx, dy, dz, axis in EDGES:
            ex, ey, ez = dx + (axis == 0), dy + (axis == 1), dz + (axis == 2)
            f0, f1 = tsdf[kk + dz, jj + dy, ii + dx], tsdf[kk + ez, jj + ey, ii + ex]
            cross = (f0 < 0) != (f1 < 0)
            t = np.where(cross, f0 / (f0 - f1), F(0)).astype(F)
            zero = np.zeros(V, F)
            sx = np.where(cross, sx + (F(dx) + (t if axis == 0 else zero)), sx).astype(F)
            sy = np.where(cross, sy + (F(dy) + (t if axis == 1 else zero)), sy).astype(F)
            sz = np.where(cross, sz + (F(dz) + (t if axis == 2 else zero)), sz).astype(F)
            n += cross
            w0 = np.where(attr_weight[kk + dz, jj + dy, ii + dx] == 0, F(0), F(1.0) - t).astype(F)
            w1 = np.where(attr_weight[kk + ez, jj + ey, ii + ex] == 0, F(0), t).astype(F)
            sw_new = (sw + w0) + w1
            sa_new = (sa + w0[:, None] * attr[kk + dz, jj + dy, ii + dx]) + w1[:, None] * attr[kk + ez, jj + ey, ii + ex]
            sw = np.where(cross, sw_new, sw).astype(F)
            sa = np.where(cross[:, None], sa_new, sa).astype(F)
        fn = n.astype(F)
        vertices = np.stack([lo[0] + (ii.astype(F) + sx / fn) * h, lo[1] + (jj.astype(F) + sy / fn) * h,
                             lo[2] + (kk.astype(F) + sz / fn) * h], axis=1).astype(F)
        r = np.where(sw[:, None] > 0, sa / sw[:, None], F(0)).astype(F)
        length = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]).astype(F)
        normals = np.where(length[:, None] > 0, r[:, :3] / length[:, None], F(0)).astype(F)
    # ---- faces: every grid edge (sample, axis), ordered by (sample index, axis)
    G = (Gx, Gy, Gz)
    quads = []
    K, J, I = np.meshgrid(np.arange(Gz), np.arange(Gy), np.arange(Gx), indexing="ij")
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        p = [I, J, K]
        exists = (p[axis] + 1 < G[axis]) & (p[u] >= 1) & (p[u] + 1 < G[u]) & (p[v] >= 1) & (p[v] + 1 < G[v])
        k0, j0, i0 = np.nonzero(exists)
        q = [i0.copy(), j0.copy(), k0.copy()]
        q[axis] += 1
        in0, in1 = inside[k0, j0, i0], inside[q[2], q[1], q[0]]
        keep = in0 != in1
        cells = []
        for du, dv in ((-1, -1), (0, -1), (0, 0), (-1, 0)):  # counter-clockwise as seen from the + end of the axis
            r_ = [i0.copy(), j0.copy(), k0.copy()]
            r_[u] += du
            r_[v] += dv
            keep &= valid[r_[2], r_[1], r_[0]]
            cells.append(vid[r_[2], r_[1], r_[0]])
        a, b, c, d = (x[keep] for x in cells)
        flip = ~in0[keep]  # the outside (positive) end is the sample itself
        b, d = np.where(flip, d, b), np.where(flip, b, d)
        sample = (k0[keep] * Gy + j0[keep]) * Gx + i0[keep]
        quads.append((sample * 3 + axis, a, b, c, d))
    key = np.concatenate([q[0] for q in quads])
    order = np.argsort(key, kind="stable")
    a, b, c, d = (np.concatenate([q[i] for q in quads])[order] for i in (1, 2, 3, 4))
    faces = np.stack([a, b, c, a, c, d], axis=1).reshape(-1, 3).astype(np.int32)
    return dict(vertices=vertices, faces=faces, normals=normals, albedo=r[:, 3:6].copy(), roughness=r[:, 6].copy(),
                metallic=r[:, 7].copy())


# ---- analytic fields and mesh checks the tests share ----------------------------------------------------------------------
def sphere_grid(dims, shift=(0.013, -0.007, 0.004), span=1.7):
    """(lo, h): the grid of `dims` samples with h = span / (max(dims) - 1), centred on the origin and shifted."""
    h = span / (max(dims) - 1)
    lo = np.array([-0.5 * (d - 1) * h + s for d, s in zip(dims, shift)])
    return lo.astype(F), F(h)


def sphere_field(dims, radius=0.6, **kw):
    """clip((|s| - radius) / (3 h), -1, 1) on sphere_grid(dims) -> (lo, h, tsdf [Gz,Gy,Gx])."""
    lo, h = sphere_grid(dims, **kw)
    Gx, Gy, Gz = dims
    x = lo[0].astype(np.float64) + np.arange(Gx) * float(h)
    y = lo[1].astype(np.float64) + np.arange(Gy) * float(h)
    z = lo[2].astype(np.float64) + np.arange(Gz) * float(h)
    r = np.sqrt(x[None, None, :] ** 2 + y[None, :, None] ** 2 + z[:, None, None] ** 2)
    return lo, h, np.clip((r - radius) / (3.0 * float(h)), -1.0, 1.0).astype(F)


def edge_counts(faces):
    """{undirected edge: number of triangles} as (unique edges [E,2], counts [E])."""
    f = np.asarray(faces, dtype=np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    e.sort(axis=1)
    return np.unique(e, axis=0, return_counts=True)


def euler(n_vertices, faces):
    edges, _ = edge_counts(faces)
    return int(n_vertices) - len(edges) + len(faces)


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0


def enclosed_volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def check_closed_sphere(vertices, faces, h, radius=0.6):
    """The conditions of a closed, outward-oriented mesh of the analytic sphere; returns the measured figures."""
    vertices, faces = np.asarray(vertices), np.asarray(faces)
    assert faces.size and faces.min() >= 0 and faces.max() < len(vertices)
    _, counts = edge_counts(faces)
    assert (counts == 2).all(), "edges with %s triangles" % sorted(set(counts.tolist()))
    chi = euler(len(vertices), faces)
    assert chi == 2, chi
    nrm, centre = face_normals(vertices, faces)
    assert (np.einsum("ij,ij->i", nrm, centre) > 0).all(), "a face normal points towards the origin"
    err = float(np.abs(np.linalg.norm(vertices.astype(np.float64), axis=1) - radius).max() / float(h))
    assert err <= 0.25, err
    vol = enclosed_volume(vertices, faces) / (4.0 / 3.0 * np.pi * radius ** 3)
    assert vol >= 0.95, vol
    return dict(radius_error_h=err, volume_ratio=vol)
