"""CPU restatement of csrc/mesh_raster.hip in numpy float32 / int64, in the operation order include/gigs_hip.h states:
projection of the vertices to 24.8 fixed-point screen coordinates, the visibility buffer (the minimum of
(bits(z) << 32) | triangle index over the triangles whose integer edge functions cover a pixel centre) and the resolve
into the blend kernel's inference planes.  Every array operation rounds once per element in float32, as the kernels do
under -ffp-contract=off; divisions are IEEE.  raster() can also count the covering triangles per pixel."""
import numpy as np

F = np.float32
NEAR = F(0.2)
GUARD = F(16384.0)
SUB = 256
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(vertices, cam):
    """-> view_pos [V,3] float32, screen [V,2] int32, flags [V] uint8."""
    v = np.asarray(vertices, dtype=F).reshape(-1, 3)
    m = np.asarray(cam["viewmatrix"], dtype=F).reshape(16)
    W, H = int(cam["image_width"]), int(cam["image_height"])
    fx = F(W) / (F(2.0) * F(cam["tanfovx"]))
    fy = F(H) / (F(2.0) * F(cam["tanfovy"]))
    cx, cy = F(W - 1) / F(2.0), F(H - 1) / F(2.0)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        px = m[0] * x + m[4] * y + m[8] * z + m[12]
        py = m[1] * x + m[5] * y + m[9] * z + m[13]
        pz = m[2] * x + m[6] * y + m[10] * z + m[14]
        u = px / pz * fx + cx
        w = py / pz * fy + cy
        ok = (pz > NEAR) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pz) & (np.abs(u) <= GUARD) & (np.abs(w) <= GUARD)
        X = np.where(ok, np.rint(u * F(SUB)), F(0)).astype(np.int32)
        Y = np.where(ok, np.rint(w * F(SUB)), F(0)).astype(np.int32)
    return np.stack([px, py, pz], axis=1).astype(F), np.stack([X, Y], axis=1), (~ok).astype(np.uint8)


def _setup(t, faces, V, screen, flags, view_pos):
    """The triangle as the kernels see it -- (vertex indices, X, Y, 1 / z, float(A)) with A > 0 -- or None if dropped."""
    idx = [int(i) for i in faces[t]]
    if any(i < 0 or i >= V for i in idx) or any(flags[i] for i in idx):
        return None
    X = [int(screen[i, 0]) for i in idx]
    Y = [int(screen[i, 1]) for i in idx]
    A = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
    if A == 0:
        return None
    if A < 0:
        idx[1], idx[2], X[1], X[2], Y[1], Y[2], A = idx[2], idx[1], X[2], X[1], Y[2], Y[1], -A
    with np.errstate(all="ignore"):
        iz = [F(1.0) / F(view_pos[i, 2]) for i in idx]
    return idx, X, Y, iz, F(np.int64(A))


def _sample(tri, qx, qy):
    """Arrays of pixel centres (int64, in sub-pixel units) -> (covered and usable [n] bool, w0, w1, w2, s, z)."""
    _, X, Y, iz, fA = tri
    E, inside = [], np.ones(qx.shape, bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        e = dx * (qy - Y[a]) - dy * (qx - X[a])
        inside &= (e > 0) | ((e == 0) & (dy < 0 or (dy == 0 and dx > 0)))
        E.append(e)
    with np.errstate(all="ignore"):
        w = [(e.astype(F) / fA) * k for e, k in zip(E, iz)]
        s = (w[0] + w[1]) + w[2]
        z = F(1.0) / s
        ok = inside & (z > 0) & np.isfinite(z)
    return ok, w[0], w[1], w[2], s, z


def raster(faces, view_pos, screen, flags, W, H, counts=False):
    """-> vis [H,W] uint64 (all ones where nothing covers); with counts also the number of covering triangles [H,W]."""
    faces = np.asarray(faces).reshape(-1, 3)
    V = len(flags)
    vis = np.full((H, W), EMPTY, np.uint64)
    n = np.zeros((H, W), np.int32)
    for t in range(len(faces)):
        tri = _setup(t, faces, V, screen, flags, view_pos)
        if tri is None:
            continue
        _, X, Y, _, _ = tri
        i0, i1 = max(0, -(-min(X) // SUB)), min(W - 1, max(X) // SUB)
        j0, j1 = max(0, -(-min(Y) // SUB)), min(H - 1, max(Y) // SUB)
        if i0 > i1 or j0 > j1:
            continue
        jj, ii = np.mgrid[j0:j1 + 1, i0:i1 + 1]
        ok, _, _, _, _, z = _sample(tri, ii.astype(np.int64) * SUB, jj.astype(np.int64) * SUB)
        key = (z.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(t)
        sub = vis[j0:j1 + 1, i0:i1 + 1]
        sub[ok] = np.minimum(sub[ok], key[ok])
        n[j0:j1 + 1, i0:i1 + 1] += ok
    return (vis, n) if counts else vis


def resolve(vis, faces, view_pos, screen, flags, normals, albedo, roughness, metallic, viewmatrix):
    """-> dict of the planes: opacity, depth, roughness, metallic [1,H,W], pos, normal, normal_view, albedo [3,H,W] float32,
    tri_id [H,W] int32."""
    faces = np.asarray(faces).reshape(-1, 3)
    H, W = vis.shape
    V, nF = len(flags), len(faces)
    m = np.asarray(viewmatrix, dtype=F).reshape(16)
    out = dict(opacity=np.zeros((1, H, W), F), depth=np.zeros((1, H, W), F), pos=np.zeros((3, H, W), F),
               normal=np.zeros((3, H, W), F), albedo=np.zeros((3, H, W), F), roughness=np.ones((1, H, W), F),
               metallic=np.zeros((1, H, W), F), tri_id=np.full((H, W), -1, np.int32))
    normals, albedo = np.asarray(normals, dtype=F).reshape(-1, 3), np.asarray(albedo, dtype=F).reshape(-1, 3)
    roughness, metallic = np.asarray(roughness, dtype=F).reshape(-1), np.asarray(metallic, dtype=F).reshape(-1)
    tri_of = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for t in np.unique(tri_of[vis != EMPTY]):
        if t >= nF:
            continue
        tri = _setup(int(t), faces, V, screen, flags, view_pos)
        if tri is None:
            continue
        jj, ii = np.nonzero((tri_of == t) & (vis != EMPTY))
        ok, w0, w1, w2, s, z = _sample(tri, ii.astype(np.int64) * SUB, jj.astype(np.int64) * SUB)
        jj, ii, w0, w1, w2, s, z = (a[ok] for a in (jj, ii, w0, w1, w2, s, z))
        a, b, c = tri[0]
        mix = lambda x: ((w0 * x[a] + w1 * x[b]) + w2 * x[c]) / s  # noqa: E731
        out["opacity"][0, jj, ii] = F(1.0)
        out["depth"][0, jj, ii] = z
        out["tri_id"][jj, ii] = t
        for k in range(3):
            out["pos"][k, jj, ii] = mix(view_pos[:, k])
            out["normal"][k, jj, ii] = mix(normals[:, k])
            out["albedo"][k, jj, ii] = mix(albedo[:, k])
        out["roughness"][0, jj, ii] = mix(roughness)
        out["metallic"][0, jj, ii] = mix(metallic)
    nx, ny, nz = out["normal"]
    with np.errstate(all="ignore"):  # normalize3(xform_vec_4x3(n, viewmatrix)): NaN for the zero vector
        vx = m[0] * nx + m[4] * ny + m[8] * nz
        vy = m[1] * nx + m[5] * ny + m[9] * nz
        vz = m[2] * nx + m[6] * ny + m[10] * nz
        inv = F(1.0) / np.sqrt(vx * vx + vy * vy + vz * vz)
        out["normal_view"] = np.stack([vx * inv, vy * inv, vz * inv]).astype(F)
    return out


def render(mesh, cam, counts=False):
    """The three stages on a mesh dict (vertices, faces, normals, albedo, roughness, metallic) -> the planes, plus
    view_pos / screen / flags and, with counts, `cover` [H,W]."""
    W, H = int(cam["image_width"]), int(cam["image_height"])
    view_pos, screen, flags = project(mesh["vertices"], cam)
    r = raster(mesh["faces"], view_pos, screen, flags, W, H, counts=counts)
    vis, cover = r if counts else (r, None)
    out = resolve(vis, mesh["faces"], view_pos, screen, flags, mesh["normals"], mesh["albedo"], mesh["roughness"],
                  mesh["metallic"], cam["viewmatrix"])
    out.update(view_pos=view_pos, screen=screen, flags=flags, vis=vis)
    if counts:
        out["cover"] = cover
    return out


# ---- what the tests share ---------------------------------------------------------------------------------------------------
SPHERE_DIMS = (28, 24, 26)
PW, PH = 40, 56
FOVX = 0.6911


def sphere_mesh(seed=7):
    """mesh_ref's analytic sphere (radius 0.6) through surface nets with all weights 1 and seeded random attributes: a
    closed mesh of 1710 vertices and 3416 faces.  -> (mesh dict, h)."""
    import mesh_ref
    lo, h, tsdf = mesh_ref.sphere_field(SPHERE_DIMS)
    rng = np.random.default_rng(seed)
    attr = rng.uniform(-1.0, 1.0, size=tsdf.shape + (8,)).astype(F)
    attr[..., 3:] = np.abs(attr[..., 3:])
    m = mesh_ref.surface_nets(tsdf, np.ones_like(tsdf), np.ones_like(tsdf), attr, lo, h)
    return m, float(h)


def sphere_cameras(seventh=False):
    import scenes
    cams = [scenes.orbit_camera(i, 6, PW, PH, radius=3.0, fovx=FOVX, elevation=0.5 if i % 2 == 0 else -0.6) for i in range(6)]
    if seventh:  # close up: the mesh covers the whole image and its triangles' boxes reach 81 pixels
        cams.append(scenes.look_at_camera((0.05, 0.02, 1.0), (0.0, 0.0, 0.0), PW, PH, FOVX, up=(0.0, 1.0, 0.0)))
    return cams


def analytic_sphere(cam, radius=0.6):
    """(hit [H,W] bool, z-depth [H,W]) of the sphere |x| = radius at the rasterizer's pixel centres (integers, principal
    point ((W - 1) / 2, (H - 1) / 2)), in double."""
    W, H = cam["image_width"], cam["image_height"]
    m = np.asarray(cam["viewmatrix"], np.float64).reshape(16)
    c = np.array([m[12], m[13], m[14]])  # the origin in view space
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    dx = (np.arange(W) - (W - 1) / 2.0) / fx
    dy = (np.arange(H) - (H - 1) / 2.0) / fy
    d = np.stack(np.broadcast_arrays(dx[None, :], dy[:, None], np.ones((H, W))), axis=-1)
    a, b = (d * d).sum(-1), d @ c
    disc = b * b - a * (c @ c - radius * radius)
    hit = disc > 0
    return hit, np.where(hit, (b - np.sqrt(np.maximum(disc, 0.0))) / a, 0.0)


def owner_rule_case():
    """Hand-made fixed-point vertices on a 32 x 48 image (shared with the GPU suite): the two triangles of a quad whose
    shared diagonal, horizontal and vertical edges pass exactly through pixel centres, and a fan of eight around a vertex
    at a pixel centre.  -> (screen [V,2] int32, faces [F,3] int32, union mask [H,W])."""
    W, H = 32, 48
    S = SUB
    quad = [(4, 4), (14, 4), (14, 14), (4, 14)]  # corners at pixel centres: the diagonal (4,4)-(14,14) crosses ten more
    c = (22, 30)
    ring = [(28, 30), (27, 35), (22, 37), (17, 35), (16, 30), (17, 25), (22, 23), (27, 25)]
    pts = quad + [c] + ring
    screen = np.array([(x * S, y * S) for x, y in pts], np.int32)
    faces = [(0, 1, 2), (0, 2, 3)]
    faces += [(4, 5 + k, 5 + (k + 1) % 8) for k in range(8)]
    faces[3], faces[5] = faces[3][::-1], faces[5][::-1]  # both orientations occur
    union = np.zeros((H, W), bool)
    union[5:14, 5:14] = True  # the quad's interior pixel centres (the border's ownership is the rule's business)
    return screen, np.array(faces, np.int32), union, (W, H)
