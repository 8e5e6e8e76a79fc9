"""CPU restatement of gigs_mesh_resolve_textured (csrc/mesh_raster.hip) in numpy float32, in the operation order
include/gigs_hip.h states under "Rendering meshes": mesh_raster_ref's set-up and sampling of the winning triangle, the
perspective-correct UV of the face's corners (swapped with the vertices where the set-up swapped them), texel coordinates
with v = 0 at the bottom row, the clamp to [-1, Wt] x [-1, Ht] that turns a NaN into -1, and the bilinear lookup in
mesh.sample_atlas's order.  Every array operation rounds once per element in float32."""
import numpy as np

import mesh_raster_ref as rr

F = rr.F


def tex_axis(c, n):
    """Texel coordinate(s) c along an axis of n texels -> (first tap, second tap, weight of the second)."""
    with np.errstate(all="ignore"):
        c = np.fmin(np.fmax(np.asarray(c, F), F(-1.0)), F(n))  # fmax / fmin return the non-NaN argument
        c0 = np.floor(c)
        f = (c - c0).astype(F)
        i = c0.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), f


def bilinear(planes, u, v):
    """planes [C,Ht,Wt] float32 at the UVs (u, v) [n] float32 -> [C,n] float32."""
    planes = np.asarray(planes, F)
    _, Ht, Wt = planes.shape
    with np.errstate(all="ignore"):
        xa, xb, fx = tex_axis(u * F(Wt) - F(0.5), Wt)
        ya, yb, fy = tex_axis((F(1.0) - v) * F(Ht) - F(0.5), Ht)
        gx, gy = F(1.0) - fx, F(1.0) - fy
        top = gx * planes[:, ya, xa] + fx * planes[:, ya, xb]
        bot = gx * planes[:, yb, xa] + fx * planes[:, yb, xb]
        return (gy * top + fy * bot).astype(F)


def resolve_textured(vis, faces, view_pos, screen, flags, uvs, albedo, orm, normal, normals, viewmatrix):
    """-> dict of the planes: mesh_raster_ref.resolve's, and occlusion [1,H,W].  normal: [3,Ht,Wt] or None (then `normals`
    [V,3] is interpolated as in mesh_raster_ref.resolve)."""
    faces = np.asarray(faces).reshape(-1, 3)
    H, W = vis.shape
    V, nF = len(flags), len(faces)
    m = np.asarray(viewmatrix, dtype=F).reshape(16)
    uvs = np.asarray(uvs, F).reshape(-1, 3, 2)
    out = dict(opacity=np.zeros((1, H, W), F), depth=np.zeros((1, H, W), F), pos=np.zeros((3, H, W), F),
               normal=np.zeros((3, H, W), F), albedo=np.zeros((3, H, W), F), roughness=np.ones((1, H, W), F),
               metallic=np.zeros((1, H, W), F), occlusion=np.ones((1, H, W), F), tri_id=np.full((H, W), -1, np.int32))
    if normal is None:
        normals = np.asarray(normals, dtype=F).reshape(-1, 3)
    tri_of = (vis & np.uint64(0xFFFFFFFF)).astype(np.int64)
    for t in np.unique(tri_of[vis != rr.EMPTY]):
        if t >= nF:
            continue
        tri = rr._setup(int(t), faces, V, screen, flags, view_pos)
        if tri is None:
            continue
        jj, ii = np.nonzero((tri_of == t) & (vis != rr.EMPTY))
        ok, w0, w1, w2, s, z = rr._sample(tri, ii.astype(np.int64) * rr.SUB, jj.astype(np.int64) * rr.SUB)
        jj, ii, w0, w1, w2, s, z = (a[ok] for a in (jj, ii, w0, w1, w2, s, z))
        a, b, c = tri[0]
        # a dropped triangle aside (i1 == i2 has no area), the set-up swapped vertices 1 and 2 iff the second index changed
        k1, k2 = (2, 1) if b != int(faces[t][1]) else (1, 2)
        with np.errstate(all="ignore"):
            mix = lambda x0, x1, x2: ((w0 * x0 + w1 * x1) + w2 * x2) / s  # noqa: E731
            out["opacity"][0, jj, ii] = F(1.0)
            out["depth"][0, jj, ii] = z
            out["tri_id"][jj, ii] = t
            for k in range(3):
                out["pos"][k, jj, ii] = mix(view_pos[a, k], view_pos[b, k], view_pos[c, k])
            u = mix(uvs[t, 0, 0], uvs[t, k1, 0], uvs[t, k2, 0]).astype(F)
            v = mix(uvs[t, 0, 1], uvs[t, k1, 1], uvs[t, k2, 1]).astype(F)
            out["albedo"][:, jj, ii] = bilinear(albedo, u, v)
            o_r_m = bilinear(orm, u, v)
            out["occlusion"][0, jj, ii], out["roughness"][0, jj, ii], out["metallic"][0, jj, ii] = o_r_m
            if normal is not None:
                out["normal"][:, jj, ii] = bilinear(normal, u, v)
            else:
                for k in range(3):
                    out["normal"][k, jj, ii] = mix(normals[a, k], normals[b, k], normals[c, k])
    nx, ny, nz = out["normal"]
    with np.errstate(all="ignore"):  # normalize3(xform_vec_4x3(n, viewmatrix)): NaN for the zero vector
        vx = m[0] * nx + m[4] * ny + m[8] * nz
        vy = m[1] * nx + m[5] * ny + m[9] * nz
        vz = m[2] * nx + m[6] * ny + m[10] * nz
        inv = F(1.0) / np.sqrt(vx * vx + vy * vy + vz * vz)
        out["normal_view"] = np.stack([vx * inv, vy * inv, vz * inv]).astype(F)
    return out


def render_textured(mesh, uvs, albedo, orm, normal, cam):
    """project, raster and resolve_textured on a mesh dict (vertices, faces and, without a normal texture, normals)."""
    W, H = int(cam["image_width"]), int(cam["image_height"])
    view_pos, screen, flags = rr.project(mesh["vertices"], cam)
    vis = rr.raster(mesh["faces"], view_pos, screen, flags, W, H)
    out = resolve_textured(vis, mesh["faces"], view_pos, screen, flags, uvs, albedo, orm, normal, mesh.get("normals"),
                           cam["viewmatrix"])
    out.update(view_pos=view_pos, screen=screen, flags=flags, vis=vis)
    return out


# ---- what the tests share ---------------------------------------------------------------------------------------------------
QUAD = dict(x0=-0.5, x1=0.55, y0=-0.6, y1=0.62)  # world x and y of the quad's sides
# The float32 error of a lookup in quad_case against quad_expected, in units of e = 2^-24 (u, v <= 1; values up to M = 4;
# Wt = Ht = 8, so the texture changes by 1/8 per texel along x and by 3/8 along y):
#   the perspective interpolation (b = E / A, b / z, their sum, three products, two sums, a division): <= 10 e relative, so
#     10 e in u and in v, and 13 e in a component of `pos` (|pos| <= 1.3);
#   x = 8 u - 0.5: 80 e and a rounding of the product and of the difference at <= 8: 96 e of a texel; y has the rounding of
#     1 - v as well: 104 e.  In value: 96 / 8 + 3 * 104 / 8 = 51 e;
#   x - floor(x) is exact; 1 - fx, 1 - fy and the seven operations of the bilinear form on values <= M: 11 roundings, 44 e;
#   the texels are float32 roundings of u + 3 v <= 4, and the lookup is a convex combination of them: 4 e;
#   the expectation reads the float32 `pos` plane: 13 e of position are 13 / 1.05 * 7 / 8 = 11 e of u and 13 / 1.22 * 7 / 8 =
#     9.4 e of v: 11 + 3 * 9.4 = 39 e.
# 51 + 44 + 4 + 39 = 138 e.  The tests assert 256 e = 2^-16; a UV attached to the wrong corner is off by a texel or more (0.1).
QUAD_BOUND = 2.0 ** -16


def quad_case(W=rr.PW, H=rr.PH, Wt=8, Ht=8, back=False):
    """A quad of two triangles parallel to the image plane, the second listed with the opposite winding (from the front
    the second takes the A < 0 path of the set-up, from behind the first), with UVs on texel centres and the texture
    t = u + 3 v sampled at the texel centres: bilinear interpolation reproduces a function linear in texel coordinates
    between them.  -> (mesh dict, uvs [2,3,2], planes [3,Ht,Wt]: t, t / 4, 1 - t / 8, cam)."""
    q = QUAD
    vertices = np.array([(q["x0"], q["y0"], 0.0), (q["x1"], q["y0"], 0.0), (q["x1"], q["y1"], 0.0), (q["x0"], q["y1"], 0.0)],
                        np.float32)
    faces = np.array([(0, 1, 2), (0, 3, 2)], np.int32)
    corner = np.array([(0.5 / Wt, 0.5 / Ht), ((Wt - 0.5) / Wt, 0.5 / Ht), ((Wt - 0.5) / Wt, (Ht - 0.5) / Ht),
                       (0.5 / Wt, (Ht - 0.5) / Ht)], np.float32)
    uvs = np.ascontiguousarray(corner[faces])
    us, vs = (np.arange(Wt) + 0.5) / Wt, 1.0 - (np.arange(Ht) + 0.5) / Ht  # u and v of the texel centres; row 0 is the top
    tex = (us[None, :] + 3.0 * vs[:, None]).astype(np.float32)
    planes = np.stack([tex, 0.25 * tex, 1.0 - 0.125 * tex]).astype(np.float32)
    vm = np.eye(4, dtype=np.float32)  # p_view = [x y z 1] @ vm
    if back:  # a half turn about the y axis: the quad is seen from its other side
        vm[0, 0] = vm[2, 2] = -1.0
    vm[3, 2] = 2.0  # two units in front of the camera either way
    cam = dict(viewmatrix=vm, tanfovx=0.36, tanfovy=0.36 * H / W, image_width=W, image_height=H)
    mesh = dict(vertices=vertices, faces=faces, normals=np.tile(np.array([[0.0, 0.0, -1.0]], np.float32), (4, 1)))
    return mesh, uvs, planes, cam


def quad_expected(pos, cam, Wt=8, Ht=8):
    """t = u + 3 v [H,W] float64 of quad_case at the view-space positions `pos` [3,H,W] (the resolve's own plane, which no
    texture arithmetic touches): UV is affine in the world x and y of the quad."""
    q = QUAD
    sign = float(np.asarray(cam["viewmatrix"]).reshape(4, 4)[0, 0])  # -1 from behind: world x = -view x
    x, y = sign * pos[0].astype(np.float64), pos[1].astype(np.float64)
    u = 0.5 / Wt + (x - q["x0"]) / (q["x1"] - q["x0"]) * (Wt - 1.0) / Wt
    v = 0.5 / Ht + (y - q["y0"]) / (q["y1"] - q["y0"]) * (Ht - 1.0) / Ht
    return u + 3.0 * v
