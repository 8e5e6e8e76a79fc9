"""A trained scene as a mesh with its recovered materials: TSDF fusion of rendered planes, then naive surface nets.

    TSDFVolume(lo, voxel, dims, trunc)   the volume: integrate(cams, planes) fuses views (gigs_tsdf_integrate, up to 8 per
                                         launch), extract(min_weight) makes the mesh (gigs_mesh_count, two scans,
                                         gigs_mesh_write)
    auto_bounds(g)                       a box around the opaque Gaussians
    fuse_views(g, sh_degree, cams, gi, volume)   rasterizes each view (pipeline.rasterize, inference=True) and integrates
                                         its opacity, depth, world normal, albedo, roughness and metallic planes
    components(mesh)                     the connected components of a mesh's faces (gigs_mesh_cc_hook / _flatten until a
                                         pass changes nothing, gigs_mesh_cc_count)
    keep_threshold(counts, K, M)         the face count a component needs to be kept (host arithmetic)
    clean(mesh, keep_largest, min_faces) drops the components below that count, the invalid faces and the vertices no
                                         kept face references (gigs_mesh_mark, two scans, gigs_mesh_compact)
    cluster_map(mesh, cell, origin)      the cell cluster of every vertex (gigs_mesh_cluster_keys, a stable sort, a scan)
    simplify(mesh, cell, origin, reg)    one vertex per occupied cell, placed by the plane quadrics of its faces; collapsed
                                         and duplicate faces go (gigs_mesh_cluster_faces, gigs_mesh_cluster_solve,
                                         gigs_mesh_face_dedupe, then the mark / compact pair of clean)
    sample_surface(mesh, n, seed)        n stratified, area-weighted surface samples from a counter hash
                                         (gigs_mesh_face_areas, a scan, gigs_mesh_sample_surface)
    triangle_grid(mesh, cell)            a uniform grid of triangle lists (gigs_mesh_grid_count, a scan, gigs_mesh_grid_pairs,
                                         a sort)
    closest_point(points, mesh_b, ...)   the exact closest triangle of every point by an expanding-shell search of that grid
                                         (gigs_mesh_closest)
    distance(a, b, samples, ...)         both surfaces sampled and searched both ways: Chamfer, Hausdorff, one-sided
                                         statistics, precision / recall / F-score per threshold
    raycast(origins, directions, mesh)   the nearest usable face every ray hits, by a slab traversal of that grid
                                         (gigs_mesh_raycast)
    occlusion_directions(rays, rotations)   the bake's default direction table: a cosine-weighted spiral lattice (host)
    bake_occlusion(mesh, rays, ...)      per-vertex ambient occlusion, 1 = open: a wave per vertex casts `rays`
                                         cosine-distributed rays and counts the hits (gigs_mesh_bake_occlusion)
    trace_hemispheres(mesh, rays, ...)   the same rays with every hit recorded: face, side and weights
                                         (gigs_mesh_trace_hemisphere)
    gather_light(mesh, hits, cube, bounces)   per-vertex irradiance under an environment cube over those records: the
                                         shadowed sky plus `bounces` diffuse inter-reflections, a launch per pass
                                         (gigs_mesh_gather_light); bake_light runs both, sky_cube pools a light's cube (torch)
    gather_points(points, normals, mesh, cube, radiosity)   the same rays from ANY surface points (a G-buffer's pixels):
                                         occlusion, shadowed sky and bounced light in one launch (gigs_mesh_gather_points);
                                         final_gather bakes the vertex radiosity first
    reflect_points(points, normals, views, roughness, mesh, cube, radiosity)   a GGX lobe of rays about each point's mirror
                                         direction: traced specular radiance and specular occlusion
                                         (gigs_mesh_reflect_points); ggx_directions is its table of half vectors (host)
    atlas_layout(F, block, width)        the texture atlas of equal per-face charts, face_uvs(F, layout) its UVs (host)
    transfer_attributes(points, src, values)   per-vertex channels of src interpolated at the closest point of src to
                                         every query (gigs_mesh_closest, gigs_mesh_transfer)
    bake_atlas(dst, src, block, ...)     src's materials as albedo / ORM / normal planes over dst's atlas: a surface point
                                         per texel (gigs_mesh_atlas_points), the search, the transfer; sample_atlas looks
                                         the planes up again (torch)

The route is the one of 2DGS and GOF: depth and material planes of the training views go into a truncated signed
distance volume, and the mesh is its zero level set.  The arithmetic of both halves is stated in include/gigs_hip.h and
restated in numpy by tests/mesh_ref.py.  There is no CPU path: the volume lives on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

import gigs_lib

PLANE_KEYS = ("opacity", "depth", "normal", "albedo", "roughness", "metallic")
_PLANE_CHANNELS = {"opacity": 1, "depth": 1, "normal": 3, "albedo": 3, "roughness": 1, "metallic": 1}


class Mesh(NamedTuple):
    vertices: torch.Tensor   # [V,3]
    faces: torch.Tensor      # [F,3] int32
    normals: torch.Tensor    # [V,3] world, unit length (zero where no view gave one)
    albedo: torch.Tensor     # [V,3]
    roughness: torch.Tensor  # [V]
    metallic: torch.Tensor   # [V]


class MeshOverflow(RuntimeError):
    """The writing pass met an index outside its outputs: the volume changed between the counting and the writing pass."""


class MeshComponents(NamedTuple):
    labels: torch.Tensor       # [V] int32: the smallest vertex index of the vertex's component
    face_labels: torch.Tensor  # [F] int32: labels[faces[f,0]], -1 for an invalid face
    roots: torch.Tensor        # [C] int32: the components (roots with at least one face), ascending
    counts: torch.Tensor       # [C] int32: their valid faces
    invalid_faces: int
    rounds: int                # hook passes, the confirming one included


class ComponentsNotConverged(RuntimeError):
    """The labelling reached its cap on hook passes (cc_round_cap) with faces still joining trees: no labels are returned."""


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr() if t.numel() else None


def _sized(dev, v: int, f: int) -> Mesh:
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    return Mesh(torch.empty((v, 3), **f32), torch.empty((f, 3), **i32), torch.empty((v, 3), **f32),
                torch.empty((v, 3), **f32), torch.empty((v,), **f32), torch.empty((v,), **f32))


class TSDFVolume:
    """Samples s(i,j,k) = lo + (i,j,k) voxel, dims = (Gx, Gy, Gz), x fastest.  `tsdf` (initially 1), `weight` (0) and
    `attr_weight` (0) are [Gz,Gy,Gx] tensors; the eight attributes are kept planar ([8,Gz,Gy,Gx]: the hot pair tsdf /
    weight apart from the cold block) and `attributes()` gives them as [Gz,Gy,Gx,8] (world normal xyz, albedo rgb,
    roughness, metallic)."""

    def __init__(self, lo, voxel: float, dims, trunc: float, opacity_min: float = 0.5, carve: bool = True, device="cuda"):
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or any(d < 1 or d > gigs_lib.TSDF_MAX_AXIS for d in dims):
            raise ValueError("TSDFVolume: dims must be three sizes in 1..%d, got %s" % (gigs_lib.TSDF_MAX_AXIS, dims))
        if dims[0] * dims[1] * dims[2] >= 2 ** 31:
            raise ValueError("TSDFVolume: %d x %d x %d samples: the limit is 2^31 - 1" % dims)
        if not (voxel > 0 and trunc > 0):
            raise ValueError("TSDFVolume: voxel and trunc must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume: the volume must live on a CUDA/HIP device: gigs-hip has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lo = tuple(float(np.float32(v)) for v in lo)
        self.voxel, self.trunc, self.opacity_min, self.carve = float(np.float32(voxel)), float(np.float32(trunc)), float(
            np.float32(opacity_min)), bool(carve)
        self.dims = dims
        Gx, Gy, Gz = dims
        f32 = dict(dtype=torch.float32, device=self.device)
        self.tsdf = torch.ones((Gz, Gy, Gx), **f32)
        self.weight = torch.zeros((Gz, Gy, Gx), **f32)
        self.attr_weight = torch.zeros((Gz, Gy, Gx), **f32)
        self._attr = torch.zeros((8, Gz, Gy, Gx), **f32)

    @property
    def n_samples(self) -> int:
        return self.dims[0] * self.dims[1] * self.dims[2]

    def attributes(self) -> torch.Tensor:
        return self._attr.permute(1, 2, 3, 0).contiguous()

    def load(self, tsdf, weight, attr_weight, attributes) -> None:
        """Replace the fields: tsdf, weight, attr_weight [Gz,Gy,Gx], attributes [Gz,Gy,Gx,8] (tensors or arrays)."""
        Gx, Gy, Gz = self.dims
        t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(self.device)  # noqa: E731
        tsdf, weight, attr_weight, attributes = t(tsdf), t(weight), t(attr_weight), t(attributes)
        for name, a, shape in (("tsdf", tsdf, (Gz, Gy, Gx)), ("weight", weight, (Gz, Gy, Gx)),
                               ("attr_weight", attr_weight, (Gz, Gy, Gx)), ("attributes", attributes, (Gz, Gy, Gx, 8))):
            if tuple(a.shape) != shape:
                raise ValueError("TSDFVolume.load: %s must be %s, got %s" % (name, shape, tuple(a.shape)))
        self.tsdf.copy_(tsdf)
        self.weight.copy_(weight)
        self.attr_weight.copy_(attr_weight)
        self._attr.copy_(attributes.permute(3, 0, 1, 2))

    def _grid(self) -> gigs_lib.TsdfGrid:
        g = gigs_lib.TsdfGrid()
        g.lo[:] = self.lo
        g.dims[:] = self.dims
        g.voxel, g.trunc, g.opacity_min, g.carve = self.voxel, self.trunc, self.opacity_min, int(self.carve)
        g.tsdf, g.weight, g.attr_weight, g.attr = (self.tsdf.data_ptr(), self.weight.data_ptr(), self.attr_weight.data_ptr(),
                                                   self._attr.data_ptr())
        return g

    def _plane(self, p: Dict, key: str, H: int, W: int) -> torch.Tensor:
        t = p[key]
        if not isinstance(t, torch.Tensor) or t.device != self.device:
            raise RuntimeError("TSDFVolume.integrate: plane %r must be a tensor on %s" % (key, self.device))
        c = _PLANE_CHANNELS[key]
        if t.numel() != c * H * W or tuple(t.shape[-2:]) != (H, W):
            raise ValueError("TSDFVolume.integrate: plane %r must be [%d,%d,%d], got %s" % (key, c, H, W, tuple(t.shape)))
        return t.detach().float().contiguous()

    def integrate(self, cams, planes) -> None:
        """Fuse views in order.  `cams`: a camera dict (viewmatrix, tanfovx, tanfovy, image_width, image_height) or a list
        of them; `planes`: per view a dict with the PLANE_KEYS tensors ([C,H,W]; [H,W] for one channel).  Lists go to the
        device eight views per launch."""
        if isinstance(cams, dict):
            cams, planes = [cams], [planes]
        cams, planes = list(cams), list(planes)
        if len(cams) != len(planes):
            raise ValueError("TSDFVolume.integrate: %d cameras, %d plane sets" % (len(cams), len(planes)))
        lib = gigs_lib.lib()
        grid = self._grid()
        with torch.cuda.device(self.device):
            for b in range(0, len(cams), gigs_lib.TSDF_MAX_VIEWS):
                chunk = list(zip(cams[b:b + gigs_lib.TSDF_MAX_VIEWS], planes[b:b + gigs_lib.TSDF_MAX_VIEWS]))
                views = (gigs_lib.TsdfView * len(chunk))()
                keep = []
                for v, (cam, p) in zip(views, chunk):
                    H, W = int(cam["image_height"]), int(cam["image_width"])
                    vm = cam["viewmatrix"]
                    vm = vm.detach().cpu().numpy() if isinstance(vm, torch.Tensor) else np.asarray(vm)
                    v.viewmatrix[:] = [float(x) for x in np.ascontiguousarray(vm, dtype=np.float32).reshape(16)]
                    v.tanfovx, v.tanfovy, v.width, v.height = float(cam["tanfovx"]), float(cam["tanfovy"]), W, H
                    for key in PLANE_KEYS:
                        t = self._plane(p, key, H, W)
                        keep.append(t)
                        setattr(v, key, t.data_ptr())
                gigs_lib.check(lib.gigs_tsdf_integrate(C.byref(grid), len(chunk), views, _stream()), "tsdf_integrate")
                del keep  # the launch is queued on the current stream: the caching allocator keeps stream order

    def extract(self, min_weight: float = 1) -> Mesh:
        """The zero level set by naive surface nets: one vertex per active cell (ascending cell index), two triangles per
        crossed grid edge whose four cells are valid (ordered by sample index, then axis)."""
        dev = self.device
        i32 = dict(dtype=torch.int32, device=dev)
        Gx, Gy, Gz = self.dims
        cells = (Gx - 1) * (Gy - 1) * (Gz - 1)
        if cells == 0:
            return _sized(dev, 0, 0)
        lib = gigs_lib.lib()
        grid = self._grid()
        with torch.cuda.device(dev):
            flags = torch.empty(cells, **i32)
            quads = torch.empty(self.n_samples, **i32)
            gigs_lib.check(lib.gigs_mesh_count(C.byref(grid), float(min_weight), flags.data_ptr(), quads.data_ptr(), _stream()),
                           "mesh_count")
            cell_incl = torch.cumsum(flags, 0, dtype=torch.int32)
            quad_incl = torch.cumsum(quads, 0, dtype=torch.int32)
            V, Q = (int(x) for x in torch.stack((cell_incl[-1], quad_incl[-1])).cpu())  # the one read-back
            if V == 0:
                return _sized(dev, 0, 0)
            cell_off, quad_off = cell_incl - flags, quad_incl - quads
            F = 2 * Q
            m = _sized(dev, V, F)
            overflow = torch.zeros(1, **i32)
            gigs_lib.check(lib.gigs_mesh_write(C.byref(grid), float(min_weight), cell_off.data_ptr(), quad_off.data_ptr(), V, F,
                                               m.vertices.data_ptr(), m.normals.data_ptr(), m.albedo.data_ptr(),
                                               m.roughness.data_ptr(), m.metallic.data_ptr(), m.faces.data_ptr() if F else None,
                                               overflow.data_ptr(), _stream()), "mesh_write")
            if int(overflow.item()) != 0:
                raise MeshOverflow("TSDFVolume.extract: an index left the outputs (%d vertices, %d faces)" % (V, F))
        return m


def auto_bounds(g: Dict, quantile: float = 0.01, margin: float = 0.05):
    """(lo, hi), two float32 arrays [3]: per axis the [quantile, 1 - quantile] range of the centres of the Gaussians
    with opacity > 0.5, grown on both sides by `margin` times its length.  `g`: means3D [P,3], opacities [P,1] (tensors or
    arrays)."""
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    xyz = as_np(g["means3D"]).astype(np.float64)
    keep = as_np(g["opacities"]).reshape(-1) > 0.5
    if not keep.any():
        raise ValueError("auto_bounds: no Gaussian has opacity > 0.5")
    lo = np.quantile(xyz[keep], quantile, axis=0)
    hi = np.quantile(xyz[keep], 1.0 - quantile, axis=0)
    pad = margin * (hi - lo)
    return (lo - pad).astype(np.float32), (hi + pad).astype(np.float32)


def grid_for_bounds(lo, hi, grid: int):
    """(voxel, dims): `grid` samples along the longest axis of the box, the other axes cut to cover theirs."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    if grid < 2 or not (ext > 0).all():
        raise ValueError("grid_for_bounds: need grid >= 2 and a box with positive extent")
    voxel = float(ext.max()) / (grid - 1)
    dims = tuple(int(min(grid, max(2, int(np.ceil(e / voxel - 1e-9)) + 1))) for e in ext)
    return voxel, dims


def view_planes(out) -> Dict[str, torch.Tensor]:
    """The planes integrate() takes, out of the operator's 12-tuple (pipeline.rasterize)."""
    return dict(opacity=out[2], depth=out[3], normal=out[5], albedo=out[7], roughness=out[8], metallic=out[9])


def fuse_views(g: Dict[str, torch.Tensor], sh_degree: int, cams: Sequence[Dict], gi: Dict, volume: TSDFVolume,
               keep_planes: bool = False) -> List[Dict[str, torch.Tensor]]:
    """Rasterize every camera of `cams` (inference mode, black background) and integrate it into `volume`, eight views per
    launch.  Returns the planes of every view with keep_planes (for tests), else an empty list."""
    import pipeline
    dev = volume.device
    bg = torch.zeros(3, device=dev)
    kept: List[Dict[str, torch.Tensor]] = []
    with torch.no_grad():
        for b in range(0, len(cams), gigs_lib.TSDF_MAX_VIEWS):
            batch = list(cams[b:b + gigs_lib.TSDF_MAX_VIEWS])
            planes = [view_planes(pipeline.rasterize(c, g, sh_degree, bg, gi, inference=True)[0]) for c in batch]
            volume.integrate(batch, planes)
            if keep_planes:
                kept.extend(planes)
    return kept


# ---- cleaning: connected components, the keep rule, compaction (include/gigs_hip.h, "Cleaning meshes") -----------------------
def cc_round_cap(n_vertices: int) -> int:
    """The most hook passes components() runs: 2 ceil(log2 V) + 8.  In every pass and under every schedule, a tree that a
    face joins to a tree with a smaller root stops being a root: only the local minima among the trees survive a pass.
    In the synchronous model of a pass (every face reads the forest the last pass left) a tree that survives two passes
    in a row has taken every neighbouring tree into itself -- had one of them gone elsewhere, it went under a smaller
    root, which the survivor then touches -- so it absorbed at least one tree, and that tree is its alone: the trees of a
    component at least halve every two passes, 2 ceil(log2 V) passes plus the confirming one.  (One pass does not halve
    them: a star whose centre has the largest root loses only the centre.)  The asynchronous schedule differs from the
    model in that a root may be offered a vertex further down its neighbour's chain, or overtaken; it is not proved to keep
    the factor, hence the margin of 7 passes, and hence an error and no labels at the cap ("Cleaning meshes",
    has the observed counts).  Progress never depends on the cap: a pass that changes something removes a root."""
    return 2 * max(int(n_vertices) - 1, 0).bit_length() + 8


def _mesh_tensors(mesh, what: str) -> Mesh:
    m = mesh if isinstance(mesh, Mesh) else Mesh(*mesh)
    dev = m.vertices.device if isinstance(m.vertices, torch.Tensor) else None
    for name, t in zip(Mesh._fields, m):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda" or t.device != dev:
            raise RuntimeError("%s: %s must be a tensor on one CUDA/HIP device: gigs-hip has no CPU path" % (what, name))
    V = int(m.vertices.shape[0])
    if m.faces.dtype != torch.int32 or m.faces.dim() != 2 or m.faces.shape[1] != 3:
        raise ValueError("%s: faces must be [F,3] int32, got %s %s" % (what, tuple(m.faces.shape), m.faces.dtype))
    for name, shape in (("vertices", (V, 3)), ("normals", (V, 3)), ("albedo", (V, 3)), ("roughness", (V,)), ("metallic", (V,))):
        t = getattr(m, name)
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError("%s: %s must be %s float32, got %s %s" % (what, name, shape, tuple(t.shape), t.dtype))
    return Mesh(*(t.contiguous() for t in m))


def _label(m: Mesh):
    """-> (labels [V], face_labels [F], count [V] per root, invalid (device int [1]), rounds)."""
    dev = m.vertices.device
    i32 = dict(dtype=torch.int32, device=dev)
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    lib = gigs_lib.lib()
    parent = torch.arange(V, **i32)
    face_labels, count = torch.empty(F, **i32), torch.empty(V, **i32)
    flag = torch.zeros(2, **i32)  # changed, invalid faces
    rounds = 0
    if V and F:
        cap = cc_round_cap(V)
        while True:
            gigs_lib.check(lib.gigs_mesh_cc_hook(V, F, _p(m.faces), _p(parent), flag.data_ptr(), _stream()), "mesh_cc_hook")
            rounds += 1
            if int(flag[0].item()) == 0:  # the one read-back of a round
                break
            if rounds >= cap:
                raise ComponentsNotConverged("components: %d hook passes over %d vertices and faces still join trees" % (rounds, V))
            gigs_lib.check(lib.gigs_mesh_cc_flatten(V, _p(parent), _stream()), "mesh_cc_flatten")
    gigs_lib.check(lib.gigs_mesh_cc_count(V, F, _p(m.faces), _p(parent), _p(face_labels), _p(count), flag[1:].data_ptr(),
                                          _stream()), "mesh_cc_count")
    return parent, face_labels, count, flag[1:], rounds


def components(mesh) -> MeshComponents:
    """The connected components of the valid faces of `mesh` (a Mesh on the device), by vertex connectivity: two shells that
    share one vertex are one component.  V == 0 or F == 0 launches nothing."""
    m = _mesh_tensors(mesh, "components")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    if V == 0 or F == 0:
        return MeshComponents(torch.arange(V, **i32), torch.full((F,), -1, **i32), torch.empty(0, **i32), torch.empty(0, **i32),
                              F, 0)
    with torch.cuda.device(dev):
        labels, face_labels, count, invalid, rounds = _label(m)
        roots = torch.nonzero(count > 0).reshape(-1).to(torch.int32)  # a face's label is a root: count > 0 only at roots
        counts = count[roots.long()]
        return MeshComponents(labels, face_labels, roots, counts, int(invalid.item()), rounds)


def keep_threshold(counts, keep_largest: int = 0, min_faces: int = 0) -> int:
    """The face count a component needs: max(min_faces, c_K, 1) with c_K the keep_largest-th largest of `counts` (the face
    counts of the components, each >= 1; a tensor, an array or a list), 0 for keep_largest <= 0 and the smallest count for
    keep_largest >= len(counts).  Components tied with the K-th reach it too.  Sorts where the counts live."""
    c = torch.as_tensor(counts).reshape(-1)
    K, n = int(keep_largest), int(c.numel())
    c_k = 0
    if K > 0 and n > 0:
        c_k = int(torch.sort(c, descending=True).values[min(K, n) - 1].item())
    return max(int(min_faces), c_k, 1)


def _compact(what: str, src: Mesh, faces, face_labels, root_keep, extra=(), check=None):
    """The tail of clean() and simplify(): keeps the valid faces of `faces` ([F,3], indices into the vertex rows of `src`;
    src.faces is not read) whose label ([F]) has root_keep ([rows] uint8) set, and the vertices they reference:
    gigs_mesh_mark, two scans, the one read-back, gigs_mesh_compact.  `extra`: 1-D int32 device tensors fetched in that
    read-back; `check(values)` sees their values before anything is sized.  -> (Mesh, values).  Errors name `what`."""
    dev = src.vertices.device
    V, F = int(src.vertices.shape[0]), int(faces.shape[0])
    i32 = dict(dtype=torch.int32, device=dev)
    lib = gigs_lib.lib()
    face_keep, vertex_keep = torch.empty(F, **i32), torch.empty(V, **i32)
    gigs_lib.check(lib.gigs_mesh_mark(V, F, _p(faces), _p(face_labels), _p(root_keep), _p(face_keep), _p(vertex_keep), _stream()),
                   "mesh_mark")
    v_incl = torch.cumsum(vertex_keep, 0, dtype=torch.int32)
    f_incl = torch.cumsum(face_keep, 0, dtype=torch.int32)
    V2, F2, *got = (int(x) for x in torch.cat((v_incl[-1:], f_incl[-1:], *extra)).cpu())
    if check is not None:
        check(got)
    out = _sized(dev, V2, F2)
    if V2 and F2:
        v_off, f_off = v_incl - vertex_keep, f_incl - face_keep
        overflow = torch.zeros(1, **i32)
        gigs_lib.check(lib.gigs_mesh_compact(
            V, F, _p(src.vertices), _p(src.normals), _p(src.albedo), _p(src.roughness), _p(src.metallic), _p(faces),
            _p(vertex_keep), _p(v_off), _p(face_keep), _p(f_off), V2, F2, _p(out.vertices), _p(out.normals), _p(out.albedo),
            _p(out.roughness), _p(out.metallic), _p(out.faces), overflow.data_ptr(), _stream()), "mesh_compact")
        if int(overflow.item()) != 0:
            raise MeshOverflow("%s: an index left the outputs (%d vertices, %d faces)" % (what, V2, F2))
    return out, got


def clean(mesh, keep_largest: int = 0, min_faces: int = 0) -> Tuple[Mesh, Dict]:
    """(the mesh without the components of fewer than keep_threshold faces, a report).  Invalid faces and the vertices no
    kept face references go too; with keep_largest = min_faces = 0 nothing else does.  Kept vertices and faces stay in
    their order, values are copied bit for bit.  Report: components, components_kept, faces_removed, vertices_removed,
    invalid_faces, rounds, threshold."""
    m = _mesh_tensors(mesh, "clean")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    if V == 0 or F == 0:
        return _sized(dev, 0, 0), dict(components=0, components_kept=0, faces_removed=F, vertices_removed=V, invalid_faces=F,
                                       rounds=0, threshold=keep_threshold([], keep_largest, min_faces))
    with torch.cuda.device(dev):
        labels, face_labels, count, invalid, rounds = _label(m)
        comp = count > 0
        thr = keep_threshold(count[comp], keep_largest, min_faces)
        root_keep = (count >= thr).to(torch.uint8)
        n = lambda t: t.sum().to(torch.int32).reshape(1)  # noqa: E731
        out, (n_comp, n_kept, n_invalid) = _compact("clean", m, m.faces, face_labels, root_keep, (n(comp), n(root_keep), invalid))
    V2, F2 = int(out.vertices.shape[0]), int(out.faces.shape[0])
    return out, dict(components=n_comp, components_kept=n_kept, faces_removed=F - F2, vertices_removed=V - V2,
                     invalid_faces=n_invalid, rounds=rounds, threshold=thr)


# ---- simplifying: vertex clustering with quadric placement (include/gigs_hip.h, "Simplifying meshes") ------------------------
CELL_AXIS = 1 << 21  # cell coordinates per axis: three of them share an int64 key


def cluster_grid(lo, hi, cell, origin=None):
    """(origin float32 [3], inv float32) of the cell grid over vertices with the finite extent lo .. hi (float32 [3] each;
    lo = +inf where no vertex is finite).  Host arithmetic.  ValueError for a cell that is not positive (or whose
    reciprocal is not finite in float32), an origin that is not finite, or an extent that needs a cell coordinate of 2^21
    or more on some axis."""
    cell32 = np.float32(cell)
    if not (np.isfinite(cell32) and cell32 > 0):
        raise ValueError("simplify: cell must be positive, got %r" % (cell,))
    with np.errstate(over="ignore", invalid="ignore"):
        inv = np.float32(1) / cell32
        if not np.isfinite(inv):
            raise ValueError("simplify: 1 / cell is not finite in float32 (cell = %r)" % (cell,))
        lo, hi = np.asarray(lo, np.float32).reshape(3), np.asarray(hi, np.float32).reshape(3)
        some = bool(np.isfinite(lo).all() and np.isfinite(hi).all())
        if some:
            top = np.floor((hi - lo) * inv)
            if not bool((top < CELL_AXIS).all()):
                raise ValueError("simplify: the extent %s at cell %g needs more than 2^21 cells on an axis"
                                 % ((hi.astype(np.float64) - lo).tolist(), float(cell32)))
    if origin is None:
        org = lo.copy() if some else np.zeros(3, np.float32)
    else:
        org = np.asarray(origin, np.float32).reshape(3).copy()
        if not np.isfinite(org).all():
            raise ValueError("simplify: origin must be finite, got %r" % (origin,))
    return org, inv


class _Clusters(NamedTuple):
    cluster_of: torch.Tensor    # [V] int32, -1 for an unclustered vertex
    n: int                      # C
    order: torch.Tensor         # [V] int64: the vertices sorted by (key, index), the unclustered ones first
    member_start: torch.Tensor  # [C+1] int64: the first row of every cluster in `order`, then V
    keys: torch.Tensor          # [C] int64
    unclustered: torch.Tensor   # [] the number of unclustered vertices, on the device
    origin: np.ndarray
    inv: np.float32


def _c_origin(org):
    return (C.c_float * 3)(*(float(x) for x in org))


def _cluster(m: Mesh, cell, origin) -> _Clusters:
    """Two read-backs: the extent and C."""
    dev = m.vertices.device
    V = int(m.vertices.shape[0])
    v = m.vertices
    finite = torch.isfinite(v).all(1, keepdim=True)
    ext = torch.stack((v.masked_fill(~finite, float("inf")).amin(0), v.masked_fill(~finite, float("-inf")).amax(0))).cpu().numpy()
    org, inv = cluster_grid(ext[0], ext[1], cell, origin)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_cluster_keys(V, _p(v), _c_origin(org), float(inv), _p(keys), _stream()),
                   "mesh_cluster_keys")
    skeys, order = torch.sort(keys, stable=True)
    head = torch.ones(V, dtype=torch.bool, device=dev)
    head[1:] = skeys[1:] != skeys[:-1]
    head &= skeys >= 0
    ids = torch.cumsum(head, 0, dtype=torch.int32) - 1  # -1 on the unclustered rows: they sort first
    cluster_of = torch.empty(V, dtype=torch.int32, device=dev)
    cluster_of[order] = ids
    starts = torch.nonzero(head).reshape(-1)  # its length is C: the read-back
    member_start = torch.cat((starts, starts.new_tensor([V])))
    return _Clusters(cluster_of, int(starts.numel()), order, member_start, skeys[starts], (skeys < 0).sum(), org, inv)


def _check_cell(cell, reg=1e-3):
    if not (float(cell) > 0):
        raise ValueError("simplify: cell must be positive, got %r" % (cell,))
    if not (0 < float(reg) <= 1):
        raise ValueError("simplify: reg must lie in (0, 1], got %r" % (reg,))


def cluster_map(mesh, cell, origin=None) -> Tuple[torch.Tensor, int]:
    """(cluster_of [V] int32, C): the cluster of every vertex of `mesh` on the grid of `cell`-sized cells from `origin`
    (default: the minimum of the finite vertices), -1 for a vertex that is not finite or lies outside the 2^21 cells of an
    axis.  Clusters are numbered in ascending key order (x fastest)."""
    _check_cell(cell)
    m = _mesh_tensors(mesh, "cluster_map")
    if int(m.vertices.shape[0]) == 0:
        return torch.empty(0, dtype=torch.int32, device=m.vertices.device), 0
    with torch.cuda.device(m.vertices.device):
        cl = _cluster(m, cell, origin)
    return cl.cluster_of, cl.n


def median_edge(mesh) -> float:
    """The (lower) median length of the 3 F' edges of the F' valid faces of `mesh`, computed where the mesh lives; 0.0
    without a valid face with finite edges."""
    m = _mesh_tensors(mesh, "median_edge")
    V = int(m.vertices.shape[0])
    f = m.faces.long()
    f = f[((f >= 0) & (f < V)).all(1)]
    if f.numel() == 0:
        return 0.0
    p = m.vertices[f]  # [F',3,3]
    e = (p - p.roll(-1, 1)).double().norm(dim=2).reshape(-1)
    e = e[torch.isfinite(e)]
    return float(e.median().item()) if e.numel() else 0.0


def simplify(mesh, cell, origin=None, reg: float = 1e-3) -> Tuple[Mesh, Dict]:
    """(the mesh with one vertex per occupied cell of the `cell`-sized grid from `origin`, a report).  The vertex of a cell
    minimises the area-weighted plane quadrics of the faces that touch the cell, regularised towards the member mean by
    `reg` and clamped to the cell; its attributes are the member means (the normal: the normalised member sum).  Faces
    with two vertices in one cell, faces that repeat an earlier face's cluster triple and invalid faces go, then the
    clusters nothing references.  Report: clusters, vertices, faces, faces_in, vertices_in, faces_collapsed,
    faces_duplicate, faces_invalid, vertices_unclustered, cell, origin.  V == 0 or F == 0 launches nothing."""
    _check_cell(cell, reg)
    m = _mesh_tensors(mesh, "simplify")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)

    def report(org, **kw):
        r = dict(clusters=0, vertices=0, faces=0, faces_in=F, vertices_in=V, faces_collapsed=0, faces_duplicate=0,
                 faces_invalid=0, vertices_unclustered=0, cell=float(np.float32(cell)), origin=[float(x) for x in org])
        r.update(kw)
        return r

    if V == 0 or F == 0:
        org = np.zeros(3, np.float32) if origin is None else np.asarray(origin, np.float32).reshape(3)
        return _sized(dev, 0, 0), report(org, faces_invalid=F if V == 0 else 0)
    lib = gigs_lib.lib()
    with torch.cuda.device(dev):
        cl = _cluster(m, cell, origin)
        Cn = cl.n
        if Cn == 0:
            return _sized(dev, 0, 0), report(cl.origin, faces_invalid=F, vertices_unclustered=V)
        triples, pairs, counts = torch.empty((F, 3), **i32), torch.empty(3 * F, **i64), torch.empty(2, **i32)
        gigs_lib.check(lib.gigs_mesh_cluster_faces(V, F, Cn, _p(m.faces), _p(cl.cluster_of), _p(triples), _p(pairs), _p(counts),
                                                   _stream()), "mesh_cluster_faces")
        pairs = torch.sort(pairs).values  # (cluster, face) ascending; the sentinels last
        pair_start = torch.searchsorted(pairs, torch.arange(Cn + 1, **i64) << 32)
        cv = _sized(dev, Cn, 0)
        flags = torch.zeros(2, **i32)  # overflow, duplicates
        gigs_lib.check(lib.gigs_mesh_cluster_solve(
            V, F, Cn, _p(m.vertices), _p(m.normals), _p(m.albedo), _p(m.roughness), _p(m.metallic), _p(m.faces), _p(cl.order),
            _p(cl.member_start), _p(pairs), _p(pair_start), _p(cl.keys), _c_origin(cl.origin), float(np.float32(cell)), float(reg),
            _p(cv.vertices), _p(cv.normals), _p(cv.albedo), _p(cv.roughness), _p(cv.metallic), flags.data_ptr(), _stream()),
            "mesh_cluster_solve")
        # the faces in the order of their triples, ties in ascending face index: two stable sorts, last column first
        t = triples.long()
        by_last = torch.sort(t[:, 2], stable=True).indices
        order = by_last[torch.sort(((t[:, 0] << 32) | t[:, 1])[by_last], stable=True).indices]
        faces = torch.empty((F, 3), **i32)
        gigs_lib.check(lib.gigs_mesh_face_dedupe(F, _p(triples), _p(order), _p(faces), flags[1:].data_ptr(), flags.data_ptr(),
                                                 _stream()), "mesh_face_dedupe")
        # clean(.., 0, 0)'s compaction without its labelling: every face that is still a triple is kept
        def solved(got):  # its own flag, from the same read-back and before anything is compacted
            if got[2] != 0:
                raise MeshOverflow("simplify: an index left its range (%d clusters, %d faces)" % (Cn, F))

        out, (n_invalid, n_collapsed, _, n_dup, n_unclustered) = _compact(
            "simplify", cv, faces, torch.zeros(F, **i32), torch.ones(Cn, dtype=torch.uint8, device=dev),
            (counts, flags, cl.unclustered.to(torch.int32).reshape(1)), solved)
    V2, F2 = int(out.vertices.shape[0]), int(out.faces.shape[0])
    return out, report(cl.origin, clusters=Cn, vertices=V2, faces=F2, faces_collapsed=n_collapsed, faces_duplicate=n_dup,
                       faces_invalid=n_invalid, vertices_unclustered=n_unclustered)


# ---- comparing: surface samples, the triangle grid, the closest triangle (include/gigs_hip.h, "Comparing meshes") ------------
GRID_AXIS = 256  # cells per axis of the triangle grid


class _Areas(NamedTuple):
    areas: torch.Tensor  # [F] float64, 0 for an unusable face
    skipped: torch.Tensor  # [1] int32 on the device


def _face_areas(m: Mesh) -> _Areas:
    dev = m.vertices.device
    F = int(m.faces.shape[0])
    areas, skipped = torch.empty(F, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_face_areas(int(m.vertices.shape[0]), F, _p(m.vertices), _p(m.faces), _p(areas),
                                                       skipped.data_ptr(), _stream()), "mesh_face_areas")
    return _Areas(areas, skipped)


def sample_surface(mesh, n: int, seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(points [n,3] float32, face [n] int32, bary [n,2] float32): n stratified, area-weighted samples of the usable faces
    of `mesh` (indices in range, finite corners, area > 0), a pure function of (mesh, n, seed): sample i takes the i-th of n
    equal slices of the cumulative area and its random numbers from a counter hash of (seed, i).  A mesh without area, or
    n == 0, gives empty tensors and launches nothing."""
    m = _mesh_tensors(mesh, "sample_surface")
    dev = m.vertices.device
    n, seed = int(n), int(seed)
    if n < 0 or n >= 2 ** 31:
        raise ValueError("sample_surface: n must lie in [0, 2^31), got %d" % n)
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    empty = (torch.empty((0, 3), **f32), torch.empty((0,), **i32), torch.empty((0, 2), **f32))
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    if n == 0 or V == 0 or F == 0:
        return empty
    with torch.cuda.device(dev):
        cum = torch.cumsum(_face_areas(m).areas, 0)
        A = float(cum[-1].item())  # the one read-back
        if not (A > 0 and np.isfinite(A)):
            return empty
        points, face, bary = torch.empty((n, 3), **f32), torch.empty(n, **i32), torch.empty((n, 2), **f32)
        overflow = torch.zeros(1, **i32)
        gigs_lib.check(gigs_lib.lib().gigs_mesh_sample_surface(V, F, _p(m.vertices), _p(m.faces), _p(cum), n,
                                                               seed & 0xFFFFFFFFFFFFFFFF, _p(points), _p(face), _p(bary),
                                                               overflow.data_ptr(), _stream()), "mesh_sample_surface")
        if int(overflow.item()) != 0:
            raise MeshOverflow("sample_surface: a sample fell on a face with an index outside the %d vertices" % V)
    return points, face, bary


class TriangleGrid(NamedTuple):
    lo: np.ndarray             # [3] float32: the minimum corner of the usable faces
    cell: float
    dims: Tuple[int, int, int]
    cell_start: torch.Tensor   # [cells + 1] int64
    pairs: torch.Tensor        # [n_pairs] int64, sorted: cell << 32 | face
    faces_skipped: int
    hi: np.ndarray = None      # [3] float32: the maximum corner of the usable faces


def grid_dims(lo, hi, cell) -> Tuple[float, Tuple[int, int, int]]:
    """(cell, (Gx, Gy, Gz)): `cell` as a float32 value, raised if the longest axis of lo .. hi would need more than 256 of
    them; G = clamp(ceil(extent / cell), 1, 256) per axis.  Host arithmetic."""
    ext = np.asarray(hi, np.float32).astype(np.float64) - np.asarray(lo, np.float32).astype(np.float64)
    cell = float(np.float32(cell))
    need = float(ext.max()) / GRID_AXIS
    if cell < need:
        cell = float(np.nextafter(np.float32(need), np.float32(np.inf)))
    return cell, tuple(int(min(max(np.ceil(e / cell), 1), GRID_AXIS)) for e in ext)


def _c_grid(lo, dims):
    return (C.c_float * 3)(*(float(x) for x in lo)), (C.c_int * 3)(*(int(d) for d in dims))


def triangle_grid(mesh, cell=None):
    """The uniform grid of triangle lists over the usable faces of `mesh`, or None if it has none.  `cell` defaults to twice
    median_edge(mesh); it is doubled while the lists would hold more than 8 F + 4096 (cell, face) pairs.  Read-backs: the
    box (with the skipped faces), and the pair total of every attempt."""
    m = _mesh_tensors(mesh, "triangle_grid")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    if V == 0 or F == 0:
        return None
    if cell is not None and not (float(cell) > 0 and np.isfinite(float(cell))):
        raise ValueError("triangle_grid: cell must be positive and finite, got %r" % (cell,))
    lib = gigs_lib.lib()
    with torch.cuda.device(dev):
        ar = _face_areas(m)
        usable = ar.areas > 0
        corners = m.vertices[m.faces[usable].long().reshape(-1)]
        if corners.shape[0] == 0:  # a shape: the mask was read back by the indexing
            return None
        box = torch.cat((corners.amin(0), corners.amax(0), ar.skipped.float())).cpu().numpy()
        lo, hi, skipped = box[:3].astype(np.float32), box[3:6].astype(np.float32), int(box[6])
        if cell is None:
            cell = 2.0 * median_edge(m)
            if not (cell > 0 and np.isfinite(cell)):
                cell = float((hi.astype(np.float64) - lo).max())
        counts = torch.empty(F, dtype=torch.int32, device=dev)
        while True:
            cell, dims = grid_dims(lo, hi, cell)
            c_lo, c_dims = _c_grid(lo, dims)
            gigs_lib.check(lib.gigs_mesh_grid_count(V, F, _p(m.vertices), _p(m.faces), _p(ar.areas), c_lo, cell, c_dims,
                                                    _p(counts), _stream()), "mesh_grid_count")
            incl = torch.cumsum(counts, 0, dtype=torch.int64)
            total = int(incl[-1].item())
            if total <= 8 * F + 4096:
                break
            cell = 2.0 * cell
        pairs = torch.empty(total, dtype=torch.int64, device=dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        gigs_lib.check(lib.gigs_mesh_grid_pairs(V, F, _p(m.vertices), _p(m.faces), _p(ar.areas), c_lo, cell, c_dims,
                                                _p(incl - counts), total, _p(pairs), overflow.data_ptr(), _stream()),
                       "mesh_grid_pairs")
        pairs = torch.sort(pairs).values
        cells = dims[0] * dims[1] * dims[2]
        cell_start = torch.searchsorted(pairs, torch.arange(cells + 1, dtype=torch.int64, device=dev) << 32)
        if int(overflow.item()) != 0:
            raise MeshOverflow("triangle_grid: a face's cells left the %d pairs counted for them" % total)
    return TriangleGrid(lo, cell, dims, cell_start, pairs, skipped, hi)


def _closest(points: torch.Tensor, m: Mesh, grid, max_distance):
    """-> (distance [N] float32, face [N] int32, flags [3] int32 on the device: far, invalid, overflow)."""
    dev = m.vertices.device
    N = int(points.shape[0])
    distance = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    face = torch.full((N,), -1, dtype=torch.int32, device=dev)
    flags = torch.zeros(3, dtype=torch.int32, device=dev)
    if N == 0:
        return distance, face, flags
    if grid is None:  # no usable face: nothing is launched
        flags[1] = (~torch.isfinite(points).all(1)).sum()
        return distance, face, flags
    order = _cell_order(points.double(), grid)  # lanes of a wave share lists
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_closest(
        int(m.vertices.shape[0]), int(m.faces.shape[0]), _p(m.vertices), _p(m.faces), c_lo, grid.cell, c_dims,
        _p(grid.cell_start), _p(grid.pairs), int(grid.pairs.shape[0]), N, _p(points), _p(order),
        float("inf") if max_distance is None else float(max_distance), _p(distance), _p(face), flags.data_ptr(),
        flags[2:].data_ptr(), _stream()), "mesh_closest")
    return distance, face, flags


def _check_max_distance(max_distance):
    if max_distance is not None and not (float(max_distance) >= 0):
        raise ValueError("max_distance must be >= 0 or None, got %r" % (max_distance,))


def closest_point(points, mesh_b, cell=None, max_distance=None, grid=None) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """(distance [N] float32, face [N] int32, report): for every point of `points` ([N,3] float32 on the mesh's device) the
    distance to the closest usable triangle of `mesh_b` and its index (the smallest among equally close ones).  With
    `max_distance`, a point with no triangle within it gets that distance and face -1 (report: far), and the search stops
    there: without it a point far from the mesh walks O(G^3) cell headers alone.  A point with a non-finite coordinate
    gets +inf and -1 (queries_invalid), as does every point if the mesh has no usable face.  `cell`: the grid's cell
    (triangle_grid), or pass a `grid` built before.  Report: n, far, queries_invalid, faces_skipped, cell, dims, pairs."""
    _check_max_distance(max_distance)
    m = _mesh_tensors(mesh_b, "closest_point")
    dev = m.vertices.device
    points = _check_points(points, dev, "closest_point")
    N = int(points.shape[0])
    if N == 0:  # nothing is launched, so nothing is known about the faces either
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        return torch.empty(0, **f32), torch.empty(0, **i32), dict(n=0, far=0, queries_invalid=0, faces_skipped=None, cell=0.0,
                                                                  dims=[0, 0, 0], pairs=0)
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        distance, face, flags = _closest(points, m, grid, max_distance)
        flags = [int(x) for x in flags.cpu()]  # the one read-back
        if flags[2] != 0:
            raise MeshOverflow("closest_point: an index left its range (%d faces, %d queries)" % (int(m.faces.shape[0]), N))
    report = dict(n=N, far=flags[0], queries_invalid=flags[1])
    report.update(_grid_report(grid, int(m.faces.shape[0])))
    return distance, face, report


def distance(a, b, samples: int = 100000, seed: int = 0, taus=(), max_distance=None) -> Dict:
    """How far two meshes are apart: `samples` surface samples of each (sample_surface, `seed`) against the other
    (closest_point).  Per direction (a_to_b, b_to_a): n, far, mean, rms, median (the lower one), max; chamfer = the mean of
    the two means, hausdorff = the larger max; per tau: precision (the share of a's samples within tau of b), recall (b's
    within tau of a) and fscore = 2 P R / (P + R), 0 when both are 0.  A sample farther than `max_distance` counts with that
    distance.  Also faces_skipped, cell and dims of both grids, samples and seed.  Float64 reductions where the distances
    live, one read-back for them."""
    _check_max_distance(max_distance)
    ma, mb = _mesh_tensors(a, "distance"), _mesh_tensors(b, "distance")
    if ma.vertices.device != mb.vertices.device:
        raise RuntimeError("distance: the two meshes must live on one device")
    taus = [float(t) for t in taus]
    dev = ma.vertices.device
    rows, grids, ns = [], [], []
    with torch.cuda.device(dev):
        t = torch.tensor(taus, dtype=torch.float64, device=dev)
        for src, dst in ((ma, mb), (mb, ma)):
            pts = sample_surface(src, samples, seed)[0]
            grid = triangle_grid(dst)
            d, _, flags = _closest(pts, dst, grid, max_distance)
            grids.append(grid)
            ns.append(int(d.shape[0]))
            d64 = d.double()
            if ns[-1]:
                stats = torch.stack((d64.mean(), (d64 * d64).mean().sqrt(), d.median().double(), d64.max()))
                within = (d64[None, :] <= t[:, None]).double().mean(1)
            else:
                stats, within = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros_like(t)
            rows.append(torch.cat((stats, flags.double(), within)))
        got = torch.stack(rows).cpu().numpy()  # the one read-back of the reductions
    if got[:, 6].any():
        raise MeshOverflow("distance: an index left its range")
    out = {}
    for name, row, n in (("a_to_b", got[0], ns[0]), ("b_to_a", got[1], ns[1])):
        out[name] = dict(n=n, far=int(row[4]), mean=float(row[0]), rms=float(row[1]), median=float(row[2]), max=float(row[3]))
    out["chamfer"] = 0.5 * (out["a_to_b"]["mean"] + out["b_to_a"]["mean"])
    out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"])
    out["taus"] = []
    for k, tau in enumerate(taus):
        P, R = float(got[0, 7 + k]), float(got[1, 7 + k])
        out["taus"].append(dict(tau=tau, precision=P, recall=R, fscore=2.0 * P * R / (P + R) if P + R > 0 else 0.0))
    gb, ga = grids  # the first direction searched b's grid
    out["faces_skipped"] = dict(a=ga.faces_skipped if ga is not None else int(ma.faces.shape[0]),
                                b=gb.faces_skipped if gb is not None else int(mb.faces.shape[0]))
    out["grid"] = dict(a=dict(cell=ga.cell, dims=list(ga.dims)) if ga is not None else None,
                       b=dict(cell=gb.cell, dims=list(gb.dims)) if gb is not None else None)
    out["samples"], out["seed"] = int(samples), int(seed)
    return out


# ---- baking occlusion: what a ray hits, the occlusion of every vertex (include/gigs_hip.h, "Baking occlusion") ---------------
BAKE_MAX_RAYS, BAKE_MAX_ROTATIONS = 1024, 64


def _cell_order(p64: torch.Tensor, grid: TriangleGrid) -> torch.Tensor:
    """The rows of p64 [N,3] (float64) sorted by the grid cell they fall in (clamped; a NaN goes to 0)."""
    dev = p64.device
    lo = torch.from_numpy(grid.lo.astype(np.float64)).to(dev)
    G = torch.tensor(grid.dims, dtype=torch.float64, device=dev)
    c = torch.nan_to_num(((p64 - lo) / grid.cell).floor(), nan=0.0).clamp_(min=0).minimum(G - 1).long()
    return torch.sort((c[:, 2] * grid.dims[1] + c[:, 1]) * grid.dims[0] + c[:, 0]).indices


def _entry_order(origins: torch.Tensor, directions: torch.Tensor, grid: TriangleGrid) -> torch.Tensor:
    """The rays sorted by the cell of the point where they enter the grid's box (their origin if it lies inside, the
    clamped cell for a ray that misses the box): the lanes of a wave start on the same lists."""
    dev = origins.device
    o, d = origins.double(), directions.double()
    lo = torch.from_numpy(grid.lo.astype(np.float64)).to(dev)
    hi = lo + torch.tensor(grid.dims, dtype=torch.float64, device=dev) * grid.cell
    t0, t1 = (lo - o) / d, (hi - o) / d
    near = torch.nan_to_num(torch.minimum(t0, t1), nan=float("-inf"), neginf=float("-inf"), posinf=float("inf"))
    t = torch.nan_to_num(near.amax(1).clamp_(min=0.0), posinf=0.0)
    return _cell_order(o + t[:, None] * d, grid)


def _raycast(origins: torch.Tensor, directions: torch.Tensor, m: Mesh, grid, t_max, sort: bool = True):
    """-> (t [N] float32, face [N] int32, bary [N,2] float32, flags [3] int32 on the device: hits, invalid, overflow)."""
    dev = m.vertices.device
    N = int(origins.shape[0])
    t = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    face = torch.full((N,), -1, dtype=torch.int32, device=dev)
    bary = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    flags = torch.zeros(3, dtype=torch.int32, device=dev)
    if N == 0:
        return t, face, bary, flags
    if grid is None:  # no usable face: nothing is launched
        valid = torch.isfinite(origins).all(1) & torch.isfinite(directions).all(1) & (directions != 0).any(1)
        flags[1] = (~valid).sum()
        return t, face, bary, flags
    order = _entry_order(origins, directions, grid) if sort else None
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_raycast(
        int(m.vertices.shape[0]), int(m.faces.shape[0]), _p(m.vertices), _p(m.faces), c_lo, grid.cell, c_dims,
        _p(grid.cell_start), _p(grid.pairs), int(grid.pairs.shape[0]), _scale(grid), N, _p(origins), _p(directions),
        _p(order) if order is not None else None, float("inf") if t_max is None else float(t_max), _p(t), _p(face), _p(bary),
        flags.data_ptr(), flags[2:].data_ptr(), _stream()), "mesh_raycast")
    return t, face, bary, flags


def _scale(grid: TriangleGrid) -> float:
    """M of sigma: the largest |coordinate| of a corner of a usable face."""
    if grid.hi is None:
        raise ValueError("the grid carries no `hi`: build it with triangle_grid")
    return float(max(np.abs(grid.lo.astype(np.float64)).max(), np.abs(grid.hi.astype(np.float64)).max()))


def _grid_report(grid, F: int) -> Dict:
    return dict(faces_skipped=grid.faces_skipped if grid is not None else F, cell=grid.cell if grid is not None else 0.0,
                dims=list(grid.dims) if grid is not None else [0, 0, 0], pairs=int(grid.pairs.shape[0]) if grid is not None else 0)


def raycast(origins, directions, mesh, t_max=None, cell=None, grid=None):
    """(t [N] float32, face [N] int32, bary [N,2] float32, report): for every ray origins[i] + t directions[i] ([N,3] float32
    each, on the mesh's device; the direction need not be a unit vector and t is in its units) the nearest usable face of
    `mesh` it hits within 0 <= t <= t_max (None: no limit) and the barycentric weights of the face's second and third
    vertex at the hit.  Faces are two-sided; of faces hit at the same t the smallest index wins; a ray within about 1e-6
    rad of a face's plane misses that face by definition (include/gigs_hip.h, "Baking occlusion").  A miss gives +inf,
    -1, (0, 0), as does a ray with a non-finite component or a zero direction (rays_invalid) and every ray if the mesh has
    no usable face.  The result does not depend on the grid: `cell` (triangle_grid) or a `grid` built before only change
    the time.  Report: n, hits, rays_invalid, faces_skipped, cell, dims, pairs.  One read-back."""
    if t_max is not None and not (float(t_max) >= 0):
        raise ValueError("raycast: t_max must be >= 0 or None, got %r" % (t_max,))
    m = _mesh_tensors(mesh, "raycast")
    dev = m.vertices.device
    origins = _check_points(origins, dev, "raycast", "origins")
    directions = _check_points(directions, dev, "raycast", "directions")
    if origins.shape[0] != directions.shape[0]:
        raise ValueError("raycast: %d origins, %d directions" % (origins.shape[0], directions.shape[0]))
    N = int(origins.shape[0])
    if N == 0:  # nothing is launched, so nothing is known about the faces either
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        return torch.empty(0, **f32), torch.empty(0, **i32), torch.empty((0, 2), **f32), dict(
            n=0, hits=0, rays_invalid=0, faces_skipped=None, cell=0.0, dims=[0, 0, 0], pairs=0)
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        t, face, bary, flags = _raycast(origins, directions, m, grid, t_max)
        flags = [int(x) for x in flags.cpu()]  # the one read-back
        if flags[2] != 0:
            raise MeshOverflow("raycast: an index left its range (%d faces, %d rays)" % (int(m.faces.shape[0]), N))
    report = dict(n=N, hits=flags[0], rays_invalid=flags[1])
    report.update(_grid_report(grid, int(m.faces.shape[0])))
    return t, face, bary, report


def occlusion_directions(rays: int = 256, rotations: int = 16) -> np.ndarray:
    """[rotations, rays, 3] float32: a cosine-weighted spiral lattice on the hemisphere z >= 0 -- point i of R has
    u = (i + 1/2) / R, radius sqrt(u), azimuth i times the golden angle and z = sqrt(1 - u) -- turned about z by
    2 pi k / K for the k-th of K rotations.  numpy float64 on the host: the device does no trigonometry."""
    R, K = int(rays), int(rotations)
    i = np.arange(R, dtype=np.float64)
    u = (i + 0.5) / R
    r, z = np.sqrt(u), np.sqrt(1.0 - u)
    golden = np.pi * (3.0 - np.sqrt(5.0))
    phi = i[None, :] * golden + (2.0 * np.pi * np.arange(K, dtype=np.float64) / K)[:, None]
    return np.stack([r[None] * np.cos(phi), r[None] * np.sin(phi), np.broadcast_to(z, phi.shape)], -1).astype(np.float32)


def _hemisphere_args(what: str, rays, rotations, directions, max_distance, bias):
    """The checks bake_occlusion and trace_hemispheres share.  -> (R, K, the table [K,R,3] float32 numpy)."""
    if directions is None:
        R, K = int(rays), int(rotations)
    else:
        directions = np.ascontiguousarray(directions, dtype=np.float32)
        if directions.ndim != 3 or directions.shape[2] != 3:
            raise ValueError("%s: directions must be [K,R,3], got %s" % (what, directions.shape,))
        K, R = int(directions.shape[0]), int(directions.shape[1])
    if R < 64 or R > BAKE_MAX_RAYS or R % 64 != 0:
        raise ValueError("%s: rays must be a multiple of 64 in [64, %d], got %d" % (what, BAKE_MAX_RAYS, R))
    if K < 1 or K > BAKE_MAX_ROTATIONS:
        raise ValueError("%s: rotations must lie in [1, %d], got %d" % (what, BAKE_MAX_ROTATIONS, K))
    if directions is None:
        directions = occlusion_directions(R, K)
    elif not (np.isfinite(directions).all() and (directions[..., 2] >= 0).all()):
        raise ValueError("%s: directions must be finite with z >= 0" % what)
    for name, x in (("max_distance", max_distance), ("bias", bias)):
        if x is not None and not (float(x) >= 0 and np.isfinite(float(x))):
            raise ValueError("%s: %s must be finite and >= 0 or None, got %r" % (what, name, x))
    return R, K, directions


def _no_normal(m: Mesh) -> torch.Tensor:
    """[V] bool: the vertices the hemisphere kernels give no rays (a position that is not finite, a normal not of unit length)."""
    n2 = (m.normals.double() ** 2).sum(1)
    return ~(torch.isfinite(m.vertices).all(1) & (n2 >= 1.0 - 2.0 ** -10) & (n2 <= 1.0 + 2.0 ** -10))


def _bake_occlusion(mesh, rays=256, max_distance=None, bias=None, seed=0, rotations=16, directions=None, cell=None, grid=None,
                    sort: bool = True):
    """bake_occlusion with the per-vertex hit counts: -> (occlusion [V] float32, hits [V] int32, report)."""
    m = _mesh_tensors(mesh, "bake_occlusion")
    dev = m.vertices.device
    R, K, directions = _hemisphere_args("bake_occlusion", rays, rotations, directions, max_distance, bias)
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    occlusion = torch.ones(V, dtype=torch.float32, device=dev)
    hits = torch.zeros(V, dtype=torch.int32, device=dev)
    report = dict(n=V, hits_total=0, no_normal=0, rays=R, rotations=K, seed=seed,
                  max_distance=0.0 if max_distance is None else float(max_distance), bias=0.0 if bias is None else float(bias))
    if V == 0:
        report.update(_grid_report(None, F))
        return occlusion, hits, report
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        report.update(_grid_report(grid, F))
        if grid is None:  # no usable face: every vertex is open and nothing is launched
            report["no_normal"] = int(_no_normal(m).sum().item())
            return occlusion, hits, report
        if max_distance is None:
            max_distance = 0.1 * (max(grid.dims) * grid.cell)
        if bias is None:
            bias = 1e-3 * float(max_distance)
        report["max_distance"], report["bias"] = float(max_distance), float(bias)
        order = _cell_order(m.vertices.double(), grid) if sort else None
        table = torch.from_numpy(directions).to(dev)
        counts = torch.zeros(3, dtype=torch.int64, device=dev)  # hits in all, no normal; overflow (an int32 in its low half)
        c_lo, c_dims = _c_grid(grid.lo, grid.dims)
        gigs_lib.check(gigs_lib.lib().gigs_mesh_bake_occlusion(
            V, F, _p(m.vertices), _p(m.normals), _p(m.faces), c_lo, grid.cell, c_dims, _p(grid.cell_start), _p(grid.pairs),
            int(grid.pairs.shape[0]), _scale(grid), _p(order) if order is not None else None, _p(table), R, K, seed, float(max_distance),
            float(bias), _p(occlusion), _p(hits), counts.data_ptr(), counts[2:].data_ptr(), _stream()), "mesh_bake_occlusion")
        got = [int(x) for x in counts.cpu()]  # the one read-back
        if got[2] != 0:
            raise MeshOverflow("bake_occlusion: an index left its range (%d vertices, %d faces)" % (V, F))
        report["hits_total"], report["no_normal"] = got[0], got[1]
    return occlusion, hits, report


def bake_occlusion(mesh, rays=256, max_distance=None, bias=None, seed=0, rotations=16, directions=None, cell=None, grid=None):
    """(occlusion [V] float32, report): for every vertex the cosine-weighted share of the hemisphere about its stored normal
    that is open within `max_distance` -- 1 means open, the convention of the SSAO `occlusion` plane and of the shade's
    `occlusion` input.  A wave per vertex casts `rays` rays (a multiple of 64 in [64, 1024]) from vertex + bias normal and
    counts the ones that hit a usable face (mesh.raycast's rule) within max_distance: occlusion = (rays - hits) / rays,
    a plain count because the directions are cosine-distributed.  They come from a table [rotations, rays, 3] in the local
    frame (default: occlusion_directions; `directions` overrides it, and then sets rays and rotations); vertex v uses the
    rotation mix64(seed 2^32 + v) mod rotations, so the result is a pure function of the arguments.  The stored normal is
    used as it is; a vertex whose normal is not of unit length within 2^-10 (the zero normals the extraction can leave) or
    whose position is not finite gets 1 and counts as no_normal.  max_distance defaults to 0.1 of the longest axis of the
    grid's box and bias to 1e-3 max_distance: conventions, not measurements.  Report: n, hits_total, no_normal, rays,
    rotations, seed, max_distance, bias, faces_skipped, cell, dims, pairs.  One read-back."""
    occlusion, _, report = _bake_occlusion(mesh, rays, max_distance, bias, seed, rotations, directions, cell, grid)
    return occlusion, report


# ---- baking light: the hemispheres traced once, then gathers over the records (include/gigs_hip.h, "Baking light") ---------
TRACE_MEMORY_LIMIT = 8 << 30  # bytes of records (12 V R) trace_hemispheres allocates without being told otherwise
SKY_MAX_RES = 4096


class HemisphereHits(NamedTuple):
    face: torch.Tensor       # [V,R] int32: -1 a miss, f a front hit of face f, -2 - f a back hit
    bary: torch.Tensor       # [V,R,2] float32: the weights of the face's second and third vertex at the hit
    directions: np.ndarray   # [K,R,3] float32: the table the rays came from
    seed: int
    rays: int
    rotations: int


def trace_hemispheres(mesh, rays=256, max_distance=None, bias=None, seed=0, rotations=16, directions=None, cell=None, grid=None,
                      memory_limit=TRACE_MEMORY_LIMIT):
    """(HemisphereHits, report): bake_occlusion's rays -- the same table, rotation, frame, origin and no_normal rule -- with
    what every ray hit RECORDED in place of a count, for gather_light to light the mesh any number of times without
    tracing again.  face [V,R] int32: -1 a miss, f a hit on the FRONT of face f (direction . geometric normal < 0; the
    extraction orients faces outward), -2 - f a hit on its back, which carries no light; bary [V,R,2] float32 as
    mesh.raycast's.  max_distance=None traces without a limit, because light rays see the whole scene; a finite value works
    as in bake_occlusion, and a hit beyond it is a miss that sees the sky.  bias defaults to 1e-4 of the longest axis of the
    grid's box, the value bake_occlusion ends up with (a convention).  The records take 12 V R bytes; above `memory_limit`
    (8 GiB) the call raises ValueError instead of tracing in chunks.  A no_normal vertex has -1 in all its records.  Report:
    n, misses, front_hits, back_hits, no_normal, rays, rotations, seed, max_distance (None: unlimited), bias, record_bytes,
    faces_skipped, cell, dims, pairs.  V == 0 or a mesh with no usable face launches nothing.  One read-back."""
    R, K, directions = _hemisphere_args("trace_hemispheres", rays, rotations, directions, max_distance, bias)
    first = (mesh if isinstance(mesh, Mesh) else Mesh(*mesh)).vertices  # a malformed mesh is _mesh_tensors' to report, below
    V = int(first.shape[0]) if isinstance(first, torch.Tensor) and first.dim() == 2 else 0
    if 12 * V * R > int(memory_limit):  # before the device check: the limit is about the arguments alone
        raise ValueError("trace_hemispheres: the records of %d vertices x %d rays take %d bytes, more than memory_limit = %d; "
                         "trace fewer rays or a simplified mesh (a trace in chunks would re-trace for every bounce)"
                         % (V, R, 12 * V * R, int(memory_limit)))
    m = _mesh_tensors(mesh, "trace_hemispheres")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    face = torch.full((V, R), -1, dtype=torch.int32, device=dev)
    bary = torch.zeros((V, R, 2), dtype=torch.float32, device=dev)
    hits = HemisphereHits(face, bary, directions, seed, R, K)
    report = dict(n=V, misses=0, front_hits=0, back_hits=0, no_normal=0, rays=R, rotations=K, seed=seed,
                  max_distance=None if max_distance is None else float(max_distance), bias=0.0 if bias is None else float(bias),
                  record_bytes=12 * V * R)
    if V == 0:
        report.update(_grid_report(None, F))
        return hits, report
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        report.update(_grid_report(grid, F))
        if grid is None:  # no usable face: every ray of a vertex with a normal sees the sky and nothing is launched
            report["no_normal"] = int(_no_normal(m).sum().item())
            report["misses"] = R * (V - report["no_normal"])
            return hits, report
        if bias is None:  # bake_occlusion's: 1e-3 of its default max_distance, 0.1 of the grid's longest axis
            bias = 1e-3 * (0.1 * (max(grid.dims) * grid.cell))
        report["bias"] = float(bias)
        order = _cell_order(m.vertices.double(), grid)
        table = torch.from_numpy(directions).to(dev)
        counts = torch.zeros(5, dtype=torch.int64, device=dev)  # misses, front, back, no normal; overflow (an int32 in its low half)
        c_lo, c_dims = _c_grid(grid.lo, grid.dims)
        gigs_lib.check(gigs_lib.lib().gigs_mesh_trace_hemisphere(
            V, F, _p(m.vertices), _p(m.normals), _p(m.faces), c_lo, grid.cell, c_dims, _p(grid.cell_start), _p(grid.pairs),
            int(grid.pairs.shape[0]), _scale(grid), _p(order), _p(table), R, K, seed,
            float("inf") if max_distance is None else float(max_distance), float(bias), _p(face), _p(bary), counts.data_ptr(),
            counts[4:].data_ptr(), _stream()), "mesh_trace_hemisphere")
        got = [int(x) for x in counts.cpu()]  # the one read-back
        if got[4] != 0:
            raise MeshOverflow("trace_hemispheres: an index left its range (%d vertices, %d faces)" % (V, F))
        report["misses"], report["front_hits"], report["back_hits"], report["no_normal"] = got[:4]
    return hits, report


def _check_cube(cube, what: str) -> torch.Tensor:
    if not isinstance(cube, torch.Tensor):
        raise ValueError("%s: the cube must be a [6,n,n,3] float32 tensor, got %s" % (what, type(cube).__name__))
    if (cube.dtype != torch.float32 or cube.dim() != 4 or cube.shape[0] != 6 or cube.shape[1] != cube.shape[2] or cube.shape[3] != 3
            or not 1 <= cube.shape[1] <= SKY_MAX_RES):
        raise ValueError("%s: the cube must be [6,n,n,3] float32 with 1 <= n <= %d, got %s %s" % (what, SKY_MAX_RES,
                                                                                                   tuple(cube.shape), cube.dtype))
    cube = cube.detach()
    if not bool((torch.isfinite(cube) & (cube >= 0)).all()):
        raise ValueError("%s: the cube must be finite and >= 0" % what)
    return cube.contiguous()


def _gather_light(mesh, hits: HemisphereHits, cube, bounces: int = 1, reflectance=None):
    """gather_light with every pass: -> (irradiance [bounces + 1, V, 3], radiosity likewise, report)."""
    bounces = int(bounces)
    if bounces < 0:
        raise ValueError("gather_light: bounces must be >= 0, got %d" % bounces)
    cube = _check_cube(cube, "gather_light")
    m = _mesh_tensors(mesh, "gather_light")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    if cube.device != dev:
        raise RuntimeError("gather_light: the cube must be a tensor on the mesh's device: gigs-hip has no CPU path")
    R, K = int(hits.rays), int(hits.rotations)
    table = np.ascontiguousarray(hits.directions, dtype=np.float32)
    if (not isinstance(hits.face, torch.Tensor) or hits.face.device != dev or hits.face.dtype != torch.int32
            or tuple(hits.face.shape) != (V, R) or not isinstance(hits.bary, torch.Tensor) or hits.bary.device != dev
            or hits.bary.dtype != torch.float32 or tuple(hits.bary.shape) != (V, R, 2) or table.shape != (K, R, 3)):
        raise ValueError("gather_light: the records are not those of this mesh (%d vertices, %d rays, %d rotations)" % (V, R, K))
    _hemisphere_args("gather_light", R, K, table, None, None)
    if reflectance is None:
        reflectance = m.albedo * (1.0 - m.metallic)[:, None]
    elif (not isinstance(reflectance, torch.Tensor) or reflectance.device != dev or reflectance.dtype != torch.float32
          or tuple(reflectance.shape) != (V, 3)):
        raise ValueError("gather_light: reflectance must be a [%d,3] float32 tensor on the mesh's device" % V)
    reflectance = reflectance.detach().contiguous()
    n = int(cube.shape[1])
    passes = torch.zeros((bounces + 1, V, 3), dtype=torch.float32, device=dev)
    radiosity = torch.zeros_like(passes)
    report = dict(n=V, rays=R, bounces=bounces, passes=bounces + 1, sky_res=n, mean_irradiance=[0.0] * (bounces + 1))
    if V == 0:
        return passes, radiosity, report
    with torch.cuda.device(dev):
        face, bary, d_table = hits.face.contiguous(), hits.bary.contiguous(), torch.from_numpy(table).to(dev)
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        for b in range(bounces + 1):
            gigs_lib.check(gigs_lib.lib().gigs_mesh_gather_light(
                V, F, _p(m.vertices), _p(m.normals), _p(m.faces), _p(d_table), R, K, int(hits.seed) & 0xFFFFFFFFFFFFFFFF, _p(face),
                _p(bary), n, _p(cube), _p(reflectance), radiosity[b - 1].data_ptr() if b else None, passes[b].data_ptr(),
                radiosity[b].data_ptr(), overflow.data_ptr(), _stream()), "mesh_gather_light")
        got = torch.cat((overflow.double(), passes.double().mean(dim=(1, 2)))).cpu().tolist()  # the one read-back
        if got[0] != 0:
            raise MeshOverflow("gather_light: a record or a face index left its range (%d vertices, %d faces)" % (V, F))
        report["mean_irradiance"] = got[1:]
    return passes, radiosity, report


def gather_light(mesh, hits: HemisphereHits, cube, bounces: int = 1, reflectance=None, return_passes: bool = False):
    """(irradiance [V,3] float32, report): the light every vertex receives from the environment `cube` ([6,n,n,3] float32,
    finite and >= 0, the cube of the lights with the world's axes, looked up at the NEAREST texel: sky_cube makes one) over
    the records of trace_hemispheres, after `bounces` diffuse inter-reflections.  The irradiance is the cosine-weighted MEAN
    of the incoming radiance, the normalisation of the shade's diffuse cube.  Pass 0 is the shadowed sky: a ray that
    escaped brings its sky texel, a ray that hit brings nothing.  Pass b adds, at every front hit, the radiosity
    reflectance x I(b-1) of the face's vertices interpolated at the hit: a Jacobi iteration over the same rays, one launch
    per pass, bounces + 1 in all (gigs_mesh_gather_light).  `reflectance` [V,3] float32 defaults to
    albedo * (1 - metallic)[:, None].  return_passes=True returns [bounces + 1, V, 3], every pass.  A no_normal vertex gets
    0.  The result is a pure function of the arguments: no float atomics, a fixed summation order.  Report: n, rays,
    bounces, passes, sky_res, mean_irradiance (per pass, over vertices and channels).  V == 0 launches nothing.  One
    read-back (after the cube's check)."""
    passes, _, report = _gather_light(mesh, hits, cube, bounces, reflectance)
    return (passes if return_passes else passes[-1]), report


def bake_light(mesh, cube, rays=256, bounces=1, reflectance=None, max_distance=None, bias=None, seed=0, rotations=16,
               directions=None, cell=None, grid=None, memory_limit=TRACE_MEMORY_LIMIT, return_passes: bool = False):
    """(irradiance [V,3] float32, report): trace_hemispheres, then gather_light over its records; the report is the two
    reports in one.  To light one mesh under several cubes, trace once and gather per cube: the bits are the same."""
    hits, report = trace_hemispheres(mesh, rays, max_distance, bias, seed, rotations, directions, cell, grid, memory_limit)
    irradiance, gathered = gather_light(mesh, hits, cube, bounces, reflectance, return_passes)
    report.update(gathered)
    return irradiance, report


# ---- ray-traced light per point: a final gather (include/gigs_hip.h, "Ray-traced light per point") -------------------------
class PointLight(NamedTuple):
    occlusion: torch.Tensor   # [N] float32: the open share of the hemisphere within ao_distance, 1 = open
    hits: torch.Tensor        # [N] int32: the rays with a face within ao_distance
    irradiance: torch.Tensor  # [N,3] float32 or None (no cube): the shadowed sky plus the bounced light
    indirect: torch.Tensor    # [N,3] float32 or None: the bounced light alone


def _check_radiosity(radiosity, m: Mesh, what: str) -> torch.Tensor:
    V = int(m.vertices.shape[0])
    if (not isinstance(radiosity, torch.Tensor) or radiosity.device != m.vertices.device or radiosity.dtype != torch.float32
            or tuple(radiosity.shape) != (V, 3)):
        raise ValueError("%s: radiosity must be a [%d,3] float32 tensor on the mesh's device" % (what, V))
    radiosity = radiosity.detach().contiguous()
    if not bool(torch.isfinite(radiosity).all()):
        raise ValueError("%s: radiosity must be finite" % what)
    return radiosity


def _gather_points(points, normals, m: Mesh, grid, cube, radiosity, R, K, directions, ao_distance, max_distance, bias, seed,
                   mask, report):
    """The launch of gather_points on checked arguments (grid is not None, N > 0) -> PointLight; fills the counters of report."""
    dev = m.vertices.device
    N, V, F = int(points.shape[0]), int(m.vertices.shape[0]), int(m.faces.shape[0])
    hits = torch.zeros(N, dtype=torch.int32, device=dev)
    occlusion = torch.ones(N, dtype=torch.float32, device=dev)
    irradiance = torch.zeros((N, 3), dtype=torch.float32, device=dev) if cube is not None else None
    indirect = torch.zeros((N, 3), dtype=torch.float32, device=dev) if cube is not None else None
    order = _cell_order(points.double(), grid)
    table = torch.from_numpy(directions).to(dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)  # misses, front, back, no normal, masked; overflow (an int32 in its low half)
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_gather_points(
        V, F, _p(m.vertices), _p(m.faces), c_lo, grid.cell, c_dims, _p(grid.cell_start), _p(grid.pairs), int(grid.pairs.shape[0]),
        _scale(grid), N, _p(points), _p(normals), _p(mask) if mask is not None else None, _p(order), _p(table), R, K, seed,
        float(ao_distance), float("inf") if max_distance is None else float(max_distance), float(bias),
        int(cube.shape[1]) if cube is not None else 0, _p(cube) if cube is not None else None,
        _p(radiosity) if radiosity is not None else None, _p(hits), _p(occlusion),
        _p(irradiance) if cube is not None else None, _p(indirect) if cube is not None else None, counts.data_ptr(),
        counts[5:].data_ptr(), _stream()), "mesh_gather_points")
    got = [int(x) for x in counts.cpu()]  # the one read-back
    if got[5] != 0:
        raise MeshOverflow("gather_points: an index left its range (%d points, %d vertices, %d faces)" % (N, V, F))
    report["misses"], report["front_hits"], report["back_hits"], report["no_normal"], report["masked"] = got[:5]
    return PointLight(occlusion, hits, irradiance, indirect)


def gather_points(points, normals, mesh, cube=None, radiosity=None, rays=256, ao_distance=None, max_distance=None, bias=None,
                  seed=0, rotations=16, directions=None, mask=None, cell=None, grid=None):
    """(PointLight(occlusion, hits, irradiance, indirect), report): bake_occlusion and one pass of gather_light for ANY surface
    points -- `points` and `normals` [N,3] float32 on the mesh's device, in practice the covered pixels of a G-buffer -- in one
    launch (gigs_mesh_gather_points): a wave per point casts bake_occlusion's rays (the same table, frame, origin
    point + bias normal, and rotation mix64(seed 2^32 + q) mod rotations of point q) against `mesh`.  hits [N] int32 counts
    the rays whose nearest face lies within `ao_distance`, occlusion [N] = (rays - hits) / rays, 1 = open.  With a `cube`
    ([6,n,n,3] float32, as gather_light's) the rays run to `max_distance` (None: no limit, as trace_hemispheres) and
    irradiance [N,3] is the cosine-weighted mean of what they bring: the sky texel where a ray escapes, `radiosity` [V,3]
    float32 (finite; the mesh's baked reflectance x irradiance; None: nothing) interpolated where it meets the front of a
    face, nothing at a back; indirect [N,3] is the share of the front hits.  Without a cube both are None and the rays stop
    at ao_distance, which changes no count.  A point with mask [N] (uint8 or bool) == 0 is `masked`, a point whose position
    is not finite or whose normal is not of unit length within 2^-10 is `no_normal`: occlusion 1, hits 0, no light.
    ao_distance and bias default as bake_occlusion's max_distance and bias.  The result is a pure function of the arguments
    and does not depend on the grid (`cell`, `grid`).  N == 0 or a mesh with no usable face launches nothing and leaves every
    point open, and then no light is gathered either: irradiance and indirect are 0.  Report: n, misses, front_hits,
    back_hits, no_normal, masked, rays, rotations, seed, ao_distance, max_distance (None: unlimited), bias, sky_res (None: no
    cube), radiosity (bool), faces_skipped, cell, dims, pairs.  One read-back (after the checks of cube and radiosity)."""
    what = "gather_points"
    R, K, directions = _hemisphere_args(what, rays, rotations, directions, max_distance, bias)
    if ao_distance is not None and not (float(ao_distance) >= 0 and np.isfinite(float(ao_distance))):
        raise ValueError("%s: ao_distance must be finite and >= 0 or None, got %r" % (what, ao_distance))
    m = _mesh_tensors(mesh, what)
    dev = m.vertices.device
    points = _check_points(points, dev, what)
    normals = _check_points(normals, dev, what, "normals")
    N, F = int(points.shape[0]), int(m.faces.shape[0])
    if int(normals.shape[0]) != N:
        raise ValueError("%s: %d points, %d normals" % (what, N, int(normals.shape[0])))
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool)
                or tuple(mask.shape) != (N,)):
            raise ValueError("%s: mask must be a [%d] uint8 or bool tensor on the mesh's device" % (what, N))
        mask = mask.detach().to(torch.uint8).contiguous()
    if cube is not None:
        cube = _check_cube(cube, what)
        if cube.device != dev:
            raise RuntimeError("%s: the cube must be a tensor on the mesh's device: gigs-hip has no CPU path" % what)
    if radiosity is not None:
        radiosity = _check_radiosity(radiosity, m, what)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    report = dict(n=N, misses=0, front_hits=0, back_hits=0, no_normal=0, masked=0, rays=R, rotations=K, seed=seed,
                  ao_distance=0.0 if ao_distance is None else float(ao_distance),
                  max_distance=None if max_distance is None else float(max_distance), bias=0.0 if bias is None else float(bias),
                  sky_res=int(cube.shape[1]) if cube is not None else None, radiosity=radiosity is not None)
    f32 = dict(dtype=torch.float32, device=dev)
    light = (torch.zeros((N, 3), **f32), torch.zeros((N, 3), **f32)) if cube is not None else (None, None)
    empty = PointLight(torch.ones(N, **f32), torch.zeros(N, dtype=torch.int32, device=dev), *light)
    if N == 0:
        report.update(_grid_report(None, F))
        return empty, report
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        report.update(_grid_report(grid, F))
        if grid is None:  # no usable face: every point is open and nothing is launched
            live = mask != 0 if mask is not None else torch.ones(N, dtype=torch.bool, device=dev)
            n2 = (normals.double() ** 2).sum(1)
            bad = live & ~(torch.isfinite(points).all(1) & (n2 >= 1.0 - 2.0 ** -10) & (n2 <= 1.0 + 2.0 ** -10))
            got = torch.stack(((~live).sum(), bad.sum())).cpu().tolist()
            report["masked"], report["no_normal"] = int(got[0]), int(got[1])
            report["misses"] = R * (N - report["masked"] - report["no_normal"])
            return empty, report
        if ao_distance is None:
            ao_distance = 0.1 * (max(grid.dims) * grid.cell)
        if bias is None:
            bias = 1e-3 * float(ao_distance)
        report["ao_distance"], report["bias"] = float(ao_distance), float(bias)
        return _gather_points(points, normals, m, grid, cube, radiosity, R, K, directions, ao_distance, max_distance, bias, seed,
                              mask, report), report


def final_gather(points, normals, mesh, cube, bounces=1, reflectance=None, light_rays=None, rays=256, ao_distance=None,
                 max_distance=None, bias=None, seed=0, rotations=16, directions=None, mask=None, cell=None, grid=None,
                 memory_limit=TRACE_MEMORY_LIMIT):
    """(PointLight, report): the irradiance of every point after `bounces` diffuse inter-reflections, a lightmap final gather:
    bake_light's passes 0 .. bounces - 1 on the VERTICES (trace_hemispheres with `light_rays` rays, default `rays`, then
    gather_light), then gather_points with the radiosity of pass bounces - 1 (bounces = 0: none, the shadowed sky alone).
    Both traces share table parameters, seed, bias, max_distance and the grid, so with points = the vertices, normals = the
    mesh's and light_rays = rays the irradiance is bake_light(bounces)'s bit for bit.  `directions` overrides the table of
    both.  The report is gather_points' with `bounces` and, under "bake", the vertex passes' report (None for bounces = 0)."""
    bounces = int(bounces)
    if bounces < 0:
        raise ValueError("final_gather: bounces must be >= 0, got %d" % bounces)
    if cube is None:
        raise ValueError("final_gather: a cube is needed; gather_points(cube=None) gives the occlusion alone")
    m = _mesh_tensors(mesh, "final_gather")
    radiosity, baked = None, None
    with torch.cuda.device(m.vertices.device):
        if grid is None:
            grid = triangle_grid(m, cell)
        if bounces > 0 and grid is not None:
            if bias is None:  # one bias for both traces: gather_points' default
                ao = ao_distance if ao_distance is not None else 0.1 * (max(grid.dims) * grid.cell)
                bias = 1e-3 * float(ao)
            hits, baked = trace_hemispheres(m, rays if light_rays is None else light_rays, max_distance, bias, seed, rotations,
                                            directions, cell, grid, memory_limit)
            _, radiosities, gathered = _gather_light(m, hits, cube, bounces - 1, reflectance)
            baked.update(gathered)
            radiosity = radiosities[bounces - 1]
        light, report = gather_points(points, normals, m, cube, radiosity, rays, ao_distance, max_distance, bias, seed, rotations,
                                      directions, mask, cell, grid)
    report["bounces"], report["bake"] = bounces, baked
    return light, report


# ---- ray-traced reflections per point (include/gigs_hip.h, "Ray-traced reflections per point") -----------------------------
REFLECT_MAX_LEVELS = 64
REFLECT_COUNTERS = ("misses", "front_hits", "back_hits", "below_horizon", "no_normal", "no_view", "masked")


class Reflection(NamedTuple):
    specular: torch.Tensor    # [N,3] float32 or None (no cube): the radiance the GGX lobe brings, sky and mesh
    reflected: torch.Tensor   # [N,3] float32 or None: the share of the front hits (the mesh's radiosity) alone
    visibility: torch.Tensor  # [N] float32: the n.l-weighted share of the lobe that escapes, 1 = open
    valid: torch.Tensor       # [N] int32: the rays above the horizon
    blocked: torch.Tensor     # [N] int32: those of them that hit a face


def ggx_directions(rays: int = 64, rotations: int = 16, levels: int = 16) -> np.ndarray:
    """[levels, rotations, rays, 3] float32: GGX-distributed HALF vectors in the tangent frame (z is the normal), the table of
    reflect_points.  Level l of L stands for roughness r_l = (l + 1/2) / L, alpha = r_l^2; point i of R has u = (i + 1/2) / R,
    cos^2(theta) = (1 - u) / (1 + (alpha^2 - 1) u) -- the inverse of the GGX distribution's CDF (Karis 2013) -- and the
    azimuth of occlusion_directions' spiral, i times the golden angle + 2 pi k / K for rotation k.  numpy float64 on the
    host, rounded to float32: the device does no trigonometry and no sqrt."""
    R, K, L = int(rays), int(rotations), int(levels)
    if R < 64 or R > BAKE_MAX_RAYS or R % 64 != 0:
        raise ValueError("ggx_directions: rays must be a multiple of 64 in [64, %d], got %d" % (BAKE_MAX_RAYS, R))
    if K < 1 or K > BAKE_MAX_ROTATIONS:
        raise ValueError("ggx_directions: rotations must lie in [1, %d], got %d" % (BAKE_MAX_ROTATIONS, K))
    if L < 1 or L > REFLECT_MAX_LEVELS:
        raise ValueError("ggx_directions: levels must lie in [1, %d], got %d" % (REFLECT_MAX_LEVELS, L))
    i = np.arange(R, dtype=np.float64)
    u = (i + 0.5) / R
    alpha = ((np.arange(L, dtype=np.float64) + 0.5) / L) ** 2
    cos2 = (1.0 - u)[None, :] / (1.0 + (alpha[:, None] ** 2 - 1.0) * u[None, :])  # [L,R]
    z, r = np.sqrt(cos2), np.sqrt(1.0 - cos2)
    golden = np.pi * (3.0 - np.sqrt(5.0))
    phi = i[None, :] * golden + (2.0 * np.pi * np.arange(K, dtype=np.float64) / K)[:, None]  # [K,R]
    return np.stack([r[:, None, :] * np.cos(phi)[None], r[:, None, :] * np.sin(phi)[None],
                     np.broadcast_to(z[:, None, :], (L, K, R))], -1).astype(np.float32)


def _reflect_args(what: str, rays, rotations, levels, directions, max_distance, bias):
    """The checks of reflect_points' table.  -> (R, K, L, the table [L,K,R,3] float32 numpy)."""
    if directions is None:
        directions = ggx_directions(rays, rotations, levels)
    else:
        directions = np.ascontiguousarray(directions, dtype=np.float32)
        if directions.ndim != 4 or directions.shape[3] != 3:
            raise ValueError("%s: directions must be [L,K,R,3], got %s" % (what, directions.shape,))
        if not (np.isfinite(directions).all() and (directions[..., 2] >= 0).all()):
            raise ValueError("%s: directions must be finite with z >= 0" % what)
    L, K, R = (int(x) for x in directions.shape[:3])
    if R < 64 or R > BAKE_MAX_RAYS or R % 64 != 0:
        raise ValueError("%s: rays must be a multiple of 64 in [64, %d], got %d" % (what, BAKE_MAX_RAYS, R))
    if K < 1 or K > BAKE_MAX_ROTATIONS:
        raise ValueError("%s: rotations must lie in [1, %d], got %d" % (what, BAKE_MAX_ROTATIONS, K))
    if L < 1 or L > REFLECT_MAX_LEVELS:
        raise ValueError("%s: levels must lie in [1, %d], got %d" % (what, REFLECT_MAX_LEVELS, L))
    for name, x in (("max_distance", max_distance), ("bias", bias)):
        if x is not None and not (float(x) >= 0 and np.isfinite(float(x))):
            raise ValueError("%s: %s must be finite and >= 0 or None, got %r" % (what, name, x))
    return R, K, L, directions


def _reflect_points(points, normals, views, roughness, m: Mesh, grid, cube, radiosity, table, max_distance, bias, seed, mask,
                    report):
    """The launch of reflect_points on checked arguments (grid is not None, N > 0) -> Reflection; fills the counters of report.
    table: [L,K,R,3] float32 on the device."""
    dev = m.vertices.device
    N, V, F = int(points.shape[0]), int(m.vertices.shape[0]), int(m.faces.shape[0])
    L, K, R = (int(x) for x in table.shape[:3])
    visibility = torch.ones(N, dtype=torch.float32, device=dev)
    valid = torch.zeros(N, dtype=torch.int32, device=dev)
    blocked = torch.zeros(N, dtype=torch.int32, device=dev)
    specular = torch.zeros((N, 3), dtype=torch.float32, device=dev) if cube is not None else None
    reflected = torch.zeros((N, 3), dtype=torch.float32, device=dev) if cube is not None else None
    order = _cell_order(points.double(), grid)
    counts = torch.zeros(8, dtype=torch.int64, device=dev)  # the seven counters; overflow (an int32 in its low half)
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_reflect_points(
        V, F, _p(m.vertices), _p(m.faces), c_lo, grid.cell, c_dims, _p(grid.cell_start), _p(grid.pairs), int(grid.pairs.shape[0]),
        _scale(grid), N, _p(points), _p(normals), _p(views), _p(roughness), _p(mask) if mask is not None else None, _p(order),
        _p(table), L, R, K, seed, float("inf") if max_distance is None else float(max_distance), float(bias),
        int(cube.shape[1]) if cube is not None else 0, _p(cube) if cube is not None else None,
        _p(radiosity) if radiosity is not None else None, _p(specular) if cube is not None else None,
        _p(reflected) if cube is not None else None, _p(visibility), _p(valid), _p(blocked), counts.data_ptr(),
        counts[7:].data_ptr(), _stream()), "mesh_reflect_points")
    got = [int(x) for x in counts.cpu()]  # the one read-back
    if got[7] != 0:
        raise MeshOverflow("reflect_points: an index left its range (%d points, %d vertices, %d faces)" % (N, V, F))
    report.update(zip(REFLECT_COUNTERS, got[:7]))
    return Reflection(specular, reflected, visibility, valid, blocked)


def reflect_points(points, normals, views, roughness, mesh, cube=None, radiosity=None, rays=64, levels=16, rotations=16,
                   max_distance=None, bias=None, seed=0, directions=None, mask=None, cell=None, grid=None):
    """(Reflection(specular, reflected, visibility, valid, blocked), report): the traced counterpart of the shade's lookup in
    the pre-filtered environment cube, for ANY surface points -- `points`, `normals`, `views` [N,3] and `roughness` [N]
    float32 on the mesh's device, in practice the covered pixels of a G-buffer; `views` are unit vectors from the surface
    towards the eye (mesh_render.prepare_views) -- in one launch (gigs_mesh_reflect_points).  A wave per point casts `rays`
    rays (a multiple of 64 in [64, 1024]) from point + bias normal: row i of the point's level and rotation of the table
    ggx_directions(rays, rotations, levels) is a GGX half vector h in the point's frame (gather_points' frame and rotation;
    the level is min(levels - 1, floor(roughness levels))), and the ray is the view mirrored about it,
    l = 2 (v.h) h - v.  A ray with v.h <= 0 or n.l <= 0 is below the horizon and is not cast.  With a `cube` ([6,n,n,3]
    float32, as gather_light's) specular [N,3] is the n.l-weighted mean of what the rays bring -- the sky texel where a ray
    escapes, `radiosity` [V,3] float32 (finite; None: nothing) interpolated where it meets the front of a face, nothing at a
    back -- which is the first sum of the split-sum approximation taken about the true view direction; reflected [N,3] is
    the share of the front hits; a hit returns DIFFUSE radiosity only, there is no specular inter-reflection.  visibility [N]
    is the n.l-weighted share of the rays that escape (1 = open; specular occlusion), valid and blocked [N] int32 count the
    rays cast and those that hit a face.  Without a cube specular and reflected are None and the rest is the same.  The rays
    run to `max_distance` (None: no limit).  A point with mask [N] (uint8 or bool) == 0 is `masked`, a point whose position
    is not finite or whose normal is not of unit length within 2^-10 is `no_normal`, one whose view is not finite or not of
    unit length within 2^-10 is `no_view`: no rays, specular 0, visibility 1.  bias defaults as gather_points'.
    `directions` [L,K,R,3] overrides the table.  The result is a pure function of the arguments and does not depend on the
    grid (`cell`, `grid`).  N == 0 or a mesh with no usable face launches nothing and leaves every point open, and then
    nothing is reflected either: specular and reflected are 0, valid and blocked 0, and no ray is counted.  Report: n, misses,
    front_hits, back_hits, below_horizon, no_normal, no_view, masked, rays, rotations, levels, seed, max_distance (None:
    unlimited), bias, sky_res (None: no cube), radiosity (bool), faces_skipped, cell, dims, pairs.  One read-back (after the
    checks of cube and radiosity)."""
    what = "reflect_points"
    R, K, L, directions = _reflect_args(what, rays, rotations, levels, directions, max_distance, bias)
    m = _mesh_tensors(mesh, what)
    dev = m.vertices.device
    points = _check_points(points, dev, what)
    normals = _check_points(normals, dev, what, "normals")
    views = _check_points(views, dev, what, "views")
    N, F = int(points.shape[0]), int(m.faces.shape[0])
    if int(normals.shape[0]) != N or int(views.shape[0]) != N:
        raise ValueError("%s: %d points, %d normals, %d views" % (what, N, int(normals.shape[0]), int(views.shape[0])))
    if (not isinstance(roughness, torch.Tensor) or roughness.device != dev or roughness.dtype != torch.float32
            or tuple(roughness.shape) != (N,)):
        raise ValueError("%s: roughness must be a [%d] float32 tensor on the mesh's device" % (what, N))
    roughness = roughness.detach().contiguous()
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool)
                or tuple(mask.shape) != (N,)):
            raise ValueError("%s: mask must be a [%d] uint8 or bool tensor on the mesh's device" % (what, N))
        mask = mask.detach().to(torch.uint8).contiguous()
    if cube is not None:
        cube = _check_cube(cube, what)
        if cube.device != dev:
            raise RuntimeError("%s: the cube must be a tensor on the mesh's device: gigs-hip has no CPU path" % what)
    if radiosity is not None:
        radiosity = _check_radiosity(radiosity, m, what)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    report = dict(n=N, rays=R, rotations=K, levels=L, seed=seed, max_distance=None if max_distance is None else float(max_distance),
                  bias=0.0 if bias is None else float(bias), sky_res=int(cube.shape[1]) if cube is not None else None,
                  radiosity=radiosity is not None)
    report.update(dict.fromkeys(REFLECT_COUNTERS, 0))
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    light = (torch.zeros((N, 3), **f32), torch.zeros((N, 3), **f32)) if cube is not None else (None, None)
    empty = Reflection(*light, torch.ones(N, **f32), torch.zeros(N, **i32), torch.zeros(N, **i32))
    if N == 0:
        report.update(_grid_report(None, F))
        return empty, report
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        report.update(_grid_report(grid, F))
        if grid is None:  # no usable face: every point is open and nothing is launched
            live = mask != 0 if mask is not None else torch.ones(N, dtype=torch.bool, device=dev)
            n2, v2 = (normals.double() ** 2).sum(1), (views.double() ** 2).sum(1)
            lo, hi = 1.0 - 2.0 ** -10, 1.0 + 2.0 ** -10
            bad = live & ~(torch.isfinite(points).all(1) & (n2 >= lo) & (n2 <= hi))
            blind = live & ~bad & ~(torch.isfinite(views).all(1) & (v2 >= lo) & (v2 <= hi))
            got = torch.stack(((~live).sum(), bad.sum(), blind.sum())).cpu().tolist()
            report["masked"], report["no_normal"], report["no_view"] = int(got[0]), int(got[1]), int(got[2])
            return empty, report
        if bias is None:
            bias = 1e-3 * (0.1 * (max(grid.dims) * grid.cell))
        report["bias"] = float(bias)
        table = torch.from_numpy(directions).to(dev)
        return _reflect_points(points, normals, views, roughness, m, grid, cube, radiosity, table, max_distance, bias, seed, mask,
                               report), report


# ---- shadows of analytic lights per point (include/gigs_hip.h, "Shadows of analytic lights") --------------------------------
SHADOW_MAX_SAMPLES, SHADOW_MAX_ROTATIONS = 64, 64
SHADOW_COUNTERS = ("rays", "blocked", "below_horizon", "no_normal", "masked")


def shadow_points(points, normals, mesh, lights, samples=1, rotations=16, bias=None, max_distance=None, seed=0, mask=None,
                  grid=None):
    """(visibility [N,L] float32, lit [N,L] int32, report): for every point (`points`, `normals` [N,3] float32 on the mesh's
    device, gather_points' conventions for `mask` and the no_normal rule) and every one of the L analytic lights (a sequence of
    analytic_lights.AnalyticLight, or their packed [L,8] float32 rows) the share of the light's `samples` samples that reach
    the point past `mesh`, in one launch of any-hit shadow rays (gigs_mesh_shadow_points): the origin is point + bias normal,
    sample s of a point light aims at centre + radius u, of a directional light at -direction + tan(angle) u, with u row s of
    rotation mix64(seed 2^32 + q) mod rotations of analytic_lights.ball_offsets(samples, rotations); samples = 1 is the hard
    shadow towards the light's centre.  A sample whose direction does not rise above the point's tangent plane is dark
    without a ray; a directional light's rays stop at `max_distance` (None: no limit).  lit counts the samples that arrive,
    visibility = lit / samples; a masked or no_normal point gets visibility 1 and no rays.  bias defaults as gather_points'.
    The result is a pure function of the arguments and does not depend on the `grid`.  N == 0 or a mesh with no usable face
    launches nothing and returns 1 everywhere a ray would have been cast.  Report: n, lights, samples, rotations, seed,
    bias, max_distance (None: unlimited), rays, blocked, below_horizon, no_normal, masked, faces_skipped, cell, dims, pairs.
    One read-back."""
    import analytic_lights
    what = "shadow_points"
    S, K = int(samples), int(rotations)
    if S < 1 or S > SHADOW_MAX_SAMPLES:
        raise ValueError("%s: samples must lie in [1, %d], got %d" % (what, SHADOW_MAX_SAMPLES, S))
    if K < 1 or K > SHADOW_MAX_ROTATIONS:
        raise ValueError("%s: rotations must lie in [1, %d], got %d" % (what, SHADOW_MAX_ROTATIONS, K))
    for name, x in (("max_distance", max_distance), ("bias", bias)):
        if x is not None and not (float(x) >= 0 and np.isfinite(float(x))):
            raise ValueError("%s: %s must be finite and >= 0 or None, got %r" % (what, name, x))
    rows = analytic_lights.light_rows(lights, what)
    L = int(rows.shape[0])
    m = _mesh_tensors(mesh, what)
    dev = m.vertices.device
    points = _check_points(points, dev, what)
    normals = _check_points(normals, dev, what, "normals")
    N, V, F = int(points.shape[0]), int(m.vertices.shape[0]), int(m.faces.shape[0])
    if int(normals.shape[0]) != N:
        raise ValueError("%s: %d points, %d normals" % (what, N, int(normals.shape[0])))
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool)
                or tuple(mask.shape) != (N,)):
            raise ValueError("%s: mask must be a [%d] uint8 or bool tensor on the mesh's device" % (what, N))
        mask = mask.detach().to(torch.uint8).contiguous()
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    report = dict(n=N, lights=L, samples=S, rotations=K, seed=seed, bias=0.0 if bias is None else float(bias),
                  max_distance=None if max_distance is None else float(max_distance))
    report.update(dict.fromkeys(SHADOW_COUNTERS, 0))
    visibility = torch.ones((N, L), dtype=torch.float32, device=dev)
    lit = torch.full((N, L), S, dtype=torch.int32, device=dev)
    if N == 0:
        report.update(_grid_report(None, F))
        return visibility, lit, report
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m)
        report.update(_grid_report(grid, F))
        if bias is None and grid is not None:
            bias = 1e-3 * (0.1 * (max(grid.dims) * grid.cell))
            report["bias"] = float(bias)
        if grid is None:  # no usable face: nothing is launched; what would have been a ray arrives
            return _shadow_points_open(points, normals, rows, analytic_lights.ball_offsets(S, K), seed, 0.0 if bias is None else bias,
                                       mask, report)
        counts = _shadow_points(points, normals, m, grid, rows, analytic_lights.ball_offsets(S, K), seed, bias, max_distance, mask,
                                lit, visibility)
        got = [int(x) for x in counts.cpu()]  # the one read-back
        if got[5] != 0:
            raise MeshOverflow("shadow_points: an index left its range (%d points, %d vertices, %d faces)" % (N, V, F))
    report.update(zip(SHADOW_COUNTERS, got[:5]))
    return visibility, lit, report


def _shadow_points(points, normals, m: Mesh, grid, rows, offsets, seed, bias, max_distance, mask, lit, visibility, sort: bool = True):
    """The launch of shadow_points on checked arguments (grid is not None, N > 0) into lit and visibility [N,L] -> counts [6]
    int64 on the device: the five counters and overflow (an int32 in its low half).  sort=False: the points as they come."""
    dev = m.vertices.device
    N, L, (K, S) = int(points.shape[0]), int(rows.shape[0]), offsets.shape[:2]
    order = _cell_order(points.double(), grid) if sort else None
    d_rows, table = torch.from_numpy(rows).to(dev), torch.from_numpy(offsets).to(dev)
    counts = torch.zeros(6, dtype=torch.int64, device=dev)
    c_lo, c_dims = _c_grid(grid.lo, grid.dims)
    gigs_lib.check(gigs_lib.lib().gigs_mesh_shadow_points(
        int(m.vertices.shape[0]), int(m.faces.shape[0]), _p(m.vertices), _p(m.faces), c_lo, grid.cell, c_dims, _p(grid.cell_start),
        _p(grid.pairs), int(grid.pairs.shape[0]), _scale(grid), N, _p(points), _p(normals), _p(mask) if mask is not None else None,
        _p(order) if order is not None else None, L, _p(d_rows), _p(table), int(S), int(K), seed, float(bias),
        float("inf") if max_distance is None else float(max_distance), _p(lit), _p(visibility), counts.data_ptr(),
        counts[5:].data_ptr(), _stream()), "mesh_shadow_points")
    return counts


def _shadow_points_open(points, normals, rows, offsets, seed, bias, mask, report):
    """shadow_points against a mesh with no usable face, in torch float64: the classification of every sample with nothing
    to block it -> (visibility, lit, report).  Not a fall-back for the kernel: there is nothing to trace."""
    dev = points.device
    N, L, (K, S) = int(points.shape[0]), int(rows.shape[0]), offsets.shape[:2]
    live = mask != 0 if mask is not None else torch.ones(N, dtype=torch.bool, device=dev)
    n = normals.double()
    n2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    good = live & torch.isfinite(points).all(1) & (n2 >= 1.0 - 2.0 ** -10) & (n2 <= 1.0 + 2.0 ** -10)
    o = points.double() + float(bias) * n
    q = np.arange(N, dtype=np.uint64)
    with np.errstate(over="ignore"):
        k = (_mix64((np.uint64(seed) << np.uint64(32)) + q) % np.uint64(K)).astype(np.int64)
    u = torch.from_numpy(offsets.astype(np.float64)).to(dev)[torch.from_numpy(k).to(dev)]  # [N,S,3]
    r = torch.from_numpy(rows.astype(np.float64)).to(dev)
    lit = torch.full((N, L), int(S), dtype=torch.int32, device=dev)
    below = 0
    for l in range(L):
        e = r[l, 4]
        d = (r[l, 1:4] + e * u) - o[:, None, :] if rows[l, 0] == 0 else (-r[l, 1:4]) + e * u
        rise = (d[..., 0] * n[:, None, 0] + d[..., 1] * n[:, None, 1]) + d[..., 2] * n[:, None, 2]
        dark = ~(rise > 0) & good[:, None]
        lit[:, l] -= dark.sum(1).to(torch.int32)
        below += int(dark.sum())
    visibility = (lit.double() / float(S)).float()
    report["masked"], report["no_normal"] = int((~live).sum()), int((live & ~good).sum())
    report["below_horizon"], report["blocked"] = below, 0
    report["rays"] = int(good.sum()) * L * int(S) - below
    return visibility, lit, report


def _mix64(z):
    """The splitmix64 finaliser on uint64 arrays: the counter hash of the kernels (csrc/mesh_grid.h)."""
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sky_cube(light_or_base, res: int = 32) -> torch.Tensor:
    """[6,res,res,3] float32: a light's base cube ([6,N,N,3], a CubemapLight or its `base`) average-pooled to `res` texels an
    edge (N a multiple of res; res >= N returns the cube as it is) and clamped at 0, in torch: the sky gather_light looks up
    at the nearest texel.  A coarser sky trades angular detail for less noise at a few hundred rays; the default of 32, and
    the trade, are conventions, not measurements."""
    base = getattr(light_or_base, "base", light_or_base)
    if not isinstance(base, torch.Tensor) or base.dim() != 4 or base.shape[0] != 6 or base.shape[1] != base.shape[2] or base.shape[3] != 3:
        raise ValueError("sky_cube: expected a [6,N,N,3] cube, got %s" % (tuple(base.shape) if isinstance(base, torch.Tensor) else type(base).__name__,))
    base, N, res = base.detach().float(), int(base.shape[1]), int(res)
    if res < 1:
        raise ValueError("sky_cube: res must be >= 1, got %d" % res)
    if res < N:
        if N % res != 0:
            raise ValueError("sky_cube: the cube's edge %d is no multiple of res = %d" % (N, res))
        k = N // res
        base = base.view(6, res, k, res, k, 3).mean(dim=(2, 4))
    return base.clamp_min(0.0).contiguous()


# ---- texturing: the atlas of per-face charts, texel -> surface point, transfer (include/gigs_hip.h, "Texturing meshes") ------
TRANSFER_MAX_CHANNELS = 16
ATLAS_MAX_BLOCK = 1024


class AtlasLayout(NamedTuple):
    block: int           # B: a block is (B + 1) x B texels and holds two faces
    width: int           # W
    height: int          # H = rows B
    blocks_per_row: int  # W // (B + 1)
    n_blocks: int        # ceil(F / 2)


class Atlas(NamedTuple):
    layout: AtlasLayout
    uvs: torch.Tensor       # [F,3,2] float32, v = 0 at the bottom row of the image
    albedo: torch.Tensor    # [3,H,W] float32
    orm: torch.Tensor       # [3,H,W]: occlusion, roughness, metallic
    normal: torch.Tensor    # [3,H,W]: the world normal as interpolated, not normalised
    coverage: torch.Tensor  # [H,W] uint8: 1 where a texel was baked
    extra: torch.Tensor = None  # [C,H,W]: bake_atlas' `extra` channels (a light-map, say), None without them


def atlas_layout(F: int, block: int = 8, width=None) -> AtlasLayout:
    """The atlas of equal per-face charts for F faces: blocks of (block + 1) x block texels, two faces to a block (face f in
    block f // 2, half f % 2), row-major, width // (block + 1) to a row; height = rows * block.  `width` defaults to the
    smallest power of two whose square image holds the ceil(F / 2) blocks.  Host arithmetic."""
    B, F = int(block), int(F)
    if B < 3 or B > ATLAS_MAX_BLOCK:
        raise ValueError("atlas_layout: block must lie in [3, %d], got %d" % (ATLAS_MAX_BLOCK, B))
    if F < 0:
        raise ValueError("atlas_layout: F must be >= 0, got %d" % F)
    n_blocks = (F + 1) // 2
    if width is None:
        width = 1
        while width < B + 1 or (width // (B + 1)) * (width // B) < n_blocks:
            width *= 2
    width = int(width)
    if width < B + 1:
        raise ValueError("atlas_layout: a width of %d holds no block of %d x %d texels" % (width, B + 1, B))
    per_row = width // (B + 1)
    lay = AtlasLayout(B, width, -(-n_blocks // per_row) * B, per_row, n_blocks)
    if n_blocks * B * (B + 1) >= 2 ** 31:
        raise ValueError("atlas_layout: %d blocks of %d x %d texels are more than 2^31 texels" % (n_blocks, B + 1, B))
    return lay


def face_uvs(F: int, layout: AtlasLayout, device=None) -> torch.Tensor:
    """[F,3,2] float32: the UV of every face corner in `layout`, each the centre of a texel of the face's half of its block:
    (X / W, 1 - Y / H) for the point (X, Y) in texel coordinates, Y down the image rows, so v = 0 is the bottom row (the
    OBJ convention; include/gigs_hip.h, "Texturing meshes", 3).  Host arithmetic in float64, rounded once."""
    B, W, H, per_row = layout.block, layout.width, layout.height, layout.blocks_per_row
    F = int(F)
    if (F + 1) // 2 > layout.n_blocks:
        raise ValueError("face_uvs: %d faces do not fit the layout's %d blocks" % (F, layout.n_blocks))
    if F == 0:
        return torch.zeros((0, 3, 2), dtype=torch.float32, device=device)
    f = np.arange(F, dtype=np.int64)
    b, half = f // 2, f % 2
    corner = np.array([[(0, 0), (B - 2, 0), (0, B - 2)], [(B, B - 1), (2, B - 1), (B, 1)]], np.int64)[half]
    X = ((b % per_row) * (B + 1))[:, None] + corner[..., 0] + 0.5
    Y = ((b // per_row) * B)[:, None] + corner[..., 1] + 0.5
    uv = np.stack([X / float(W), 1.0 - Y / float(H)], -1).astype(np.float32)
    return torch.from_numpy(uv).to(device) if device is not None else torch.from_numpy(uv)


def _atlas_points(m: Mesh, lay: AtlasLayout):
    """-> (points [Q,3], bary [Q,2], texel_face [Q] int32, dest [Q] int64, overflow [1] int32 on the device)."""
    dev = m.vertices.device
    Q = lay.n_blocks * lay.block * (lay.block + 1)
    points, bary = torch.empty((Q, 3), dtype=torch.float32, device=dev), torch.empty((Q, 2), dtype=torch.float32, device=dev)
    texel_face, dest = torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.int64, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    if Q:
        gigs_lib.check(gigs_lib.lib().gigs_mesh_atlas_points(
            int(m.vertices.shape[0]), int(m.faces.shape[0]), _p(m.vertices), _p(m.faces), lay.block, lay.width, lay.height,
            lay.n_blocks, _p(points), _p(bary), _p(texel_face), _p(dest), overflow.data_ptr(), _stream()), "mesh_atlas_points")
    return points, bary, texel_face, dest, overflow


def atlas_points(mesh, layout: AtlasLayout):
    """(points [Q,3] float32, bary [Q,2] float32, texel_face [Q] int32, dest [Q] int64) for the Q = n_blocks B (B + 1) texels
    of `layout`'s blocks, block-major: the point of `mesh`'s surface each texel stands for, its weights (w1, w2) on its
    face, the face (-1 for a slot past F) and the texel's index y W + x in the image -- -1, with a NaN point, where nothing
    is to be baked (gigs_mesh_atlas_points).  One read-back (the flag)."""
    m = _mesh_tensors(mesh, "atlas_points")
    if (int(m.faces.shape[0]) + 1) // 2 != layout.n_blocks:
        raise ValueError("atlas_points: the layout is not the one of %d faces" % int(m.faces.shape[0]))
    with torch.cuda.device(m.vertices.device):
        points, bary, texel_face, dest, overflow = _atlas_points(m, layout)
        if int(overflow.item()) != 0:
            raise MeshOverflow("atlas_points: a texel left the %d x %d image" % (layout.width, layout.height))
    return points, bary, texel_face, dest


def _transfer(points: torch.Tensor, face: torch.Tensor, m: Mesh, values: torch.Tensor, dest=None, plane: int = 0):
    """-> (out ([N,C], or [C,plane] with dest; zero where nothing is stored), coverage [plane] uint8 or None, bary [N,2],
    counts [3] int64 on the device: transferred, skipped, overflow (an int32 in its low half))."""
    dev = m.vertices.device
    N, Cn = int(points.shape[0]), int(values.shape[1])
    out = torch.zeros((Cn, plane) if dest is not None else (N, Cn), dtype=torch.float32, device=dev)
    coverage = torch.zeros(plane, dtype=torch.uint8, device=dev) if dest is not None else None
    bary = torch.zeros((N, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros(3, dtype=torch.int64, device=dev)
    if N:
        gigs_lib.check(gigs_lib.lib().gigs_mesh_transfer(
            int(m.vertices.shape[0]), int(m.faces.shape[0]), _p(m.vertices), _p(m.faces), Cn, _p(values), N, _p(points), _p(face),
            _p(dest) if dest is not None else None, int(plane), out.data_ptr(),
            coverage.data_ptr() if coverage is not None else None, _p(bary), counts.data_ptr(), counts[2:].data_ptr(), _stream()),
            "mesh_transfer")
    return out, coverage, bary, counts


def _check_values(values, m: Mesh, what: str) -> torch.Tensor:
    dev = m.vertices.device
    if not isinstance(values, torch.Tensor) or values.device != dev:
        raise RuntimeError("%s: values must be a tensor on the mesh's device: gigs-hip has no CPU path" % what)
    if values.dim() == 1:
        values = values[:, None]
    if (values.dtype != torch.float32 or values.dim() != 2 or values.shape[0] != m.vertices.shape[0]
            or not 1 <= values.shape[1] <= TRANSFER_MAX_CHANNELS):
        raise ValueError("%s: values must be [V,C] float32 with 1 <= C <= %d, got %s %s" % (what, TRANSFER_MAX_CHANNELS,
                                                                                        tuple(values.shape), values.dtype))
    return values.contiguous()


def _check_points(points, dev, what: str, name: str = "points") -> torch.Tensor:
    if not isinstance(points, torch.Tensor) or points.device != dev:
        raise RuntimeError("%s: %s must be a tensor on the mesh's device: gigs-hip has no CPU path" % (what, name))
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError("%s: %s must be [N,3] float32, got %s %s" % (what, name, tuple(points.shape), points.dtype))
    return points.contiguous()


def transfer_at(points, face, src, values):
    """(out [N,C] float32, bary [N,2] float32, report): transfer_attributes without its search -- `face` [N] int32 names the
    face of `src` each point is projected on (-1: none; the point keeps 0).  Report: n, transferred, skipped.  A face index
    >= F raises MeshOverflow.  One read-back."""
    m = _mesh_tensors(src, "transfer_at")
    dev = m.vertices.device
    values = _check_values(values, m, "transfer_at")
    points = _check_points(points, dev, "transfer_at")
    N = int(points.shape[0])
    if not isinstance(face, torch.Tensor) or face.device != dev or face.dtype != torch.int32 or tuple(face.shape) != (N,):
        raise ValueError("transfer_at: face must be a [%d] int32 tensor on the mesh's device" % N)
    with torch.cuda.device(dev):
        out, _, bary, counts = _transfer(points, face.contiguous(), m, values)
        got = [int(x) for x in counts.cpu()]  # the one read-back
        if got[2] != 0:
            raise MeshOverflow("transfer_at: an index left its range (%d faces, %d queries)" % (int(m.faces.shape[0]), N))
    return out, bary, dict(n=N, transferred=got[0], skipped=got[1])


def transfer_attributes(points, src, values, cell=None, max_distance=None, grid=None):
    """(out [N,C] float32, face [N] int32, bary [N,2] float32, distance [N] float32, report): the per-vertex channels
    `values` ([V,C] float32, 1 <= C <= 16) of the mesh `src`, interpolated at the point of `src` closest to every point of
    `points` ([N,3] float32 on the mesh's device).  closest_point's search finds the face and the distance;
    gigs_mesh_transfer finds where on that face the closest point lies -- `bary` holds the weights of the face's second and
    third vertex -- and interpolates there.  A point the search gives no face (far, non-finite, no usable face) keeps 0 in
    `out` and `bary`.  With points = another mesh's vertices this is a per-vertex transfer.  `cell`, `grid`, `max_distance`
    as in closest_point.  Report: n, transferred, skipped, far, queries_invalid, faces_skipped, cell, dims, pairs.  One
    read-back."""
    _check_max_distance(max_distance)
    m = _mesh_tensors(src, "transfer_attributes")
    dev = m.vertices.device
    values = _check_values(values, m, "transfer_attributes")
    points = _check_points(points, dev, "transfer_attributes")
    N, F = int(points.shape[0]), int(m.faces.shape[0])
    if N == 0:
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        report = dict(n=0, transferred=0, skipped=0, far=0, queries_invalid=0)
        report.update(_grid_report(None, F))
        return (torch.empty((0, values.shape[1]), **f32), torch.empty(0, **i32), torch.empty((0, 2), **f32), torch.empty(0, **f32),
                report)
    with torch.cuda.device(dev):
        if grid is None:
            grid = triangle_grid(m, cell)
        distance, face, flags = _closest(points, m, grid, max_distance)
        out, _, bary, counts = _transfer(points, face, m, values)
        got = [int(x) for x in torch.cat((flags.long(), counts)).cpu()]  # the one read-back
        if got[2] != 0 or got[5] != 0:
            raise MeshOverflow("transfer_attributes: an index left its range (%d faces, %d queries)" % (F, N))
    report = dict(n=N, transferred=got[3], skipped=got[4], far=got[0], queries_invalid=got[1])
    report.update(_grid_report(grid, F))
    return out, face, bary, distance, report


def bake_atlas(dst, src, block: int = 8, width=None, occlusion=None, max_distance=None, cell=None, grid=None, extra=None):
    """(Atlas, report): the materials of the mesh `src` baked into a texture atlas over the mesh `dst` (a simplification of
    src, usually).  Every face of dst gets a chart of its own in atlas_layout(F, block, width); every texel of a chart
    stands for a point of its face (gigs_mesh_atlas_points; the one row of texels past the chart's long edge for the
    extrapolated point of the face's plane: the gutter), the closest face of src to that point is searched
    (triangle_grid(src) unless `grid` is passed, gigs_mesh_closest), and src's albedo, occlusion, roughness, metallic and
    normal are interpolated at the closest point (gigs_mesh_transfer, nine channels in one launch).  `occlusion`: [V_src]
    float32 such as bake_occlusion's, 1 where None.  `extra`: [V_src, C] float32, C <= 7, more per-vertex channels of src (the
    irradiance of bake_light, for a light-map) interpolated in the same launch and returned as Atlas.extra [C,H,W]; None
    changes nothing.  The normal plane holds the interpolated world normal as it is, not
    normalised.  Texels of no face, of an unusable face of dst, or with no face of src within `max_distance` stay 0 with
    coverage 0.  max_distance=None searches without a limit: a texel far from src then walks O(G^3) cell headers alone
    (closest_point), which a dst that is a simplification of src never does.  The result is a pure function of (dst, src,
    block, width, occlusion, max_distance): `cell` and `grid` only change the time.  Report: texels (= W H), baked,
    unbaked, far, queries_invalid, faces_skipped, block, width, height, blocks_per_row, n_blocks, cell, dims, pairs,
    distance_mean, distance_max (texel to src, over the baked texels).  F == 0 launches nothing.  One read-back."""
    _check_max_distance(max_distance)
    d, m = _mesh_tensors(dst, "bake_atlas"), _mesh_tensors(src, "bake_atlas")
    dev = m.vertices.device
    if d.vertices.device != dev:
        raise RuntimeError("bake_atlas: the two meshes must live on one device")
    V, F_src, F = int(m.vertices.shape[0]), int(m.faces.shape[0]), int(d.faces.shape[0])
    if occlusion is None:
        occlusion = torch.ones(V, dtype=torch.float32, device=dev)
    elif (not isinstance(occlusion, torch.Tensor) or occlusion.device != dev or occlusion.dtype != torch.float32
          or tuple(occlusion.shape) != (V,)):
        raise ValueError("bake_atlas: occlusion must be a [%d] float32 tensor on the mesh's device" % V)
    Ce = 0
    if extra is not None:
        if (not isinstance(extra, torch.Tensor) or extra.device != dev or extra.dtype != torch.float32 or extra.dim() != 2
                or extra.shape[0] != V or not 1 <= extra.shape[1] <= TRANSFER_MAX_CHANNELS - 9):
            raise ValueError("bake_atlas: extra must be a [%d,C] float32 tensor on the mesh's device with 1 <= C <= %d"
                             % (V, TRANSFER_MAX_CHANNELS - 9))
        Ce = int(extra.shape[1])
    lay = atlas_layout(F, block, width)
    W, H = lay.width, lay.height
    report = dict(texels=W * H, baked=0, unbaked=W * H, far=0, queries_invalid=0, **lay._asdict())
    with torch.cuda.device(dev):
        uvs = face_uvs(F, lay, device=dev)
        if F == 0:
            z3 = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
            report.update(_grid_report(None, F_src), distance_mean=0.0, distance_max=0.0)
            return Atlas(lay, uvs, z3, z3.clone(), z3.clone(), torch.zeros((H, W), dtype=torch.uint8, device=dev),
                         torch.zeros((Ce, H, W), dtype=torch.float32, device=dev) if Ce else None), report
        values = torch.cat((m.albedo, occlusion[:, None], m.roughness[:, None], m.metallic[:, None], m.normals)
                           + ((extra,) if Ce else ()), 1).contiguous()
        points, _, _, dest, flag = _atlas_points(d, lay)
        if grid is None:
            grid = triangle_grid(m, cell)
        distance, face, flags = _closest(points, m, grid, max_distance)
        out, coverage, _, counts = _transfer(points, face, m, values, dest, W * H)
        near = face >= 0
        dn = torch.where(near, distance, torch.zeros_like(distance)).double()
        stats = torch.stack((dn.sum(), dn.max(), near.sum().double()))
        got = torch.cat((flags.double(), counts.double(), flag.double(), stats)).cpu().tolist()  # the one read-back
        if got[2] != 0 or got[5] != 0 or got[6] != 0:
            raise MeshOverflow("bake_atlas: an index left its range (%d faces, %d texels)" % (F_src, int(points.shape[0])))
    baked = int(got[3])
    report.update(baked=baked, unbaked=W * H - baked, far=int(got[0]), queries_invalid=int(got[1]),
                  distance_mean=got[7] / got[9] if got[9] else 0.0, distance_max=got[8])
    report.update(_grid_report(grid, F_src))
    planes = out.view(9 + Ce, H, W)
    return Atlas(lay, uvs, planes[0:3], planes[3:6], planes[6:9], coverage.view(H, W), planes[9:] if Ce else None), report


def sample_atlas(atlas_planes: torch.Tensor, layout: AtlasLayout, face: torch.Tensor, bary: torch.Tensor) -> torch.Tensor:
    """[N,C] float64: the planes [C,H,W] of an atlas looked up bilinearly at the UV of the points (face [N], bary [N,2] =
    the weights of the face's second and third vertex): uv = w0 uv0 + w1 uv1 + w2 uv2 on face_uvs' float32 corners, texel
    coordinates x = u W - 1/2, y = (1 - v) H - 1/2, the four taps clamped to the image.  Torch gathers in float64 on the
    planes' device: host glue for tests and reports, not a kernel."""
    dev = atlas_planes.device
    Cn, H, W = (int(s) for s in atlas_planes.shape)
    face = face.to(dev).long()
    N = int(face.shape[0])
    if N == 0 or H == 0:
        return torch.zeros((N, Cn), dtype=torch.float64, device=dev)
    uv = face_uvs(2 * layout.n_blocks, layout, device=dev).double()[face]  # [N,3,2]
    b = bary.to(dev).double()
    w1, w2 = b[:, 0], b[:, 1]
    w0 = (1.0 - w1) - w2
    u = (w0 * uv[:, 0, 0] + w1 * uv[:, 1, 0]) + w2 * uv[:, 2, 0]
    v = (w0 * uv[:, 0, 1] + w1 * uv[:, 1, 1]) + w2 * uv[:, 2, 1]
    x, y = u * W - 0.5, (1.0 - v) * H - 0.5
    x0, y0 = x.floor(), y.floor()
    fx, fy = x - x0, y - y0
    xa, xb = x0.clamp(0, W - 1).long(), (x0 + 1).clamp(0, W - 1).long()
    ya, yb = y0.clamp(0, H - 1).long(), (y0 + 1).clamp(0, H - 1).long()
    flat = atlas_planes.reshape(Cn, H * W).double()
    top = (1.0 - fx) * flat[:, ya * W + xa] + fx * flat[:, ya * W + xb]
    bot = (1.0 - fx) * flat[:, yb * W + xa] + fx * flat[:, yb * W + xb]
    return ((1.0 - fy) * top + fy * bot).T.contiguous()
