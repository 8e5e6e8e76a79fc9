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
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        empty = Mesh(torch.empty((0, 3), **f32), torch.empty((0, 3), **i32), torch.empty((0, 3), **f32),
                     torch.empty((0, 3), **f32), torch.empty((0,), **f32), torch.empty((0,), **f32))
        Gx, Gy, Gz = self.dims
        cells = (Gx - 1) * (Gy - 1) * (Gz - 1)
        if cells == 0:
            return empty
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
                return empty
            cell_off, quad_off = cell_incl - flags, quad_incl - quads
            F = 2 * Q
            m = Mesh(torch.empty((V, 3), **f32), torch.empty((F, 3), **i32), torch.empty((V, 3), **f32),
                     torch.empty((V, 3), **f32), torch.empty((V,), **f32), torch.empty((V,), **f32))
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


def _p(t):
    return t.data_ptr() if t.numel() else None


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


def clean(mesh, keep_largest: int = 0, min_faces: int = 0) -> Tuple[Mesh, Dict]:
    """(the mesh without the components of fewer than keep_threshold faces, a report).  Invalid faces and the vertices no
    kept face references go too; with keep_largest = min_faces = 0 nothing else does.  Kept vertices and faces stay in
    their order, values are copied bit for bit.  Report: components, components_kept, faces_removed, vertices_removed,
    invalid_faces, rounds, threshold."""
    m = _mesh_tensors(mesh, "clean")
    dev = m.vertices.device
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)

    def sized(v, f):
        return Mesh(torch.empty((v, 3), **f32), torch.empty((f, 3), **i32), torch.empty((v, 3), **f32),
                    torch.empty((v, 3), **f32), torch.empty((v,), **f32), torch.empty((v,), **f32))

    if V == 0 or F == 0:
        return sized(0, 0), dict(components=0, components_kept=0, faces_removed=F, vertices_removed=V, invalid_faces=F,
                                 rounds=0, threshold=keep_threshold([], keep_largest, min_faces))
    lib = gigs_lib.lib()
    with torch.cuda.device(dev):
        labels, face_labels, count, invalid, rounds = _label(m)
        comp = count > 0
        thr = keep_threshold(count[comp], keep_largest, min_faces)
        root_keep = (count >= thr).to(torch.uint8)
        face_keep, vertex_keep = torch.empty(F, **i32), torch.empty(V, **i32)
        gigs_lib.check(lib.gigs_mesh_mark(V, F, _p(m.faces), _p(face_labels), _p(root_keep), _p(face_keep), _p(vertex_keep),
                                          _stream()), "mesh_mark")
        v_incl = torch.cumsum(vertex_keep, 0, dtype=torch.int32)
        f_incl = torch.cumsum(face_keep, 0, dtype=torch.int32)
        V2, F2, n_comp, n_kept, n_invalid = (int(x) for x in torch.stack(
            (v_incl[-1], f_incl[-1], comp.sum().to(torch.int32), root_keep.sum().to(torch.int32), invalid[0])).cpu())
        out = sized(V2, F2)
        v_off, f_off = v_incl - vertex_keep, f_incl - face_keep
        if V2 and F2:
            overflow = torch.zeros(1, **i32)
            gigs_lib.check(lib.gigs_mesh_compact(
                V, F, _p(m.vertices), _p(m.normals), _p(m.albedo), _p(m.roughness), _p(m.metallic), _p(m.faces), _p(vertex_keep),
                _p(v_off), _p(face_keep), _p(f_off), V2, F2, _p(out.vertices), _p(out.normals),
                _p(out.albedo), _p(out.roughness), _p(out.metallic), _p(out.faces), overflow.data_ptr(), _stream()),
                "mesh_compact")
            if int(overflow.item()) != 0:
                raise MeshOverflow("clean: an index left the outputs (%d vertices, %d faces)" % (V2, F2))
    return out, dict(components=n_comp, components_kept=n_kept, faces_removed=F - F2, vertices_removed=V - V2,
                     invalid_faces=n_invalid, rounds=rounds, threshold=thr)
