"""Rendering and relighting a triangle mesh with per-vertex materials (mesh.Mesh, the PLY of extract_mesh.py) or with a
texture atlas (mesh.Atlas, the OBJ + PNGs of texture_mesh.py): a visibility-buffer rasterizer fills the G-buffer planes the blend kernel writes in inference mode, and the deferred chain
behind them is the existing one, unchanged.

    mesh_arrays(mesh)                 a mesh.Mesh, a dict of scene_io.read_mesh_ply or a path -> checked numpy arrays
    device_mesh(source, device)       those arrays as a mesh.Mesh on the device: what the mesh tools load a PLY with
    MeshRasterizer(mesh)(cam)         gigs_mesh_project, gigs_mesh_raster, gigs_mesh_resolve -> opacity, depth, pos, normal,
                                      normal_view, albedo, roughness, metallic ([C,H,W]) and tri_id [H,W] (-1 = background)
    TexturedMeshRasterizer(mesh, uvs, albedo, orm, normal)(cam)   the same rasterizer over a mesh whose materials live in a
                                      texture atlas (mesh.bake_atlas's planes, texture_mesh.py's OBJ + PNGs): project and raster
                                      are inherited, the resolve is gigs_mesh_resolve_textured -> the same planes and
                                      `occlusion` [1,H,W], the atlas's baked O channel.  from_atlas(mesh, atlas) takes a
                                      mesh.Atlas as it is; load_textured_mesh(path.obj) reads the files back
    mesh_planes(rast, cam, gi, occlusion="ssao")   those planes plus the derived normals (gigs_derive_normal) and the
                                      occlusion: SSAO with the GI settings ("ssao"), the atlas's baked channel ("baked", no
                                      SSAO launch) or their product ("both"): the rasterizer's twelve outputs, by name
    MeshGBuffer(gi, metallic)(cam, rast)   the G-buffer source of relight.py's relighters: mesh_planes, then
                                      relight.gbuffer_from_planes (G-buffer post, the reference's F0 quirk)
    MeshRelighter / MeshMultiRelighter / MeshTurntableRelighter   relight.py's three relighters constructed over that source:
                                      rl(cam, rast, view_dirs).  Only the G-buffer differs; shade, SSR march and the sRGB /
                                      median finish are theirs, and the result gains the source's extra planes
    RaytracedLight(mesh, rays, cube)  a mesh as occluder and bounce surface of any view's pixels: .planes(pos_view, normal,
                                      viewmatrix, mask) -> occlusion, hits, irradiance, indirect by mesh.gather_points
                                      (gigs_mesh_gather_points): a final gather per pixel over the mesh's baked radiosity
    RaytracedGBuffer(inner, tracer)   a G-buffer source around MeshGBuffer or relight.SplatGBuffer whose occlusion plane is the
                                      traced one, or its product with the inner plane: the relighters take it through source=;
                                      reflections=True adds the traced specular planes to its extras
    RaytracedLight.reflections(pos_view, normal, roughness, viewmatrix, campos, mask)   a GGX lobe of rays about every pixel's
                                      mirror direction by mesh.reflect_points (gigs_mesh_reflect_points): specular, reflected,
                                      visibility; prepare_views(points, campos) makes its view vectors
    compose_reflections(normals, views, roughness, radiance, ...)   the shade's specular_rgb = radiance (F0 fg.x + fg.y) on a
                                      supplied radiance (gigs_reflect_compose)

The arithmetic is stated in include/gigs_hip.h and restated in numpy by tests/mesh_raster_ref.py (the textured resolve by
tests/mesh_texture_ref.py).  There is no clipping:
a triangle with a vertex behind the near cull (view z <= 0.2) or outside the guard band of 16384 pixels is dropped whole.
There is no CPU path, and no hipGraph replay (the source says so: relight.py's replay is keyed on the Gaussian tensors and
asynchronous binning): graphs=True raises.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

import denoise as denoise_ops
import gigs_lib
import mesh as mesh_ops
import relight
from diff_gaussian_rasterization import _C as _ops, _derive_normal

_lib = gigs_lib.lib()

MESH_KEYS = ("vertices", "faces", "normals", "albedo", "roughness", "metallic")
PLANES = {"opacity": 1, "depth": 1, "pos": 3, "normal": 3, "normal_view": 3, "albedo": 3, "roughness": 1, "metallic": 1}
TEXTURED_PLANES = dict(PLANES, occlusion=1)  # gigs_mesh_resolve_textured's float planes, in its argument order
OCCLUSION_MODES = ("ssao", "baked", "both")
TEXTURE_MAX = 16384  # texels a side: gigs_mesh_resolve_textured's limit


def mesh_arrays(mesh) -> Dict[str, np.ndarray]:
    """{vertices [V,3], faces [F,3] int32, normals, albedo [V,3], roughness, metallic [V]} as contiguous numpy arrays, from a
    mesh.Mesh (or any sequence in its field order), a dict with MESH_KEYS (scene_io.read_mesh_ply's) or the path of a PLY
    written by scene_io.save_mesh_ply.  Face indices are NOT checked here: the kernels drop a face with a bad index."""
    if isinstance(mesh, str):
        import scene_io
        mesh = scene_io.read_mesh_ply(mesh)
    if not isinstance(mesh, dict):
        mesh = dict(zip(MESH_KEYS, mesh))
    missing = [k for k in MESH_KEYS if k not in mesh]
    if missing:
        raise ValueError("mesh_arrays: the mesh lacks %s" % ", ".join(missing))
    a = {k: (mesh[k].detach().cpu().numpy() if isinstance(mesh[k], torch.Tensor) else np.asarray(mesh[k])) for k in MESH_KEYS}
    out = {"faces": np.ascontiguousarray(a["faces"], dtype=np.int32).reshape(-1, 3)}
    for k in ("vertices", "normals", "albedo"):
        out[k] = np.ascontiguousarray(a[k], dtype=np.float32).reshape(-1, 3)
    for k in ("roughness", "metallic"):
        out[k] = np.ascontiguousarray(a[k], dtype=np.float32).reshape(-1)
    V = out["vertices"].shape[0]
    for k in ("normals", "albedo", "roughness", "metallic"):
        if out[k].shape[0] != V:
            raise ValueError("mesh_arrays: %s has %d rows for %d vertices" % (k, out[k].shape[0], V))
    return out


def device_mesh(source, device) -> mesh_ops.Mesh:
    """mesh_arrays(source) as a mesh.Mesh of tensors on `device`."""
    arrays = mesh_arrays(source)
    return mesh_ops.Mesh(*(torch.from_numpy(arrays[k]).to(device) for k in mesh_ops.Mesh._fields))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


class MeshRasterizer:
    """The mesh on the device and the scratch a view needs (projected vertices, the key plane, the list of large
    triangles), reused from view to view.  small_max: the largest box, in pixels, a triangle's own thread walks (None =
    gigs_lib.MESH_SMALL_MAX); the result does not depend on it."""

    def __init__(self, mesh, device="cuda", small_max: Optional[int] = None):
        self._set_device(device)
        arrays = mesh_arrays(mesh)
        self._upload({k: torch.from_numpy(v) for k, v in arrays.items()}, small_max)

    def _set_device(self, device) -> None:
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("MeshRasterizer: the mesh must live on a CUDA/HIP device: gigs-hip has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _upload(self, tensors: Dict[str, torch.Tensor], small_max: Optional[int]) -> None:
        """The checked arrays on the device, and the scratch of a view."""
        self.V, self.F = int(tensors["vertices"].shape[0]), int(tensors["faces"].shape[0])
        self.small_max = small_max
        self._mesh = {k: v.to(self.device) for k, v in tensors.items()}
        dev = self.device
        self._view_pos = torch.empty((self.V, 3), dtype=torch.float32, device=dev)
        self._screen = torch.empty((self.V, 2), dtype=torch.int32, device=dev)
        self._flags = torch.empty((self.V,), dtype=torch.uint8, device=dev)
        self._list = torch.empty(int(_lib.gigs_mesh_raster_scratch_bytes(self.F)), dtype=torch.uint8, device=dev)
        self._vis = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        self._mesh = self._view_pos = self._screen = self._flags = self._list = self._vis = None

    def _check(self):
        if self._mesh is None:
            raise RuntimeError("MeshRasterizer: closed")

    @staticmethod
    def _viewmatrix(cam, dev) -> torch.Tensor:
        vm = cam["viewmatrix"]
        vm = vm if isinstance(vm, torch.Tensor) else torch.as_tensor(np.asarray(vm, dtype=np.float32))
        return vm.detach().to(device=dev, dtype=torch.float32).contiguous()

    def project(self, cam: Dict):
        """gigs_mesh_project -> (view_pos [V,3], screen [V,2] int32, flags [V] uint8): the rasterizer's own buffers,
        overwritten by the next view."""
        self._check()
        W, H = int(cam["image_width"]), int(cam["image_height"])
        vm = self._viewmatrix(cam, self.device)
        with torch.cuda.device(self.device):
            gigs_lib.check(_lib.gigs_mesh_project(self.V, _p(self._mesh["vertices"]), vm.data_ptr(), float(cam["tanfovx"]),
                                                  float(cam["tanfovy"]), W, H, _p(self._view_pos), _p(self._screen),
                                                  _p(self._flags), _stream()), "mesh_project")
        return self._view_pos, self._screen, self._flags

    def raster(self, width: int, height: int, view_pos=None, screen=None, flags=None, small_max: Optional[int] = None,
               faces=None) -> torch.Tensor:
        """gigs_mesh_raster on the projected arrays (by default the last project()'s) -> the key plane [H,W] as int64 (the
        kernel's uint64 bits; -1 = empty), overwritten by the next view."""
        self._check()
        W, H = int(width), int(height)
        dev = self.device
        view_pos = self._view_pos if view_pos is None else view_pos
        screen = self._screen if screen is None else screen
        flags = self._flags if flags is None else flags
        faces = self._mesh["faces"] if faces is None else faces
        F = int(faces.shape[0])
        scratch = self._list
        if F != self.F:
            scratch = torch.empty(int(_lib.gigs_mesh_raster_scratch_bytes(F)), dtype=torch.uint8, device=dev)
        if self._vis is None or tuple(self._vis.shape) != (H, W):
            self._vis = torch.empty((H, W), dtype=torch.int64, device=dev)
        sm = self.small_max if small_max is None else small_max
        with torch.cuda.device(dev):
            self._vis.fill_(-1)
            gigs_lib.check(_lib.gigs_mesh_raster(int(flags.shape[0]), F, _p(faces), _p(view_pos), _p(screen), _p(flags), W, H,
                                                 -1 if sm is None else int(sm), self._vis.data_ptr(), scratch.data_ptr(),
                                                 _stream()), "mesh_raster")
        return self._vis

    def resolve(self, cam: Dict, vis: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """gigs_mesh_resolve of a key plane (by default the last raster()'s) with the last project()'s arrays -> fresh
        planes."""
        self._check()
        W, H = int(cam["image_width"]), int(cam["image_height"])
        dev = self.device
        vis = self._vis if vis is None else vis
        if vis is None or tuple(vis.shape) != (H, W):
            raise ValueError("MeshRasterizer.resolve: no key plane of %d x %d" % (H, W))
        vm = self._viewmatrix(cam, dev)
        out = {k: torch.empty((c, H, W), dtype=torch.float32, device=dev) for k, c in PLANES.items()}
        out["tri_id"] = torch.empty((H, W), dtype=torch.int32, device=dev)
        m = self._mesh
        with torch.cuda.device(dev):
            gigs_lib.check(_lib.gigs_mesh_resolve(
                self.V, self.F, _p(m["faces"]), _p(self._view_pos), _p(self._screen), _p(self._flags), _p(m["normals"]),
                _p(m["albedo"]), _p(m["roughness"]), _p(m["metallic"]), vm.data_ptr(), W, H, vis.data_ptr(),
                *(out[k].data_ptr() for k in PLANES), out["tri_id"].data_ptr(), _stream()), "mesh_resolve")
        return out

    @torch.no_grad()
    def __call__(self, cam: Dict, small_max: Optional[int] = None) -> Dict[str, torch.Tensor]:
        self.project(cam)
        self.raster(cam["image_width"], cam["image_height"], small_max=small_max)
        return self.resolve(cam)


def _texture(t, name: str) -> torch.Tensor:
    """A [3,Ht,Wt] float32 plane set as a contiguous tensor (wherever it lives), 1 <= Wt, Ht <= TEXTURE_MAX."""
    if not isinstance(t, torch.Tensor):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != 3:
        raise ValueError("TexturedMeshRasterizer: %s must be [3,Ht,Wt] float32, got %s %s" % (name, tuple(t.shape), t.dtype))
    if not (1 <= t.shape[1] <= TEXTURE_MAX and 1 <= t.shape[2] <= TEXTURE_MAX):
        raise ValueError("TexturedMeshRasterizer: %s is %d x %d texels; 1 to %d a side" % (name, t.shape[2], t.shape[1],
                                                                                        TEXTURE_MAX))
    return t.detach().contiguous()



class TexturedMeshRasterizer(MeshRasterizer):
    """MeshRasterizer over a mesh whose materials are textures.  mesh: a dict with vertices [V,3] and faces [F,3] (and
    normals [V,3], needed only without a normal texture), a mesh.Mesh or any sequence in its field order; per-vertex
    albedo / roughness / metallic are not looked at.  uvs [F,3,2] float32: one UV per face corner (mesh.face_uvs',
    scene_io.read_mesh_obj()["uvs"]; v = 0 is the bottom row).  albedo, orm (occlusion, roughness, metallic) and normal (the
    world normal, not normalised; None = interpolate the vertex normals) are [3,Ht,Wt] float32 tensors or arrays of one
    size.  project and raster are MeshRasterizer's; resolve calls gigs_mesh_resolve_textured."""

    def __init__(self, mesh, uvs, albedo, orm, normal=None, device="cuda", small_max: Optional[int] = None):
        self._set_device(device)
        if not isinstance(mesh, dict):
            mesh = dict(zip(MESH_KEYS, mesh))
        if "vertices" not in mesh or "faces" not in mesh:
            raise ValueError("TexturedMeshRasterizer: the mesh lacks vertices or faces")

        def tensor(a, dtype, cols):
            t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            return t.to(dtype).reshape(-1, *cols).contiguous()

        tensors = dict(vertices=tensor(mesh["vertices"], torch.float32, (3,)), faces=tensor(mesh["faces"], torch.int32, (3,)))
        V, F = int(tensors["vertices"].shape[0]), int(tensors["faces"].shape[0])
        if mesh.get("normals") is not None:
            tensors["normals"] = tensor(mesh["normals"], torch.float32, (3,))
            if int(tensors["normals"].shape[0]) != V:
                raise ValueError("TexturedMeshRasterizer: normals has %d rows for %d vertices" % (tensors["normals"].shape[0], V))
        elif normal is None:
            raise ValueError("TexturedMeshRasterizer: without a normal texture the mesh needs per-vertex normals")
        uv = uvs.detach() if isinstance(uvs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(uvs))
        if uv.dtype != torch.float32 or tuple(uv.shape) != (F, 3, 2):
            raise ValueError("TexturedMeshRasterizer: uvs must be [%d,3,2] float32, got %s %s" % (F, tuple(uv.shape), uv.dtype))
        tensors["uvs"] = uv.contiguous()
        tensors["tex_albedo"], tensors["tex_orm"] = _texture(albedo, "albedo"), _texture(orm, "orm")
        if normal is not None:
            tensors["tex_normal"] = _texture(normal, "normal")
        size = tuple(tensors["tex_albedo"].shape)
        for k in ("tex_orm", "tex_normal"):
            if k in tensors and tuple(tensors[k].shape) != size:
                raise ValueError("TexturedMeshRasterizer: %s is %s, albedo is %s" % (k[4:], tuple(tensors[k].shape), size))
        self.texture_size = (int(size[2]), int(size[1]))  # (Wt, Ht)
        self._upload(tensors, small_max)

    @classmethod
    def from_atlas(cls, mesh, atlas, device=None, small_max: Optional[int] = None):
        """The rasterizer over a mesh.Atlas of `mesh` (mesh.bake_atlas's): its float planes as they are, no quantisation."""
        return cls(mesh, atlas.uvs, atlas.albedo, atlas.orm, atlas.normal, device=atlas.albedo.device if device is None else device,
                   small_max=small_max)

    def resolve(self, cam: Dict, vis: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """gigs_mesh_resolve_textured of a key plane (by default the last raster()'s) with the last project()'s arrays ->
        fresh planes: MeshRasterizer.resolve's, and occlusion [1,H,W]."""
        self._check()
        W, H = int(cam["image_width"]), int(cam["image_height"])
        dev = self.device
        vis = self._vis if vis is None else vis
        if vis is None or tuple(vis.shape) != (H, W):
            raise ValueError("TexturedMeshRasterizer.resolve: no key plane of %d x %d" % (H, W))
        vm = self._viewmatrix(cam, dev)
        out = {k: torch.empty((c, H, W), dtype=torch.float32, device=dev) for k, c in TEXTURED_PLANES.items()}
        out["tri_id"] = torch.empty((H, W), dtype=torch.int32, device=dev)
        m = self._mesh
        Wt, Ht = self.texture_size
        with torch.cuda.device(dev):
            gigs_lib.check(_lib.gigs_mesh_resolve_textured(
                self.V, self.F, _p(m["faces"]), _p(self._view_pos), _p(self._screen), _p(self._flags), _p(m["uvs"]),
                _p(m.get("normals")), Wt, Ht, m["tex_albedo"].data_ptr(), m["tex_orm"].data_ptr(), _p(m.get("tex_normal")),
                vm.data_ptr(), W, H, vis.data_ptr(), *(out[k].data_ptr() for k in TEXTURED_PLANES), out["tri_id"].data_ptr(),
                _stream()), "mesh_resolve_textured")
        return out


def load_textured_mesh(path_obj: str) -> Dict:
    """An OBJ of scene_io.save_mesh_obj with the PNGs its .mtl names (texture_mesh.py's output) -> the arguments of
    TexturedMeshRasterizer: {mesh: {vertices, faces, normals (or None)}, uvs [F,3,2], albedo, orm, normal [3,Ht,Wt] float32}.
    The PNGs are decoded on the host (PIL): albedo and ORM as c / 255, the normal as 2 c / 255 - 1, the inverse of
    texture_mesh.normal_image up to the 8 bits; it is not renormalised (the resolve does not ask for unit length)."""
    from PIL import Image

    import scene_io
    obj = scene_io.read_mesh_obj(path_obj)
    folder = os.path.dirname(path_obj)

    def png(name):
        with Image.open(os.path.join(folder, obj["textures"][name])) as im:
            c = np.asarray(im.convert("RGB"), dtype=np.uint8)
        return np.ascontiguousarray(c.transpose(2, 0, 1)).astype(np.float32)

    albedo, orm, normal = png("albedo") / np.float32(255.0), png("orm") / np.float32(255.0), png("normal")
    normal = np.float32(2.0) * normal / np.float32(255.0) - np.float32(1.0)
    if albedo.shape != orm.shape or albedo.shape != normal.shape:
        raise ValueError("%s: the albedo, ORM and normal images differ in size" % path_obj)
    return dict(mesh=dict(vertices=obj["vertices"], faces=obj["faces"], normals=obj["normals"]), uvs=obj["uvs"], albedo=albedo,
                orm=orm, normal=normal)


@torch.no_grad()
def mesh_planes(rast: MeshRasterizer, cam: Dict, gi: Dict, occlusion: str = "ssao") -> Dict[str, torch.Tensor]:
    """What GaussianRasterizer.forward returns for the Gaussians (inference, derive_normal), for the mesh and by name:
    the resolve's planes, normal_from_depth and depth_pos (gigs_derive_normal of the depth plane: 3x3 median, depth to
    normal, bilateral filter, median of the positions) and occlusion_map: "ssao", SSAO of normal_view over depth_pos;
    "baked", the occlusion plane of a TexturedMeshRasterizer's resolve, with no SSAO launch; "both", their product.  A
    textured rasterizer's result also holds that plane as baked_occlusion."""
    if occlusion not in OCCLUSION_MODES:
        raise ValueError("mesh_planes: occlusion is one of %s, got %r" % (", ".join(OCCLUSION_MODES), occlusion))
    textured = isinstance(rast, TexturedMeshRasterizer)
    if occlusion != "ssao" and not textured:
        raise ValueError("mesh_planes: occlusion=%r needs a TexturedMeshRasterizer: a plain mesh has no baked channel" % occlusion)
    W, H = int(cam["image_width"]), int(cam["image_height"])
    if W < 2 or H < 2:
        raise ValueError("mesh_planes: the derived normals need an image of at least 2 x 2")
    o = rast(cam)
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    vm = rast._viewmatrix(cam, rast.device)
    with torch.cuda.device(rast.device):
        normal_from_depth, depth_pos = _derive_normal(W, H, fx, fy, vm, o["depth"])
        if occlusion == "baked":
            occlusion_map = o["occlusion"]
        else:
            occlusion_map = _ops.SSAO(W, H, fx, fy, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"],
                                      o["normal_view"], depth_pos)
            if occlusion == "both":
                occlusion_map = occlusion_map * o["occlusion"]
    r = dict(opacity_map=o["opacity"], depth_map=o["depth"], normal_map_from_depth=normal_from_depth,
             normal_map=o["normal"], occlusion_map=occlusion_map, albedo_map=o["albedo"], roughness_map=o["roughness"],
             metallic_map=o["metallic"], out_normal_view=o["normal_view"], depth_pos=depth_pos, pos=o["pos"],
             tri_id=o["tri_id"], viewmatrix=vm)
    if textured:
        r["baked_occlusion"] = o["occlusion"]
    return r


class MeshGBuffer:
    """The G-buffer of a mesh (relight.py documents its keys): source(cam, rast) runs mesh_planes over a MeshRasterizer and
    relight.gbuffer_from_planes.  `radii` is None and `extra` holds tri_id, opacity_map and the material planes, and
    baked_occlusion for a TexturedMeshRasterizer; `occlusion` is mesh_planes' ("baked" and "both" need one).  The source
    owns the scratch planes of its result, which is valid until its next call."""
    replayable = False  # relight.ViewReplay is keyed on Gaussian tensors and asynchronous binning

    def __init__(self, gi: Dict, metallic: bool = False, occlusion: str = "ssao"):
        if occlusion not in OCCLUSION_MODES:
            raise ValueError("MeshGBuffer: occlusion is one of %s, got %r" % (", ".join(OCCLUSION_MODES), occlusion))
        self.gi, self.metallic, self.occlusion = gi, bool(metallic), occlusion
        self._scratch = relight.Scratch()

    @torch.no_grad()
    def __call__(self, cam: Dict, rast: MeshRasterizer) -> Dict:
        if not isinstance(rast, MeshRasterizer):
            raise TypeError("MeshGBuffer: the second argument is a MeshRasterizer")
        r = mesh_planes(rast, cam, self.gi, self.occlusion)
        b = relight.gbuffer_from_planes(r, r["viewmatrix"], self.metallic, self._scratch)
        b["extra"] = {k: r[k] for k in ("tri_id", "opacity_map", "albedo_map", "roughness_map", "metallic_map")}
        if "baked_occlusion" in r:
            b["extra"]["baked_occlusion"] = r["baked_occlusion"]
        return b


class MeshRelighter(relight.Relighter):
    """relight.Relighter(fused=True) on a mesh: rl(cam, rast, view_dirs, alpha_mask=None, albedo_ratio=None).  occlusion:
    mesh_planes' ("ssao", or "baked" / "both" over a TexturedMeshRasterizer); the same keyword on the other two."""

    def __init__(self, light, gi: Dict, metallic: bool = False, tone: bool = False, gamma: bool = False,
                 brdf_lut: Optional[torch.Tensor] = None, graphs: bool = False, occlusion: str = "ssao"):
        super().__init__(light, gi, 0, metallic=metallic, tone=tone, gamma=gamma, fused=True, brdf_lut=brdf_lut, graphs=graphs,
                         source=MeshGBuffer(gi, metallic, occlusion))


class MeshMultiRelighter(relight.MultiRelighter):
    """relight.MultiRelighter on a mesh: up to relight.MAX_LIGHTS lights over one G-buffer."""

    def __init__(self, lights, gi: Dict, metallic: bool = False, tone: bool = False, gamma: bool = False,
                 graphs: bool = False, brdf_lut: Optional[torch.Tensor] = None, occlusion: str = "ssao"):
        super().__init__(lights, gi, 0, metallic=metallic, tone=tone, gamma=gamma, graphs=graphs, brdf_lut=brdf_lut,
                         source=MeshGBuffer(gi, metallic, occlusion))


class MeshTurntableRelighter(relight.TurntableRelighter):
    """relight.TurntableRelighter on a mesh: any number of lights, the SSR march recorded once."""

    def __init__(self, lights, gi: Dict, metallic: bool = False, tone: bool = False, gamma: bool = False,
                 brdf_lut: Optional[torch.Tensor] = None, graphs: bool = False, occlusion: str = "ssao"):
        if graphs:
            raise ValueError("MeshTurntableRelighter replays no hipGraph: graphs=False only")
        super().__init__(lights, gi, 0, metallic=metallic, tone=tone, gamma=gamma, brdf_lut=brdf_lut,
                         source=MeshGBuffer(gi, metallic, occlusion))


# ---- ray-traced light per pixel: a G-buffer's covered pixels traced against a mesh (mesh.gather_points) ---------------------
RAYTRACED_MODES = ("replace", "multiply")
NORMAL_SPACES = ("world", "view")


def occluder_mesh(rast: MeshRasterizer) -> mesh_ops.Mesh:
    """The geometry a rasterizer holds as a mesh.Mesh on its device, for an occlusion-only RaytracedLight: vertices and faces
    as they are; the normals and materials a textured rasterizer lacks are zero (rays start from pixels, not vertices)."""
    rast._check()
    m = rast._mesh
    V = int(m["vertices"].shape[0])
    zero3, zero1 = torch.zeros((V, 3), device=rast.device), torch.zeros(V, device=rast.device)
    return mesh_ops.Mesh(m["vertices"], m["faces"], m.get("normals", zero3), m.get("albedo", zero3), m.get("roughness", zero1),
                         m.get("metallic", zero1))


@torch.no_grad()
def prepare_points(pos_view, normal, viewmatrix, mask, normal_space, dev):
    """RaytracedLight.prepare's transform on device `dev`; its text states the arithmetic."""
    if normal_space not in NORMAL_SPACES:
        raise ValueError("RaytracedLight: normal_space is one of %s, got %r" % (", ".join(NORMAL_SPACES), normal_space))
    if not (isinstance(pos_view, torch.Tensor) and isinstance(normal, torch.Tensor) and pos_view.dim() == 3
            and pos_view.shape[0] == 3 and normal.shape == pos_view.shape):
        raise ValueError("RaytracedLight: pos_view and normal are [3,H,W] tensors")
    _, H, W = pos_view.shape
    if not isinstance(mask, torch.Tensor) or mask.numel() != H * W:
        raise ValueError("RaytracedLight: mask is a tensor of %d x %d pixels" % (H, W))
    M = MeshRasterizer._viewmatrix(dict(viewmatrix=viewmatrix), dev).double()
    R = [[float(x) for x in row] for row in M[:3, :3].cpu().tolist()]
    t = [float(x) for x in M[3, :3].cpu().tolist()]
    p = pos_view.detach().to(dev).double().reshape(3, H * W)
    v = normal.detach().to(dev).double().reshape(3, H * W)
    d = [p[j] - t[j] for j in range(3)]
    points = torch.stack([(d[0] * R[i][0] + d[1] * R[i][1]) + d[2] * R[i][2] for i in range(3)], 1)
    if normal_space == "view":
        w = [-((v[0] * R[i][0] + v[1] * R[i][1]) + v[2] * R[i][2]) for i in range(3)]
    else:
        w = [v[0], v[1], v[2]]
    length = torch.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    normals = torch.stack([w[i] / length for i in range(3)], 1)
    return points.float().contiguous(), normals.float().contiguous(), (mask.detach().to(dev).reshape(H * W) != 0).to(torch.uint8)


@torch.no_grad()
def prepare_views(points, campos):
    """[N,3] float32: the unit vectors from `points` [N,3] float32 (prepare_points') towards the eye `campos` [3], the `views`
    of mesh.reflect_points and compose_reflections, on the points' device.  In float64 on the float32 inputs, elementwise
    and in this order:
        d_i = c_i - p_i;   v_i = d_i / sqrt((d_0 d_0 + d_1 d_1) + d_2 d_2)
    rounded to float32.  The sqrt is taken here, in torch on the host's side of the launch: the trace kernel has none.  A
    point at the eye or one that is not finite gives NaN: a no_view point if its mask is set."""
    if not (isinstance(points, torch.Tensor) and points.dim() == 2 and points.shape[1] == 3):
        raise ValueError("prepare_views: points is an [N,3] tensor")
    c = torch.as_tensor(campos, dtype=torch.float32).detach().reshape(-1).cpu().tolist()
    if len(c) != 3:
        raise ValueError("prepare_views: campos has three components")
    p = points.detach().double()
    d = [float(c[i]) - p[:, i] for i in range(3)]
    length = torch.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    return torch.stack([d[i] / length for i in range(3)], 1).float().contiguous()


@torch.no_grad()
def compose_reflections(normals, views, roughness, radiance, albedo=None, metallic=None, mask=None, visibility=None,
                        brdf_lut=None):
    """[N,3] float32: specular_rgb = radiance * (F0 * fg.x + fg.y), the specular half of pbr_shading with a supplied
    `radiance` [N,3] (mesh.reflect_points' specular) in the place of the lookup in the pre-filtered cube
    (gigs_reflect_compose; include/gigs_hip.h, "Ray-traced reflections per point", restates the shade's float32 lines):
    nov = clamp(n.v, 1e-4, 1), fg the bilinear, clamped lookup of `brdf_lut` (None: pbr.get_brdf_lut()) at (nov, roughness),
    F0 = (1 - m) 0.04 + albedo m, or 0.04 without `metallic` [N] (`albedo` [N,3] is then not needed).  normals, views [N,3]
    and roughness [N] are float32 on one device; a point with mask [N] (uint8 or bool) == 0 gets 0.  With `visibility` [N]
    the radiance is multiplied by it first: an external radiance -- a splat shade's cube lookup -- under traced specular
    occlusion."""
    what = "compose_reflections"
    if not isinstance(normals, torch.Tensor) or not normals.is_cuda:
        raise RuntimeError("%s: normals must be a CUDA/HIP tensor: gigs-hip has no CPU path" % what)
    dev, N = normals.device, int(normals.shape[0])

    def arr(t, name, shape, optional=False):
        if t is None and optional:
            return None
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise ValueError("%s: %s must be a %s float32 tensor on the normals' device" % (what, name, list(shape)))
        return t.detach().contiguous()

    normals, views = arr(normals, "normals", (N, 3)), arr(views, "views", (N, 3))
    roughness, radiance = arr(roughness, "roughness", (N,)), arr(radiance, "radiance", (N, 3))
    metallic, visibility = arr(metallic, "metallic", (N,), True), arr(visibility, "visibility", (N,), True)
    albedo = arr(albedo, "albedo", (N, 3), metallic is None)
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool)
                or tuple(mask.shape) != (N,)):
            raise ValueError("%s: mask must be a [%d] uint8 or bool tensor on the normals' device" % (what, N))
        mask = mask.detach().to(torch.uint8).contiguous()
    if brdf_lut is None:
        from pbr import get_brdf_lut
        brdf_lut = get_brdf_lut()
    lut = brdf_lut.detach().to(dev).float().contiguous()
    if lut.dim() < 3 or lut.shape[-1] != 2:
        raise ValueError("%s: brdf_lut is [..., h, w, 2], got %s" % (what, tuple(lut.shape)))
    out = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        gigs_lib.check(_lib.gigs_reflect_compose(N, _p(normals), _p(views), _p(albedo), _p(roughness), _p(metallic), _p(mask),
                                                 _p(radiance), _p(visibility), _p(lut), int(lut.shape[-2]), int(lut.shape[-3]),
                                                 _p(out), _stream()), "reflect_compose")
    return out


class RaytracedLight:
    """A mesh as the occluder and bounce surface of any view's pixels: the triangle grid is built once, and with a `cube`
    ([6,n,n,3] float32, mesh.sky_cube's) so is the vertex radiosity of the passes 0 .. bounces - 1 (mesh.trace_hemispheres with
    `light_rays` rays, mesh.gather_light); planes() then runs mesh.gather_points with `rays` rays per pixel.  mesh: what
    mesh_arrays takes.  ao_distance and bias default as mesh.bake_occlusion's max_distance and bias; the light rays have no
    distance limit.  Without a cube only the occlusion is traced.  close() / `with` as the rasterizers."""

    def __init__(self, mesh, rays: int = 64, ao_distance=None, bias=None, seed: int = 0, rotations: int = 16, cube=None,
                 bounces: int = 1, reflectance=None, light_rays: int = 256, device="cuda"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("RaytracedLight: the mesh must live on a CUDA/HIP device: gigs-hip has no CPU path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.bounces = int(bounces)
        if self.bounces < 0:
            raise ValueError("RaytracedLight: bounces must be >= 0, got %d" % self.bounces)
        self.rays, self.seed, self.rotations = int(rays), int(seed), int(rotations)
        mesh_ops._hemisphere_args("RaytracedLight", self.rays, self.rotations, None, ao_distance, bias)
        self.mesh = mesh if isinstance(mesh, mesh_ops.Mesh) and mesh.vertices.device == dev else device_mesh(mesh, dev)
        self.cube = None if cube is None else mesh_ops._check_cube(cube, "RaytracedLight").to(dev)
        with torch.cuda.device(dev):
            self.grid = mesh_ops.triangle_grid(self.mesh)
        if self.grid is not None:
            if ao_distance is None:
                ao_distance = 0.1 * (max(self.grid.dims) * self.grid.cell)
            if bias is None:
                bias = 1e-3 * float(ao_distance)
        self.ao_distance, self.bias = ao_distance, bias
        self.radiosity, self.bake_report = None, None  # [bounces, V, 3]: the radiosity of the vertex passes
        if self.cube is not None and self.bounces > 0 and self.grid is not None:
            hits, self.bake_report = mesh_ops.trace_hemispheres(self.mesh, int(light_rays), None, self.bias, self.seed, self.rotations,
                                                                grid=self.grid)
            _, self.radiosity, gathered = mesh_ops._gather_light(self.mesh, hits, self.cube, self.bounces - 1, reflectance)
            self.bake_report.update(gathered)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        self.mesh = self.grid = self.cube = self.radiosity = None

    def _check(self):
        if self.mesh is None:
            raise RuntimeError("RaytracedLight: closed")

    @torch.no_grad()
    def prepare(self, pos_view, normal, viewmatrix, mask, normal_space: str = "world"):
        """(points [H W,3], normals [H W,3] float32, mask [H W] uint8) on the device, row-major over the pixels, from the
        view-space positions pos_view [3,H,W], the normal plane [3,H,W] and the pixel mask [H,W] or [1,H,W] (non-zero:
        trace).  viewmatrix M [4,4] is the rasterizers' (p_view = p_world M[:3,:3] + M[3,:3]).  In float64 on the float32
        inputs, elementwise and in this order, R = M[:3,:3], t = M[3,:3], the rotation taken as orthonormal:
            d_j = p_view_j - t_j;   p_world_i = (d_0 R_i0 + d_1 R_i1) + d_2 R_i2
            normal_space "world": w = normal;  "view": the G-buffer's normals_view = -(n_world R), so
                                  w_i = -((v_0 R_i0 + v_1 R_i1) + v_2 R_i2)
            n_i = w_i / sqrt((w_0 w_0 + w_1 w_1) + w_2 w_2)
        and both are rounded to float32.  A zero normal gives NaN: a no_normal point if its mask is set."""
        self._check()
        return prepare_points(pos_view, normal, viewmatrix, mask, normal_space, self.device)

    @torch.no_grad()
    def planes(self, pos_view, normal, viewmatrix, mask, normal_space: str = "world", bounces=None, rays=None) -> Dict:
        """prepare(), then mesh.gather_points -> {occlusion [1,H,W] float32, hits [H,W] int32, irradiance, indirect [3,H,W]
        float32 or None (no cube), points, normals, mask (the prepared arrays), report}.  bounces (None: the constructor's)
        picks the vertex pass whose radiosity the front hits bring: irradiance is the light after that many bounces.  rays
        (None: the constructor's) as in reflections(): a converged trace of the same view for comparison."""
        points, normals, m = self.prepare(pos_view, normal, viewmatrix, mask, normal_space)
        _, H, W = pos_view.shape
        b = self.bounces if bounces is None else int(bounces)
        if b < 0 or b > self.bounces:
            raise ValueError("RaytracedLight: bounces must lie in [0, %d], got %d" % (self.bounces, b))
        radiosity = self.radiosity[b - 1] if (b > 0 and self.radiosity is not None) else None
        light, report = mesh_ops.gather_points(points, normals, self.mesh, self.cube, radiosity, self.rays if rays is None else int(rays),
                                               self.ao_distance, None,
                                               self.bias, self.seed, self.rotations, mask=m, grid=self.grid)
        report["bounces"] = b if self.cube is not None else None
        plane3 = lambda x: None if x is None else x.t().reshape(3, H, W).contiguous()  # noqa: E731
        return dict(occlusion=light.occlusion.reshape(1, H, W), hits=light.hits.reshape(H, W), irradiance=plane3(light.irradiance),
                    indirect=plane3(light.indirect), points=points, normals=normals, mask=m, report=report)

    @torch.no_grad()
    def shadows(self, pos_view, normal, viewmatrix, mask, lights, samples: int = 1, normal_space: str = "world"):
        """prepare(), then mesh.shadow_points of the analytic `lights` (analytic_lights.AnalyticLight) with the tracer's grid,
        bias, seed and rotations -> (visibility [L,H,W] float32, points, normals, mask: the prepared arrays, report)."""
        points, normals, m = self.prepare(pos_view, normal, viewmatrix, mask, normal_space)
        _, H, W = pos_view.shape
        visibility, _, report = mesh_ops.shadow_points(points, normals, self.mesh, lights, samples, self.rotations, self.bias, None,
                                                       self.seed, m, self.grid)
        return visibility.t().reshape(-1, H, W).contiguous(), points, normals, m, report

    @torch.no_grad()
    def reflections(self, pos_view, normal, roughness, viewmatrix, campos, mask, normal_space: str = "world", bounces=None,
                    rays=None, levels: int = 16, cube=None) -> Dict:
        """prepare() and prepare_views(points, campos), then mesh.reflect_points with the tracer's grid, bias, seed and rotations
        -> {specular, reflected [3,H,W] float32 or None (no cube), visibility [1,H,W] float32, valid, blocked [H,W] int32,
        points, normals, views, roughness, mask (the prepared arrays), report}.  roughness: the plane [1,H,W] or [H,W];
        campos [3]: the eye in world space.  rays (None: the constructor's) and levels size the table mesh.ggx_directions.
        cube (None: the tracer's) is the sky the escaping rays look up: a finer one than the diffuse gather's may be given,
        because a 32 x 32 sky is coarse for a glossy lobe; the front hits bring the radiosity of the tracer's own cube after
        `bounces` - 1 vertex passes (planes()' rule; None: the constructor's)."""
        points, normals, m = self.prepare(pos_view, normal, viewmatrix, mask, normal_space)
        _, H, W = pos_view.shape
        if not isinstance(roughness, torch.Tensor) or roughness.numel() != H * W:
            raise ValueError("RaytracedLight: roughness is a plane of %d x %d pixels" % (H, W))
        b = self.bounces if bounces is None else int(bounces)
        if b < 0 or b > self.bounces:
            raise ValueError("RaytracedLight: bounces must lie in [0, %d], got %d" % (self.bounces, b))
        sky = self.cube if cube is None else mesh_ops._check_cube(cube, "RaytracedLight").to(self.device)
        radiosity = self.radiosity[b - 1] if (b > 0 and self.radiosity is not None and sky is not None) else None
        views = prepare_views(points, campos)
        rough = roughness.detach().to(self.device).float().reshape(H * W).contiguous()
        got, report = mesh_ops.reflect_points(points, normals, views, rough, self.mesh, sky, radiosity, self.rays if rays is None else rays,
                                              levels, self.rotations, None, self.bias, self.seed, mask=m, grid=self.grid)
        report["bounces"] = b if sky is not None else None
        plane3 = lambda x: None if x is None else x.t().reshape(3, H, W).contiguous()  # noqa: E731
        return dict(specular=plane3(got.specular), reflected=plane3(got.reflected), visibility=got.visibility.reshape(1, H, W),
                    valid=got.valid.reshape(H, W), blocked=got.blocked.reshape(H, W), points=points, normals=normals, views=views,
                    roughness=rough, mask=m, report=report)

    DIFFUSE_PLANES = (("occlusion", 1), ("irradiance", 3), ("indirect", 3))
    GLOSSY_PLANES = (("specular", 3), ("reflected", 3), ("visibility", 1))

    def plane_distance(self):
        """The denoiser's default plane_distance: 0.1 x ao_distance, a hundredth of the grid's largest extent with the default
        ao_distance -- some pixels' spacing on a surface that fills the view, far below the gaps the tracer resolves.  None
        for an empty mesh (denoise.atrous then takes it from the points)."""
        return None if self.ao_distance is None or not float(self.ao_distance) > 0.0 else 0.1 * float(self.ao_distance)

    @torch.no_grad()
    def denoise(self, traced: Dict, iterations: int = denoise_ops.ITERATIONS, **kw) -> Dict:
        """The dict planes() or reflections() returned with its traced planes filtered by ONE denoise.atrous call over the
        prepared points, normals and mask it carries: occlusion, irradiance and indirect (groups [1, 3, 3]), or specular,
        reflected and visibility (groups [3, 3, 1]) with the prepared roughness as a further guide; the planes a tracer without
        a cube leaves None are left out.  The result is a copy with those planes replaced, <plane>_variance [1,H,W] added for
        each, and denoise_report.  kw: denoise.atrous's; plane_distance defaults to self.plane_distance()."""
        self._check()
        if not isinstance(traced, dict) or not ("occlusion" in traced or "specular" in traced):
            raise ValueError("RaytracedLight.denoise: takes the dict planes() or reflections() returned")
        glossy = "specular" in traced
        names = [(k, c) for k, c in (self.GLOSSY_PLANES if glossy else self.DIFFUSE_PLANES) if traced.get(k) is not None]
        H, W = (int(x) for x in traced[names[0][0]].shape[-2:])
        signal = torch.cat([traced[k].to(self.device).float().reshape(c, H, W) for k, c in names], 0)
        kw = dict(kw)
        kw.setdefault("plane_distance", self.plane_distance())
        if glossy:
            kw.setdefault("roughness", traced["roughness"])
        filtered, variance, report = denoise_ops.atrous(signal, traced["points"], traced["normals"], traced["mask"],
                                                        [c for _, c in names], iterations, **kw)
        out, c0 = dict(traced), 0
        for j, (k, c) in enumerate(names):
            out[k] = filtered[c0:c0 + c].reshape(traced[k].shape).contiguous()
            out[k + "_variance"] = variance[j:j + 1].contiguous()
            c0 += c
        out["denoise_report"] = dict(report, planes=[k for k, _ in names])
        return out


def denoise_iterations(what: str, n) -> int:
    """The denoise= keyword of the traced sources: 0 (off) .. denoise.MAX_ITERATIONS a-trous iterations."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 0 <= int(n) <= denoise_ops.MAX_ITERATIONS:
        raise ValueError("%s: denoise is 0 (off) or 1 to %d a-trous iterations, got %r" % (what, denoise_ops.MAX_ITERATIONS, n))
    return int(n)


class RaytracedGBuffer:
    """A G-buffer source around another (MeshGBuffer, relight.SplatGBuffer) whose `occlusion` plane is ray-traced against a
    RaytracedLight's mesh: source(cam, scene) calls inner(cam, scene), traces from its depth_pos, normals_view (normal_space
    "view") and mask_u8 with cam's viewmatrix, and puts the traced plane ("replace") or its product with the inner plane
    ("multiply") in its place, shape and dtype kept.  `extra` gains raytraced_occlusion, and raytraced_irradiance and
    raytraced_indirect when the tracer has a cube; `report` is the tracer's of the last view.  The relighters take it through
    source=; graphs=True raises there, because a traced view replays no hipGraph.  depth_pos comes from the FILTERED depth and
    lies off the mesh by up to the depth range of a pixel's 3x3 neighbourhood: give the tracer a `bias` above that, or the points
    under the surface see its back (the report's back_hits show it).  reflections=True also traces the view's glossy
    reflections (RaytracedLight.reflections from the same planes, the inner roughness_map and cam's campos): `extra` gains
    raytraced_specular, raytraced_reflected (with a cube) and raytraced_specular_visibility, `reflection_report` is that
    trace's report, and every other output is what it is without.  denoise=n > 0 filters the traced planes with n a-trous
    iterations (RaytracedLight.denoise) before they go into `occlusion` and `extra`; denoise_report and
    reflection_denoise_report are the filter's reports.  0, the default, launches nothing and changes no bit."""
    replayable = False

    def __init__(self, inner, tracer: RaytracedLight, occlusion: str = "replace", reflections: bool = False, denoise: int = 0):
        if occlusion not in RAYTRACED_MODES:
            raise ValueError("RaytracedGBuffer: occlusion is one of %s, got %r" % (", ".join(RAYTRACED_MODES), occlusion))
        if not isinstance(tracer, RaytracedLight):
            raise TypeError("RaytracedGBuffer: the tracer is a RaytracedLight")
        self.inner, self.tracer, self.occlusion = inner, tracer, occlusion
        self.metallic = inner.metallic
        self.reflections = bool(reflections)
        self.denoise = denoise_iterations("RaytracedGBuffer", denoise)
        self.report = self.reflection_report = self.denoise_report = self.reflection_denoise_report = None

    @torch.no_grad()
    def __call__(self, cam: Dict, scene) -> Dict:
        b = dict(self.inner(cam, scene))
        t = self.tracer.planes(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], normal_space="view")
        self.report = t["report"]
        if self.denoise:
            t = self.tracer.denoise(t, self.denoise)
            self.denoise_report = t["denoise_report"]
        inner = b["occlusion"]
        plane = t["occlusion"].to(inner.device)
        if self.occlusion == "multiply":
            plane = inner.reshape(plane.shape) * plane
        b["occlusion"] = plane.to(inner.dtype).reshape(inner.shape).contiguous()
        extra = dict(b.get("extra", {}), raytraced_occlusion=t["occlusion"])
        if t["irradiance"] is not None:
            extra["raytraced_irradiance"], extra["raytraced_indirect"] = t["irradiance"], t["indirect"]
        if self.reflections:
            r = self.tracer.reflections(b["depth_pos"], b["normals_view"], b["roughness_map"], cam["viewmatrix"], cam["campos"],
                                        b["mask_u8"], normal_space="view")
            self.reflection_report = r["report"]
            if self.denoise:
                r = self.tracer.denoise(r, self.denoise)
                self.reflection_denoise_report = r["denoise_report"]
            extra["raytraced_specular_visibility"] = r["visibility"]
            if r["specular"] is not None:
                extra["raytraced_specular"], extra["raytraced_reflected"] = r["specular"], r["reflected"]
        b["extra"] = extra
        return b
