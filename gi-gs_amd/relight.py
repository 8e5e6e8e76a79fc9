"""Relighting a trained scene under a new environment map: the per-view operator sequence of the reference's
relight.py, on the HIP library (BASELINE config C3: inference-only PBR + indirect).

    latlong_to_cubemap(latlong_map, res)      relight.py:92-111   (gigs_latlong_to_cubemap)
    make_light(hdri, res=256)                 relight.py:278-285  (CubemapLight + latlong_to_cubemap, eval mode)
    Relighter(...)(cam, gaussians, ...)       relight.py:153-251  per view: render(inference=True) -> pbr_shading ->
                                              Gaussian_SSR -> linear_to_srgb -> 3x3 median -> + direct -> * alpha_mask
                                              with light.build_mips() ONCE per run (:141), not per view

Two formulations with identical results (tests/test_gpu_relight.py): `fused=False` is the reference's op sequence
spelled with this package's drop-in operators (pipeline.render, pbr.pbr_shading, Gaussian_SSR, torch elementwise
ops); `fused=True` (default) runs the same arithmetic as five library launches after the rasterizer
(gigs_gbuffer_post, gigs_shade_fwd_ex in planar layout with the sRGB->linear epilogue, gigs_ssr,
gigs_stage2_loss_fwd for linear_to_srgb + median + sum) on the rasterizer's [C,H,W] planes.

The fused paths have two seams.  WHO MAKES THE G-BUFFER: a source, source(cam, scene) -> the dict of planes documented below
(SplatGBuffer for Gaussians, mesh_render.MeshGBuffer for a mesh; both end in gbuffer_from_planes).  WHAT IS DONE WITH IT:
a relighter's from_gbuffer(cam, b, view_dirs, ...); rl(cam, scene, ...) is rl.from_gbuffer(cam, rl.source(cam, scene), ...),
replayed from one hipGraph (ViewReplay) where graphs=True and the source allows it.

    MultiRelighter(lights, ...)               relight_all.bash's loop over target maps, one view at a time, at most 16 lights:
                                              the rasterizer, G-buffer post, SSAO and the SSR march run ONCE, then
                                              K-light launches (gigs_shade_fwd_multi, gigs_ssr_multi) and K finishes
    TurntableRelighter(lights, ...)           the same light loop under ANY number of lights (a turntable: N rotations of one
                                              map): the march runs once and records its hit list (gigs_ssr_hits), then every
                                              chunk of <= 16 lights is a shade, a gather at the recorded hits
                                              (gigs_ssr_apply_multi) and the per-light finish; eager only
    RelightEvaluator(light_names).add(...)    relight_eval.py without the file I/O: per light the PSNR / SSIM of the
                                              8-bit-quantised prediction against its ground truth, kept on the device
    rotation_about / yaw_rotations / rotated_lights / rotate_light   lights turned in their own frame: the BASE is resampled
                                              under the rotation and then pre-filtered like any other light (DESIGN.md,
                                              "Turntables": the pre-filters are not rotation-covariant)

Reference quirks kept on purpose, by every relighter alike: the `metallic` branches for F0 are swapped
(relight.py:236-240, fused_f0):
with metallic=True the shade uses the metallic map but SSR receives F0 = 0.04 and a zero metallic plane; with
metallic=False (`metallic` is the Python bool) SSR receives F0 = (1 - False) * 0.04 + albedo * metallic_map.  The
per-channel albedo ratio read from albedo_ratio.json (:203-220) scales the shade's albedo only.  Image I/O
(read_hdr, save_image, the JSON) is relight_scene.py's, on top of image_writer.py.  RelightEvaluator computes LPIPS when given an `lpips.LPIPS`
(this package's drop-in, gigs_lpips_vgg) as `lpips=`, as in evaluate.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

import gigs_lib
import pipeline
from diff_gaussian_rasterization import Gaussian_SSR, _C as _ops, _gi_scratch, filters
from pbr import CubemapLight, get_brdf_lut, pbr_shading
from pbr.shade import _ptr_array

_lib = gigs_lib.lib()



def _complete(light) -> None:
    """A light whose last build_mips() left the fine levels to a stepper's sparse fill holds one view's texels only."""
    if getattr(light, "fine_levels_partial", False):
        raise RuntimeError("this light's fine GGX levels were filtered for one training view only "
                           "(build_mips(sparse=...)): call light.build_mips() before relighting with it")


def latlong_to_cubemap(latlong_map: torch.Tensor, res: List[int]) -> torch.Tensor:
    """relight.py:92-111: [H, W, C] equirectangular map -> [6, res[0], res[1], C] cubemap."""
    if not latlong_map.is_cuda:
        raise RuntimeError("latlong_map must be a CUDA/HIP tensor: gigs-hip has no CPU path")
    lat = latlong_map.contiguous().float()
    Hl, Wl, Cn = lat.shape
    cube = torch.empty((6, int(res[0]), int(res[1]), Cn), dtype=torch.float32, device=lat.device)
    with torch.cuda.device(lat.device):
        gigs_lib.check(_lib.gigs_latlong_to_cubemap(int(res[0]), int(res[1]), Hl, Wl, Cn, lat.data_ptr(), cube.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "latlong_to_cubemap")
    return cube


def make_light(hdri: torch.Tensor, res: int = 256) -> CubemapLight:
    """relight.py:278-285."""
    light = CubemapLight(base_res=res, device=hdri.device)
    light.base.data = latlong_to_cubemap(hdri, [res, res])
    light.eval()
    return light


# ---- rotated lights ---------------------------------------------------------------------------------------------------
# Rotations live in the light's own frame: the cube / latitude-longitude frame of relight.py:75-111, +y towards tv = 0 (the
# shade's swizzle (-n.y, n.z, -n.x) maps world +z to it: the up axis of a Blender scene).  R is a right-handed 3x3 rotation
# and the rotated environment is env_R(d) = env(R^T d).  Anchor: torch.roll(latlong, +s, dims=1) is the rotation about +y by
# -2 pi s / W (tu = atan2(x, -z) / 2 pi + 0.5 grows with the angle of a right-handed turn about +y).
MAX_ROTATIONS = 1024  # gigs_latlong_to_cubemap_rot


def rotation_about(axis: Sequence[float], angle: float) -> torch.Tensor:
    """The right-handed rotation by `angle` (radians) about `axis` as a [3,3] float64 tensor (Rodrigues).  Entries within
    1e-15 of an integer are that integer, so whole quarter turns about a coordinate axis are exact signed permutations and
    angle 0 is exactly the identity."""
    a = torch.as_tensor(axis, dtype=torch.float64).reshape(3)
    n = float(a.norm())
    if not n > 0.0:
        raise ValueError("rotation_about: the axis has no direction")
    x, y, z = (a / n).tolist()
    k = torch.tensor([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]], dtype=torch.float64)
    import math
    r = torch.eye(3, dtype=torch.float64) + math.sin(angle) * k + (1.0 - math.cos(angle)) * (k @ k)
    return torch.where((r - r.round()).abs() < 1e-15, r.round() + 0.0, r)


def yaw_rotations(n: int, axis: Sequence[float] = (0.0, 1.0, 0.0)) -> torch.Tensor:
    """[n,3,3]: n equal right-handed steps of a full turn about `axis` (default +y, the light's up), the identity first."""
    import math
    if n < 1:
        raise ValueError("yaw_rotations: n must be at least 1")
    return torch.stack([rotation_about(axis, 2.0 * math.pi * k / n) for k in range(n)])


def _rotations_f32(rotations, dev) -> torch.Tensor:
    r = torch.as_tensor(rotations).detach().to(torch.float64).reshape(-1, 3, 3)
    if r.shape[0] < 1:
        raise ValueError("no rotation given")
    return r.to(device=dev, dtype=torch.float32).contiguous()


def latlong_to_cubemap_rot(latlong_map: torch.Tensor, res: List[int], rotations) -> torch.Tensor:
    """latlong_to_cubemap under each of `rotations` [n,3,3] in one launch: [n, 6, res[0], res[1], C].  The slice of an exact
    identity equals latlong_to_cubemap bit for bit."""
    if not latlong_map.is_cuda:
        raise RuntimeError("latlong_map must be a CUDA/HIP tensor: gigs-hip has no CPU path")
    lat = latlong_map.contiguous().float()
    rot = _rotations_f32(rotations, lat.device)
    n = int(rot.shape[0])
    if n > MAX_ROTATIONS:
        raise ValueError(f"latlong_to_cubemap_rot: at most {MAX_ROTATIONS} rotations per call, got {n}")
    Hl, Wl, Cn = lat.shape
    cube = torch.empty((n, 6, int(res[0]), int(res[1]), Cn), dtype=torch.float32, device=lat.device)
    with torch.cuda.device(lat.device):
        gigs_lib.check(_lib.gigs_latlong_to_cubemap_rot(int(res[0]), int(res[1]), Hl, Wl, Cn, lat.data_ptr(), n, rot.data_ptr(),
                                                        cube.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "latlong_to_cubemap_rot")
    return cube


def _light_of(base: torch.Tensor) -> CubemapLight:
    light = CubemapLight(base_res=int(base.shape[1]), device=base.device)
    light.base.data = base.contiguous()
    light.eval()
    return light


def rotated_lights(hdri: torch.Tensor, rotations, res: int = 256) -> List[CubemapLight]:
    """make_light for every rotation of a latitude-longitude map: what relight.py would build if it were handed the
    rotated .hdr (the base cubemap sampled at R^T dir; the mips are built from it, unchanged, by whoever uses the light)."""
    rot = torch.as_tensor(rotations).reshape(-1, 3, 3)
    lights: List[CubemapLight] = []
    for first in range(0, int(rot.shape[0]), MAX_ROTATIONS):
        cubes = latlong_to_cubemap_rot(hdri, [res, res], rot[first:first + MAX_ROTATIONS])
        lights.extend(_light_of(c) for c in cubes)
    return lights


def cube_texel_dirs(res: int, dev) -> torch.Tensor:
    """[6,res,res,3]: the unnormalised texel-centre directions of a cubemap (relight.py:75-89 over linspace(-1 + 1/res, ..))."""
    lin = torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, device=dev)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    one = torch.ones_like(gx)
    faces = ((one, -gy, -gx), (-one, -gy, gx), (gx, one, gy), (gx, -one, -gy), (gx, -gy, one), (-gx, -gy, -one))
    return torch.stack([torch.stack(f, dim=-1) for f in faces])


@torch.no_grad()
def rotate_light(light: CubemapLight, rotations) -> List[CubemapLight]:
    """A cube light (the trained light of a checkpoint) under each rotation: base_R = the cube lookup of light.base at R^T dir
    of the texel-centre directions (pbr.texture.cube_texture's lookup with its texel coordinates formed in double,
    cube_texture_precise: the float lookup's coordinate rounding grows with the resolution and would be written into every
    texel).  This is a bilinear cube resample, so it LOW-PASSES the base (every rotation that is not a cube symmetry blurs it
    by up to a texel, and rotating twice blurs twice): rotate the original light by the composed rotation, and prefer
    rotated_lights when the latitude-longitude source exists."""
    from pbr.texture import cube_texture_precise
    base = light.base.detach()
    dirs = cube_texel_dirs(int(base.shape[1]), base.device)
    out = []
    for r in _rotations_f32(rotations, base.device):
        out.append(_light_of(cube_texture_precise(base, dirs @ r)))  # row vector times R = R^T dir
    return out


# ---- the G-buffer ---------------------------------------------------------------------------------------------------------
# A G-buffer is a dict of planes on one device, made by a source (SplatGBuffer here, mesh_render.MeshGBuffer) and read, never
# written, by everything behind it.  [C,H,W] float32 unless noted:
#
#     radii          [P] int32, the Gaussians' screen radii, or None (a mesh)        the result
#     depth_map      [1,H,W]                                                        the result
#     occlusion      [1,H,W] SSAO                                                   shade; the result
#     albedo_map     [3,H,W]                                                        shade (times the albedo ratio), SSR
#     roughness_map  [1,H,W]                                                        shade, SSR, finish
#     metallic_map   [1,H,W]                                                        shade (metallic=True), fused_f0
#     depth_pos      [3,H,W] view-space positions from the filtered depth           SSR
#     normals_view   [3,H,W] the shading normal, gigs_gbuffer_post's                shade; the result's normal_map
#     onv            [3,H,W] the view-space normal the march reflects about         SSR
#     mask_u8        [H,W] uint8, pixels with a normal                              shade; the result's normal_mask
#     mask_f         [1,H,W] the same as floats                                     finish
#     F0             [3,H,W] fused_f0's                                             SSR
#     metallic_in    [1,H,W] fused_f0's: the metallic plane SSR receives            SSR, finish
#     extra          {name: plane} copied into every relighter's result unchanged: empty for splats; tri_id, opacity_map,
#                    albedo_map, roughness_map and metallic_map for a mesh
class Scratch(dict):
    """Named planes reused from view to view: scratch(name, shape, dtype, dev) allocates on the first use and when the shape
    or the device changed."""

    def __call__(self, name, shape, dtype, dev):
        t = self.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.device != dev:
            t = self[name] = torch.empty(shape, dtype=dtype, device=dev)
        return t


def fused_f0(albedo_map, roughness_map, metallic_map, metallic: bool):
    """relight.py:236-240 as the fused paths form it -> (F0, metallic_in).  The branches are the reference's, swapped as they
    are there: metallic=True gives F0 = 0.04 and a zero metallic plane."""
    if metallic:
        return torch.full_like(albedo_map, 0.04), torch.zeros_like(roughness_map)
    return torch.addcmul(torch.full_like(albedo_map, (1.0 - float(metallic)) * 0.04), albedo_map, metallic_map), metallic_map


def gbuffer_from_planes(planes: Dict, viewmatrix: torch.Tensor, metallic: bool, scratch: Scratch) -> Dict:
    """The G-buffer of a rasterizer's planes (by mesh_render.mesh_planes' names: depth_map, normal_map, occlusion_map,
    albedo_map, roughness_map, metallic_map, out_normal_view, depth_pos, and radii where there are any): gigs_gbuffer_post into
    `scratch`'s planes, then fused_f0.  viewmatrix: [4,4] float32, contiguous, on the planes' device."""
    albedo_map, roughness_map, metallic_map = planes["albedo_map"], planes["roughness_map"], planes["metallic_map"]
    if not albedo_map.is_cuda:
        raise RuntimeError("gbuffer_from_planes needs CUDA/HIP tensors: gigs-hip has no CPU path")
    dev = albedo_map.device
    _, H, W = albedo_map.shape
    normals_view, onv = scratch("normals_view", (3, H, W), torch.float32, dev), scratch("onv", (3, H, W), torch.float32, dev)
    mask_u8, mask_f = scratch("mask_u8", (H, W), torch.uint8, dev), scratch("mask_f", (1, H, W), torch.float32, dev)
    with torch.cuda.device(dev):
        gigs_lib.check(_lib.gigs_gbuffer_post(H, W, planes["normal_map"].data_ptr(), planes["out_normal_view"].data_ptr(),
                                              viewmatrix.data_ptr(), normals_view.data_ptr(), mask_u8.data_ptr(),
                                              mask_f.data_ptr(), onv.data_ptr(), torch.cuda.current_stream().cuda_stream),
                       "gbuffer_post")
        F0, metallic_in = fused_f0(albedo_map, roughness_map, metallic_map, metallic)
    return dict(radii=planes.get("radii"), depth_map=planes["depth_map"], occlusion=planes["occlusion_map"],
                albedo_map=albedo_map, roughness_map=roughness_map, metallic_map=metallic_map, depth_pos=planes["depth_pos"],
                normals_view=normals_view, onv=onv, mask_u8=mask_u8, mask_f=mask_f, F0=F0, metallic_in=metallic_in, extra={})


class SplatGBuffer:
    """The G-buffer of Gaussians: source(cam, g) runs the rasterizer (inference, derived normals, SSAO) and
    gbuffer_from_planes.  The source owns the scratch planes of its result, which is valid until its next call."""
    replayable = True  # a view over it can be captured into a hipGraph (ViewReplay, keyed on the Gaussian tensors)

    def __init__(self, gi: Dict, sh_degree: int, metallic: bool = False):
        self.gi, self.sh_degree, self.metallic = gi, sh_degree, bool(metallic)
        self._scratch = Scratch()

    @torch.no_grad()
    def __call__(self, cam: Dict, g: Dict[str, torch.Tensor]) -> Dict:
        background = torch.zeros(3, device=g["means3D"].device)
        (out, _, st) = pipeline.rasterize(cam, g, self.sh_degree, background, self.gi, inference=True, derive_normal=True)
        (_, radii, _, depth_map, _, normal_map, occlusion, albedo_map, roughness_map, metallic_map, out_normal_view,
         depth_pos) = out
        planes = dict(radii=radii, depth_map=depth_map, normal_map=normal_map, occlusion_map=occlusion, albedo_map=albedo_map,
                      roughness_map=roughness_map, metallic_map=metallic_map, out_normal_view=out_normal_view,
                      depth_pos=depth_pos)
        return gbuffer_from_planes(planes, st.viewmatrix.contiguous().float(), self.metallic, self._scratch)


class ViewReplay:
    """A whole view of Gaussians replayed from one hipGraph under asynchronous binning; its owner closes it."""

    def __init__(self, sh_degree: int, who: str):
        self.sh_degree, self.who = sh_degree, who
        self._graph = self._key = self._bin = None
        self._capacity = 0

    def __call__(self, cam, g, inputs, core, names, key_extra=None, on_capture=None):
        """Replay the view graph of core(cam, *inputs) -> tuple named `names`, capturing it first (under asynchronous
        binning) when the image, the field of view, the Gaussian tensors or key_extra changed; the camera pose and
        `inputs` are the graph's inputs, and whatever else core needs (the Gaussians) it captures itself.  on_capture() runs
        after every capture (the warm-up runs are real runs)."""
        from diff_gaussian_rasterization import AsyncBinning, BinningOverflow
        key = (pipeline.camera_model(cam), tuple(sorted((k, v.data_ptr()) for k, v in g.items())), key_extra)
        for _ in range(4):
            if self._graph is None or self._key != key:
                if self._capacity <= 0:
                    self._capacity = pipeline.first_capacity(cam, g, self.sh_degree, inference=True)
                self._bin = AsyncBinning(self._capacity, g["means3D"].device)
                scalars = {k: v for k, v in cam.items() if not isinstance(v, torch.Tensor)}

                def pose_core(viewmatrix, projmatrix, campos, *rest):
                    return core(dict(scalars, viewmatrix=viewmatrix, projmatrix=projmatrix, campos=campos), *rest)

                with self._bin:
                    self._graph = pipeline._graphed_inference(pose_core, (cam["viewmatrix"], cam["projmatrix"],
                                                                          cam["campos"], *inputs))
                self._key = key
                if on_capture is not None:
                    on_capture()
            out = dict(zip(names, self._graph(cam["viewmatrix"], cam["projmatrix"], cam["campos"], *inputs)))
            self._bin.snapshot()
            try:
                out["num_rendered"] = self._bin.check()
                return out
            except BinningOverflow as ex:
                self._capacity = pipeline.grown_capacity(ex.needed)
                self.close()
        raise RuntimeError(f"{self.who}: the binning capacity kept overflowing")

    def close(self) -> None:
        """Release the view graph with the device idle before and after (see pipeline.WholeStepGraph._drop_graphs)."""
        if self._graph is not None:
            torch.cuda.synchronize()
            self._graph = self._key = None
            torch.cuda.synchronize()


def _gi_args(cam: Dict, gi: Dict):
    """(W, H, fx, fy, radius, bias, thick, delta, step, start): the screen-space march's arguments."""
    H, W = cam["image_height"], cam["image_width"]
    return (W, H, float(W / (2.0 * cam["tanfovx"])), float(H / (2.0 * cam["tanfovy"])), float(gi["radius"]),
            float(gi["bias"]), float(gi["thick"]), float(gi["delta"]), int(gi["step"]), int(gi["start"]))


def _p(t):
    return None if t is None else t.data_ptr()


def shade_ssr(light: CubemapLight, brdf_lut, gi: Dict, metallic: bool, tone: bool, gamma: bool, cam: Dict, view_dirs, b: Dict,
              albedo_shade, scratch: Scratch, parts: bool = False):
    """The launches behind a G-buffer `b` under one light: shade (planar, with the sRGB->linear epilogue) of albedo_shade, SSR
    with b's F0 / metallic_in, then render_rgb = render_direct + median3x3(linear_to_srgb(IRR)) -> (render_direct, IRR,
    render_rgb).  Of `b` it reads the planes that the table above gives to shade, SSR and finish, so
    evaluate.NovelViewEvaluator hands it its own (the pad_normal post, render.py's F0 branch).  parts=True also has the shade
    write pbr_shading's diffuse_rgb and specular_rgb [3,H,W] and returns them behind the three planes."""
    albedo_map, roughness_map = b["albedo_map"], b["roughness_map"]
    dev = albedo_map.device
    H, W = cam["image_height"], cam["image_width"]
    render_direct, linear_rgb = torch.empty((3, H, W), device=dev), scratch("linear_rgb", (3, H, W), torch.float32, dev)
    render_rgb = torch.empty((3, H, W), device=dev)
    acc, loss = scratch("acc", (4 + 4 * 256,), torch.float32, dev), scratch("loss", (1,), torch.float32, dev)
    diffuse_rgb, specular_rgb = (torch.empty((3, H, W), device=dev) for _ in range(2)) if parts else (None, None)
    _complete(light)
    spec = [s.contiguous() for s in light.specular]
    spec_ptr = _ptr_array(spec)
    spec_res = (C.c_int * len(spec))(*[int(s.shape[1]) for s in spec])
    lut = brdf_lut
    ext = gigs_lib.ShadeExt(planar=1, rough_scale=1.0, rough_bias=0.0, out_linear=_p(linear_rgb))
    vd = view_dirs.contiguous().float()
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream
        gigs_lib.check(_lib.gigs_shade_fwd_ex(
            gigs_lib.ctx_ptr(), H, W, _p(b["normals_view"]), _p(vd), _p(albedo_shade), _p(roughness_map), _p(b["mask_u8"]),
            _p(b["occlusion"]), _p(b["metallic_map"]) if metallic else None, None, _p(light.diffuse), int(light.diffuse.shape[1]),
            len(spec), spec_ptr, spec_res, _p(lut), int(lut.shape[-2]), int(lut.shape[-3]), int(tone), int(gamma),
            _p(render_direct), _p(diffuse_rgb), _p(specular_rgb), None, C.addressof(ext), s), "shade_fwd_ex")
        IRR, _ = _ops.SSR(W, H, W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"]), gi["radius"], gi["bias"],
                          gi["thick"], gi["delta"], gi["step"], gi["start"], b["onv"], b["depth_pos"], linear_rgb, albedo_map,
                          roughness_map, b["metallic_in"], b["F0"])
        # render_rgb = render_direct + median3x3(linear_to_srgb(IRR)); the loss this entry point also forms is unused
        gigs_lib.check(_lib.gigs_stage2_loss_fwd(H, W, _p(render_direct), _p(IRR), _p(render_direct), _p(b["mask_f"]),
                                                 _p(roughness_map), _p(b["metallic_in"]), _p(render_rgb), _p(acc), _p(loss), s),
                       "stage2_loss_fwd")
    if parts:
        return render_direct, IRR, render_rgb, diffuse_rgb, specular_rgb
    return render_direct, IRR, render_rgb


MAX_LIGHTS = 16  # GIGS_MAX_LIGHTS (include/gigs_hip.h)
RESULT_NAMES = ("render_rgb", "render_direct", "IRR", "occlusion", "depth_map", "normal_map", "normal_mask", "radii")


def _albedo_shade(albedo_map, albedo_ratio):
    """relight.py:203-220: the albedo ratio scales the shade's albedo only."""
    if albedo_ratio is None:
        return albedo_map
    return albedo_map * torch.as_tensor(albedo_ratio, dtype=torch.float32, device=albedo_map.device)[:, None, None]


def _result(b: Dict, render_rgb, render_direct, IRR, alpha_mask) -> Dict:
    """What every relighter returns for the G-buffer `b`: RESULT_NAMES and b's extra planes."""
    if alpha_mask is not None:
        render_rgb = render_rgb * alpha_mask
    return dict(render_rgb=render_rgb, render_direct=render_direct, IRR=IRR, occlusion=b["occlusion"],
                depth_map=b["depth_map"], normal_map=b["normals_view"], normal_mask=b["mask_u8"].bool()[None],
                radii=b["radii"], **b.get("extra", {}))


def _check_lights(who: str, lights) -> None:
    res = {tuple(l.base.shape) for l in lights}
    if len(res) != 1:
        raise ValueError(f"{who}: the lights differ in base resolution: {sorted(res)}")


def _build_lights(who: str, lights) -> None:
    with torch.no_grad():
        for light in lights:
            light.build_mips()  # relight.py:141: once per run and light
    levels = {tuple(int(s.shape[1]) for s in l.specular) for l in lights}
    if len(levels) != 1 or len({int(l.diffuse.shape[1]) for l in lights}) != 1:
        raise ValueError(f"{who}: the lights' mip chains differ in level count or resolution")


class _Relighter:
    """What the relighters share: the shading settings, a G-buffer source (SplatGBuffer unless one is given), scratch planes
    of their own and a ViewReplay.  rl(cam, scene, ...) is rl.from_gbuffer(cam, rl.source(cam, scene), ...), replayed from one
    hipGraph with graphs=True; a subclass says in from_gbuffer what is done with a G-buffer."""

    def __init__(self, who, lights, gi, sh_degree, metallic, tone, gamma, brdf_lut, graphs, source):
        _check_lights(who, lights)
        self.gi, self.sh_degree, self.metallic = gi, sh_degree, bool(metallic)
        self.tone, self.gamma = bool(tone), bool(gamma)
        self.source = SplatGBuffer(gi, sh_degree, metallic) if source is None else source
        if self.source.metallic != self.metallic:
            raise ValueError(f"{who}: the source forms F0 for metallic={self.source.metallic}")
        if graphs and not self.source.replayable:
            raise ValueError(f"{who}: a view over {type(self.source).__name__} replays no hipGraph (the replay is keyed on "
                             "Gaussian tensors): graphs=False only")
        self.graphs = bool(graphs)
        self.brdf_lut = (brdf_lut if brdf_lut is not None else get_brdf_lut()).to(lights[0].base.device)
        self._scratch = Scratch()
        self._view = ViewReplay(sh_degree, who)
        _build_lights(who, lights)

    def __call__(self, cam: Dict, scene, view_dirs: torch.Tensor, alpha_mask: Optional[torch.Tensor] = None,
                 albedo_ratio: Optional[Sequence[float]] = None) -> Dict:
        """`scene` is what the source takes: the Gaussians' tensors, or a mesh_render.MeshRasterizer.  The source and
        from_gbuffer run without autograd on their own."""
        if self.graphs:
            try:
                def core(c, vd):  # the graph's inputs are the pose and the view directions; the scene is baked in
                    o = self.from_gbuffer(c, self.source(c, scene), vd, None, albedo_ratio)
                    return tuple(o[n] for n in RESULT_NAMES)

                out = self._view(cam, scene, (view_dirs,), core, RESULT_NAMES,
                                 None if albedo_ratio is None else tuple(albedo_ratio))
                if alpha_mask is not None:
                    out["render_rgb"] = out["render_rgb"] * alpha_mask
                return out
            except pipeline.DenseScene:
                self.graphs = False
        return self.from_gbuffer(cam, self.source(cam, scene), view_dirs, alpha_mask, albedo_ratio)

    def close(self) -> None:
        self._view.close()


class Relighter(_Relighter):
    """render_set (relight.py:113-251) without the file I/O: build_mips once, then one call per view."""

    def __init__(self, light: CubemapLight, gi: Dict, sh_degree: int, metallic: bool = False, tone: bool = False,
                 gamma: bool = False, fused: bool = True, pad_normal: bool = False, brdf_lut: Optional[torch.Tensor] = None,
                 graphs: bool = False, source=None):
        """graphs=True (with fused): the whole view -- rasterizer under asynchronous binning, filters, SSAO, shade, SSR,
        sRGB / median / sum -- is captured once into ONE hipGraph and replayed per view (camera pose and view
        directions are its inputs; image size, field of view, GI settings and the Gaussian tensors are baked in).  The
        tensors it returns are the graph's static outputs: consume them before the next call."""
        self.light = light
        self.fused, self.pad_normal = bool(fused) and not pad_normal, bool(pad_normal)
        super().__init__("Relighter", [light], gi, sh_degree, metallic, tone, gamma, brdf_lut, bool(graphs) and self.fused,
                         source)

    def __call__(self, cam: Dict, scene, view_dirs: torch.Tensor, alpha_mask: Optional[torch.Tensor] = None,
                 albedo_ratio: Optional[Sequence[float]] = None) -> Dict:
        if not self.fused:
            return self._unfused(cam, scene, view_dirs, alpha_mask, albedo_ratio)
        return super().__call__(cam, scene, view_dirs, alpha_mask, albedo_ratio)

    # -- the reference's op sequence, operator by operator ------------------------------------------------------
    @torch.no_grad()
    def _unfused(self, cam, g, view_dirs, alpha_mask, albedo_ratio):
        dev = g["means3D"].device
        gi = self.gi
        background = torch.zeros(3, device=dev)
        r = pipeline.render(cam, g, self.sh_degree, background, gi, inference=True, derive_normal=True,
                            pad_normal=self.pad_normal)
        H, W = cam["image_height"], cam["image_width"]
        normal_mask = r["normal_mask"]
        albedo_map, roughness_map, metallic_map = r["albedo_map"], r["roughness_map"], r["metallic_map"]
        ratio = torch.ones(3, device=dev) if albedo_ratio is None else torch.as_tensor(albedo_ratio, dtype=torch.float32, device=dev)
        res = pbr_shading(light=self.light, normals=r["normal_map"].permute(1, 2, 0), view_dirs=view_dirs,
                          mask=normal_mask.permute(1, 2, 0), albedo=(albedo_map * ratio[:, None, None]).permute(1, 2, 0),
                          roughness=roughness_map.permute(1, 2, 0),
                          metallic=metallic_map.permute(1, 2, 0) if self.metallic else None, tone=self.tone,
                          occlusion=r["occlusion_map"].permute(1, 2, 0), gamma=self.gamma, brdf_lut=self.brdf_lut)
        render_direct = res["render_rgb"].permute(2, 0, 1)
        render_direct = torch.where(normal_mask, render_direct, background[:, None, None])
        ssr = Gaussian_SSR(cam["tanfovx"], cam["tanfovy"], W, H, gi["radius"], gi["bias"], gi["thick"], gi["delta"],
                           gi["step"], gi["start"])
        if self.metallic:  # relight.py:236-240, as written: the reference's own spelling, which rounds unlike fused_f0's
            F0 = torch.ones_like(albedo_map) * 0.04
            metallic_in = torch.zeros_like(roughness_map)
        else:
            F0 = (1.0 - float(self.metallic)) * 0.04 + albedo_map * metallic_map
            metallic_in = metallic_map
        linear_rgb = pipeline.srgb_to_linear(render_direct)
        IRR, _ = ssr(r["out_normal_view"], r["depth_pos"], linear_rgb, albedo_map, roughness_map, metallic_in, F0)
        IRR_s = filters.median_blur(pipeline.linear_to_srgb(IRR)[None, ...], (3, 3))[0]
        render_rgb = render_direct + IRR_s
        if alpha_mask is not None:
            render_rgb = render_rgb * alpha_mask
        return dict(render_rgb=render_rgb, render_direct=render_direct, IRR=IRR, occlusion=r["occlusion_map"],
                    depth_map=r["depth_map"], normal_map=r["normal_map"], normal_mask=normal_mask, radii=r["radii"])

    # -- the same arithmetic as five launches behind the rasterizer ----------------------------------------------
    @torch.no_grad()
    def from_gbuffer(self, cam: Dict, b: Dict, view_dirs: torch.Tensor, alpha_mask: Optional[torch.Tensor] = None,
                     albedo_ratio: Optional[Sequence[float]] = None) -> Dict:
        """Everything after the G-buffer `b` (a source's), which it reads and leaves as it is."""
        render_direct, IRR, render_rgb = shade_ssr(self.light, self.brdf_lut, self.gi, self.metallic, self.tone, self.gamma,
                                                   cam, view_dirs, b, _albedo_shade(b["albedo_map"], albedo_ratio),
                                                   self._scratch)
        return _result(b, render_rgb, render_direct, IRR, alpha_mask)


class _LightsRelighter(_Relighter):
    """One view under several lights of equal base resolution: the rasterizer, G-buffer post, SSAO and the SSR march do not
    depend on the light.  from_gbuffer runs every chunk of up to MAX_LIGHTS lights as one gigs_shade_fwd_multi (the K lights
    sampled at the same cube taps), one gather of the chunk's radiance -- gigs_ssr_apply_multi at the hits of a march recorded
    once per view, or gigs_ssr_multi, which marches itself -- and the finish render_rgb = render_direct +
    median3x3(linear_to_srgb(IRR)) per light.  Light k's outputs equal Relighter(lights[k], fused=True)'s bit for bit, with
    the same reference quirks (module docstring).  render_rgb, render_direct and IRR are [K,3,H,W]; the light-independent
    planes are returned once.  `records` (the subclass's) says whether the march is recorded."""
    records = False

    def __init__(self, who, lights, gi, sh_degree, metallic, tone, gamma, brdf_lut, graphs, source):
        super().__init__(who, lights, gi, sh_degree, metallic, tone, gamma, brdf_lut, graphs, source)
        self.lights = lights
        self._entries = None  # the hit list's {hit pixel, ray} pairs, grown on demand
        self.last_hits = None  # hits of the last view's list, None where it took the march

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self) -> None:
        self._entries = None
        self._scratch.clear()
        super().close()

    def _record_hits(self, b, a, scratch, s):
        """The march as a recording -> (offsets, entries) of a complete list, or None where there is none to be had."""
        if gigs_lib.current().option("gi_march") != 4 or not int(self.gi["start"]) < int(self.gi["step"]):
            return None
        dev = b["albedo_map"].device
        W, H = a[:2]
        n = H * W
        counts = self._scratch("hit_counts", (4 * n,), torch.int32, dev)
        offsets = self._scratch("hit_offsets", (4 * n + 1,), torch.int32, dev)
        color, abd = (self._scratch(name, (3, H, W), torch.float32, dev) for name in ("hit_color", "hit_abd"))
        # which pixel a ray hits does not depend on the radiance: any plane serves the recording passes, their outputs are unused
        planes = (_p(b["onv"]), _p(b["depth_pos"]), _p(b["albedo_map"]), _p(b["albedo_map"]), _p(b["roughness_map"]),
                  _p(b["metallic_in"]), _p(b["F0"]), _p(color), _p(abd))
        if _lib.gigs_ssr_hits(gigs_lib.ctx_ptr(), *a, *planes, 1, _p(counts), None, None, 0, _p(scratch), s) != 0:
            return None  # a march without a hit list (more steps than the projective march's table holds)
        offsets[:1].zero_()
        torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
        total = int(offsets[-1])  # the one read-back
        if total < 0:
            return None
        if self._entries is None or self._entries.device != dev or int(self._entries.shape[0]) < total:
            self._entries = torch.empty((max(1 << 16, int(1.3 * total)), 2), dtype=torch.int32, device=dev)
        capacity = int(self._entries.shape[0])
        if total > capacity:
            return None
        gigs_lib.check(_lib.gigs_ssr_hits(gigs_lib.ctx_ptr(), *a, *planes, 2, None, _p(offsets), _p(self._entries), capacity,
                                          _p(scratch), s), "ssr_hits (fill)")
        self.last_hits = total
        return offsets, self._entries

    @torch.no_grad()
    def from_gbuffer(self, cam: Dict, b: Dict, view_dirs: torch.Tensor, alpha_mask: Optional[torch.Tensor] = None,
                     albedo_ratio: Optional[Sequence[float]] = None) -> Dict:
        """Everything after the G-buffer `b` (a source's), which it reads and leaves as it is."""
        albedo_map = b["albedo_map"]
        dev = albedo_map.device
        N = len(self.lights)
        H, W = cam["image_height"], cam["image_width"]
        render_direct, IRR, render_rgb = (torch.empty((N, 3, H, W), device=dev) for _ in range(3))
        Kmax = min(N, MAX_LIGHTS)
        linear_rgb = self._scratch("linear_rgb_k", (Kmax, 3, H, W), torch.float32, dev)
        abd = self._scratch("abd_k", (Kmax, 3, H, W), torch.float32, dev)
        acc, loss = self._scratch("acc", (4 + 4 * 256,), torch.float32, dev), self._scratch("loss", (1,), torch.float32, dev)
        vd = view_dirs.contiguous().float()
        albedo_shade = _albedo_shade(albedo_map, albedo_ratio)
        scratch = _gi_scratch(W, H, dev)
        a = _gi_args(cam, self.gi)
        lut = self.brdf_lut
        self.last_hits = None
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream
            hits = packed = None
            if self.records:
                hits = self._record_hits(b, a, scratch, s)
            if hits is not None:
                packed = self._scratch("packed_rgb", (max(16, int(_lib.gigs_ssr_apply_multi_scratch_bytes(Kmax, W, H))),),
                                       torch.uint8, dev)
            for first in range(0, N, MAX_LIGHTS):
                chunk = self.lights[first:first + MAX_LIGHTS]
                K = len(chunk)
                rd, irr, rgb = render_direct[first:first + K], IRR[first:first + K], render_rgb[first:first + K]
                for light in chunk:
                    _complete(light)
                spec = [[x.contiguous() for x in light.specular] for light in chunk]
                L = len(spec[0])
                gigs_lib.check(_lib.gigs_shade_fwd_multi(
                    gigs_lib.ctx_ptr(), K, H, W, _p(b["normals_view"]), _p(vd), _p(albedo_shade), _p(b["roughness_map"]),
                    _p(b["mask_u8"]), _p(b["occlusion"]), _p(b["metallic_map"]) if self.metallic else None,
                    _ptr_array([light.diffuse for light in chunk]), int(chunk[0].diffuse.shape[1]), L,
                    _ptr_array([x for chain in spec for x in chain]), (C.c_int * L)(*[int(x.shape[1]) for x in spec[0]]),
                    _p(lut), int(lut.shape[-2]), int(lut.shape[-3]), int(self.tone), int(self.gamma), _p(rd), _p(linear_rgb), s),
                    "shade_fwd_multi")
                if hits is not None:
                    gigs_lib.check(_lib.gigs_ssr_apply_multi(
                        K, W, H, float(self.gi["delta"]), _p(hits[0]), _p(hits[1]), _p(b["onv"]), _p(b["depth_pos"]), _p(linear_rgb), _p(albedo_map),
                        _p(b["metallic_in"]), _p(b["F0"]), _p(irr), _p(abd), _p(packed), s), "ssr_apply_multi")
                else:
                    gigs_lib.check(_lib.gigs_ssr_multi(
                        gigs_lib.ctx_ptr(), K, *a, _p(b["onv"]), _p(b["depth_pos"]), _p(linear_rgb), _p(albedo_map),
                        _p(b["roughness_map"]), _p(b["metallic_in"]), _p(b["F0"]), _p(irr), _p(abd), _p(scratch), s), "ssr_multi")
                for k in range(K):  # the finish; the loss gigs_stage2_loss_fwd also forms is unused
                    gigs_lib.check(_lib.gigs_stage2_loss_fwd(H, W, _p(rd[k]), _p(irr[k]), _p(rd[k]), _p(b["mask_f"]),
                                                             _p(b["roughness_map"]), _p(b["metallic_in"]), _p(rgb[k]), _p(acc),
                                                             _p(loss), s), "stage2_loss_fwd")
        return _result(b, render_rgb, render_direct, IRR, alpha_mask)


class MultiRelighter(_LightsRelighter):
    """One view under K <= MAX_LIGHTS environment maps (relight_all.bash's list of target maps) at the cost of one G-buffer
    and one march (gigs_ssr_multi gathers the K radiance planes at the same hits); see _LightsRelighter.

    graphs=True captures the whole K-light view into one hipGraph, as Relighter(graphs=True) does (same replay, binning
    and DenseScene fallback); its outputs are the graph's static tensors: consume them before the next call."""

    def __init__(self, lights: Sequence[CubemapLight], gi: Dict, sh_degree: int, metallic: bool = False,
                 tone: bool = False, gamma: bool = False, graphs: bool = False, brdf_lut: Optional[torch.Tensor] = None,
                 source=None):
        lights = list(lights)
        if not 1 <= len(lights) <= MAX_LIGHTS:
            raise ValueError(f"MultiRelighter: 1..{MAX_LIGHTS} lights, got {len(lights)}")
        super().__init__("MultiRelighter", lights, gi, sh_degree, metallic, tone, gamma, brdf_lut, graphs, source)


class TurntableRelighter(_LightsRelighter):
    """One view under any number of lights -- usually rotated_lights(...) of one map, a turntable or a lighting sweep, but any
    list: only the shade samples and the radiance gathered at the march's hits depend on the light.  Per call the SSR march
    runs once as a recording (gigs_ssr_hits: count, prefix sum, one read-back of the total to size the entries, fill) and
    every chunk gathers at the recorded hits (the chunk's radiance packed pixel-major first); see _LightsRelighter.

    The gather is only launched with a complete list: the total read back is compared with the entries' capacity, and a
    mismatch (a total beyond 2^31 - 1 wraps the 32-bit prefix) sends the view through gigs_ssr_multi instead.  The hit list
    exists for the default march only (gi_march = proj, start < step); any other march also takes gigs_ssr_multi per chunk,
    with the same results.  Eager only (the read-back sizes a buffer): no hipGraph."""
    records = True

    def __init__(self, lights: Sequence[CubemapLight], gi: Dict, sh_degree: int, metallic: bool = False,
                 tone: bool = False, gamma: bool = False, brdf_lut: Optional[torch.Tensor] = None, source=None):
        lights = list(lights)
        if not lights:
            raise ValueError("TurntableRelighter: no lights")
        super().__init__("TurntableRelighter", lights, gi, sh_degree, metallic, tone, gamma, brdf_lut, False, source)


def quantize_8bit(x: torch.Tensor) -> torch.Tensor:
    """What torchvision.utils.save_image -> PNG -> / 255 makes of a float image: trunc(clamp(x * 255 + 0.5, 0, 255)) / 255
    (save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8); relight_eval.py reads the PNG and divides by 255)."""
    return torch.trunc(torch.clamp(x * 255 + 0.5, 0, 255)) / 255


class RelightEvaluator:
    """relight_eval.py without the file I/O: per light and view the PSNR (mean of the per-channel PSNRs) and SSIM (the
    training loss's) of the 8-bit-quantised prediction against that light's ground truth, bilinearly resized to the
    prediction's size first (align_corners=False, relight_eval.py:54).  With lpips= (an lpips.LPIPS) also LPIPS of the same
    two images, the K lights of a view as one batch.  The records stay on the device (gigs_image_metrics and
    gigs_lpips_vgg write row *slot of a table and advance the slot); results() reads them back once."""

    def __init__(self, light_names: Sequence[str], capacity: int = 1024, device="cuda", lpips=None):
        self.names = list(light_names)
        if not self.names:
            raise ValueError("RelightEvaluator: no light names")
        self._cap = int(capacity)
        self._rec = torch.zeros((len(self.names), self._cap, 7), dtype=torch.float64, device=device)
        self._slot = torch.zeros(len(self.names), dtype=torch.int32, device=device)
        self._n = 0
        self._done = []
        self._scratch = None
        self.lpips = lpips
        if lpips is not None:  # row v * K + k: view v, light k
            self._lp_rec = torch.zeros((self._cap * len(self.names), 6), dtype=torch.float64, device=device)
            self._lp_slot = torch.zeros(1, dtype=torch.int32, device=device)
            self._lp_done = []

    @torch.no_grad()
    def add(self, render_rgb: torch.Tensor, gt: torch.Tensor) -> None:
        """render_rgb [K,3,H,W] (MultiRelighter's), gt [K,3,h,w] in [0, 1]; light k is self.names[k]."""
        import torch.nn.functional as F
        from evaluate import image_metrics
        K = len(self.names)
        if render_rgb.dim() != 4 or gt.dim() != 4 or render_rgb.shape[0] != K or gt.shape[0] != K or render_rgb.shape[1] != 3:
            raise ValueError(f"RelightEvaluator.add: render_rgb and gt must be [{K},3,H,W]")
        if self._n >= self._cap:
            self._flush()
        H, W = render_rgb.shape[-2:]
        pred = quantize_8bit(render_rgb.float())
        gt = gt.float()
        if tuple(gt.shape[-2:]) != (H, W):
            gt = F.interpolate(gt, size=(H, W), mode="bilinear", align_corners=False)
        nbytes = int(_lib.gigs_image_metrics_scratch_bytes(3, H, W))
        if self._scratch is None or self._scratch.numel() < nbytes:
            self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=render_rgb.device)
        for k in range(K):
            image_metrics(pred[k], gt[k], scratch=self._scratch, slot=self._slot[k:k + 1], out=self._rec[k])
        if self.lpips is not None:
            self.lpips.record(gt, pred, slot=self._lp_slot, out=self._lp_rec)
        self._n += 1

    def _flush(self) -> None:
        if self._n:
            self._done.append(self._rec[:, :self._n].cpu())
            self._slot.zero_()
            if self.lpips is not None:
                self._lp_done.append(self._lp_rec[:self._n * len(self.names)].cpu())
                self._lp_slot.zero_()
            self._n = 0

    def records(self) -> torch.Tensor:
        """[K, n_views, 7] float64 on the host: image_metrics' records {mse_r, mse_g, mse_b, psnr, ssim, -, -}."""
        self._flush()
        return torch.cat(self._done, dim=1) if self._done else torch.zeros((len(self.names), 0, 7), dtype=torch.float64)

    def lpips_records(self) -> torch.Tensor:
        """[K, n_views, 6] float64 on the host: gigs_lpips_vgg's records {lpips, tap 0..4} (needs lpips=)."""
        if self.lpips is None:
            raise RuntimeError("RelightEvaluator: constructed without lpips=")
        self._flush()
        K = len(self.names)
        if not self._lp_done:
            return torch.zeros((K, 0, 6), dtype=torch.float64)
        return torch.cat(self._lp_done).reshape(-1, K, 6).permute(1, 0, 2).contiguous()

    def results(self) -> Dict[str, Dict[str, float]]:
        """{light name: {"psnr_avg", "ssim_avg", "n_views"} (+ "lpips_avg" with lpips=)}: relight_eval.py's per-light
        means (LPIPS: the float32 values the lpips call returns, summed in double as relight_eval.py:58 does)."""
        rec = self.records()
        n = int(rec.shape[1])
        lp = self.lpips_records() if self.lpips is not None else None
        out = {}
        for k, name in enumerate(self.names):
            if n == 0:
                out[name] = {"psnr_avg": float("nan"), "ssim_avg": float("nan"), "n_views": 0}
            else:
                out[name] = {"psnr_avg": float(rec[k, :, 3].sum() / n), "ssim_avg": float(rec[k, :, 4].sum() / n),
                             "n_views": n}
            if lp is not None:
                out[name]["lpips_avg"] = float(lp[k, :, 0].float().double().sum() / n) if n else float("nan")
        return out
