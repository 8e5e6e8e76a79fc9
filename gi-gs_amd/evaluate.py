"""Novel-view evaluation of a trained scene: the reference's render.py (render_set's pbr branch, eval_brdf) and
normal_eval.py without the file I/O (render_scene.py writes the files), on the HIP library.

    NovelViewEvaluator(light, gi, sh_degree, ...)   render.py:115-395 per view: render(inference=True, pad_normal=True,
      (cam, g, view_dirs, gt_image, alpha_mask)     derive_normal=True) -> pbr_shading -> Gaussian_SSR -> sRGB + 3x3
                                                    median -> the float planes render.py saves, plus this view's PSNR
                                                    and SSIM against the composited ground truth, kept on the device;
                                                    light.build_mips() once per run (:142)
      .results()                                    {"psnr_avg", "ssim_avg", "n_views"} (+ "lpips_avg" with lpips=):
                                                    one read-back
    albedo_ratio(gt_albedos, pred_albedos, masks)   render.py:578-586: per-channel median(gt / clamp(pred, 1e-6))
    albedo_metrics(...)                             render.py:596-631: masked MSE, then PSNR / SSIM (/ LPIPS) of
                                                    pred * ratio
    normal_mae(pred_normals, gt_rgba)               normal_eval.py: mean angular error in degrees

The per-view metrics run in libgigs_hip (gigs_image_metrics: per-channel MSE -> the mean of the per-channel PSNRs, as
utils/image_utils.py:31-33 computes psnr(a, b).mean(); mean SSIM with the training loss's separable window; masked
MSE; gigs_normal_angular_error for normal_eval.py's get_mae), reduced in double in a fixed order, so a run's numbers
are the same bit for bit every time.  LPIPS (render.py's lpips_avg, eval_brdf's albedo_lpips) is opt-in: pass an
`lpips.LPIPS` instance (this package's drop-in, gigs_lpips_vgg) as `lpips=`; without one the results leave it out.

Reference quirks kept on purpose: render.py's F0 branch is not relight.py's (:320-326): with metallic=True F0 =
(1 - True) * 0.04 + albedo * metallic, i.e. albedo * metallic, and SSR gets the metallic map; otherwise F0 = 0.04 and a
zero metallic plane (which is also the saved metallic plane).  Roughness is not remapped.  The saved planes keep their
compositing (:343-363): x * alpha + 0 * (1 - alpha) broadcast over three channels, clamped to [0, 1]; `normal` is
(clamp(normal * alpha, 0, 1) + 1) / 2.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

import gigs_lib
import pipeline
from diff_gaussian_rasterization import Gaussian_SSR, filters
from pbr import CubemapLight, get_brdf_lut, pbr_shading
from relight import Scratch, ViewReplay, shade_ssr

_lib = gigs_lib.lib()

PLANES = ("pbr", "DIR", "indirect", "albedo", "roughness", "metallic", "occlusion", "normal", "from_depth")
# extra_planes=True: render.py's diffuse / specular images (:288-317, :348-349) and the raw depth map (:376 normalises it)
EXTRA_PLANES = ("diffuse", "specular", "depth")


def _scratch(dev, C: int, H: int, W: int) -> torch.Tensor:
    return torch.empty(int(_lib.gigs_image_metrics_scratch_bytes(C, H, W)), dtype=torch.uint8, device=dev)


def image_metrics(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                  scratch: Optional[torch.Tensor] = None, slot: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gigs_image_metrics for one view, pred / gt [C,H,W]: the float64 record {mse_0..mse_{C-1}, mean psnr, mean ssim,
    masked mse, masked element count} (stride C + 4).  With `slot` (an int32 device scalar) the record goes to row
    *slot of `out` and *slot is incremented on the device."""
    if not pred.is_cuda:
        raise RuntimeError("image_metrics needs CUDA/HIP tensors: gigs-hip has no CPU path")
    a, b = pred.contiguous().float(), gt.contiguous().float()
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("image_metrics: pred and gt must both be [C,H,W]")
    C_, H, W = a.shape
    dev = a.device
    m = None
    if mask is not None:
        m = mask.reshape(H, W).to(torch.uint8).contiguous()
    if scratch is None:
        scratch = _scratch(dev, C_, H, W)
    if out is None:
        out = torch.empty(C_ + 4, dtype=torch.float64, device=dev)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        gigs_lib.check(_lib.gigs_image_metrics(C_, H, W, p(a), p(b), p(m), p(scratch), p(slot), p(out),
                                               torch.cuda.current_stream().cuda_stream), "image_metrics")
    return out


class NovelViewEvaluator:
    """render_set's pbr branch (render.py:115-395) without the file I/O.  graphs=True (the default) replays the whole
    view -- rasterizer under asynchronous binning, G-buffer post, shade, SSR, the saved planes and the metrics -- from one
    hipGraph; camera pose, view_dirs, gt_image and alpha_mask are its inputs.  The planes it returns are the graph's
    static outputs: consume them before the next call.  fused=False runs the reference's op sequence with this
    package's drop-in operators (pipeline.render, pbr_shading, Gaussian_SSR); the metrics run on the device either way."""

    def __init__(self, light: CubemapLight, gi: Dict, sh_degree: int, metallic: bool = False, tone: bool = False,
                 gamma: bool = False, graphs: bool = True, fused: bool = True, brdf_lut: Optional[torch.Tensor] = None,
                 capacity: int = 1024, lpips=None, extra_planes: bool = False):
        """extra_planes=True adds EXTRA_PLANES to the planes a call returns (the shade also writes its diffuse and
        specular parts); the default returns PLANES, exactly as before."""
        dev = light.base.device
        self.light, self.gi, self.sh_degree = light, gi, sh_degree
        self.metallic, self.tone, self.gamma, self.fused = bool(metallic), bool(tone), bool(gamma), bool(fused)
        self.graphs = bool(graphs) and self.fused
        self.brdf_lut = (brdf_lut if brdf_lut is not None else get_brdf_lut()).to(dev)
        self._scratch = Scratch()
        self._view = ViewReplay(sh_degree, "NovelViewEvaluator")
        with torch.no_grad():
            light.build_mips()  # render.py:142: once per run
        self.extra_planes = bool(extra_planes)
        self.names = PLANES + EXTRA_PLANES if self.extra_planes else PLANES
        self._cap = int(capacity)
        # 4 rows of headroom: the graph's warm-up runs write records before the slot is rewound
        self._rec = torch.zeros((self._cap + 4, 7), dtype=torch.float64, device=dev)
        self._slot = torch.zeros(1, dtype=torch.int32, device=dev)
        self._n = 0
        self._done = []
        # lpips(gt, render_rgb) per view (render.py:381): gigs_lpips_vgg records {lpips, tap 0..4} in a table of their own
        self.lpips = lpips
        if lpips is not None:
            self._lp_rec = torch.zeros((self._cap + 4, 6), dtype=torch.float64, device=dev)
            self._lp_slot = torch.zeros(1, dtype=torch.int32, device=dev)
            self._lp_done = []

    @torch.no_grad()
    def __call__(self, cam: Dict, g: Dict[str, torch.Tensor], view_dirs: torch.Tensor, gt_image: torch.Tensor,
                 alpha_mask: torch.Tensor) -> Dict[str, torch.Tensor]:
        if self._n >= self._cap:
            self._flush()
        gt_image, alpha_mask = gt_image.contiguous().float(), alpha_mask.contiguous().float()
        out = None
        if self.graphs:
            try:
                out = self._view(cam, g, (view_dirs, gt_image, alpha_mask), lambda c, *rest: self._core(c, g, *rest),
                                 self.names, on_capture=self._rewind)
            except pipeline.DenseScene:
                self.graphs = False
        if out is None:
            out = dict(zip(self.names, self._core(cam, g, view_dirs, gt_image, alpha_mask)))
        self._n += 1
        return out

    def _rewind(self) -> None:
        self._slot.fill_(self._n)
        if self.lpips is not None:
            self._lp_slot.fill_(self._n)

    def close(self) -> None:
        self._view.close()

    def _core(self, cam, g, view_dirs, gt_image, alpha_mask):
        r = (self._fused_pad if self.fused else self._unfused_pad)(cam, g, view_dirs)
        dev = alpha_mask.device
        background = torch.zeros(3, device=dev)
        bg = background[:, None, None]
        gt = (gt_image * alpha_mask + bg * (1.0 - alpha_mask)).clamp(0.0, 1.0)  # render.py:230
        mask = r["normal_mask"]
        IRR2 = r["IRR2"]
        render_rgb = torch.where(mask, r["render_rgb"], bg)  # render.py:332-337
        comp = lambda x: (x * alpha_mask + bg * (1.0 - alpha_mask)).clamp(0.0, 1.0)  # noqa: E731  (:343-363)
        planes = dict(pbr=render_rgb, DIR=render_rgb - IRR2, indirect=IRR2, albedo=comp(r["albedo"]),
                      roughness=comp(r["roughness"]), metallic=comp(r["metallic"]), occlusion=comp(r["occlusion"]),
                      normal=(comp(r["normal"]) + 1) / 2, from_depth=(r["from_depth"] + 1) / 2)
        if self.extra_planes:
            part = lambda x: comp(torch.where(mask, x.clamp(0.0, 1.0), bg))  # noqa: E731  (render.py:288-317, :348-349)
            planes.update(diffuse=part(r["diffuse"]), specular=part(r["specular"]), depth=r["depth"])
        image_metrics(render_rgb, gt, scratch=self._scratch("metrics_scratch", (int(_lib.gigs_image_metrics_scratch_bytes(
            3, *render_rgb.shape[1:])),), torch.uint8, dev), slot=self._slot, out=self._rec)
        if self.lpips is not None:
            self.lpips.record(gt, render_rgb, slot=self._lp_slot, out=self._lp_rec)
        return tuple(planes[n] for n in self.names)

    def _branch(self, albedo_map, roughness_map, metallic_map):
        """render.py:320-326: (F0, the metallic plane SSR receives and render.py saves)."""
        if self.metallic:
            return torch.addcmul(torch.full_like(albedo_map, (1.0 - float(self.metallic)) * 0.04), albedo_map,
                                 metallic_map), metallic_map
        return torch.full_like(albedo_map, 0.04), torch.zeros_like(roughness_map)

    # -- the fused sequence: the pad_normal G-buffer post, then relight.shade_ssr's shade / SSR / sRGB + median launches ----
    def _fused_pad(self, cam, g, view_dirs):
        dev = g["means3D"].device
        background = torch.zeros(3, device=dev)
        (out, _, st) = pipeline.rasterize(cam, g, self.sh_degree, background, self.gi, inference=True, derive_normal=True)
        (_, _, opacity_map, depth_map, nfd, normal_map, occlusion, albedo_map, roughness_map, metallic_map, out_normal_view,
         depth_pos) = out
        H, W = cam["image_height"], cam["image_width"]
        new = lambda name, *shape: self._scratch(name, shape, torch.float32, dev)  # noqa: E731
        normals_view, onv, nfd_out = new("normals_view", 3, H, W), new("onv", 3, H, W), new("nfd", 3, H, W)
        mask_u8 = self._scratch("mask_u8", (H, W), torch.uint8, dev)
        mask_f = new("mask_f", 1, H, W)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        vm = st.viewmatrix.contiguous().float()
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream
            gigs_lib.check(_lib.gigs_gbuffer_post_pad(H, W, p(normal_map), p(nfd), p(opacity_map), p(out_normal_view), p(vm),
                                                      p(mask_u8), p(mask_f), None, p(normals_view), p(onv), p(nfd_out),
                                                      None, s), "gbuffer_post_pad")
        F0, metallic_in = self._branch(albedo_map, roughness_map, metallic_map)
        b = dict(normals_view=normals_view, mask_u8=mask_u8, mask_f=mask_f, onv=onv, depth_pos=depth_pos, albedo_map=albedo_map,
                 roughness_map=roughness_map, metallic_map=metallic_map, occlusion=occlusion, F0=F0, metallic_in=metallic_in)
        res = shade_ssr(self.light, self.brdf_lut, self.gi, self.metallic, self.tone, self.gamma, cam, view_dirs, b, albedo_map,
                        self._scratch, parts=self.extra_planes)
        IRR, render_rgb = res[1], res[2]
        IRR2 = filters.median_blur(pipeline.linear_to_srgb(IRR)[None, ...], (3, 3))[0]
        out = dict(render_rgb=render_rgb, IRR2=IRR2, normal_mask=mask_u8.bool()[None], albedo=albedo_map,
                   roughness=roughness_map, metallic=metallic_in, occlusion=occlusion, normal=normals_view,
                   from_depth=nfd_out)
        if self.extra_planes:
            out.update(diffuse=res[3], specular=res[4], depth=depth_map)
        return out

    # -- render.py's op sequence, operator by operator -------------------------------------------------------------
    def _unfused_pad(self, cam, g, view_dirs):
        dev = g["means3D"].device
        gi = self.gi
        background = torch.zeros(3, device=dev)
        r = pipeline.render(cam, g, self.sh_degree, background, gi, inference=True, derive_normal=True, pad_normal=True)
        H, W = cam["image_height"], cam["image_width"]
        normal_mask = r["normal_mask"]
        albedo_map, roughness_map, metallic_map = r["albedo_map"], r["roughness_map"], r["metallic_map"]
        res = pbr_shading(light=self.light, normals=r["normal_map"].permute(1, 2, 0), view_dirs=view_dirs,
                          mask=normal_mask.permute(1, 2, 0), albedo=albedo_map.permute(1, 2, 0),
                          roughness=roughness_map.permute(1, 2, 0),
                          metallic=metallic_map.permute(1, 2, 0) if self.metallic else None, tone=self.tone,
                          occlusion=r["occlusion_map"].permute(1, 2, 0), gamma=self.gamma, brdf_lut=self.brdf_lut)
        render_direct = torch.where(normal_mask, res["render_rgb"].permute(2, 0, 1), background[:, None, None])
        ssr = Gaussian_SSR(cam["tanfovx"], cam["tanfovy"], W, H, gi["radius"], gi["bias"], gi["thick"], gi["delta"],
                           gi["step"], gi["start"])
        F0, metallic_in = self._branch(albedo_map, roughness_map, metallic_map)
        IRR, _ = ssr(r["out_normal_view"], r["depth_pos"], pipeline.srgb_to_linear(render_direct), albedo_map,
                     roughness_map, metallic_in, F0)
        IRR2 = filters.median_blur(pipeline.linear_to_srgb(IRR)[None, ...], (3, 3))[0]
        out = dict(render_rgb=render_direct + IRR2, IRR2=IRR2, normal_mask=normal_mask, albedo=albedo_map,
                   roughness=roughness_map, metallic=metallic_in, occlusion=r["occlusion_map"], normal=r["normal_map"],
                   from_depth=r["normal_map_from_depth"])
        if self.extra_planes:
            out.update(diffuse=res["diffuse_rgb"].permute(2, 0, 1), specular=res["specular_rgb"].permute(2, 0, 1),
                       depth=r["depth_map"])
        return out

    def _flush(self) -> None:
        n = self._n
        if n:
            self._done.append(self._rec[:n].cpu())
            self._slot.fill_(0)
            if self.lpips is not None:
                self._lp_done.append(self._lp_rec[:n].cpu())
                self._lp_slot.fill_(0)
            self._n = 0

    def records(self) -> torch.Tensor:
        """The per-view metric records so far, [n_views, 7] float64 on the host (one read-back)."""
        self._flush()
        return torch.cat(self._done) if self._done else torch.zeros((0, 7), dtype=torch.float64)

    def lpips_records(self) -> torch.Tensor:
        """The per-view LPIPS records so far, [n_views, 6] float64 {lpips, tap 0..4} on the host (needs lpips=)."""
        if self.lpips is None:
            raise RuntimeError("NovelViewEvaluator: constructed without lpips=")
        self._flush()
        return torch.cat(self._lp_done) if self._lp_done else torch.zeros((0, 6), dtype=torch.float64)

    def results(self) -> Dict[str, float]:
        """render.py:386-395: the means of the per-view PSNR and SSIM, and with lpips= the mean of the per-view LPIPS
        (each the float32 value the lpips call returns, summed in double as render.py:381 does)."""
        rec = self.records()
        n = int(rec.shape[0])
        if n == 0:
            res = {"psnr_avg": float("nan"), "ssim_avg": float("nan"), "n_views": 0}
        else:
            res = {"psnr_avg": float(rec[:, 3].sum() / n), "ssim_avg": float(rec[:, 4].sum() / n), "n_views": n}
        if self.lpips is not None:
            lp = self.lpips_records()
            res["lpips_avg"] = float(lp[:, 0].float().double().sum() / n) if n else float("nan")
        return res


def albedo_ratio(gt_albedos: Sequence[torch.Tensor], pred_albedos: Sequence[torch.Tensor],
                 masks: Sequence[torch.Tensor]) -> torch.Tensor:
    """render.py:578-586: gt / pred albedos [H,W,3] (pred as read back from the 8-bit PNG), masks [H,W] bool;
    the per-channel lower median of gt / clamp(pred, 1e-6) over the masked pixels of every view, [3]."""
    gt_all = torch.cat([a[m] for a, m in zip(gt_albedos, masks)], dim=0)
    pred_all = torch.cat([a[m] for a, m in zip(pred_albedos, masks)], dim=0)
    return (gt_all / pred_all.clamp(min=1e-6)).median(dim=0).values


def albedo_metrics(gt_albedos: Sequence[torch.Tensor], pred_albedos: Sequence[torch.Tensor],
                   masks: Sequence[torch.Tensor], ratio: Optional[torch.Tensor] = None, lpips=None) -> Dict[str, float]:
    """render.py:596-631: per view the masked MSE of the unscaled prediction, then PSNR and SSIM of pred * ratio against
    gt (all [H,W,3], masked pixels already zeroed as eval_brdf does); means over the views.  With lpips= (an
    lpips.LPIPS) also "albedo_lpips": the mean of lpips(gt, pred * ratio) (:617)."""
    if ratio is None:
        ratio = albedo_ratio(gt_albedos, pred_albedos, masks)
    psnr = ssim = mse = lp = 0.0
    n = len(gt_albedos)
    for gt, pred, m in zip(gt_albedos, pred_albedos, masks):
        gt_c, pred_c = gt.float().permute(2, 0, 1), pred.float().permute(2, 0, 1)
        mse += float(image_metrics(pred_c, gt_c, mask=m)[5])
        scaled = pred_c * ratio.to(pred_c)[:, None, None]
        rec = image_metrics(scaled, gt_c)
        psnr += float(rec[3])
        ssim += float(rec[4])
        if lpips is not None:
            lp += float(lpips(gt_c, scaled).reshape(()))
    res = {"albedo_psnr": psnr / n, "albedo_ssim": ssim / n, "roughmse": mse / n}
    if lpips is not None:
        res["albedo_lpips"] = lp / n
    return res


def normal_mae(pred_normals: Sequence[torch.Tensor], gt_rgba: Sequence[torch.Tensor]) -> float:
    """normal_eval.py: the mean angular error in degrees over all pixels of all views.  pred_normals: render.py's saved
    `normal` (or `from_depth`) planes [3,H,W] as floats -- rounded to 8 bits here as the PNG would be; gt_rgba: the
    ground-truth normal PNGs [H,W,4] (or [H,W,3]) uint8 on the device."""
    if not len(pred_normals):
        raise ValueError("normal_mae: no views")
    dev = pred_normals[0].device
    out = torch.zeros((len(pred_normals), 2), dtype=torch.float64, device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = None
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream().cuda_stream
        for pred, gt in zip(pred_normals, gt_rgba):
            a = pred.contiguous().float()
            b = gt.contiguous().to(torch.uint8)
            _, H, W = a.shape
            if b.shape[0] != H or b.shape[1] != W or b.shape[2] not in (3, 4):
                raise ValueError("normal_mae: gt must be [H,W,4] or [H,W,3] uint8 matching the prediction")
            if scratch is None or scratch.numel() < _lib.gigs_image_metrics_scratch_bytes(3, H, W):
                scratch = _scratch(dev, 3, H, W)
            gigs_lib.check(_lib.gigs_normal_angular_error(H, W, a.data_ptr(), b.data_ptr(), int(b.shape[2]),
                                                          scratch.data_ptr(), slot.data_ptr(), out.data_ptr(), s),
                           "normal_angular_error")
    tot = out.sum(dim=0).cpu()
    return float(tot[0] / tot[1])
