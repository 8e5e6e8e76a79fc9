"""The light-gradient scatter of the shade backward (csrc/shade.hip shade_bwd_kernel).  The default formulation walks
32 x 32 pixel tiles with 8 x 8 pixel waves and adds once per distinct texel of a wave into the global (fine) light
levels; the previous one (row-major 1024-pixel chunks, 16-lane runs) stays selectable as gigs_options.shade_bwd_rows.
Cases: bench.py's C2 view, a hot spot (every pixel reflects into the same texels), random per-pixel normals (more
distinct texels per wave than the deduplication takes: its fall-back), a ragged image and an all-masked one.
  * every per-pixel output (albedo, roughness and metallic gradient planes, lamb terms and the other gigs_shade_ext
    inputs included) is bit for bit the previous formulation's;
  * the light gradients match a float64 scatter of the same taps (autograd of oracle/torch_pbr_ref.py) and the previous
    formulation's (they may differ by summation order only)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import scenes
from helpers import GAUSS_KEYS
from oracle import stage2_ref
from oracle import torch_pbr_ref as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPEC_RES = (256, 128, 64, 32, 16)  # CubemapLight(base_res=256).build_mips: the three finest are scattered globally
ROUGH_SCALE, ROUGH_BIAS = 1.0 - 0.04, 0.04  # the stage-2 remap the fused step passes (gigs_shade_ext)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lut_np():
    path = os.path.join(os.path.dirname(__file__), "..", "gi-gs_amd", "pbr", "brdf_256_256.bin")
    return np.fromfile(path, dtype=np.float32).reshape(256, 256, 2)


def light(rng):
    spec = [rng.uniform(0.1, 1.0, (6, r, r, 3)).astype(np.float32) for r in SPEC_RES]
    return rng.uniform(0.1, 1.0, (6, 16, 16, 3)).astype(np.float32), spec


def unit(a):
    return (a / np.linalg.norm(a, axis=-1, keepdims=True)).astype(np.float32)


def c2_gbuffer():
    """bench.py's C2 view 0 through the product: rasterizer, filters, SSAO, gbuffer_post; [H, W, *] planes."""
    import pipeline
    sc = scenes.surface_scene(P=300_000, sh_degree=2, seed=0)
    cam = scenes.orbit_camera(0, 64, 800, 800, radius=3.5)
    g = {k: tt(sc[k]) for k in GAUSS_KEYS}
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    with torch.no_grad():
        r = pipeline.render(camt, g, 2, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS), fused_post=True)
    hwc = lambda t: np.ascontiguousarray(t.float().cpu().numpy().transpose(1, 2, 0))  # noqa: E731
    return dict(normals=hwc(r["normal_map"]), view_dirs=stage2_ref.canonical_view_dirs(cam).astype(np.float32),
                albedo=hwc(r["albedo_map"]), roughness=hwc(r["roughness_map"]), mask=hwc(r["normal_mask"]) != 0,
                occlusion=hwc(r["occlusion_map"]), metallic=hwc(r["metallic_map"]))


def synthetic(case, rng):
    H, W = {"hot_spot": (64, 96), "random_normals": (128, 192), "ragged": (75, 133), "all_masked": (64, 96)}[case]
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    if case == "hot_spot":  # one normal, one view direction: every pixel reflects into the same direction
        n = np.broadcast_to(unit(np.array([0.2, -0.3, 1.0])), (H, W, 3))
        v = np.broadcast_to(unit(np.array([0.31, 0.17, 1.0])), (H, W, 3))
    elif case == "random_normals":
        n, v = unit(rng.normal(size=(H, W, 3))), unit(rng.normal(size=(H, W, 3)))
    else:  # a smooth dome, seen from the front
        n = unit(np.stack([0.6 * xx, 0.6 * yy, np.ones_like(xx)], -1))
        v = unit(np.stack([0.2 * xx, 0.2 * yy, np.ones_like(xx)], -1))
    rough_hi = 1.0 if case == "ragged" else 0.45  # raw roughness: mostly the fine (global) levels, all levels when ragged
    mask = rng.uniform(size=(H, W, 1)) > 0.1
    if case == "all_masked":
        mask[:] = False
    return dict(normals=np.ascontiguousarray(n, np.float32), view_dirs=np.ascontiguousarray(v, np.float32),
                albedo=rng.uniform(0, 1, (H, W, 3)).astype(np.float32),
                roughness=rng.uniform(0.0, rough_hi, (H, W, 1)).astype(np.float32), mask=mask,
                occlusion=rng.uniform(0.3, 1, (H, W, 1)).astype(np.float32),
                metallic=rng.uniform(0, 1, (H, W, 1)).astype(np.float32))


def shade_bwd(g, diffuse, spec, extra, rows, tone, gamma):
    """One gigs_shade_bwd_ex call with the fused step's extension (roughness remap, albedo-product gradient, added
    roughness / metallic gradients, g_scale, lamb terms) -> (per-pixel outputs, light gradients), numpy."""
    import gigs_lib
    from pbr.shade import _ptr_array
    lib = gigs_lib.lib()
    ctx = gigs_lib.current().derive(shade_bwd_rows=int(rows))
    H, W = g["mask"].shape[:2]
    x = {k: tt(v) for k, v in g.items() if k != "mask"}
    mask8 = tt(g["mask"].astype(np.uint8))
    e = {k: tt(v) for k, v in extra.items()}
    dif, sp, lut = tt(diffuse), [tt(s) for s in spec], tt(lut_np())
    d_alb = torch.full((H, W, 3), float("nan"), device=DEV)
    d_rgh, d_met = torch.full((H, W, 1), float("nan"), device=DEV), torch.full((H, W, 1), float("nan"), device=DEV)
    d_dif, d_sp = torch.zeros_like(dif), [torch.zeros_like(s) for s in sp]
    p = lambda t: t.data_ptr()  # noqa: E731
    ext = gigs_lib.ShadeExt(planar=0, rough_scale=ROUGH_SCALE, rough_bias=ROUGH_BIAS, g_albedo_mul_a=p(e["mul_a"]),
                            g_albedo_mul_b=p(e["mul_b"]), g_roughness_add=p(e["add_r"]), g_metallic_add=p(e["add_m"]),
                            g_scale=p(e["g_scale"]), lamb_mask=p(e["lamb_mask"]), lamb_acc4=p(e["acc4"]))
    spec_res = (C.c_int * len(sp))(*[int(s.shape[1]) for s in sp])
    gigs_lib.check(lib.gigs_shade_bwd_ex(
        ctx.ptr, H, W, p(x["normals"]), p(x["view_dirs"]), p(x["albedo"]), p(x["roughness"]), p(mask8), p(x["occlusion"]),
        p(x["metallic"]), p(dif), int(dif.shape[1]), len(sp), _ptr_array(sp), spec_res, p(lut), 256, 256, int(tone),
        int(gamma), p(e["g_render"]), None, None, None, p(d_alb), p(d_rgh), p(d_met), p(d_dif), _ptr_array(d_sp),
        C.addressof(ext), torch.cuda.current_stream().cuda_stream), "shade_bwd_ex")
    torch.cuda.synchronize()
    px = dict(albedo=d_alb.cpu().numpy(), roughness=d_rgh.cpu().numpy(), metallic=d_met.cpu().numpy())
    return px, [d_dif.cpu().numpy()] + [d.cpu().numpy() for d in d_sp]


def float64_light_grads(g, diffuse, spec, g_render, tone, gamma):
    """The light gradients as autograd of the float64 restatement scatters them (same taps, same roughness remap).
    Where the restatement cannot follow the kernel the inputs are restated, not the result:
      * a pixel whose normal is 0 (the G-buffer's median filter leaves a few inside the mask) has no diffuse tap in
        the kernel, so its diffuse light is 0, while the restatement looks the zero direction up as NaN taps: it gets
        the normal -v and occlusion 0 (n.v < 0 keeps the reflected direction -v and N.V at its clamp, as in the kernel);
      * a pixel outside the mask carries no gradient: it gets finite materials (0 * NaN would be NaN in the scatter)."""
    out = ~g["mask"]  # [H, W, 1]
    flat = ~(g["normals"] != 0).any(-1, keepdims=True)
    fill = lambda a, v, where=out: np.where(where, np.float32(v), a).astype(np.float32)  # noqa: E731
    rough = fill((g["roughness"] * np.float32(ROUGH_SCALE) + np.float32(ROUGH_BIAS)).astype(np.float32), 0.5)
    normals = np.where(flat, -g["view_dirs"], g["normals"]).astype(np.float32)
    albedo, metallic = fill(g["albedo"], 0.5), fill(g["metallic"], 0.0)
    occlusion = fill(fill(g["occlusion"], 1.0), 0.0, flat)
    d64 = tp.to64(diffuse).requires_grad_(True)
    s64 = [tp.to64(s).requires_grad_(True) for s in spec]
    outs = tp.shade(tp.to64(normals), tp.to64(g["view_dirs"]), tp.to64(albedo), tp.to64(rough),
                    torch.from_numpy(g["mask"]), tp.to64(occlusion), tp.to64(metallic), None, d64, s64,
                    tp.to64(lut_np()), tone=tone, gamma=gamma)
    (outs[0] * tp.to64(g_render)).sum().backward()
    return [d64.grad.numpy()] + [s.grad.numpy() for s in s64]


@pytest.mark.parametrize("case,tone,gamma", [("c2", False, False), ("hot_spot", False, False),
                                             ("random_normals", True, True), ("ragged", False, True),
                                             ("all_masked", False, False)])
def test_scatter_matches_rows_and_float64(case, tone, gamma):
    rng = np.random.default_rng(11)
    g = c2_gbuffer() if case == "c2" else synthetic(case, rng)
    H, W = g["mask"].shape[:2]
    diffuse, spec = light(rng)
    gscale = np.float32(0.75)
    # upstream gradient of the render: positive on the hot spot, so that thousands of adds into one texel do not cancel
    g_render = (rng.uniform(0, 1, (H, W, 3)) if case == "hot_spot" else rng.normal(size=(H, W, 3))).astype(np.float32)
    lamb = g["mask"][..., 0].astype(np.float32)
    extra = dict(g_render=g_render, mul_a=rng.normal(size=(H, W, 3)).astype(np.float32),
                 mul_b=rng.uniform(0, 1, (H, W, 3)).astype(np.float32), add_r=rng.normal(size=(H, W)).astype(np.float32),
                 add_m=rng.normal(size=(H, W)).astype(np.float32), g_scale=np.array([gscale], np.float32),
                 lamb_mask=lamb, acc4=np.array([0, 0, 0, max(float(lamb.sum()), 1.0)], np.float32))
    px_t, light_t = shade_bwd(g, diffuse, spec, extra, rows=False, tone=tone, gamma=gamma)
    px_r, light_r = shade_bwd(g, diffuse, spec, extra, rows=True, tone=tone, gamma=gamma)
    for k in px_t:  # every pixel written, bit for bit the previous formulation's
        assert not np.isnan(px_t[k]).all(), k
        np.testing.assert_array_equal(px_t[k].view(np.uint32), px_r[k].view(np.uint32), err_msg=k)
    want = float64_light_grads(g, diffuse, spec, g_render.astype(np.float64) * float(gscale), tone, gamma)
    names = ["diffuse"] + ["spec%d" % r for r in SPEC_RES]
    for name, a, b, ref in zip(names, light_t, light_r, want):
        assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(ref).all(), name
        if case == "all_masked":
            assert not a.any() and not b.any() and not ref.any(), name
            continue
        scale = max(np.abs(ref).max(), 1e-20)
        # the two formulations: summation order only
        d = np.abs(a.astype(np.float64) - b).max() / scale
        assert d <= 1e-4, (name, d)
        # against float64; fp32 threshold flips (a level or texel boundary) touch isolated pixels: judge by the bulk
        err = np.abs(a.astype(np.float64) - ref)
        assert np.median(err) / scale < 1e-5 and (err / scale > 1e-3).mean() < 2e-3, (name, err.max() / scale)
    if case == "hot_spot":  # the fine levels were hit, in a handful of texels
        assert all(0 < np.count_nonzero(np.abs(s).sum(-1)) <= 16 for s in light_t[1:4])
