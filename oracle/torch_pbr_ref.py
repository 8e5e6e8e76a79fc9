"""PyTorch (CPU, float64) restatement of the deferred shade and of the cubemap light filters,
with autograd: the checker for the hand-written HIP backward kernels.

TEST INFRASTRUCTURE ONLY.  Texture sampling follows the rule written in include/gigs_hip.h
(modelled on nvdiffrast's dr.texture; third party, parity unpinned).

The `mut` arguments (cube_sample, lut_sample, get_mip, linear_to_srgb, shade, shade_with_grads) exist for ONE purpose: the
teeth tests of tests/test_shade_f64_cpu.py, which need a backward that is wrong in one named branch while every value stays
bit for bit.  Each name multiplies or adds to a GRADIENT through grad_scale / a detached difference, inside the function
that owns the branch.  With mut empty (the default, and what every checker of a kernel passes) none of that code runs and
the functions are the reference.
"""
from __future__ import annotations

import math

import numpy as np
import torch

DT = torch.float64


def cube_dir_raw(a, b, face):
    one = torch.ones_like(a)
    outs = [torch.stack(v, -1) for v in ((one, -b, -a), (-one, -b, a), (a, one, b), (a, -one, -b), (a, -b, one), (-a, -b, -one))]
    res = torch.zeros_like(outs[0])
    for f in range(6):
        res = torch.where((face == f)[..., None], outs[f], res)
    return res


def cube_face_uv(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = x.abs(), y.abs(), z.abs()
    is_z = az > torch.maximum(ax, ay)
    is_y = (~is_z) & (ay > ax)
    c = torch.where(is_z, z, torch.where(is_y, y, x))
    a = torch.where(is_z, x, torch.where(is_y, x, z))
    b = torch.where(is_z, y, torch.where(is_y, z, y))
    face = torch.where(is_z, 4, torch.where(is_y, 2, 0)) + (c < 0).long()
    m = 0.5 / c.abs()
    m0 = torch.where((face == 0) | (face == 5), -m, m)
    m1 = torch.where(face != 2, -m, m)
    u = (a * m0 + 0.5).clamp(0, 1)
    v = (b * m1 + 0.5).clamp(0, 1)
    return face, u, v


def grad_scale(x, s):
    """x, bit for bit, whose gradient is multiplied by s (a wrong backward on purpose: the `mut` arguments below)."""
    return x.detach() + (x - x.detach()) * s


def _to_integer(f):
    """distance of f to the nearest integer: how far a floor() decision is from flipping"""
    return (f - torch.round(f)).abs()


def cube_taps(res, d, info=None):
    """-> idx [...,4] (long, -1 = dropped), w [...,4], in the dtype of d.  info (a dict) receives the decisions: face,
    wrapped [...,4] (the tap was taken from a neighbouring face), edge [...,4] (which edge it left by: 0/1 = x low/high,
    2/3 = y low/high; -1 inside), dropped [...] and corner [...] (2 * y_high + x_high of the dropped tap, -1 = none), wsum
    (of the valid taps before the renormalisation) and margin [...] (texels: distance of the tap coordinates to an integer)."""
    face, u, v = cube_face_uv(d)
    fu, fv = u * res - 0.5, v * res - 0.5
    iu0, iv0 = torch.floor(fu).detach(), torch.floor(fv).detach()
    tu, tv = fu - iu0, fv - iv0
    idxs, ws, edges = [], [], []
    for k in range(4):
        ox, oy = k & 1, k >> 1
        ix, iy = iu0.long() + ox, iv0.long() + oy
        w = (tu if ox else 1 - tu) * (tv if oy else 1 - tv)
        out_x = (ix < 0) | (ix >= res)
        out_y = (iy < 0) | (iy >= res)
        inside = (face * res + iy.clamp(0, res - 1)) * res + ix.clamp(0, res - 1)
        a = 2.0 * ((ix.to(d.dtype) + 0.5) / res) - 1.0
        b = 2.0 * ((iy.to(d.dtype) + 0.5) / res) - 1.0
        f2, u2, v2 = cube_face_uv(cube_dir_raw(a, b, face))
        x2 = torch.floor(u2 * res).long().clamp(0, res - 1)
        y2 = torch.floor(v2 * res).long().clamp(0, res - 1)
        wrapped = (f2 * res + y2) * res + x2
        idx = torch.where(out_x & out_y, torch.full_like(inside, -1), torch.where(out_x | out_y, wrapped, inside))
        idxs.append(idx)
        ws.append(w)
        if info is not None:
            e = torch.where(out_x, (ix >= res).long(), torch.where(out_y, 2 + (iy >= res).long(), torch.full_like(ix, -1)))
            edges.append(torch.where(out_x & out_y, 4 + 2 * (iy >= res).long() + (ix >= res).long(), e))
    idx = torch.stack(idxs, -1)
    w = torch.stack(ws, -1)
    valid = idx >= 0
    w = torch.where(valid, w, torch.zeros_like(w))
    dropped = (~valid).any(-1, keepdim=True)
    wsum = w.sum(-1, keepdim=True)
    w = torch.where(dropped, w / wsum, w)
    if info is not None:
        e = torch.stack(edges, -1)
        info.update(face=face, wrapped=(e >= 0) & (e < 4), edge=torch.where(e < 4, e, torch.full_like(e, -1)),
                    dropped=dropped[..., 0], corner=torch.where(e >= 4, e - 4, torch.full_like(e, -1)).max(-1).values,
                    wsum=wsum.detach(), margin=torch.minimum(_to_integer(fu), _to_integer(fv)).detach())
    return idx, w


def cube_sample(tex, d, info=None, mut=()):
    """tex [6,r,r,3]; d [...,3] -> [...,3].  mut: teeth tests only (module docstring); it alters the texel gradient of wrapped
    taps / of corner pixels, never a value."""
    res = tex.shape[1]
    info = {} if (mut and info is None) else info
    idx, w = cube_taps(res, d, info)
    flat = tex.reshape(-1, tex.shape[-1])
    vals = flat[idx.clamp(min=0)]  # [...,4,3]
    if info is not None:
        info.update(idx=idx, w=w.detach())
    if "wrapped_taps_0.9" in mut:
        vals = grad_scale(vals, torch.where(info["wrapped"], 0.9, 1.0).to(w.dtype)[..., None])
    if "corner_renormalisation_lost" in mut:
        vals = grad_scale(vals, torch.where(info["dropped"][..., None], info["wsum"], torch.ones_like(w[..., :1]))[..., None])
    return (vals * w[..., None]).sum(-2)


def lut_sample(lut, u, v, info=None, mut=()):
    """lut [h,w,2], linear + clamp.  mut: teeth tests only (module docstring)."""
    h, w_ = lut.shape[0], lut.shape[1]
    fu, fv = u * w_ - 0.5, v * h - 0.5
    iu0, iv0 = torch.floor(fu).detach(), torch.floor(fv).detach()
    tu, tv = (fu - iu0)[..., None], (fv - iv0)[..., None]
    x0, x1 = iu0.long().clamp(0, w_ - 1), (iu0.long() + 1).clamp(0, w_ - 1)
    y0, y1 = iv0.long().clamp(0, h - 1), (iv0.long() + 1).clamp(0, h - 1)
    if info is not None:
        info.update(x0=x0, y0=y0, x1=x1, y1=y1, row_clamped=(y0 == y1),
                    margin=torch.minimum(_to_integer(fu), _to_integer(fv)).detach())
    out = (lut[y0, x0] * (1 - tu) * (1 - tv) + lut[y0, x1] * tu * (1 - tv) + lut[y1, x0] * (1 - tu) * tv
           + lut[y1, x1] * tu * tv)
    if "lut_slope_in_clamped_rows" in mut:
        out = out + ((v - v.detach()) * (y0 == y1).to(v.dtype))[..., None]
    return out


MIP_MINR, MIP_MAXR = 0.08, 0.5


def get_mip(r, L, mut=()):
    """pbr/light.py:142-152.  mut: teeth tests only (module docstring): a slope where the reference has none / a wrong one."""
    MINR, MAXR = MIP_MINR, MIP_MAXR
    lo = (r.clamp(MINR, MAXR) - MINR) / (MAXR - MINR) * (L - 2)
    hi = (r.clamp(MAXR, 1.0) - MAXR) / (1.0 - MAXR) + L - 2
    if "mip_slope_below_min_kept" in mut:
        lo = lo + (r - r.detach()) * (r < MINR).to(r.dtype) / (MAXR - MINR) * (L - 2)
    if "mip_slope_high_branch_1.25" in mut:
        hi = grad_scale(hi, 1.25)
    return torch.where(r < MAXR, lo, hi)


SRGB_KNEE = 0.0031308


def linear_to_srgb(x, mut=()):
    """pbr/shade.py:50-63.  mut: teeth tests only (module docstring): the slope below the knee halved."""
    eps = torch.finfo(torch.float32).eps
    if "srgb_slope_below_knee_halved" in mut:
        x = grad_scale(x, torch.where(x <= SRGB_KNEE, 0.5, 1.0).to(x.dtype))
    return torch.where(x <= 0.0031308, 323 / 25 * x, (211 * x.clamp(min=eps) ** (5 / 12) - 11) / 200)


def srgb_to_linear(x):
    """train.py:70-81 (gigs_shade_ext.out_linear)"""
    return torch.where(x <= 0.04045, 25 / 323 * x, ((x.clamp(min=0.04045) + 0.055) / 1.055) ** 2.4)


def aces(x):
    a, b, c, d, e = 2.51, 0.03, 2.43, 0.59, 0.14
    return (x * (a * x + b)) / (x * (c * x + d) + e)


def shade(normals, view_dirs, albedo, roughness, mask, occlusion, metallic, background, diffuse, specular, lut,
          tone=False, gamma=False, details=None, mut=()):
    """pbr/shade.py:108-241 on [H,W,*] tensors, evaluated in their dtype (float64: the reference; float32: the same formulae
    in the same order at the kernels' precision, the noise-floor comparator).  `details` (a dict) receives the per-pixel
    decisions: the cube_taps info of the diffuse lookup ("diffuse") and of every specular level ("spec", a list), l0, l1, lf,
    the LUT cell ("lut"), pre_clamp (the value the [0, 1] clamp sees), the three sRGB arguments ("srgb_args": render,
    diffuse_rgb, specular_rgb), F0, and "margin" [H,W]: the smallest distance of any decision of the pixel to its
    threshold (tap and LUT coordinates in texels, everything else relative).  `mut` is for the teeth tests only (module
    docstring): it names deliberate errors of the BACKWARD, values stay bit for bit; a checker of a kernel never passes it."""
    n, v = normals, view_dirs
    ref = 2.0 * (n * v).sum(-1, keepdim=True).clamp(min=0.0) * n - v
    T = torch.tensor([[0, -1, 0], [0, 0, 1], [-1, 0, 0]], dtype=n.dtype)
    nt, vt, rt = n @ T.T, v @ T.T, ref @ T.T
    want = details is not None
    d_info = {} if want else None
    dl = cube_sample(diffuse, nt, d_info, mut)
    if occlusion is not None:
        if "occlusion_missing_in_scatter" in mut:
            dl = grad_scale(dl, torch.where(occlusion > 0, 1.0 / occlusion.clamp(min=1e-30), torch.ones_like(occlusion)))
        dl = dl * occlusion
    drgb = dl * albedo
    nov = (nt * vt).sum(-1).clamp(1e-4, 1.0)
    lut_info = {} if want else None
    fg = lut_sample(lut, nov, roughness[..., 0], lut_info, mut)
    L = len(specular)
    lvl_raw = get_mip(roughness[..., 0], L, mut)
    lvl = lvl_raw.clamp(0, L - 1)
    l0 = torch.floor(lvl).detach().long().clamp(max=L - 1)
    l1 = (l0 + 1).clamp(max=L - 1)
    lf = (lvl - l0)[..., None]
    s_info = [{} for _ in specular] if want else [None] * L
    samples = torch.stack([cube_sample(s, rt, i, mut) for s, i in zip(specular, s_info)], 0)  # [L,H,W,3]
    s0 = torch.gather(samples, 0, l0[None, ..., None].expand(1, *l0.shape, 3))[0]
    s1 = torch.gather(samples, 0, l1[None, ..., None].expand(1, *l1.shape, 3))[0]
    blend = s0 * (1 - lf) + s1 * lf
    if "level_weights_exchanged" in mut:
        a, b = lf.detach(), 1 - lf.detach()
        blend = blend.detach() + (s0 - s0.detach()) * a + (s1 - s1.detach()) * b + (lf - lf.detach()) * (s1 - s0).detach()
    spec = torch.where((l1 != l0)[..., None], blend, s0)
    F0 = torch.full_like(albedo, 0.04) if metallic is None else (1.0 - metallic) * 0.04 + albedo * metallic
    if "metallic_gradient_full_albedo" in mut and metallic is not None:
        F0 = F0 + (metallic - metallic.detach()) * 0.04
    refl = F0 * fg[..., 0:1] + fg[..., 1:2]
    srgb = spec * refl
    render = drgb + srgb
    pre_clamp = aces(render) if tone else render
    render = pre_clamp.clamp(0, 1)
    if "clamp_passes_gradient" in mut:
        render = pre_clamp + (render - pre_clamp).detach()
    if want:
        rel = lambda x, t: ((x - t).abs() / t).detach()  # noqa: E731
        r = roughness[..., 0]
        frac = torch.where((lvl_raw <= 0) | (lvl_raw >= L - 1), torch.full_like(lvl, 0.5), _to_integer(lvl))
        m = torch.stack([d_info["margin"], lut_info["margin"], rel(r, MIP_MINR), rel(r, MIP_MAXR), rel(r, 1.0), frac.detach()], 0)
        for x in (nt, rt):
            a = x.detach().abs().sort(-1).values
            m = torch.cat([m, ((a[..., 2] - a[..., 1]) / a[..., 2])[None]], 0)
        used = torch.stack([i["margin"] for i in s_info], 0)
        m = torch.cat([m, torch.gather(used, 0, l0[None]), torch.gather(used, 0, l1[None])], 0)
        inside = mask[..., 0] if mask.dim() == nov.dim() + 1 else mask
        big = torch.full_like(nov, 1e30)
        m = torch.cat([m, torch.where(inside, rel(pre_clamp, 1.0).min(-1).values, big)[None]], 0)
        if gamma:
            m = torch.cat([m, torch.where(inside, rel(render, SRGB_KNEE).min(-1).values, big)[None],
                           rel(drgb, SRGB_KNEE).min(-1).values[None], rel(srgb, SRGB_KNEE).min(-1).values[None]], 0)
        details.update(diffuse=d_info, spec=s_info, lut=lut_info, l0=l0, l1=l1, lf=lf[..., 0].detach(), F0=F0.detach(),
                       pre_clamp=pre_clamp.detach(), srgb_args=(render.detach(), drgb.detach(), srgb.detach()),
                       roughness=r.detach(), n_dot_v=(n * v).sum(-1).detach(), margin=m.min(0).values)
    if gamma:
        render, drgb, srgb = linear_to_srgb(render, mut), linear_to_srgb(drgb, mut), linear_to_srgb(srgb, mut)
    bg = torch.zeros_like(render) if background is None else background
    render = torch.where(mask, render, bg)
    return render, drgb, srgb, dl


def restate_inputs(g):
    """The G-buffer (numpy, keys normals, view_dirs, albedo, roughness, mask, occlusion | None, metallic | None) with the
    inputs the restatement cannot follow restated, so that it computes what the kernels do:
      * a pixel whose normal is 0 (the G-buffer's median filter leaves a few inside the mask) has no diffuse tap in the
        kernel, so its diffuse light is 0 and nothing is scattered, while the restatement would look the zero direction up
        as NaN taps: it gets the normal -v and occlusion 0 (n.v < 0 keeps the reflected direction -v and N.V at its clamp,
        as in the kernel);
      * a pixel outside the mask whose materials are not finite gets finite ones (its render gradient is ignored, and
        0 * NaN would be NaN in the scatter).
    tests/test_gpu_shade_bwd_scatter.float64_light_grads keeps an older, coarser statement of the second rule: it replaces
    the materials of EVERY masked-out pixel.  That is equivalent there (only g_render is given, which such a pixel ignores)
    and wrong here: g_diffuse_rgb, g_specular_rgb and g_diffuse_light flow through masked-out pixels with the materials
    they have, so only values the restatement cannot evaluate may be replaced.  That test is left as it was; a later
    change can make it call this function."""
    g = dict(g)
    out = ~np.asarray(g["mask"], bool).reshape(g["normals"].shape[:-1] + (1,))
    flat = ~(g["normals"] != 0).any(-1, keepdims=True)
    g["normals"] = np.where(flat, -g["view_dirs"], g["normals"]).astype(g["normals"].dtype)
    if flat.any():
        occ = np.ones(flat.shape, g["normals"].dtype) if g.get("occlusion") is None else g["occlusion"]
        g["occlusion"] = np.where(flat, 0, occ).astype(occ.dtype)
    for k, fill in (("albedo", 0.5), ("roughness", 0.5), ("metallic", 0.0), ("occlusion", 1.0)):
        if g.get(k) is not None:
            bad = out & ~np.isfinite(g[k]).all(-1, keepdims=True)
            g[k] = np.where(bad, np.asarray(fill, g[k].dtype), g[k])
    return g


def as_dtype(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a, np.float64), dtype=torch.float64).to(dtype)


def shade_with_grads(g, diffuse, specular, lut, grads, tone=False, gamma=False, ext=None, dtype=DT, mut=(), background=None):
    """gigs_shade_fwd_ex / gigs_shade_bwd_ex restated: the forward of `shade` on restate_inputs(g) and autograd of
        sum_k <out_k, g_k>  (grads: g_render, g_diffuse_rgb, g_specular_rgb, g_diffuse_light, any may be None)
    evaluated in `dtype`, with the gigs_shade_ext terms when ext (a dict) is given: roughness = raw * rough_scale +
    rough_bias (d_roughness is w.r.t. raw: autograd multiplies by the scale), g_scale on g_render and on mul_a, d_albedo +=
    mul_a * mul_b, add_r / add_m on the remapped roughness / metallic gradient, and the two lamb lines -/+ lamb_mask /
    lamb_cnt * 0.001 * g_scale.  -> dict: the four planes, roughness_used, details, and d_albedo, d_roughness, d_metallic
    (None without metallic), d_diffuse, d_spec (list), numpy float64."""
    ext = ext or {}
    g = restate_inputs(g)
    t = lambda a: as_dtype(a, dtype)  # noqa: E731
    leaf = lambda a: None if a is None else t(a).requires_grad_(True)  # noqa: E731
    albedo, raw, metallic = leaf(g["albedo"]), leaf(g["roughness"]), leaf(g.get("metallic"))
    dif, spec = leaf(diffuse), [leaf(s) for s in specular]
    rough = raw * ext.get("rough_scale", 1.0) + ext.get("rough_bias", 0.0) if ext else raw
    mask = torch.from_numpy(np.ascontiguousarray(g["mask"], dtype=bool).reshape(raw.shape))
    details = {}
    outs = shade(t(g["normals"]), t(g["view_dirs"]), albedo, rough, mask, t(g.get("occlusion")), metallic, t(background),
                 dif, spec, t(lut), tone=tone, gamma=gamma, details=details, mut=mut)
    gscale = float(ext.get("g_scale", 1.0))
    loss = dif.sum() * 0.0
    for o, k in zip(outs, ("g_render", "g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light")):
        if grads.get(k) is not None:
            loss = loss + (o * (t(grads[k]) * gscale if k == "g_render" else t(grads[k]))).sum()
    if ext.get("mul_a") is not None:
        loss = loss + (albedo * (t(ext["mul_a"]) * gscale * t(ext["mul_b"]))).sum()
    add_r = torch.zeros_like(raw[..., 0])
    add_m = torch.zeros_like(raw[..., 0])
    if ext.get("add_r") is not None:
        add_r = add_r + t(ext["add_r"])
    if ext.get("add_m") is not None:
        add_m = add_m + t(ext["add_m"])
    if ext.get("lamb_mask") is not None:
        lamb = t(ext["lamb_mask"]) / float(ext["lamb_cnt"]) * (0.001 * gscale)
        add_r, add_m = add_r - lamb, add_m + lamb
    loss = loss + (rough[..., 0] * add_r).sum()
    if metallic is not None:
        loss = loss + (metallic[..., 0] * add_m).sum()
    loss.backward()
    np64 = lambda x: None if x is None else x.detach().to(DT).numpy()  # noqa: E731
    zero = lambda x: None if x is None else (np64(x.grad) if x.grad is not None else np.zeros(tuple(x.shape)))  # noqa: E731
    res = dict(render_rgb=np64(outs[0]), diffuse_rgb=np64(outs[1]), specular_rgb=np64(outs[2]), diffuse_light=np64(outs[3]),
               roughness_used=np64(rough), details=details, d_albedo=zero(albedo), d_roughness=zero(raw),
               d_metallic=zero(metallic), d_diffuse=zero(dif), d_spec=[zero(s) for s in spec])
    return res


# ---- cubemap filters (dense float64 restatement of RU/cubemap.cu) ---------------------------
def texel_dirs(N):
    s, y, x = torch.meshgrid(torch.arange(6), torch.arange(N), torch.arange(N), indexing="ij")
    fx = 2.0 * ((x.to(DT) + 0.5) / N) - 1.0
    fy = 2.0 * ((y.to(DT) + 0.5) / N) - 1.0
    d = cube_dir_raw(fx, fy, s)
    return (d / d.norm(dim=-1, keepdim=True)).reshape(-1, 3)


def pixel_areas(N):
    H = N // 2
    i = (torch.arange(N) - H).abs().to(DT)
    a = torch.atan((i + 1) / H) - torch.atan(i / H)
    return (a[:, None] * a[None, :])[None].expand(6, N, N).reshape(-1)


def diffuse_cubemap(cubemap):
    N = cubemap.shape[1]
    d = texel_dirs(N)
    w = (d @ d.T).clamp(0.0, 0.999) * pixel_areas(N)[None, :] / 3.141592
    return (w @ cubemap.reshape(-1, 3)).reshape(6, N, N, 3)


def bounds_mask(bounds):
    """[out, in] membership of texel `in` in the per-face AABB stored for texel `out`
    (RU/cubemap.cu:181-244; the AABBs are discrete structure taken from the C oracle)."""
    N = bounds.shape[1]
    b = torch.as_tensor(np.asarray(bounds)).reshape(6 * N * N, 6, 4).long()
    s, y, x = torch.meshgrid(torch.arange(6), torch.arange(N), torch.arange(N), indexing="ij")
    s, y, x = s.reshape(-1), y.reshape(-1), x.reshape(-1)
    bb = b[:, s, :]  # [out, in, 4]
    return (x[None] >= bb[..., 0]) & (x[None] <= bb[..., 1]) & (y[None] >= bb[..., 2]) & (y[None] <= bb[..., 3])


def specular_cubemap_rgbw(cubemap, roughness, cos_cutoff, bounds=None):
    N = cubemap.shape[1]
    d = texel_dirs(N)
    dp = d @ d.T  # [out, in]
    if bounds is not None:
        dp = torch.where(bounds_mask(bounds), dp, torch.full_like(dp, -2.0))
    alphaSqr = roughness ** 4
    Hh = d[:, None, :] + d[None, :, :]
    Hh = Hh / Hh.norm(dim=-1, keepdim=True).clamp(min=1e-30)
    vdh = (d[:, None, :] * Hh).sum(-1).clamp(0, 1)
    dd = (vdh * alphaSqr - vdh) * vdh + 1.0
    ndf = alphaSqr / (dd * dd * math.pi)
    w = torch.where(dp >= cos_cutoff, dp.clamp(min=0) * ndf * pixel_areas(N)[None, :] / 4.0, torch.zeros_like(dp))
    rgb = w @ cubemap.reshape(-1, 3)
    return torch.cat([rgb, w.sum(-1, keepdim=True)], -1).reshape(6, N, N, 4)


def cubemap_mip_bwd(dout):
    """pbr/light.py:62-79 with the sampling rule above. dout [6,r,r,3] -> [6,2r,2r,3]"""
    r = dout.shape[1]
    res = 2 * r
    out = torch.zeros(6, res, res, 3, dtype=DT)
    lin = torch.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, dtype=DT)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    for s in range(6):
        d = cube_dir_raw(gx, gy, torch.full_like(gx, s).long())
        d = d / d.norm(dim=-1, keepdim=True)
        out[s] = cube_sample(dout * 0.25, d)
    return out


def to64(a):
    return torch.tensor(np.asarray(a, np.float64), dtype=DT)
