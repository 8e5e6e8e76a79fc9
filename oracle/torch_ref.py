"""Independent PyTorch (CPU, float64) restatement of the rasterizer FORWARD, used only to
check the hand-written BACKWARD of the oracle (and through it the HIP backward) by autograd.

TEST INFRASTRUCTURE ONLY (see oracle/gigs_oracle.cpp header).

It is written from the maths, not from the kernels' instruction order: projection, EWA
covariance J W Sigma W^T J^T + 0.3 I, conic = inverse, SH colour, front-to-back alpha
blending.  The discrete structure (which Gaussians a tile sees, and in which order) is taken
from the oracle's `point_list` / `ranges`, because binning is integer work that has its own
bit-exact tests.

The reference's backward is NOT the exact gradient of its forward; the restatement encodes
the documented deviations so that autograd reproduces what the reference computes
(R/cuda_rasterizer/backward.cu):
  * normal / albedo / roughness / metallic / depth planes do not feed dL_dalpha (:580-590):
    their blend weights are detached;
  * the depth gradient ignores the forward's division by the accumulated opacity (:590 vs
    forward.cu:619): the surrogate plane is sum_i w_i * z_i;
  * dL_dnormal is zeroed on the image border (:497-501);
  * when the projected centre is clamped to 1.3 * tan(fov) the clamped coordinate is treated
    as independent of t.z and dL_dt{x,y} is zeroed (:177-178, :264-266);
  * SH colours clamped at 0 pass no gradient (:30-35); the quaternion is used un-normalised;
  * the 0.99 alpha cap is applied to the value only: the backward multiplies dL_dalpha by the
    opacity and G whether or not the cap was hit (:545, :609), so the cap passes the gradient;
  * dL_dscale is the gradient with respect to the MODIFIED scale mod * s: the chain rule's
    factor scale_modifier is left out (:300, :327-330);
  * the conic's backward divides by det^2 + 1e-7 instead of det^2 (:205): the gradient that
    reaches the 2D covariance is the exact one times det^2 / (det^2 + 1e-7).

Each deviation has a name in DEVIATIONS and can be switched off (`off=`), which yields a WRONG
reference on purpose: tests/test_backward_f64_cpu.py uses them to show that a comparison with
this module tells the encoded branch from its absence.  Precomputed colours / 3D covariances
are differentiable leaves like the others, culled Gaussians are kept out of the maths (their
gradients are zero by construction), and `book` carries the bookkeeping the per-Gaussian
tests assert their branch populations from.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import numpy as np
import torch

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
      -0.4570457994644658, 1.445305721320277, -0.5900435899266435]


def _sh_color(deg, sh, dirs):
    """sh: [P, M, 3]; dirs: [P, 3] unit. Real SH basis as in forward.cu:22-80."""
    x, y, z = dirs[:, 0:1], dirs[:, 1:2], dirs[:, 2:3]
    res = C0 * sh[:, 0]
    if deg > 0:
        res = res - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2 * zz - xx - yy) * sh[:, 6]
               + C2[3] * xz * sh[:, 7] + C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        res = (res + C3[0] * y * (3 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10]
               + C3[2] * y * (4 * zz - xx - yy) * sh[:, 11] + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[:, 12]
               + C3[4] * x * (4 * zz - xx - yy) * sh[:, 13] + C3[5] * z * (xx - yy) * sh[:, 14]
               + C3[6] * x * (xx - 3 * yy) * sh[:, 15])
    return res + 0.5


def _quat_R(q):
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([
        1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(-1, 3, 3)


DEVIATIONS = ("sh_clamp", "fov_clamp", "detach_weights", "depth_surrogate", "border_normal", "raw_quaternion",
              "alpha_cap", "cap_passes_grad", "conic_eps", "scale_modifier_grad")


class _ScaleGrad(torch.autograd.Function):
    """Identity whose backward multiplies the incoming gradient by `f`."""

    @staticmethod
    def forward(ctx, x, f):
        ctx.save_for_backward(f)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        (f,) = ctx.saved_tensors
        return g * f, None


def render_with_grads(inp: Dict[str, np.ndarray], cam: Dict, bg: np.ndarray, point_list: np.ndarray,
                      ranges: np.ndarray, visible: np.ndarray, pix_grads: Dict[str, np.ndarray],
                      scale_modifier: float = 1.0, colors_precomp: Optional[np.ndarray] = None,
                      cov3D_precomp: Optional[np.ndarray] = None, off: Sequence[str] = ()) -> Dict[str, np.ndarray]:
    """Returns the forward planes and d(sum_k <plane_k, pix_grads[k]>)/d(input) for every input.

    `visible` = radii > 0 of the binning that produced `point_list` / `ranges`; `off` = names of DEVIATIONS to leave out.
    Besides d_<input> the result holds d_colors (w.r.t. the per-Gaussian colour that is blended) and d_cov3D (w.r.t. the six
    stored entries of the 3D covariance, an off-diagonal one standing for both of its places) in every mode."""
    dt = torch.float64
    on = {k: (k not in off) for k in DEVIATIONS}
    assert set(off) <= set(DEVIATIONS), off
    W, H = cam["image_width"], cam["image_height"]
    names = ["means3D", "opacities", "normal", "albedo", "roughness", "metallic"]
    names += ["scales", "rotations"] if cov3D_precomp is None else []
    names += ["shs"] if colors_precomp is None else []
    t = {k: torch.tensor(np.asarray(inp[k], np.float64), dtype=dt, requires_grad=True) for k in names}
    if cov3D_precomp is not None:
        t["cov3D_precomp"] = torch.tensor(np.asarray(cov3D_precomp, np.float64), dtype=dt, requires_grad=True)
    if colors_precomp is not None:
        t["colors_precomp"] = torch.tensor(np.asarray(colors_precomp, np.float64), dtype=dt, requires_grad=True)
    P = t["means3D"].shape[0]
    deg = int(inp["sh_degree"])
    vm = torch.tensor(np.asarray(cam["viewmatrix"], np.float64))
    pm = torch.tensor(np.asarray(cam["projmatrix"], np.float64))
    campos = torch.tensor(np.asarray(cam["campos"], np.float64))
    tanx, tany = cam["tanfovx"], cam["tanfovy"]
    fx, fy = W / (2.0 * tanx), H / (2.0 * tany)
    ndc_off = torch.zeros(P, 2, dtype=dt, requires_grad=True)  # receives "means2D.grad"
    vis = torch.tensor(np.asarray(visible, bool))

    # culled Gaussians (near plane, empty tile rectangle) never reach a pixel: a benign stand-in position one unit in front
    # of the camera keeps 1/t.z finite, and torch.where gives their inputs the exact zero gradient
    benign = (torch.tensor([0.0, 0.0, 1.0, 1.0], dtype=dt) @ torch.linalg.inv(vm))[:3]
    means = torch.where(vis[:, None], t["means3D"], benign[None])
    hom = torch.cat([means, torch.ones(P, 1, dtype=dt)], dim=1)
    pv = hom @ vm  # [P,4] view space (row-vector convention)
    ph = hom @ pm
    pw = 1.0 / (ph[:, 3] + 1e-7)
    ndc = ph[:, :2] * pw[:, None] + ndc_off
    pix = torch.stack([((ndc[:, 0] + 1.0) * W - 1.0) * 0.5, ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5], dim=1)

    # 3D covariance
    if cov3D_precomp is None:
        q = t["rotations"]
        if not on["raw_quaternion"]:
            q = q / q.norm(dim=1, keepdim=True)
        R = _quat_R(q)
        sc = t["scales"]
        if on["scale_modifier_grad"]:
            sc = _ScaleGrad.apply(sc, torch.tensor(1.0 / scale_modifier, dtype=dt))
        S = torch.diag_embed(scale_modifier * sc)
        Mm = R @ S
        Sigma = Mm @ Mm.transpose(1, 2)
    else:
        c6 = t["cov3D_precomp"]
        Sigma = torch.stack([c6[:, 0], c6[:, 1], c6[:, 2], c6[:, 1], c6[:, 3], c6[:, 4],
                             c6[:, 2], c6[:, 4], c6[:, 5]], dim=-1).reshape(P, 3, 3)
    Sigma.retain_grad()

    # EWA projection with the reference's clamp semantics
    tz = pv[:, 2]
    limx, limy = 1.3 * tanx, 1.3 * tany
    rx, ry = pv[:, 0] / tz, pv[:, 1] / tz
    cl_x = (rx < -limx) | (rx > limx)
    cl_y = (ry < -limy) | (ry > limy)
    cx, cy = rx.clamp(-limx, limx) * tz, ry.clamp(-limy, limy) * tz
    if on["fov_clamp"]:
        cx, cy = cx.detach(), cy.detach()
    tx = torch.where(cl_x, cx, pv[:, 0])
    ty = torch.where(cl_y, cy, pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz),
                     zero, fy / tz, -(fy * ty) / (tz * tz)], dim=-1).reshape(P, 2, 3)
    Rw2c = vm[:3, :3].T  # column-vector rotation
    T = J @ Rw2c
    cov = T @ Sigma @ T.transpose(1, 2)
    a = cov[:, 0, 0] + 0.3
    b = cov[:, 0, 1]
    c = cov[:, 1, 1] + 0.3
    if on["conic_eps"]:
        d2 = (a * c - b * b).detach() ** 2
        f = d2 / (d2 + 1e-7)
        a, b, c = _ScaleGrad.apply(a, f), _ScaleGrad.apply(b, f), _ScaleGrad.apply(c, f)
    det = a * c - b * b
    conic = torch.stack([c / det, -b / det, a / det], dim=1)

    # colour
    sh_clamped = np.zeros((P, 3), bool)
    if colors_precomp is None:
        dirs = means - campos[None]
        dirs = dirs / dirs.norm(dim=1, keepdim=True)
        raw = _sh_color(deg, t["shs"], dirs)
        rgb = torch.clamp_min(raw, 0.0)
        sh_clamped = (raw.detach() < 0).numpy() & np.asarray(visible, bool)[:, None]
        if not on["sh_clamp"]:
            rgb = raw + (rgb - raw).detach()
    else:
        rgb = t["colors_precomp"] * 1.0
    rgb.retain_grad()

    opac = t["opacities"][:, 0]
    zview = pv[:, 2]

    g = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in pix_grads.items()}
    gn = g["normal"].clone()
    if on["border_normal"]:
        gn[:, 0, :] = 0
        gn[:, -1, :] = 0
        gn[:, :, 0] = 0
        gn[:, :, -1] = 0
    gmat = torch.cat([g["albedo"], g["roughness"], g["metallic"]], dim=0)  # [5,H,W]

    gx = (W + 15) // 16
    gy = (H + 15) // 16
    planes = {k: torch.zeros(n, H, W, dtype=dt) for k, n in
              [("color", 3), ("opacity", 1), ("depth_sur", 1), ("normal", 3), ("albedo", 3),
               ("roughness", 1), ("metallic", 1)]}
    n_contrib = np.zeros((H, W), np.int64)
    bgt = torch.tensor(np.asarray(bg, np.float64))
    mats = torch.cat([t["albedo"], t["roughness"], t["metallic"]], dim=1)  # [P,5]
    pl = torch.tensor(np.asarray(point_list, np.int64))
    loss = torch.zeros((), dtype=dt)
    contributes = np.zeros(P, bool)   # the Gaussian is blended into at least one pixel
    candidate = np.zeros(P, bool)     # ... passes the power / alpha tests somewhere (possibly behind a terminated pixel)
    capped = np.zeros(P, bool)        # ... is blended somewhere with its alpha cut to 0.99
    on_border = np.zeros(P, bool)     # ... is blended into a pixel of the image border
    book = dict(cap_pairs=0, terminated_pixels=0, margin_power=np.inf, margin_alpha=np.inf, margin_T=np.inf,
                list_lengths=[], survivors=[])
    for tile in range(gx * gy):
        ty_, tx_ = divmod(tile, gx)
        x0, y0 = tx_ * 16, ty_ * 16
        x1, y1 = min(x0 + 16, W), min(y0 + 16, H)
        lo, hi = int(ranges[2 * tile]), int(ranges[2 * tile + 1])
        n = hi - lo
        book["list_lengths"].append(n)
        hh, ww = y1 - y0, x1 - x0
        sl = (slice(None), slice(y0, y1), slice(x0, x1))
        if n == 0:
            planes["color"][sl] = bgt[:, None, None]
            continue
        ys, xs = torch.meshgrid(torch.arange(y0, y1, dtype=dt), torch.arange(x0, x1, dtype=dt), indexing="ij")
        ys, xs = ys.reshape(1, -1), xs.reshape(1, -1)
        idx = pl[lo:hi]
        dx = pix[idx, 0:1] - xs  # [n, npix]
        dy = pix[idx, 1:2] - ys
        cA, cB, cC = conic[idx, 0:1], conic[idx, 1:2], conic[idx, 2:3]
        power = -0.5 * (cA * dx * dx + cC * dy * dy) - cB * dx * dy
        a_raw = opac[idx, None] * torch.exp(power)
        if not on["alpha_cap"]:
            alpha = a_raw
        elif on["cap_passes_grad"]:
            alpha = a_raw + (torch.clamp_max(a_raw, 0.99) - a_raw).detach()
        else:
            alpha = torch.clamp_max(a_raw, 0.99)
        with torch.no_grad():
            cand = (power <= 0) & (alpha >= 1.0 / 255.0)
        om = torch.where(cand, 1 - alpha, torch.ones_like(alpha))
        Tincl = torch.cumprod(om, dim=0)
        Tbefore = torch.cat([torch.ones(1, om.shape[1], dtype=dt), Tincl[:-1]], dim=0)
        test_T = Tbefore * (1 - alpha)
        with torch.no_grad():
            term = cand & (test_T < 0.0001)
            nterm = torch.cumsum(term.to(torch.int64), dim=0)
            ok = cand & (nterm == 0)
            reached = (nterm - term.to(torch.int64)) == 0  # the pixel was still walking when it met this instance
        w = torch.where(ok, alpha * Tbefore, torch.zeros_like(alpha))
        T_final = torch.prod(torch.where(ok, 1 - alpha, torch.ones_like(alpha)), dim=0)
        wd = w.detach() if on["detach_weights"] else w
        col = w.transpose(0, 1) @ rgb[idx] + T_final[:, None] * bgt[None]  # [npix,3]
        opa = w.sum(0)
        nrm = wd.transpose(0, 1) @ t["normal"][idx]
        mat = wd.transpose(0, 1) @ mats[idx]
        dep = wd.transpose(0, 1) @ zview[idx]
        if not on["depth_surrogate"]:
            dep = dep / torch.where(opa > 0, opa, torch.ones_like(opa))

        def tile_of(x):
            return x[sl].reshape(x.shape[0], -1).transpose(0, 1)

        loss = (loss + (col * tile_of(g["color"])).sum() + (opa * tile_of(g["opacity"])[:, 0]).sum()
                + (dep * tile_of(g["depth"])[:, 0]).sum() + (nrm * tile_of(gn)).sum() + (mat * tile_of(gmat)).sum())
        with torch.no_grad():
            planes["color"][sl] = col.transpose(0, 1).reshape(3, hh, ww)
            planes["opacity"][sl] = opa.reshape(1, hh, ww)
            planes["depth_sur"][sl] = dep.reshape(1, hh, ww)
            planes["normal"][sl] = nrm.transpose(0, 1).reshape(3, hh, ww)
            planes["albedo"][sl] = mat[:, :3].transpose(0, 1).reshape(3, hh, ww)
            planes["roughness"][sl] = mat[:, 3].reshape(1, hh, ww)
            planes["metallic"][sl] = mat[:, 4].reshape(1, hh, ww)
            pos1 = torch.arange(1, n + 1, dtype=torch.int64)[:, None]
            n_contrib[y0:y1, x0:x1] = (pos1 * ok).max(dim=0).values.reshape(hh, ww).numpy()
            # ---- bookkeeping
            book["cap_pairs"] += int((ok & (a_raw > 0.99)).sum())
            book["terminated_pixels"] += int(term.any(dim=0).sum())
            mag = 0.5 * (cA.abs() * dx * dx + cC.abs() * dy * dy) + (cB * dx * dy).abs()
            r = reached
            if bool(r.any()):
                book["margin_power"] = min(book["margin_power"], float((power.abs() / mag)[r].min()))
            r2 = reached & (power <= 0)
            if bool(r2.any()):
                book["margin_alpha"] = min(book["margin_alpha"], float(((alpha - 1.0 / 255.0).abs() * 255.0)[r2].min()))
            r3 = reached & cand
            if bool(r3.any()):
                book["margin_T"] = min(book["margin_T"], float(((test_T - 1e-4).abs() / 1e-4)[r3].min()))
            idn = idx.numpy()
            contributes[idn[ok.any(dim=1).numpy()]] = True
            candidate[idn[cand.any(dim=1).numpy()]] = True
            capped[idn[(ok & (a_raw > 0.99)).any(dim=1).numpy()]] = True
            edge = ((xs == 0) | (xs == W - 1) | (ys == 0) | (ys == H - 1)).reshape(-1)
            on_border[idn[ok[:, edge].any(dim=1).numpy()]] = True
            # survivors per (8x8 quadrant, chunk of 64 counted from the back of the list): what the backward walk pairs up
            qid = ((ys.reshape(-1) - y0) // 8).to(torch.int64) * 2 + ((xs.reshape(-1) - x0) // 8).to(torch.int64)
            chunk = (n - 1 - np.arange(n)) // 64
            for qd in range(4):
                sel = qid == qd
                if not bool(sel.any()):
                    continue
                hit = ok[:, sel].any(dim=1).numpy()
                for ck in range(int(chunk.max()) + 1):
                    book["survivors"].append((tile, qd, ck, int(hit[chunk == ck].sum())))

    loss.backward()

    def grad(v):
        return v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))

    out = {("d_" + k): grad(v) for k, v in t.items()}
    out["d_means2D"] = grad(ndc_off)
    out["d_colors"] = grad(rgb)
    sg = grad(Sigma)
    out["d_cov3D"] = np.stack([sg[:, 0, 0], sg[:, 0, 1] + sg[:, 1, 0], sg[:, 0, 2] + sg[:, 2, 0], sg[:, 1, 1],
                               sg[:, 1, 2] + sg[:, 2, 1], sg[:, 2, 2]], axis=1)
    if cov3D_precomp is not None:
        out["d_scales"], out["d_rotations"] = np.zeros((P, 3)), np.zeros((P, 4))
    if colors_precomp is not None:
        out["d_shs"] = np.zeros((P, 0, 3))
    for k, v in planes.items():
        out[k] = v.detach().numpy()
    out["n_contrib"] = n_contrib
    visn = np.asarray(visible, bool)
    clx, cly = cl_x.numpy() & visn, cl_y.numpy() & visn
    out["clamped_any"] = bool((clx | cly).any())
    book.update(sh_clamped=sh_clamped, fov_clamped_x=clx, fov_clamped_y=cly, contributes=contributes, capped=capped,
                on_border=on_border, behind_terminated=candidate & ~contributes, margin=min(book["margin_power"], book["margin_alpha"],
                                                                     book["margin_T"]))
    out["book"] = book
    return out
