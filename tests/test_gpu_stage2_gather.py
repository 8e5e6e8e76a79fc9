"""The fused stage-2 node's two gathered / folded kernels against the sequences they replace.

  * gigs_stage2_loss_gather (csrc/stage2.hip: the loss, its unit gradient planes and the four sums without global atomics
    and without cleared buffers) against gigs_stage2_loss_fwd_grad on the same inputs;
  * gigs_shade_fwd_post (csrc/shade.hip: the G-buffer post-processing inside the shade forward) against gigs_gbuffer_post
    followed by gigs_shade_fwd_ex;
  * stage2_fused._Stage2Fused with the switches stage2_gather / shade_post_fused on and off.

Sizes: 5 x 7 (smaller than any tile: every pixel at a border), 9 x 70 (ragged both ways, across the 64-pixel tile edge and a
tile-row edge), 40 x 130 (a few tiles).

Bounds.  render_rgb, d_direct_unit and every plane of the post + shade are the same expressions on the same operands: bit
for bit.  A texel of d_irr_unit is the sum of the n <= 9 terms +-t, t = |gs * d lin2srgb(irr)|, of the neighbours whose
median selected it; with n <= 1 there is one order, so bit for bit; otherwise two orders of n terms of magnitude t
differ by at most 2 (n - 1) 2^-24 n t (each of the n - 1 roundings of either order is at most 2^-24 of a partial sum
<= n t).  n comes from the selection repeated on the host on the library's own lin2srgb values (read back through the
loss entry from an image of 3 x 3 replicated texels, whose block centres have constant windows); t from the sRGB
derivative in float64 (its fp32 rounding moves the bound by 1e-7 of itself).  loss / acc4: the deviation from a float64 sum
of the same fp32 terms must not exceed twice the atomic entry's plus one ulp (the atomic entry's own order is not fixed).
The light gradients of the node come out of the shade backward's atomics from bit-identical operands in both settings:
1e-4 of the peak, the bound tests/test_gpu_shade_bwd_scatter.py sets for two orders of those sums."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import scenes  # noqa: F401  (the package path)
from helpers import set_options

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(5, 7), (9, 70), (40, 130)]
N_ACC = 4 + 4 * 256  # GIGS_STAGE2_ACC_FLOATS


def p(t):
    return None if t is None else t.data_ptr()


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- loss ---------------------------------------------------------------------------------------------------------
def loss_old(x, grad=True):
    import gigs_lib
    lib = gigs_lib.lib()
    H, W = x["direct"].shape[1:]
    o = dict(rgb=torch.empty(3, H, W, device=DEV), acc=torch.empty(N_ACC, device=DEV), loss=torch.empty(1, device=DEV),
             du=torch.empty(3, H, W, device=DEV), iu=torch.empty(3, H, W, device=DEV))
    a = (H, W, p(x["direct"]), p(x["irr"]), p(x["gt"]), p(x["mask"]), p(x["rough"]), p(x["metal"]), p(o["rgb"]), p(o["acc"]),
         p(o["loss"]))
    if grad:
        gigs_lib.check(lib.gigs_stage2_loss_fwd_grad(*a, p(o["du"]), p(o["iu"]), stream()), "loss_fwd_grad")
    else:
        gigs_lib.check(lib.gigs_stage2_loss_fwd(*a, stream()), "loss_fwd")
    torch.cuda.synchronize()
    o["acc"] = o["acc"][:4].clone()
    return o


def loss_new(x):
    """gigs_stage2_loss_gather into NaN-filled outputs and scratch: it must not rely on a cleared buffer."""
    import gigs_lib
    lib = gigs_lib.lib()
    H, W = x["direct"].shape[1:]
    nan = float("nan")
    nbytes = int(lib.gigs_stage2_loss_gather_scratch_bytes(H, W))
    assert nbytes > 0 and nbytes % 16 == 0
    scratch = torch.full((nbytes // 4,), nan, device=DEV)
    o = dict(rgb=torch.full((3, H, W), nan, device=DEV), acc=torch.full((4,), nan, device=DEV),
             loss=torch.full((1,), nan, device=DEV), du=torch.full((3, H, W), nan, device=DEV),
             iu=torch.full((3, H, W), nan, device=DEV))
    gigs_lib.check(lib.gigs_stage2_loss_gather(H, W, p(x["direct"]), p(x["irr"]), p(x["gt"]), p(x["mask"]), p(x["rough"]),
                                               p(x["metal"]), p(o["rgb"]), p(o["acc"]), p(o["loss"]), p(o["du"]), p(o["iu"]),
                                               p(scratch), nbytes, stream()), "loss_gather")
    torch.cuda.synchronize()
    return o


def loss_inputs(H, W, with_nan):
    g = torch.Generator(device="cpu").manual_seed(1000 * H + W)
    rnd = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    direct, irr, gt = rnd(3, H, W), rnd(3, H, W) * 0.3, rnd(3, H, W)
    irr[:, H // 2:H // 2 + 3, W // 2:W // 2 + 4] = 0.2   # a constant patch: ties, the first-tap rule
    irr[:, 0:2, W - 3:W] = 0.0                            # zeros: ties with the padding taps as well
    irr[:, H - 2:H, 0:3] = -0.01 - 0.05 * rnd(3, 2, 3)    # negative values in a corner
    irr[:, 0, 1:5] = -0.02                                # top border: 3 negative taps, 3 padding zeros, 3 positive -> the median is a padding zero
    if with_nan:
        irr[0, 1:4, 0:3] = float("nan")                   # a NaN 3 x 3 patch (channel 0) and a NaN pixel (channel 1); see below
        irr[1, H - 1, W - 1] = float("nan")
        direct[2, H // 2, 1] = float("nan")               # diff is NaN: sign 0, nothing routed, the L1 sum and the loss are NaN
    x = dict(direct=direct, irr=irr, gt=gt, mask=(rnd(1, H, W) > 0.3).float(), rough=rnd(1, H, W), metal=rnd(1, H, W))
    x = {k: v.to(DEV).contiguous() for k, v in x.items()}
    # pixels whose ground truth IS the rendered value: diff == 0, sign 0, nothing routed
    rgb = loss_old(x)["rgb"]
    hit = torch.zeros(3, H, W, dtype=torch.bool, device=DEV)
    hit[:, ::3, ::5] = True
    hit &= torch.isfinite(rgb)
    x["gt"] = torch.where(hit, rgb, x["gt"]).contiguous()
    return x, int(hit.sum())


def device_srgb(irr):
    """lin2srgb(irr) as the library computes it, bit for bit: every texel replicated 3 x 3, so that the window of a block's
    centre is constant and render_rgb = 0 + median = the value itself."""
    _, H, W = irr.shape
    up = irr.repeat_interleave(3, 1).repeat_interleave(3, 2).contiguous()
    z3, z1 = torch.zeros_like(up), torch.zeros(1, 3 * H, 3 * W, device=DEV)
    o = loss_old(dict(direct=z3, irr=up, gt=z3, mask=z1, rough=z1, metal=z1), grad=False)
    return o["rgb"][:, 1::3, 1::3].cpu()


def selection_counts(S, sgn):
    """S [3,H,W]: the sRGB plane; sgn: d_direct_unit.  -> n [3,H,W] (contributions a texel receives), the number of
    gradients dropped on a padding tap."""
    _, H, W = S.shape
    Sp = F.pad(S, (1, 1, 1, 1))
    taps = torch.stack([Sp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)], -1)  # row-major taps
    has_nan = taps.isnan().any(-1)
    med = taps.sort(-1).values[..., 4]
    first = ((taps == med[..., None]).cumsum(-1) == 0).sum(-1)  # index of the first tap equal to the median
    active = ~has_nan & (sgn != 0) & (first < 9)
    c, y, x = torch.meshgrid(torch.arange(3), torch.arange(H), torch.arange(W), indexing="ij")
    ty, tx = y + first // 3 - 1, x + first % 3 - 1
    inside = (ty >= 0) & (ty < H) & (tx >= 0) & (tx < W)
    sel = active & inside
    n = torch.zeros(3, H, W, dtype=torch.int64)
    n.index_put_((c[sel], ty[sel], tx[sel]), torch.ones(int(sel.sum()), dtype=torch.int64), accumulate=True)
    return n, int((active & ~inside).sum())


def srgb_slope64(irr):
    x = irr.double()
    eps = 1.1920929e-07
    pw = 211.0 * (5.0 / 12.0) * x.clamp_min(eps) ** (5.0 / 12.0) / x.clamp_min(eps) / 200.0
    d = torch.where(irr <= np.float32(0.0031308), torch.full_like(x, 323.0 / 25.0), torch.where(x >= eps, pw, torch.zeros_like(x)))
    return d.nan_to_num(0.0)


def sums64(x, rgb):
    """The four sums in float64 of the fp32 terms the kernels form, and the loss."""
    H, W = rgb.shape[1:]
    m = x["mask"].cpu()
    acc = [(rgb.cpu() - x["gt"].cpu()).abs().double().sum(), ((1.0 - x["rough"].cpu()) * m).double().sum(),
           (x["metal"].cpu() * m).double().sum(), m.double().sum()]
    acc = [float(a) for a in acc]
    loss = acc[0] / (3.0 * H * W) + float(np.float32(0.001)) * (acc[1] / acc[3] + acc[2] / acc[3])
    return acc, loss


@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("H,W", SIZES)
def test_loss_gather_matches_the_atomic_entry(H, W, with_nan):
    x, n_zero_diff = loss_inputs(H, W, with_nan)
    old, new = loss_old(x), loss_new(x)
    assert bits_equal(new["rgb"], old["rgb"])
    assert bits_equal(new["du"], old["du"])
    assert n_zero_diff > 0 and int((old["du"] == 0).sum()) >= n_zero_diff
    # d_irr_unit
    n, n_padding = selection_counts(device_srgb(x["irr"]), old["du"].cpu())
    gs = float(np.float32(1.0) / (np.float32(3.0) * np.float32(H) * np.float32(W)))
    t = gs * srgb_slope64(x["irr"].cpu())
    iu_old, iu_new = old["iu"].cpu(), new["iu"].cpu()
    single = n <= 1
    assert torch.equal(bits(iu_new)[single], bits(iu_old)[single])
    assert not iu_new[n == 0].any()
    nd = n.double()
    bound = 2.0 * (nd - 1.0) * 2.0 ** -24 * nd * t
    diff = (iu_new.double() - iu_old.double()).abs()
    assert bool((diff[~single] <= bound[~single]).all()), float((diff - bound)[~single].max())
    # the cases are there: several contributions on one texel, a gradient dropped on a padding tap, routed gradients
    assert int(n.max()) >= 2 and n_padding > 0 and int((iu_new != 0).sum()) > 0
    if with_nan:
        # lin2srgb clamps with fmaxf, which drops a NaN: the NaN texels of irr give finite sRGB values and slope 0;
        # the NaN of `direct` reaches render_rgb and the sum: sign 0 there, and a NaN loss from both entries
        assert not iu_new[x["irr"].isnan().cpu()].any()
        at = (2, H // 2, 1)
        assert bool(torch.isnan(new["rgb"][at])) and float(new["du"][at]) == 0.0 and int(torch.isnan(new["rgb"]).sum()) == 1
        assert bool(torch.isnan(new["loss"]).all()) and bool(torch.isnan(old["loss"]).all())
    # loss and the four sums against float64
    ref_acc, ref_loss = sums64(x, old["rgb"])
    pairs = [("acc%d" % k, float(new["acc"][k]), float(old["acc"][k]), ref_acc[k]) for k in range(4)]
    pairs.append(("loss", float(new["loss"]), float(old["loss"]), ref_loss))
    for name, v_new, v_old, ref in pairs:
        if np.isnan(ref):
            assert np.isnan(v_new) and np.isnan(v_old), name
            continue
        dev_new, dev_old = abs(v_new - ref), abs(v_old - ref)
        ulp = float(np.spacing(np.float32(abs(ref))))
        print("%dx%d nan=%d %s: gather %.3e  atomic %.3e  (ulp %.3e)" % (H, W, with_nan, name, dev_new, dev_old, ulp))
        assert dev_new <= 2.0 * dev_old + ulp, (name, dev_new, dev_old, ulp)
    # deterministic: a second call gives the same bits in every output
    again = loss_new(x)
    for k in new:
        assert bits_equal(new[k], again[k]), k


def test_loss_gather_refuses_a_short_scratch():
    import gigs_lib
    lib = gigs_lib.lib()
    H, W = 9, 70
    x, _ = loss_inputs(H, W, False)
    o = torch.empty(3, H, W, device=DEV)
    s4 = torch.empty(8, device=DEV)
    assert lib.gigs_stage2_loss_gather(H, W, p(x["direct"]), p(x["irr"]), p(x["gt"]), p(x["mask"]), p(x["rough"]), p(x["metal"]),
                                       p(o), p(s4), p(s4), p(o), p(o), p(s4), 16, stream()) != 0
    assert int(lib.gigs_stage2_loss_gather_scratch_bytes(0, 5)) == 0


# ---- G-buffer post + shade ----------------------------------------------------------------------------------------
def gbuffer_inputs(H, W):
    g = torch.Generator(device="cpu").manual_seed(77 * H + W)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)  # noqa: E731
    nm, onv = rn(3, H, W), rn(3, H, W)
    nm[:, 0:2, 0:3] = 0.0                 # zero normals: mask 0, normalize_where passes them, medians tie with padding
    nm[1, H // 2, W // 2] = 0.0           # one zero channel: mask 0 as well
    nm[:, H - 1, W - 2] = float("nan")    # a NaN normal: its windows give NaN
    nm[:, H // 2:H // 2 + 2, 1:4] = nm[:, H // 2:H // 2 + 1, 1:2]  # equal normals: ties
    onv[:, 1, W - 1] = float("nan")
    onv[:, H - 2:H, 0:2] = 0.0
    vm = torch.eye(4)
    q, _ = torch.linalg.qr(rn(3, 3))
    vm[:3, :3] = q
    vm[:3, 3] = rn(3)
    vd = F.normalize(rn(H, W, 3), dim=-1)
    x = dict(nm=nm, onv=onv, vm=vm, vd=vd, albedo=ru(3, H, W), rough=ru(1, H, W), occ=0.3 + 0.7 * ru(1, H, W), metal=ru(1, H, W))
    return {k: v.to(DEV).contiguous() for k, v in x.items()}


@pytest.fixture(scope="module")
def light():
    import pbr
    torch.manual_seed(5)
    lt = pbr.CubemapLight(base_res=64, device=DEV)  # 64, 32, 16: three specular levels
    with torch.no_grad():
        lt.base.copy_(torch.rand_like(lt.base) * 0.8 + 0.2)
        lt.build_mips()
    return lt.diffuse.detach().contiguous(), [s.detach().contiguous() for s in lt.specular], pbr.get_brdf_lut().to(DEV)


@pytest.mark.parametrize("metallic", [True, False])
@pytest.mark.parametrize("H,W", SIZES)
def test_post_inside_the_shade_equals_the_two_launches(light, H, W, metallic):
    import gigs_lib
    from pbr.shade import _ptr_array
    lib = gigs_lib.lib()
    diffuse, spec, lut = light
    x = gbuffer_inputs(H, W)
    spec_ptr = _ptr_array(spec)
    spec_res = (C.c_int * len(spec))(*[int(s.shape[1]) for s in spec])
    met = p(x["metal"]) if metallic else None

    def outputs():
        f = lambda c: torch.full((c, H, W), float("nan"), device=DEV)  # noqa: E731
        o = dict(nv=f(3), mask_f=f(1), onv=f(3), direct=f(3), F0=f(3), linear=f(3), rough=f(1))
        o["mask_u8"] = torch.full((H, W), 7, dtype=torch.uint8, device=DEV)
        ext = gigs_lib.ShadeExt(planar=1, rough_scale=1.0 - 0.04, rough_bias=0.04, out_F0=p(o["F0"]), out_linear=p(o["linear"]),
                                out_roughness=p(o["rough"]))
        return o, ext

    light_args = (p(diffuse), int(diffuse.shape[1]), len(spec), spec_ptr, spec_res, p(lut), int(lut.shape[-2]), int(lut.shape[-3]), 1, 1)
    a, ext = outputs()
    gigs_lib.check(lib.gigs_gbuffer_post(H, W, p(x["nm"]), p(x["onv"]), p(x["vm"]), p(a["nv"]), p(a["mask_u8"]), p(a["mask_f"]),
                                         p(a["onv"]), stream()), "gbuffer_post")
    gigs_lib.check(lib.gigs_shade_fwd_ex(gigs_lib.ctx_ptr(), H, W, p(a["nv"]), p(x["vd"]), p(x["albedo"]), p(x["rough"]),
                                         p(a["mask_u8"]), p(x["occ"]), met, None, *light_args, p(a["direct"]), None, None, None,
                                         C.addressof(ext), stream()), "shade_fwd_ex")
    b, ext = outputs()
    gigs_lib.check(lib.gigs_shade_fwd_post(gigs_lib.ctx_ptr(), H, W, p(x["nm"]), p(x["onv"]), p(x["vm"]), p(b["nv"]), p(b["mask_u8"]),
                                           p(b["mask_f"]), p(b["onv"]), p(x["vd"]), p(x["albedo"]), p(x["rough"]), p(x["occ"]), met,
                                           *light_args, p(b["direct"]), C.addressof(ext), stream()), "shade_fwd_post")
    torch.cuda.synchronize()
    for k in a:
        if k == "mask_u8":
            assert torch.equal(a[k], b[k])
        else:
            assert bits_equal(a[k], b[k]), k
    # the cases are there: masked pixels, NaN windows, shaded pixels
    assert 0 < int(a["mask_u8"].sum()) < H * W and bool(torch.isnan(a["nv"]).any()) and bool(torch.isnan(a["onv"]).any())
    assert float(a["direct"].nan_to_num().abs().max()) > 0
    # the planar layout is part of the entry's contract
    ext0 = gigs_lib.ShadeExt(planar=0, rough_scale=1.0, rough_bias=0.0)
    assert lib.gigs_shade_fwd_post(gigs_lib.ctx_ptr(), H, W, p(x["nm"]), p(x["onv"]), p(x["vm"]), p(b["nv"]), p(b["mask_u8"]),
                                   p(b["mask_f"]), p(b["onv"]), p(x["vd"]), p(x["albedo"]), p(x["rough"]), p(x["occ"]), met,
                                   *light_args, p(b["direct"]), C.addressof(ext0), stream()) != 0


# ---- the fused node -----------------------------------------------------------------------------------------------
def test_fused_node_with_the_switches_on_and_off(light, monkeypatch):
    import stage2_fused
    H, W = 40, 130
    diffuse, spec, lut = light
    x = gbuffer_inputs(H, W)
    x["nm"], x["onv"] = x["nm"].nan_to_num(0.5), x["onv"].nan_to_num(0.5)  # a finite loss: the NaN cases are the entries' tests
    g = torch.Generator(device="cpu").manual_seed(3)
    fx = fy = 120.0
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 3.0 + 0.4 * torch.sin(xx / 9.0) * torch.cos(yy / 7.0)  # a wavy surface in front of the camera
    pos = torch.stack([(xx - W / 2) / fx * z, (yy - H / 2) / fy * z, z]).to(DEV).contiguous()
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    cfg = dict(H=H, W=W, gi=scenes.GI_DEFAULTS, focal_x=fx, focal_y=fy, metallic=True, indirect=True, gamma=True, tone=False)

    def run(on):
        set_options(monkeypatch, stage2_gather=int(on), shade_post_fused=int(on))
        leaves = [x["albedo"].clone().requires_grad_(True), x["rough"].clone().requires_grad_(True),
                  x["metal"].clone().requires_grad_(True), diffuse.clone().requires_grad_(True)]
        sp = [s.clone().requires_grad_(True) for s in spec]
        loss, rgb, direct, irr = stage2_fused._Stage2Fused.apply(cfg, x["nm"], x["onv"], leaves[0], leaves[1], leaves[2], x["occ"],
                                                                 pos, x["vm"], x["vd"], gt, lut, leaves[3], *sp)
        saved = loss.grad_fn.saved_tensors
        d_irr_u, abd, mask_f = saved[11].clone(), saved[12].clone(), saved[5].clone()
        (loss * 0.75).backward()
        torch.cuda.synchronize()
        grads = [t.grad.clone() for t in leaves] + [torch.cat([s.grad.flatten() for s in sp])]
        return loss.detach().clone(), (rgb, direct, irr), grads, d_irr_u, abd, mask_f

    loss_a, planes_a, grads_a, iu_a, abd, mask_f = run(False)
    loss_b, planes_b, grads_b, iu_b, _, _ = run(True)
    for name, a, b in zip(("render_rgb", "render_direct", "IRR"), planes_a, planes_b):
        assert bits_equal(a, b), name
    # the loss, against the float64 sums of the node's own planes (rough_f = raw * 0.96 + 0.04 as the shade rounds it)
    rough_f = x["rough"] * np.float32(1.0 - 0.04) + np.float32(0.04)
    _, ref_loss = sums64(dict(gt=gt, mask=mask_f, rough=rough_f, metal=x["metal"]), planes_a[0])
    dev_new, dev_old = abs(float(loss_b) - ref_loss), abs(float(loss_a) - ref_loss)
    print("node loss: gather %.3e  atomic %.3e" % (dev_new, dev_old))
    assert np.isfinite(ref_loss) and dev_new <= 2.0 * dev_old + float(np.spacing(np.float32(abs(ref_loss))))
    # roughness / metallic: per-pixel outputs of bit-identical operands (the mask count is an exact integer either way)
    assert bits_equal(grads_a[1], grads_b[1]) and bits_equal(grads_a[2], grads_b[2])
    # albedo: the shade's own term (bit-identical operands) + g * d_irr_unit * abd
    same = bits(iu_a) == bits(iu_b)
    assert torch.equal(bits(grads_a[0])[same], bits(grads_b[0])[same])
    d_alb = (grads_a[0].double() - grads_b[0].double()).abs().cpu()
    d_iu = ((iu_a.double() - iu_b.double()).abs() * abd.double().abs()).cpu() * 0.75
    ulp = torch.from_numpy(np.spacing(np.maximum(grads_a[0].abs().cpu().numpy(), grads_b[0].abs().cpu().numpy())).astype(np.float64))
    # d_albedo = shade term + fl(fl(d_irr_unit * g) * abd): the terms' difference, two product roundings each, the sums' rounding
    prod = ((iu_a.double().abs() + iu_b.double().abs()) * abd.double().abs()).cpu() * 0.75
    assert bool((d_alb <= d_iu + 2.0 ** -22 * prod + 2.0 * ulp)[~same].all())
    # light: it receives gradient only through d_render_direct, asserted bit-identical above, so the two runs differ only in
    # the order of the shade backward's own atomics; 1e-4 of the peak is the bound test_gpu_shade_bwd_scatter.py sets for two
    # orders of exactly those sums (it is not derived from the loss kernel's bounds)
    for a, b, name in ((grads_a[3], grads_b[3], "diffuse"), (grads_a[4], grads_b[4], "specular")):
        scale = max(float(a.abs().max()), 1e-20)
        assert float((a.double() - b.double()).abs().max()) / scale <= 1e-4, name
        assert float(a.abs().max()) > 0, name
