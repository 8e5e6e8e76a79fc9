"""Relighting one view under K environment maps (relight.MultiRelighter): the K-light march (gigs_ssr_multi) and shade
(gigs_shade_fwd_multi) against K single-light calls bit for bit, MultiRelighter against the CPU oracle and against K
Relighter calls at C3 size, and RelightEvaluator against evaluate.image_metrics and a float64 recomputation."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import scenes
from oracle import stage2_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = stage2_ref.KEYS
MAX_LIGHTS = 16


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cam_t(cam):
    return {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}


def view_dirs(cam):
    import pipeline
    return pipeline.view_dirs_for(cam_t(cam), pipeline.canonical_rays(cam, DEV), DEV)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _case(lights_n=1, light_res=64):
    """test_gpu_relight.py's _relight_case (176x144, 9000 Gaussians) with `lights_n` synthetic maps."""
    import relight
    W, H = 176, 144
    sc = scenes.surface_scene(P=9000, sh_degree=2, seed=4, scale_mu=0.03)
    cam = scenes.orbit_camera(1, 8, W, H, radius=3.5)
    envs = [scenes.synthetic_envmap(128, 256, seed=5 + i) for i in range(lights_n)]
    lights = [relight.make_light(tt(e), res=light_res) for e in envs]
    g = {k: tt(sc[k]) for k in KEYS}
    return sc, cam, envs, lights, g


@pytest.fixture(scope="module")
def gbuf():
    import relight
    sc, cam, envs, lights, g = _case(1)
    rl = relight.Relighter(lights[0], scenes.GI_DEFAULTS, 2)
    b = rl.source(cam_t(cam), g)
    torch.cuda.synchronize()
    return cam, b, lights[0], rl


def _radiance(K, H, W, seed=0):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    rgb = torch.rand((K, 3, H, W), generator=gen) * 1.5
    rgb[K // 2, 1, ::7, ::5] = float("nan")  # one plane with NaNs
    rgb[K - 1] *= 0.25  # distinct planes
    return rgb.to(DEV)


@pytest.mark.parametrize("march", ["default", "no_cert", "exact", "nonpow2"])
def test_ssr_multi_equals_single_light_march(gbuf, march):
    import gigs_lib
    from diff_gaussian_rasterization import _gi_scratch
    lib = gigs_lib.lib()
    cam, b, _, _ = gbuf
    H, W = cam["image_height"], cam["image_width"]
    gi = dict(scenes.GI_DEFAULTS)
    opts = {}
    if march == "no_cert":
        opts = dict(gi_cert=0)
    elif march == "exact":
        opts = dict(gi_march=0)
    elif march == "nonpow2":
        gi["step"] = 13
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    s = torch.cuda.current_stream().cuda_stream
    scratch = _gi_scratch(W, H, DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = (W, H, float(fx), float(fy), float(gi["radius"]), float(gi["bias"]), float(gi["thick"]), float(gi["delta"]),
         int(gi["step"]), int(gi["start"]))
    geo = (p(b["onv"]), p(b["depth_pos"]))
    mat = (p(b["albedo_map"]), p(b["roughness_map"]), p(b["metallic_in"]), p(b["F0"]))
    with gigs_lib.options(**opts):
        ctx = gigs_lib.ctx_ptr()
        for K in (1, 3, MAX_LIGHTS):
            rgb = _radiance(K, H, W, seed=K)
            color = torch.full((K, 3, H, W), 7.0, device=DEV)
            abd = torch.full((K, 3, H, W), 7.0, device=DEV)
            gigs_lib.check(lib.gigs_ssr_multi(ctx, K, *a, *geo, p(rgb), *mat, p(color), p(abd), p(scratch), s), "ssr_multi")
            for k in range(K):
                c1, a1 = torch.empty((3, H, W), device=DEV), torch.empty((3, H, W), device=DEV)
                gigs_lib.check(lib.gigs_ssr_ex(ctx, *a, *geo, p(rgb[k]), *mat, p(c1), p(a1), p(scratch), s), "ssr_ex")
                assert bits_equal(color[k], c1), (march, K, k)
                assert bits_equal(abd[k], a1), (march, K, k)
            assert bool(torch.isnan(color[K // 2]).any()) and float(color.nan_to_num().abs().max()) > 0
        # K = 0 and K above the maximum are refused before any launch
        dummy = torch.zeros(1, device=DEV)
        for K in (0, MAX_LIGHTS + 1):
            assert lib.gigs_ssr_multi(ctx, K, *a, *geo, p(dummy), *mat, p(dummy), p(dummy), None, s) != 0
        assert lib.gigs_ssr_multi(ctx, 2, *a, *geo, None, *mat, p(dummy), p(dummy), None, s) != 0


def test_shade_multi_equals_single_light_shade(gbuf):
    import gigs_lib
    from pbr import get_brdf_lut
    from pbr.shade import _ptr_array
    lib = gigs_lib.lib()
    cam, b, _, _ = gbuf
    H, W = cam["image_height"], cam["image_width"]
    _, _, _, lights, _ = _case(3)
    for light in lights:
        light.build_mips()
    lut = get_brdf_lut().to(DEV)
    vd = view_dirs(cam).contiguous().float()
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    K = len(lights)
    L = len(lights[0].specular)
    spec_res = (C.c_int * L)(*[int(x.shape[1]) for x in lights[0].specular])
    ctx = gigs_lib.ctx_ptr()
    for metallic, tone, gamma, occl in itertools.product((False, True), repeat=4):
        occ = p(b["occlusion"]) if occl else None
        met = p(b["metallic_map"]) if metallic else None
        out = torch.full((K, 3, H, W), 7.0, device=DEV)
        lin = torch.full((K, 3, H, W), 7.0, device=DEV)
        gigs_lib.check(lib.gigs_shade_fwd_multi(
            ctx, K, H, W, p(b["normals_view"]), p(vd), p(b["albedo_map"]), p(b["roughness_map"]), p(b["mask_u8"]), occ, met,
            _ptr_array([l.diffuse for l in lights]), int(lights[0].diffuse.shape[1]), L,
            _ptr_array([x for l in lights for x in l.specular]), spec_res, p(lut), int(lut.shape[-2]), int(lut.shape[-3]),
            int(tone), int(gamma), p(out), p(lin), s), "shade_fwd_multi")
        for k, light in enumerate(lights):
            r1, l1 = torch.empty((3, H, W), device=DEV), torch.empty((3, H, W), device=DEV)
            ext = gigs_lib.ShadeExt(planar=1, rough_scale=1.0, rough_bias=0.0, out_linear=p(l1))
            gigs_lib.check(lib.gigs_shade_fwd_ex(
                ctx, H, W, p(b["normals_view"]), p(vd), p(b["albedo_map"]), p(b["roughness_map"]), p(b["mask_u8"]), occ, met,
                None, p(light.diffuse), int(light.diffuse.shape[1]), L, _ptr_array(light.specular), spec_res, p(lut),
                int(lut.shape[-2]), int(lut.shape[-3]), int(tone), int(gamma), p(r1), None, None, None, C.addressof(ext), s),
                "shade_fwd_ex")
            assert bits_equal(out[k], r1), (metallic, tone, gamma, occl, k)
            assert bits_equal(lin[k], l1), (metallic, tone, gamma, occl, k)
        assert not bits_equal(out[0], out[1])
    # without out_linear; and invalid light counts
    out2 = torch.empty((K, 3, H, W), device=DEV)
    args = (p(b["normals_view"]), p(vd), p(b["albedo_map"]), p(b["roughness_map"]), p(b["mask_u8"]), None, None,
            _ptr_array([l.diffuse for l in lights]), int(lights[0].diffuse.shape[1]), L,
            _ptr_array([x for l in lights for x in l.specular]), spec_res, p(lut), int(lut.shape[-2]), int(lut.shape[-3]), 0, 0)
    gigs_lib.check(lib.gigs_shade_fwd_multi(ctx, K, H, W, *args, p(out2), None, s), "shade_fwd_multi")
    for K_bad in (0, MAX_LIGHTS + 1):
        assert lib.gigs_shade_fwd_multi(ctx, K_bad, H, W, *args, p(out2), None, s) != 0


@pytest.mark.parametrize("metallic,ratio", [(False, None), (True, (0.9, 1.1, 0.8))])
def test_multi_relighter_matches_oracle(orc, metallic, ratio):
    import relight
    W, H, res = 176, 144, 64
    sc, cam, envs, lights, g = _case(3, light_res=res)
    gi = scenes.GI_DEFAULTS
    rng = np.random.default_rng(0)
    alpha = (rng.uniform(size=(1, H, W)) > 0.1).astype(np.float32)
    vd = view_dirs(cam)
    mr = relight.MultiRelighter(lights, gi, 2, metallic=metallic)
    out = mr(cam_t(cam), g, vd, alpha_mask=tt(alpha), albedo_ratio=ratio)
    for k, light in enumerate(lights):
        diffuse, spec = stage2_ref.build_mips(orc, light.base.detach().cpu().numpy())
        ref = stage2_ref.relight_view(orc, sc, cam, gi, 2, diffuse, spec, alpha_mask=alpha,
                                      albedo_ratio=ratio or (1, 1, 1), metallic=metallic, pad_normal=False)
        for name in ("render_direct", "IRR", "render_rgb"):
            a, b = out[name][k].cpu().numpy(), ref[name]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (k, name)
            d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
            assert d.mean() <= 1e-4, (k, name, d.mean())
        a, b = out["occlusion"].cpu().numpy(), ref["occlusion"]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.abs(np.nan_to_num(a) - np.nan_to_num(b)).mean() <= 1e-4
        assert stage2_ref.psnr(np.nan_to_num(out["render_rgb"][k].cpu().numpy()), np.nan_to_num(ref["render_rgb"])) >= 60.0
    assert not np.array_equal(out["render_rgb"][0].cpu().numpy(), out["render_rgb"][1].cpu().numpy())


def test_multi_relighter_equals_relighter_c3_size():
    """800x800 / 300k Gaussians / 256^2 lights, K = 3: light k == Relighter(light_k) bit for bit, eager and graphed."""
    import relight
    W = H = 800
    sc = scenes.surface_scene(P=300_000, sh_degree=2, seed=0)
    gi = scenes.GI_DEFAULTS
    lights = [relight.make_light(tt(scenes.synthetic_envmap(512, 1024, seed=1 + i)), res=256) for i in range(3)]
    g = {k: tt(sc[k]) for k in KEYS}
    yy, xx = np.mgrid[0:H, 0:W]
    alpha = tt((((xx - 400) ** 2 + (yy - 400) ** 2) < 380 ** 2).astype(np.float32)[None])
    cams = [scenes.orbit_camera(11, 64, W, H, radius=3.5), scenes.orbit_camera(30, 64, W, H, radius=3.5)]
    vds = [view_dirs(c) for c in cams]
    singles = [relight.Relighter(l, gi, 2, metallic=False, fused=True) for l in lights]
    want = []
    for cm, vd in zip(cams, vds):
        per = [r(cam_t(cm), g, vd, alpha_mask=alpha) for r in singles]
        want.append({k: [o[k].clone() for o in per] for k in ("render_direct", "IRR", "render_rgb")} |
                    {k: per[0][k].clone() for k in ("occlusion", "depth_map", "normal_map", "normal_mask", "radii")})
    mr = relight.MultiRelighter(lights, gi, 2, metallic=False)
    mg = relight.MultiRelighter(lights, gi, 2, metallic=False, graphs=True)
    spec_ptrs = [[s.data_ptr() for s in l.specular] for l in lights]  # the mips are built at construction, not per view

    def check(out, w, graphed):
        for k in ("render_direct", "IRR", "render_rgb"):
            assert tuple(out[k].shape) == (3, 3, H, W)
            for i in range(3):
                assert bits_equal(out[k][i], w[k][i]), (graphed, k, i)
        for k in ("occlusion", "depth_map", "normal_map"):
            assert bits_equal(out[k], w[k]), (graphed, k)
        assert torch.equal(out["radii"], w["radii"]) and torch.equal(out["normal_mask"], w["normal_mask"])

    check(mr(cam_t(cams[0]), g, vds[0], alpha_mask=alpha), want[0], False)
    for i in (0, 1, 0):
        out = mg(cam_t(cams[i]), g, vds[i], alpha_mask=alpha)
        assert out["num_rendered"] > 1_000_000
        check(out, want[i], True)
    assert mg.graphs, "the graphed path fell back to eager"
    assert [[s.data_ptr() for s in l.specular] for l in lights] == spec_ptrs
    mg.close()


def test_relight_evaluator_matches_image_metrics():
    import evaluate
    import relight
    K, H, W = 3, 64, 80
    gen = torch.Generator(device="cpu").manual_seed(3)
    pred = (torch.rand((2, K, 3, H, W), generator=gen) * 1.2 - 0.1).to(DEV)
    gt = torch.rand((2, K, 3, 2 * H, 2 * W), generator=gen).to(DEV)
    names = ["a", "b", "c"]
    ev = relight.RelightEvaluator(names)
    for v in range(2):
        ev.add(pred[v], gt[v])
    res = ev.results()
    import torch.nn.functional as F
    for k, name in enumerate(names):
        ps, ss, ps64 = [], [], []
        for v in range(2):
            q = relight.quantize_8bit(pred[v, k])
            g = F.interpolate(gt[v, k][None], size=(H, W), mode="bilinear", align_corners=False)[0]
            rec = evaluate.image_metrics(q, g).cpu()
            ps.append(float(rec[3]))
            ss.append(float(rec[4]))
            qa, ga = q.double().cpu().numpy(), g.double().cpu().numpy()
            mse = ((qa - ga) ** 2).reshape(3, -1).mean(1)
            ps64.append(float(np.mean(20 * np.log10(1.0 / np.sqrt(mse)))))
        assert res[name]["n_views"] == 2
        assert res[name]["psnr_avg"] == sum(ps) / 2 and res[name]["ssim_avg"] == sum(ss) / 2, name
        assert abs(res[name]["psnr_avg"] - sum(ps64) / 2) <= 1e-6, (name, res[name]["psnr_avg"], sum(ps64) / 2)
    assert res["a"]["psnr_avg"] != res["b"]["psnr_avg"]
