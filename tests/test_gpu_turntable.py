"""Turntable relighting on the GPU: the rotated latitude-longitude conversion (gigs_latlong_to_cubemap_rot) and the cube
resample (relight.rotate_light) against float32 / float64 restatements, the K-plane gather over a recorded hit list
(gigs_ssr_apply_multi) against the single-plane gather and the march bit for bit, relight.TurntableRelighter against
relight.Relighter bit for bit and against the CPU oracle, and relight_scene --rotations on disk.

The view is test_gpu_relight_multi.py's scene at 170 x 140: neither side is a multiple of 8 and the pixel count is no
multiple of 256, so partial tiles and the gather's tail workgroup run."""
import numpy as np
import pytest
import torch

import scenes
from oracle import stage2_ref
from test_gpu_image_out import _png, trained  # noqa: F401  (the synthetic checkpoint; a fixture)
from test_gpu_relight_multi import DEV, KEYS, MAX_LIGHTS, _case, _radiance, bits_equal, cam_t, tt, view_dirs
from test_turntable_cpu import rot_latlong_ref, within_conversion_limits

pytestmark = pytest.mark.gpu
W, H = 170, 140
ROTS = (((0.0, 1.0, 0.0), 0.0), ((0.0, 1.0, 0.0), 0.7), ((1.0, 2.0, -0.5), 2.1))


def _rotations():
    import relight
    return torch.stack([relight.rotation_about(axis, angle) for axis, angle in ROTS])


def _camera():
    return scenes.orbit_camera(1, 8, W, H, radius=3.5)


# ---- 1. the rotated conversion ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,shape", [(16, (32, 64)), (64, (96, 200))])
def test_latlong_to_cubemap_rot_matches_restatement(res, shape):
    import gigs_lib
    import relight
    lib = gigs_lib.lib()
    env = scenes.synthetic_envmap(*shape, seed=res)
    env[3, 5] = np.inf  # non-finite texels travel through slice 0 as through the unrotated kernel
    env[shape[0] // 2, 9, 1] = np.nan
    rot = _rotations()
    plain = relight.latlong_to_cubemap(tt(env), [res, res])
    got = relight.latlong_to_cubemap_rot(tt(env), [res, res], rot)
    assert tuple(got.shape) == (3, 6, res, res, 3)
    assert bits_equal(got[0], plain) and bool(torch.isnan(plain).any())
    one = relight.latlong_to_cubemap_rot(tt(env), [res, res], rot[1:2])  # n_rot = 1
    assert tuple(one.shape) == (1, 6, res, res, 3) and bits_equal(one[0].nan_to_num(), got[1].nan_to_num())
    env = np.nan_to_num(env, nan=0.5, posinf=2.0)  # the comparisons below are on finite maps
    got = relight.latlong_to_cubemap_rot(tt(env), [res, res], rot).cpu().numpy()
    for k in range(3):
        ok, mean, mx = within_conversion_limits(got[k], rot_latlong_ref(env, res, rot[k].numpy().astype(np.float32)))
        print("rot conversion res=%d k=%d mean=%.3g max=%.3g" % (res, k, mean, mx))
        assert ok, (res, k, mean, mx)
    assert np.abs(got[1] - got[0]).mean() > 1e-3  # the rotations are not no-ops
    # roll anchor: +7 columns is the yaw by -2 pi 7 / W
    yaw = relight.rotation_about((0, 1, 0), -2 * np.pi * 7 / shape[1])[None]
    rolled = relight.latlong_to_cubemap_rot(tt(env), [res, res], yaw)[0].cpu().numpy()
    ok, mean, mx = within_conversion_limits(rolled, stage2_ref.latlong_to_cubemap(np.roll(env, 7, 1), [res, res]))
    print("roll anchor res=%d mean=%.3g max=%.3g" % (res, mean, mx))
    assert ok, (res, mean, mx)
    # n_rot outside 1..1024 is refused before any launch
    lat, out = tt(env), torch.full((6, res, res, 3), 7.0, device=DEV)
    r32 = rot.float().to(DEV).contiguous()
    s = torch.cuda.current_stream().cuda_stream
    for n_bad in (0, 1025):
        assert lib.gigs_latlong_to_cubemap_rot(res, res, shape[0], shape[1], 3, lat.data_ptr(), n_bad, r32.data_ptr(),
                                               out.data_ptr(), s) != 0
    assert lib.gigs_latlong_to_cubemap_rot(res, res, shape[0], shape[1], 3, lat.data_ptr(), 1, None, out.data_ptr(), s) != 0
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 == float(out.max())


def test_rotated_lights_are_make_light_of_the_rotated_map():
    import relight
    env = tt(scenes.synthetic_envmap(64, 128, seed=2))
    lights = relight.rotated_lights(env, relight.yaw_rotations(5), res=32)
    assert len(lights) == 5 and all(tuple(l.base.shape) == (6, 32, 32, 3) and not l.training for l in lights)
    assert bits_equal(lights[0].base.detach(), relight.make_light(env, res=32).base.detach())
    assert not bits_equal(lights[1].base.detach(), lights[4].base.detach())


# ---- 2. the cube resample ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [16, 64])
def test_rotate_light_matches_restated_lookup(res):
    """rotate_light's slice k is the cube lookup at R_k^T dir of the texel centres: the lookup against
    oracle/torch_pbr_ref.cube_sample with test_gpu_losses.py::test_cube_texture_matches_restated_lookup's tolerance (2e-6
    on a base in [0, 1)) at the float32 directions the light is sampled at, and those directions against float64 ones.

    The float lookup (gigs_cube_texture_fwd) meets that bound at 16^2 (measured 7.6e-7) and not at 64^2 (3.8e-6: half an ulp
    of the coordinate u * 64 - 0.5 alone is 1.9e-6 texels, on a base whose neighbouring texels differ by up to 1), which is
    why rotate_light samples with double-precision coordinates; what is left is the float rounding of four weights and
    their products, about 2e-7."""
    import relight
    from oracle import torch_pbr_ref as pr
    from pbr import CubemapLight
    gen = torch.Generator().manual_seed(res)
    base = torch.rand(6, res, res, 3, generator=gen)
    light = CubemapLight(base_res=res, device=DEV)
    light.base.data = base.to(DEV)
    rot = _rotations()
    out = relight.rotate_light(light, rot)
    assert len(out) == 3 and all(tuple(l.base.shape) == (6, res, res, 3) for l in out)
    lin = np.linspace(-1.0 + 1.0 / res, 1.0 - 1.0 / res, res, dtype=np.float32)
    gy, gx = np.meshgrid(lin, lin, indexing="ij")
    centres = np.stack([stage2_ref.cube_to_dir(s, gx, gy) for s in range(6)]).astype(np.float64)
    dirs32 = relight.cube_texel_dirs(res, DEV)
    # float32 linspace / product: a few ulp of a component of size <= sqrt(3)
    assert float((dirs32.cpu().double() - torch.from_numpy(centres)).abs().max()) <= 1e-6
    errs = []
    for k in range(3):
        d = dirs32 @ rot[k].float().to(DEV)
        assert float((d.cpu().double() - torch.from_numpy(centres) @ rot[k]).abs().max()) <= 2e-6
        want = pr.cube_sample(base.to(pr.DT), d.cpu().to(pr.DT))
        errs.append(float((out[k].base.detach().cpu().double() - want.double()).abs().max()))
        print("rotate_light res=%d k=%d max err %.3g" % (res, k, errs[-1]))
    assert float((out[0].base.detach().cpu() - base).abs().max()) < 2e-6  # the identity returns the base
    assert float((out[1].base.detach().cpu() - base).abs().mean()) > 1e-2
    assert max(errs) < 2e-6, (res, errs)


# ---- 3. the gather, kernel level ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gbuf():
    import relight
    sc, _, envs, lights, g = _case(1)
    cam = _camera()
    b = relight.SplatGBuffer(scenes.GI_DEFAULTS, 2)(cam_t(cam), g)
    torch.cuda.synchronize()
    return cam, b


def test_ssr_apply_multi_equals_single_gather_and_march(gbuf):
    import gigs_lib
    from diff_gaussian_rasterization import _gi_scratch
    lib = gigs_lib.lib()
    cam, b = gbuf
    N = W * H
    gi = dict(scenes.GI_DEFAULTS)
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    s = torch.cuda.current_stream().cuda_stream
    scratch = _gi_scratch(W, H, DEV)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    a = (W, H, float(fx), float(fy), float(gi["radius"]), float(gi["bias"]), float(gi["thick"]), float(gi["delta"]),
         int(gi["step"]), int(gi["start"]))
    geo = (p(b["onv"]), p(b["depth_pos"]))
    mat = (p(b["albedo_map"]), p(b["roughness_map"]), p(b["metallic_in"]), p(b["F0"]))
    mat_apply = (p(b["albedo_map"]), p(b["metallic_in"]), p(b["F0"]))
    new3 = lambda: torch.empty(3, H, W, device=DEV)  # noqa: E731
    ctx = gigs_lib.ctx_ptr()
    # record the list: count, prefix, fill
    counts = torch.zeros(4 * N, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(4 * N + 1, dtype=torch.int32, device=DEV)
    c0, a0 = new3(), new3()
    gigs_lib.check(lib.gigs_ssr_hits(ctx, *a, *geo, p(b["albedo_map"]), *mat, p(c0), p(a0), 1, p(counts), None, None, 0,
                                     p(scratch), s), "ssr_hits (count)")
    torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
    total = int(offsets[-1])
    per = counts.view(N, 4)
    assert total > 0, "no ray of the test view hits anything"
    assert bool((per.sum(1) == 0).any()), "every pixel has a hit: the empty walk is not exercised"
    assert bool((per > 0).all(1).any()), "no pixel has hits in all four wave slots"
    entries = torch.full((total, 2), -1, dtype=torch.int32, device=DEV)
    gigs_lib.check(lib.gigs_ssr_hits(ctx, *a, *geo, p(b["albedo_map"]), *mat, p(c0), p(a0), 2, None, p(offsets), p(entries),
                                     total, p(scratch), s), "ssr_hits (fill)")
    assert int((entries < 0).sum()) == 0 and int(entries[:, 0].max()) < N  # complete, and every hit inside the image
    for K in (1, 3, 5, MAX_LIGHTS):
        rgb = _radiance(K, H, W, seed=K)
        color = torch.full((K, 3, H, W), 7.0, device=DEV)
        abd = torch.full((K, 3, H, W), 7.0, device=DEV)
        nbytes = int(lib.gigs_ssr_apply_multi_scratch_bytes(K, W, H))
        assert (nbytes == 0) == (K == 1) and nbytes % 16 == 0
        packed = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)
        gigs_lib.check(lib.gigs_ssr_apply_multi(K, W, H, float(gi["delta"]), p(offsets), p(entries), *geo, p(rgb), *mat_apply,
                                                p(color), p(abd), p(packed), s), "ssr_apply_multi")
        for k in range(K):
            c1, a1, c2, a2 = new3(), new3(), new3(), new3()
            gigs_lib.check(lib.gigs_ssr_apply(W, H, float(gi["delta"]), p(offsets), p(entries), *geo, p(rgb[k]), *mat_apply,
                                              p(c1), p(a1), s), "ssr_apply")
            gigs_lib.check(lib.gigs_ssr_ex(ctx, *a, *geo, p(rgb[k]), *mat, p(c2), p(a2), p(scratch), s), "ssr_ex")
            assert bits_equal(color[k], c1) and bits_equal(abd[k], a1), (K, k, "gather")
            assert bits_equal(color[k], c2) and bits_equal(abd[k], a2), (K, k, "march")
        assert bool(torch.isnan(color[K // 2]).any()) and float(color.nan_to_num().abs().max()) > 0
        assert not bool((color == 7.0).any()) and not bool((abd == 7.0).any())  # every pixel of every plane written
    # refused before any launch: K = 0, K above the maximum, no radiance
    dummy = torch.full((4,), 7.0, device=DEV)
    for K in (0, MAX_LIGHTS + 1):
        assert lib.gigs_ssr_apply_multi(K, W, H, float(gi["delta"]), p(offsets), p(entries), *geo, p(dummy), *mat_apply,
                                        p(dummy), p(dummy), p(packed), s) != 0
    assert lib.gigs_ssr_apply_multi(2, W, H, float(gi["delta"]), p(offsets), p(entries), *geo, None, *mat_apply, p(dummy),
                                    p(dummy), p(packed), s) != 0
    assert lib.gigs_ssr_apply_multi(2, W, H, float(gi["delta"]), p(offsets), p(entries), *geo, p(dummy), *mat_apply, p(dummy),
                                    p(dummy), None, s) != 0  # more than one light needs the scratch
    torch.cuda.synchronize()
    assert float(dummy.min()) == 7.0 == float(dummy.max())


# ---- 4. end to end, exact -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def turntable():
    import relight
    sc, _, envs, _, g = _case(1)
    env = envs[0]
    lights = relight.rotated_lights(tt(env), relight.yaw_rotations(18), res=64)
    return sc, _camera(), env, lights, g


@pytest.mark.parametrize("march", ["default", "exact"])
@pytest.mark.parametrize("metallic", [False, True])
def test_turntable_relighter_equals_relighter(turntable, metallic, march):
    import gigs_lib
    import relight
    sc, cam, env, lights, g = turntable
    gi = scenes.GI_DEFAULTS
    rng = np.random.default_rng(0)
    alpha = tt((rng.uniform(size=(1, H, W)) > 0.1).astype(np.float32))
    vd = view_dirs(cam)
    ratio = (0.9, 1.1, 0.8) if metallic else None
    with gigs_lib.options(**(dict(gi_march=0) if march == "exact" else {})):
        with relight.TurntableRelighter(lights, gi, 2, metallic=metallic) as tr:
            out = tr(cam_t(cam), g, vd, alpha_mask=alpha, albedo_ratio=ratio)
            # the default march gathers at a recorded list; the exact march has none and goes through gigs_ssr_multi
            assert (tr.last_hits is not None and tr.last_hits > 0) if march == "default" else tr.last_hits is None
        for name in ("render_rgb", "render_direct", "IRR"):
            assert tuple(out[name].shape) == (18, 3, H, W)
        for k in (0, 5, 17):
            want = relight.Relighter(lights[k], gi, 2, metallic=metallic, fused=True)(cam_t(cam), g, vd, alpha_mask=alpha,
                                                                                      albedo_ratio=ratio)
            for name in ("render_rgb", "render_direct", "IRR"):
                assert bits_equal(out[name][k], want[name]), (metallic, march, k, name)
            if k == 0:
                for name in ("occlusion", "depth_map", "normal_map"):
                    assert bits_equal(out[name], want[name]), name
                assert torch.equal(out["radii"], want["radii"]) and torch.equal(out["normal_mask"], want["normal_mask"])
        plain = relight.Relighter(relight.make_light(tt(env), res=64), gi, 2, metallic=metallic)(
            cam_t(cam), g, vd, alpha_mask=alpha, albedo_ratio=ratio)
        for name in ("render_rgb", "render_direct", "IRR"):  # rotation 0 is the unrotated light
            assert bits_equal(out[name][0], plain[name]), name
    assert float((out["render_rgb"][0] - out["render_rgb"][5]).nan_to_num().abs().mean()) > 1e-4  # two rotations differ
    assert float(out["IRR"].nan_to_num().abs().max()) > 0


# ---- 5. end to end, against the oracle ------------------------------------------------------------------------------------------
def _close(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)), what
    d = float(np.abs(np.nan_to_num(a) - np.nan_to_num(b)).mean())
    print("%s mean L1 %.3g" % (what, d))
    assert d <= 1e-4, (what, d)


@pytest.mark.parametrize("metallic", [False, True])
def test_turntable_relighter_matches_oracle(orc, metallic):
    import relight
    res = 64
    sc, _, envs, _, g = _case(1)
    env, cam, gi = envs[0], _camera(), scenes.GI_DEFAULTS
    rng = np.random.default_rng(0)
    alpha = (rng.uniform(size=(1, H, W)) > 0.1).astype(np.float32)
    ratio = (0.9, 1.1, 0.8) if metallic else None
    vd = view_dirs(cam)
    lights = relight.rotated_lights(tt(env), relight.yaw_rotations(4)[:2], res=res)  # the identity and a quarter turn
    with relight.TurntableRelighter(lights, gi, 2, metallic=metallic) as tr:
        out = tr(cam_t(cam), g, vd, alpha_mask=tt(alpha), albedo_ratio=ratio)
        assert tr.last_hits
    for k, light in enumerate(lights):
        diffuse, spec = stage2_ref.build_mips(orc, light.base.detach().cpu().numpy())  # the unchanged pre-filter of the rotated base
        ref = stage2_ref.relight_view(orc, sc, cam, gi, 2, diffuse, spec, alpha_mask=alpha, albedo_ratio=ratio or (1, 1, 1),
                                      metallic=metallic, pad_normal=False)
        for name in ("render_direct", "IRR", "render_rgb"):
            _close(out[name][k].cpu().numpy(), ref[name], "oracle light %d %s" % (k, name))
        assert stage2_ref.psnr(np.nan_to_num(out["render_rgb"][k].cpu().numpy()), np.nan_to_num(ref["render_rgb"])) >= 60.0
    # the direction of rotation, end to end: yaw_rotations(4)[1] is the map rolled by minus a quarter of its width
    rolled = relight.make_light(tt(np.roll(env, -env.shape[1] // 4, 1)), res=res)
    want = relight.Relighter(rolled, gi, 2, metallic=metallic)(cam_t(cam), g, vd, alpha_mask=tt(alpha), albedo_ratio=ratio)
    for name in ("render_direct", "IRR", "render_rgb"):
        _close(out[name][1].cpu().numpy(), want[name].cpu().numpy(), "rolled map %s" % name)
    assert stage2_ref.psnr(np.nan_to_num(out["render_rgb"][1].cpu().numpy()), np.nan_to_num(want["render_rgb"].cpu().numpy())) >= 60.0
    assert float((out["render_rgb"][0] - out["render_rgb"][1]).nan_to_num().abs().mean()) > 1e-3


# ---- 6. relight_scene --rotations -----------------------------------------------------------------------------------------------
def test_relight_scene_rotations(trained, tmp_path):  # noqa: F811
    import os

    import dataset_readers as dr
    import image_writer
    import relight_scene
    src, out, ck = trained
    path = str(tmp_path / "noon.hdr")
    image_writer.write_hdr(path, scenes.synthetic_envmap(64, 128, seed=2))
    res = relight_scene.relight_scene(["-m", out, "--checkpoint", ck, "--hdri", path, "--metallic", "--skip_train",
                                       "--rotations", "3"])
    names = [ci.image_name for ci in dr.readNerfSyntheticInfo(src, False, True)["test_cameras"]]
    lights = relight_scene.rotated_names(["noon"], 3)
    listed = relight_scene.planned_paths(out, "test", 7, names, lights)
    assert res["test"]["lights"] == lights and res["test"]["files"] == len(listed) == 3 + 8 * 6
    for p in listed:
        assert os.path.exists(p), p
        im = _png(p)
        assert im.ndim == 3 and im.shape[2] == 3, p
    relight_scene.relight_scene(["-m", out, "--checkpoint", ck, "--hdri", path, "--metallic", "--skip_train"])
    for n in names[:3]:
        a, b = relight_scene.view_paths(out, "test", 7, n, ["noon_r000"]), relight_scene.view_paths(out, "test", 7, n, ["noon"])
        assert np.array_equal(_png(a[0]), _png(b[0])) and np.array_equal(_png(a[1]), _png(b[1])), n
        turned = relight_scene.view_paths(out, "test", 7, n, ["noon_r001"])
        assert not np.array_equal(_png(a[0]), _png(turned[0])), n
    assert np.array_equal(_png(os.path.join(out, "test", "envmap_relight_noon_r000.png")),
                          _png(os.path.join(out, "test", "envmap_relight_noon.png")))
