"""GPU: the a-trous denoiser (csrc/denoise.hip through denoise.atrous, mesh_render.RaytracedLight.denoise, the denoise=
keyword of RaytracedGBuffer and AnalyticRelighter, render_mesh.py and relight_scene.py --denoise).  Against the numpy float32
restatement (tests/denoise_ref.py) floats are compared as bit patterns: float32 + - * / without contraction, no tolerance.

Quality, measured on an MI355X (the open box at 48 x 36, occlusion at 64 rays against 1024 rays over 1251 covered pixels,
shipped defaults; test_filtered_occlusion_is_closer_to_the_converged_one prints it): RMSE raw 0.01077, filtered 0.00831, ratio
0.771.  The numpy restatements gave 0.01056 and 0.00804 on the CPU before ("Denoising ray-traced planes")."""
import functools
import json
import math
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import denoise_ref as dn
import mesh_light_ref as lr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def _same_bytes(a, b):
    """Two tensors hold the same bytes: NaNs (the prepared arrays of uncovered pixels) included."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


# ---- 1: the restatement -----------------------------------------------------------------------------------------------------
PLANE = 4.0  # above the depth step of 3: taps across it get a fractional weight


@functools.lru_cache(maxsize=None)
def _case(H, W, C):
    """A crease plus a depth step with perturbed points and normals, a noisy signal on region levels, a roughness ramp; every
    5th pixel masked, one NaN position, one NaN normal, one zero normal, one NaN signal value.  Read-only."""
    rng = np.random.default_rng(H * 1000 + W + C)
    p, nr, mask, region = dn.crease_guide(H, W, step_height=3.0)
    p = (p + rng.normal(0.0, 0.05, p.shape)).astype(F)
    nr = nr + rng.normal(0.0, 0.08, nr.shape)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
    level = np.array([0.2, 0.6, 0.9])[region]
    x = (level[None] * rng.uniform(0.5, 1.5, (C, 1, 1)) + rng.normal(0.0, 0.08, (C, H, W))).astype(F)
    rough = (0.2 + 0.5 * np.arange(H * W) / (H * W) + rng.normal(0.0, 0.03, H * W)).astype(F)
    mask = mask.copy()
    mask[::5] = 0
    q = [int(i) for i in rng.choice(np.flatnonzero(mask), 4, replace=False)]
    p[q[0], 1] = np.nan
    nr[q[1], 0] = np.nan
    nr[q[2]] = 0.0
    x.reshape(C, -1)[C // 2, q[3]] = np.nan
    return x, p, nr, mask, rough, q


@pytest.mark.parametrize("W,H", [(37, 29), (16, 16)])
@pytest.mark.parametrize("groups,with_roughness", [((1,), False), ((1, 3, 3), False), ((3, 3, 1), True)])
def test_atrous_equals_the_restatement(W, H, groups, with_roughness):
    import denoise
    C = sum(groups)
    x, p, nr, mask, rough, q = _case(H, W, C)
    r = rough if with_roughness else None
    args = (_dev(x), _dev(p), _dev(nr), _dev(mask))
    total = 0
    for n in (1, 2, 3, 4, 5):
        for sigma_l in (4.0, 0.0):
            kw = dict(groups=list(groups), iterations=n, plane_distance=PLANE, normal_power=32, sigma_l=sigma_l, roughness_sigma=0.25)
            got, var, report = denoise.atrous(*args, roughness=None if r is None else _dev(r), **kw)
            want, want_var = dn.atrous(x, p, nr, mask, roughness=r, **kw)
            differ = int((_bits(got) != _bits(want)).sum()), int((_bits(var) != _bits(want_var)).sum())
            moved = int((_bits(got) != _bits(x)).sum())
            print("%dx%d groups %s n=%d sigma_l=%g: bit patterns that differ: filtered %d, variance %d of %d; %d values moved" % (
                W, H, list(groups), n, sigma_l, differ[0], differ[1], var.numel(), moved))
            assert got.dtype == var.dtype == torch.float32 and tuple(got.shape) == (C, H, W) and tuple(var.shape) == (len(groups), H, W)
            assert differ == (0, 0)
            assert json.loads(json.dumps(report)) == report
            live = dn.live_pixels(x, p, nr, mask, r)
            assert report["live"] == int(live.sum()) == H * W - (H * W + 4) // 5 - 3
            assert report["launches"] == ["pack", "variance"] + ["atrous:%d" % (1 << i) for i in range(n)] + ["unpack"]
            assert (report["iterations"], report["groups"], report["plane_distance"], report["sigma_l"]) == (n, list(groups), PLANE, sigma_l)
            assert moved > C * H * W // 2  # the comparison is of a filter that filters
            dead = ~live
            assert np.array_equal(_bits(got)[:, dead], _bits(x)[:, dead]) and not var.cpu().numpy()[:, dead].any()
            total += 1
    assert total == 10


def test_two_calls_give_the_same_bits_and_the_inputs_are_left_alone():
    import denoise
    x, p, nr, mask, rough, _ = _case(29, 37, 7)
    args = [_dev(a) for a in (x, p, nr, mask)]
    kept = [a.clone() for a in args]
    a, va, ra = denoise.atrous(*args, groups=[1, 3, 3], iterations=4, plane_distance=PLANE, roughness=_dev(rough))
    b, vb, rb = denoise.atrous(*args, groups=[1, 3, 3], iterations=4, plane_distance=PLANE, roughness=_dev(rough))
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(va), _bits(vb)) and ra == rb
    assert all(np.array_equal(k.cpu().numpy().view(np.uint8), t.cpu().numpy().view(np.uint8)) for k, t in zip(kept, args))
    # plane_distance=None: PLANE_FRACTION of the largest extent of the live points, and the report says which
    c, vc, rc = denoise.atrous(*args, groups=[1, 3, 3])
    live = dn.live_pixels(x, p, nr, mask)
    pts = p[live.reshape(-1)]
    assert rc["plane_distance"] == denoise.PLANE_FRACTION * float((pts.max(0) - pts.min(0)).max())
    assert (rc["iterations"], rc["normal_power"], rc["sigma_l"], rc["roughness_sigma"]) == (denoise.ITERATIONS, denoise.NORMAL_POWER, denoise.SIGMA_L, None)
    want, want_var = dn.atrous(x, p, nr, mask, [1, 3, 3], denoise.ITERATIONS, rc["plane_distance"], denoise.NORMAL_POWER, denoise.SIGMA_L)
    assert np.array_equal(_bits(c), _bits(want)) and np.array_equal(_bits(vc), _bits(want_var))


def test_sixteen_channels_empty_images_and_what_is_refused():
    import denoise
    import gigs_lib
    H, W = 18, 21
    x, p, nr, mask, rough, _ = _case(H, W, 16)
    args = (_dev(x), _dev(p), _dev(nr), _dev(mask))
    for groups in (None, [3, 3, 3, 3, 3, 1]):  # 16 groups: the largest record, 400 (8 + 32) 4 bytes of LDS
        got, var, report = denoise.atrous(*args, groups=groups, iterations=2, plane_distance=PLANE)
        want, want_var = dn.atrous(x, p, nr, mask, groups, 2, PLANE)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(var), _bits(want_var))
        assert report["channels"] == 16 and len(report["groups"]) == (16 if groups is None else 6)
    with pytest.raises(ValueError, match="1 to 16 channels"):
        denoise.atrous(torch.zeros((17, H, W), device=DEV), *args[1:])
    for h, w in ((0, 5), (4, 0)):
        e3, e1 = torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV)
        got, var, report = denoise.atrous(torch.zeros((3, h, w), device=DEV), e3, e3, e1, groups=[3])
        assert tuple(got.shape) == (3, h, w) and tuple(var.shape) == (1, h, w) and report["live"] == 0 and report["launches"] == []
    ok = dict(signal=args[0], points=args[1], normals=args[2], mask=args[3])
    for bad in (dict(signal=args[0].double()), dict(signal=args[0][0]), dict(points=args[1][:, :2]), dict(points=args[1][:5]),
                dict(normals=args[2].double()), dict(mask=args[3].float()), dict(mask=args[3][:7]), dict(groups=[16]), dict(groups=[3, 3, 3, 3, 3]),
                dict(groups=[]), dict(groups=[1.0] * 16), dict(iterations=0), dict(iterations=6), dict(iterations=2.0), dict(plane_distance=0.0),
                dict(plane_distance=float("nan")), dict(normal_power=3), dict(normal_power=256), dict(sigma_l=-1.0),
                dict(roughness=_dev(rough)[:9]), dict(roughness=_dev(rough).double()), dict(roughness=_dev(rough), roughness_sigma=0.0)):
        with pytest.raises(ValueError, match="denoise.atrous"):
            denoise.atrous(**dict(ok, **bad))
    with pytest.raises(RuntimeError, match="no CPU path"):
        denoise.atrous(args[0].cpu(), *args[1:])
    # the library refuses what Python would not send
    lib = gigs_lib.lib()
    one = (1 * __import__("ctypes").c_int)(1)
    buf = torch.zeros(64, device=DEV)
    assert lib.gigs_denoise_atrous(2, 2, 1, 1, one, 3, 5, 1.0, 0, 0.0, 16.0, 1e-10, buf.data_ptr(), buf.data_ptr(), buf[32:].data_ptr(), None) < 0
    assert lib.gigs_denoise_atrous(2, 2, 1, 1, one, 1, 5, 1.0, 0, 0.0, 16.0, 1e-10, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None) < 0
    assert lib.gigs_denoise_variance(2, 2, 1, 1, one, 8, 1.0, 0, 0.0, buf.data_ptr(), buf.data_ptr(), buf[32:].data_ptr(), None) < 0
    assert lib.gigs_denoise_pack(2, 2, 17, 1, one, None, None, None, None, None, None, None, None) < 0
    assert b"denoise_pack" in lib.gigs_last_error()


# ---- 2: in the image ----------------------------------------------------------------------------------------------------------
IW, IH = 48, 36
R, K = 64, 16


def _box_view(tilted=False):
    """The open box on the device and the camera of the sibling tests at 48 x 36.  tilted: turned as in the shadow tests, for
    a G-buffer source (gigs_gbuffer_post masks a pixel whose world normal has a zero component: every pixel of an axis-aligned box)."""
    import scenes
    import test_gpu_mesh_shadow as ts
    v, f, n = lr.open_box()
    if tilted:
        v, n = ts._tilted(v, n)
    cam = scenes.look_at_camera((1.9, 0.35, 1.7), (0.4, 0.5, 0.3), IW, IH, 0.9)
    return ts._mesh(v, f, n, 0.25 + 0.5 * ts._rho(len(v))), {k: (_dev(x) if isinstance(x, np.ndarray) else x) for k, x in cam.items()}


def test_raytraced_light_denoise_is_atrous_on_the_prepared_arrays():
    import denoise
    import mesh_render
    m, cam = _box_view()
    sky = _dev(lr.hash_sky(8, top=2.0))
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, seed=6, cube=sky, bounces=1, light_rays=64, device=DEV) as tracer, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, seed=6, device=DEV) as bare:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        assert 300 < int(cover.sum()) < IW * IH
        assert tracer.plane_distance() == 0.1 * tracer.ao_distance
        t = tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover)
        kept = {k: x.clone() for k, x in t.items() if isinstance(x, torch.Tensor)}
        d = tracer.denoise(t)
        signal = torch.cat([t["occlusion"], t["irradiance"], t["indirect"]], 0)
        want, var, rep = denoise.atrous(signal, t["points"], t["normals"], t["mask"], [1, 3, 3], denoise.ITERATIONS,
                                        plane_distance=0.1 * tracer.ao_distance)
        assert np.array_equal(_bits(d["occlusion"]), _bits(want[0:1])) and np.array_equal(_bits(d["irradiance"]), _bits(want[1:4]))
        assert np.array_equal(_bits(d["indirect"]), _bits(want[4:7]))
        for j, k in enumerate(("occlusion", "irradiance", "indirect")):
            assert np.array_equal(_bits(d[k + "_variance"]), _bits(var[j:j + 1])) and tuple(d[k].shape) == tuple(t[k].shape)
        assert d["denoise_report"] == dict(rep, planes=["occlusion", "irradiance", "indirect"]) and rep["live"] == int(cover.sum())
        assert json.loads(json.dumps(d["denoise_report"])) == d["denoise_report"]
        assert not torch.equal(d["occlusion"], t["occlusion"]) and float(d["occlusion_variance"].max()) > 0
        assert all(_same_bytes(t[k], x) for k, x in kept.items())  # the traced dict is left as it was
        assert d["hits"] is t["hits"] and d["report"] == t["report"]
        assert np.array_equal(_bits(d["occlusion"])[0][~cover.cpu().numpy()], _bits(t["occlusion"])[0][~cover.cpu().numpy()])
        # keywords reach the filter
        d2 = tracer.denoise(t, 2, sigma_l=0.0, plane_distance=0.05)
        want2, _, rep2 = denoise.atrous(signal, t["points"], t["normals"], t["mask"], [1, 3, 3], 2, plane_distance=0.05, sigma_l=0.0)
        assert np.array_equal(_bits(d2["irradiance"]), _bits(want2[1:4])) and d2["denoise_report"]["iterations"] == 2
        # without a cube: the occlusion alone
        tb = bare.planes(o["pos"], o["normal"], cam["viewmatrix"], cover)
        db = bare.denoise(tb, 3)
        wb, vb, _ = denoise.atrous(tb["occlusion"], tb["points"], tb["normals"], tb["mask"], [1], 3, plane_distance=bare.plane_distance())
        assert np.array_equal(_bits(db["occlusion"]), _bits(wb)) and db["irradiance"] is None and "irradiance_variance" not in db
        assert db["denoise_report"]["planes"] == ["occlusion"]
        # the glossy planes, guided by the roughness as well
        r = tracer.reflections(o["pos"], o["normal"], o["roughness"], cam["viewmatrix"], cam["campos"], cover)
        dr = tracer.denoise(r, 2)
        sig = torch.cat([r["specular"], r["reflected"], r["visibility"]], 0)
        wr, vr, rr_ = denoise.atrous(sig, r["points"], r["normals"], r["mask"], [3, 3, 1], 2, plane_distance=tracer.plane_distance(),
                                     roughness=r["roughness"])
        assert np.array_equal(_bits(dr["specular"]), _bits(wr[0:3])) and np.array_equal(_bits(dr["reflected"]), _bits(wr[3:6]))
        assert np.array_equal(_bits(dr["visibility"]), _bits(wr[6:7])) and np.array_equal(_bits(dr["visibility_variance"]), _bits(vr[2:3]))
        assert dr["denoise_report"]["roughness_sigma"] == denoise.ROUGHNESS_SIGMA and dr["denoise_report"]["planes"] == ["specular", "reflected", "visibility"]
        with pytest.raises(ValueError, match="planes\\(\\) or reflections\\(\\)"):
            tracer.denoise(dict(points=t["points"]))
        with pytest.raises(ValueError, match="iterations"):
            tracer.denoise(t, 0)


def test_filtered_occlusion_is_closer_to_the_converged_one():
    """The open box at 48 x 36, occlusion at 64 rays against the same view at 1024 rays, shipped defaults: a filter that raises
    the error has no use, so RMSE(filtered) < RMSE(raw) is a condition.  Measured on an MI355X: see DESIGN.md, "Denoising
    ray-traced planes"."""
    import mesh_render
    m, cam = _box_view()
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, mesh_render.RaytracedLight(m, rays=R, rotations=K, seed=6, device=DEV) as tracer:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        t = tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover)
        ref = tracer.planes(o["pos"], o["normal"], cam["viewmatrix"], cover, rays=1024)
        assert ref["report"]["rays"] == 1024 and t["report"]["rays"] == R
        d = tracer.denoise(t)
        rmse = lambda x: float((x[0][cover].double() - ref["occlusion"][0][cover].double()).pow(2).mean().sqrt())  # noqa: E731
        raw, filtered = rmse(t["occlusion"]), rmse(d["occlusion"])
        print("occlusion at %d rays against %d rays over %d pixels: RMSE raw %.5f, filtered %.5f, ratio %.3f (%d iterations)" % (
            R, 1024, int(cover.sum()), raw, filtered, filtered / raw, d["denoise_report"]["iterations"]))
        assert raw > 0 and filtered < raw


def test_raytraced_gbuffer_denoise_keyword():
    import mesh_render
    import relight
    import scenes
    import test_gpu_mesh_gather as tg
    m, cam, vd, light = tg._relight_setup()
    gi = scenes.GI_DEFAULTS
    sky = _dev(lr.hash_sky(8, top=2.0))
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, ao_distance=1.0, bias=0.05, cube=sky, light_rays=64, device=DEV) as tracer:
        inner = mesh_render.MeshGBuffer(gi)

        def run(**kw):
            source = mesh_render.RaytracedGBuffer(inner, tracer, reflections=True, **kw)
            b = source(cam, rast)
            flat = {k: x.clone() for k, x in b.items() if isinstance(x, torch.Tensor)}
            flat.update({"extra." + k: x.clone() for k, x in b["extra"].items()})
            return flat, source

        absent, _ = run()
        zero, s0 = run(denoise=0)
        assert sorted(absent) == sorted(zero) and all(tg._same(absent[k], zero[k]) and absent[k].dtype == zero[k].dtype for k in absent)
        assert s0.denoise == 0 and s0.denoise_report is None and s0.reflection_denoise_report is None
        two, s2 = run(denoise=2)
        assert sorted(two) == sorted(absent)
        traced = {"occlusion"} | {k for k in absent if k.startswith("extra.raytraced_")}
        assert len(traced) == 7
        for k in absent:
            assert (not tg._same(absent[k], two[k])) == (k in traced), k
        b = inner(cam, rast)
        t = tracer.planes(b["depth_pos"], b["normals_view"], cam["viewmatrix"], b["mask_u8"], normal_space="view")
        d = tracer.denoise(t, 2)
        assert torch.equal(two["occlusion"], d["occlusion"]) and torch.equal(two["extra.raytraced_irradiance"], d["irradiance"])
        assert s2.denoise_report == d["denoise_report"] and s2.reflection_denoise_report["planes"] == ["specular", "reflected", "visibility"]
        assert s2.report == t["report"]
        # the relighter shades with the filtered plane
        out = relight.Relighter(light, gi, 0, source=mesh_render.RaytracedGBuffer(inner, tracer, denoise=2))(cam, rast, vd)
        assert torch.equal(out["occlusion"], d["occlusion"]) and torch.equal(out["raytraced_occlusion"], d["occlusion"])
        for bad in (-1, 6, 1.0, True):
            with pytest.raises(ValueError, match="denoise"):
                mesh_render.RaytracedGBuffer(inner, tracer, denoise=bad)


def test_analytic_relighter_denoise_keyword():
    import analytic_lights as al
    import denoise
    import mesh_render
    import scenes
    import test_gpu_mesh_shadow as ts
    m, cam = _box_view(tilted=True)
    lights = al.parse_lights(ts._image_lights())
    L = len(lights)
    source = mesh_render.MeshGBuffer(scenes.GI_DEFAULTS)
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, mesh_render.RaytracedLight(m, rotations=K, seed=6, bias=0.05, device=DEV) as tracer:
        plain = al.AnalyticRelighter(lights, source, tracer=tracer, samples=4, gamma=False)(cam, rast)
        zero = al.AnalyticRelighter(lights, source, tracer=tracer, samples=4, gamma=False, denoise=0)(cam, rast)
        assert all(_same_bytes(plain[k], zero[k]) for k in plain if isinstance(plain[k], torch.Tensor)) and plain["report"] == zero["report"]
        two = al.AnalyticRelighter(lights, source, tracer=tracer, samples=4, gamma=False, denoise=2)(cam, rast)
        assert not torch.equal(two["shadow"], plain["shadow"]) and not torch.equal(two["lights_rgb"], plain["lights_rgb"])
        for l in range(L):  # each light's plane as a one-channel call filters it
            want, _, rep = denoise.atrous(plain["shadow"][l:l + 1], plain["points"], plain["normals"], plain["mask"], None, 2,
                                          plane_distance=tracer.plane_distance())
            assert np.array_equal(_bits(two["shadow"][l:l + 1]), _bits(want)), l
        assert {k: v for k, v in two["report"].items() if k != "denoise"} == plain["report"]
        assert len(two["report"]["denoise"]) == 1 and two["report"]["denoise"][0]["channels"] == L and two["report"]["denoise"][0]["iterations"] == 2
        d, s = al.shade_lights(two["points"], two["normals"], source(cam, rast)["albedo_map"].reshape(3, -1).t().contiguous(),
                               source(cam, rast)["roughness_map"].reshape(-1), None, cam["campos"], lights,
                               two["shadow"].reshape(L, -1).t().contiguous(), two["mask"])
        assert torch.equal(two["lights_diffuse"], d.t().reshape(3, IH, IW)) and torch.equal(two["lights_specular"], s.t().reshape(3, IH, IW))
        with pytest.raises(ValueError, match="tracer"):
            al.AnalyticRelighter(lights, source, denoise=2)
        with pytest.raises(ValueError, match="denoise"):
            al.AnalyticRelighter(lights, source, tracer=tracer, denoise=6)


# ---- 3: tools -------------------------------------------------------------------------------------------------------------------
def _finite(x):
    if isinstance(x, dict):
        return all(_finite(v) for v in x.values())
    if isinstance(x, (list, tuple)):
        return all(_finite(v) for v in x)
    return x is None or isinstance(x, (str, bool)) or math.isfinite(x)


def _without(x, keys):
    """A JSON value with the dict entries of those names removed at every depth."""
    if isinstance(x, dict):
        return {k: _without(v, keys) for k, v in x.items() if k not in keys}
    if isinstance(x, list):
        return [_without(v, keys) for v in x]
    return x


def test_tools(tmp_path):
    import densify
    import optim
    import relight
    import relight_scene
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    import test_gpu_mesh_shadow as ts
    import train_iteration as ti
    from PIL import Image
    v, f, n = ts._blob()
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=1, n_test=1, size=32)
    out = str(tmp_path / "run")
    os.makedirs(out)
    scene_io.save_mesh_ply(os.path.join(out, "blob.ply"), *ts._mesh(v, f, n, 0.25 + 0.5 * ts._rho(len(v))))
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    centre, extent = 0.5 * (v.max(axis=0) + v.min(axis=0)), float((v.max(axis=0) - v.min(axis=0)).max())
    entries = [dict(kind="point", position=[float(x) for x in centre + np.array([0.0, 0.0, 2.0]) * extent], intensity=6.0 * extent * extent,
                    radius=0.1 * extent), dict(kind="directional", direction=[0.3, -0.2, -1.0], angle=1.0)]
    lights_json = str(tmp_path / "lights.json")
    with open(lights_json, "w") as fh:
        json.dump(entries, fh)
    base = ["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--split", "train", "--occlusion", "raytraced", "--lighting", "raytraced",
            "--reflections", "--lights", lights_json, "--shadow_samples", "4", "--ray_bias", "0.01"]
    folder = os.path.join(out, "mesh_train")

    def read(res):
        with open(res["raytraced_vs_screen_json"]) as fh:
            a = json.load(fh)
        with open(res["lights_report_json"]) as fh:
            b = json.load(fh)
        images = {x: np.array(Image.open(os.path.join(folder, x))) for x in sorted(os.listdir(folder)) if x.endswith(".png")}
        return a, b, images

    plain = render_mesh.render_mesh(base)
    a0, b0, img0 = read(plain)
    res = render_mesh.render_mesh(base + ["--denoise", "2", "--denoise_reference_rays", "128"])
    a1, b1, img1 = read(res)
    assert json.loads(json.dumps(res)) == res and sorted(img0) == sorted(img1) and res["files"] == plain["files"]
    # the JSONs without the flag are the JSONs with it minus the new keys
    new = {k for k in a1["views"][0] if k.startswith("psnr_denoised_")}
    assert len(new) == 5 and "denoise" not in a0 and not any(k.startswith("psnr_denoised_") for k in a0["views"][0])
    assert _without(a1, new | {"denoise"}) == a0 and _without(b1, {"denoise"}) == b0
    assert _finite(a1) and _finite(b1) and a1["denoise"]["iterations"] == 2 and a1["denoise"]["reference_rays"] == 128 and b1["denoise"] == 2
    assert a1["denoise"]["planes"]["planes"] == ["occlusion", "irradiance", "indirect"]
    assert a1["denoise"]["reflections"]["planes"] == ["specular", "reflected", "visibility"]
    rows = a1["denoise"]["rmse"]
    assert [r["image_name"] for r in rows] == [x["image_name"] for x in a1["views"]]
    for r in rows:
        assert sorted(k for k in r if k != "image_name") == ["indirect", "irradiance", "occlusion", "reflected", "specular", "visibility"]
        print("%s: RMSE against 128 rays, raw -> filtered: %s" % (r["image_name"], ", ".join(
            "%s %.4g -> %.4g" % (k, x["raw"], x["filtered"]) for k, x in r.items() if k != "image_name")))
        assert all(x["raw"] > 0 and x["filtered"] > 0 for k, x in r.items() if k != "image_name")
    assert all(len(x["denoise"]) == 1 and x["denoise"][0]["iterations"] == 2 and x["denoise"][0]["channels"] == 2 for x in b1["views"])
    # the filtered planes reach the files: the traced ones change, the rasterized ones do not
    name = a1["views"][0]["image_name"]
    for suffix, changes in (("occlusion", True), ("raytraced_diffuse", True), ("raytraced_specular", True), ("shadow_1", True),
                            ("lights", True), ("albedo", False), ("depth", False), ("normal", False)):
        x = "%s_%s.png" % (name, suffix)
        assert (not np.array_equal(img0[x], img1[x])) == changes, x
    for bad, match in ((["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--denoise", "2"], "denoise"), (base + ["--denoise", "6"], "denoise"),
                       (base + ["--denoise_reference_rays", "128"], "denoise_reference_rays"),
                       (base + ["--denoise", "2", "--denoise_reference_rays", "100"], "denoise_reference_rays"),
                       (["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--lights", lights_json, "--no_shadows", "--denoise", "1"], "denoise")):
        with pytest.raises(ValueError, match=match):
            render_mesh.render_mesh(bad)
    # relight_scene.py --denoise: needs --occluder; the occlusion and the shadows are filtered
    g = ti.raw_from_scene(scenes.surface_scene(P=2000, sh_degree=0, seed=3, scale_mu=0.05), DEV)
    opt = optim.FusedAdam([{"params": [g[k]], "lr": 0.0, "name": k} for k in g], lr=0.0, eps=1e-15)
    light = relight.make_light(torch.from_numpy(scenes.synthetic_envmap(64, 128)).to(DEV) * 0.5, res=256)
    ck = os.path.join(out, "chkpnt7.pth")
    scene_io.save_checkpoint(ck, scene_io.capture(0, g, densify.DensifyState(g["xyz"].shape[0], DEV), opt, 1.0), light.state_dict(), {}, 7)
    common = ["-m", out, "--checkpoint", ck, "--hdri", hdr, "--skip_train", "--lights", lights_json, "--occluder", "blob.ply",
              "--shadow_samples", "2", "--ray_bias", "0.02"]
    folder = os.path.join(out, "test", "ours_7", "relight")

    def read_scene(res):
        with open(res["test"]["analytic_lights"]["report_json"]) as fh:
            rep = json.load(fh)
        return rep, {x: np.array(Image.open(os.path.join(folder, x))) for x in sorted(os.listdir(folder)) if x.endswith(".png")}

    c0 = relight_scene.relight_scene(common)
    r0, i0 = read_scene(c0)
    c1 = relight_scene.relight_scene(common + ["--denoise", "3"])
    r1, i1 = read_scene(c1)
    assert json.loads(json.dumps(c1)) == c1 and sorted(i0) == sorted(i1) and c1["test"]["files"] == c0["test"]["files"]
    assert _without(r1, {"denoise"}) == r0 and r1["denoise"] == 3 and _finite(r1) and "denoise" not in r0
    assert "occluder_denoise" not in c0["test"] and c1["test"]["occluder_denoise"]["iterations"] == 3 and c1["test"]["occluder"] == c0["test"]["occluder"]
    assert c1["test"]["occluder_denoise"]["planes"] == ["occlusion"] and _finite(c1["test"]["occluder_denoise"])
    changed = sorted(x for x in i0 if not np.array_equal(i0[x], i1[x]))
    assert any(x.endswith("_shadow_1.png") for x in changed) and any(x.endswith("_lights.png") for x in changed)
    for bad in (["-m", out, "--checkpoint", ck, "--hdri", hdr, "--skip_train", "--denoise", "2"], common + ["--denoise", "-1"]):
        with pytest.raises(ValueError, match="denoise"):
            relight_scene.relight_scene(bad)
