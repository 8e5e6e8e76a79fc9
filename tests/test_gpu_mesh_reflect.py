"""GPU: ray-traced reflections per point (csrc/mesh_reflect.hip through mesh.reflect_points, mesh_render.compose_reflections,
RaytracedLight.reflections, RaytracedGBuffer(reflections=True), render_mesh.py --reflections) against the numpy restatement
(tests/mesh_reflect_ref.py).  Counts and counters by array_equal, float outputs as bit patterns: the trace is float64 + - * /
without contraction in a fixed summation order and the compose is float32 without contraction, so there is no tolerance
anywhere but for the prepared arrays of an image, which pass through torch's float64 sqrt and are held within one float32 ulp,
and for the comparison with the shade under a constant light, whose bound is derived where it is used.  The meshes and point
sets are those of tests/test_gpu_mesh_gather.py."""
import json
import os
import types
from argparse import Namespace

import numpy as np
import pytest
import torch

import mesh_gather_ref as gr
import mesh_light_ref as lr
import mesh_reflect_ref as fr
import test_gpu_mesh_gather as tg
from test_gpu_mesh_gather import DEV, _bits, _dev

pytestmark = pytest.mark.gpu

R, K = 64, 4


def _inputs(name):
    """The point set of the gather tests with views, roughness and one more dead point: a view of length 1.01."""
    p, pn, mask = tg._points(name)
    views = fr.hash_views(pn)
    views[6] = views[6] * np.float32(1.01)
    return p, pn, views, fr.hash_roughness(len(p)), mask


def _compare(what, got, report, want):
    differ = {k: int((_bits(getattr(got, k)) != _bits(want[k])).sum()) for k in fr.OUTPUTS if want[k] is not None}
    valid, blocked = got.valid.cpu().numpy(), got.blocked.cpu().numpy()
    print("%s: %d points, valid differ at %d, blocked at %d, bit patterns that differ %s; counters %s, restated %s" % (
        what, len(valid), int((valid != want["valid"]).sum()), int((blocked != want["blocked"]).sum()), differ, fr.counters(report),
        fr.counters(want)))
    assert got.valid.dtype == torch.int32 and np.array_equal(valid, want["valid"])
    assert got.blocked.dtype == torch.int32 and np.array_equal(blocked, want["blocked"])
    for k in fr.OUTPUTS:
        if want[k] is None:
            assert getattr(got, k) is None, k
        else:
            assert getattr(got, k).dtype == torch.float32 and np.array_equal(_bits(getattr(got, k)), _bits(want[k])), k
    assert fr.counters(report) == fr.counters(want)


# ---- 1: the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rays,levels,sky,extra", [
    ("open_box", R, 4, True, {}), ("crease", R, 16, True, {}), ("fan", R, 4, True, {}), ("blob", R, 16, True, {}),
    ("open_box", 128, 16, True, {}), ("open_box", R, 4, False, {}), ("crease", R, 4, True, dict(max_distance=4.0))])
def test_reflect_points_equals_the_restatement(name, rays, levels, sky, extra):
    import mesh
    v, f, n, kw, _ = tg._case(name)
    p, pn, views, rough, mask = _inputs(name)
    kw = dict(kw, **extra)
    table = fr.ggx_table(rays, K, levels)
    cube = lr.hash_sky() if sky else None
    Q = gr.hash_radiosity(len(v))
    want = fr.reflect_points(p, pn, views, rough, v, f, table, cube, Q, mask=mask, **kw)
    got, report = mesh.reflect_points(_dev(p), _dev(pn), _dev(views), _dev(rough), tg._mesh(v, f, n), None if cube is None else _dev(cube),
                                      _dev(Q), rays=rays, levels=levels, rotations=K, mask=_dev(mask), cell=want["grid"]["cell"], **kw)
    assert json.loads(json.dumps(report)) == report
    assert (report["n"], report["rays"], report["rotations"], report["levels"], report["seed"]) == (len(p), rays, K, levels, kw.get("seed", 0))
    assert report["bias"] == want["bias"] and report["max_distance"] == extra.get("max_distance")
    assert report["sky_res"] == (8 if sky else None) and report["radiosity"] is True
    _compare("%s R=%d L=%d sky=%s %s" % (name, rays, levels, sky, extra), got, report, want)
    N = len(p)
    assert report["masked"] == (N + 4) // 5 and report["no_normal"] == 3 and report["no_view"] == 1
    live = N - report["masked"] - 4
    valid = got.valid.cpu().numpy()
    assert int(valid.sum()) + report["below_horizon"] == rays * live
    assert report["misses"] + report["front_hits"] + report["back_hits"] == int(valid.sum()) > 0 and report["below_horizon"] > 0
    dead = (mask == 0) | np.isin(np.arange(N), (1, 2, 3, 6))
    assert (valid[dead] == 0).all() and (got.blocked.cpu().numpy()[dead] == 0).all() and (got.visibility.cpu().numpy()[dead] == 1).all()
    if sky:
        assert (got.specular.cpu().numpy()[dead] == 0).all() and (got.reflected.cpu().numpy()[dead] == 0).all()
        assert float(got.specular.max()) > 0 and (got.reflected.cpu().numpy() <= got.specular.cpu().numpy()).all()
    if name == "open_box" and sky:
        assert report["front_hits"] > 0 and report["misses"] > 0 and float(got.reflected.max()) > 0
    if extra:  # a finite distance: hits beyond it see the sky
        free, r0 = mesh.reflect_points(_dev(p), _dev(pn), _dev(views), _dev(rough), tg._mesh(v, f, n), _dev(cube), _dev(Q), rays=rays,
                                       levels=levels, rotations=K, mask=_dev(mask), cell=want["grid"]["cell"],
                                       **dict(kw, max_distance=None))
        assert report["misses"] > r0["misses"] and r0["max_distance"] is None
    # the table handed over as an array gives the same bits as the one computed from its parameters
    again, r1 = mesh.reflect_points(_dev(p), _dev(pn), _dev(views), _dev(rough), tg._mesh(v, f, n), None if cube is None else _dev(cube),
                                    _dev(Q), directions=table, mask=_dev(mask), cell=want["grid"]["cell"], **kw)
    assert fr.counters(r1) == fr.counters(report) and np.array_equal(_bits(again.visibility), _bits(got.visibility))


# ---- 2: the grid does not show -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["open_box", "blob"])
def test_grid_independence(name):
    import mesh
    import mesh_raycast_ref as rr
    v, f, n, kw, _ = tg._case(name)
    p, pn, views, rough, mask = _inputs(name)
    m = tg._mesh(v, f, n)
    g = rr.build_grid(v, f)
    _, bias = rr.bake_defaults(g)  # the default follows the grid's box: pin it
    args = dict(cube=_dev(lr.hash_sky()), radiosity=_dev(gr.hash_radiosity(len(v))), rays=R, rotations=K, levels=16, bias=bias,
                seed=kw.get("seed", 0), mask=_dev(mask))
    pts = (_dev(p), _dev(pn), _dev(views), _dev(rough))
    one, r1 = mesh.reflect_points(*pts, m, cell=1e6 * g["cell"], **args)
    assert r1["dims"] == [1, 1, 1] and r1["front_hits"] + r1["back_hits"] > 0
    for scale in (0.5, 3.0):
        got, r = mesh.reflect_points(*pts, m, cell=scale * g["cell"], **args)
        assert torch.equal(got.valid, one.valid) and torch.equal(got.blocked, one.blocked) and fr.counters(r) == fr.counters(r1)
        for k in fr.OUTPUTS:
            assert np.array_equal(_bits(getattr(got, k)), _bits(getattr(one, k))), (name, scale, k)


# ---- 3: empty inputs and what is refused ---------------------------------------------------------------------------------------
def test_empty_inputs_and_refusals():
    import mesh
    v, f, n, kw, _ = tg._case("crease")
    m = tg._mesh(v, f, n)
    sky = _dev(lr.hash_sky())
    e3, e1 = torch.zeros((0, 3), device=DEV), torch.zeros(0, device=DEV)
    got, rep = mesh.reflect_points(e3, e3, e3, e1, m, sky, rays=R)
    assert tuple(got.specular.shape) == (0, 3) and tuple(got.visibility.shape) == (0,) and fr.counters(rep) == (0,) * 7
    got, rep = mesh.reflect_points(e3, e3, e3, e1, m, rays=R)
    assert got.specular is None and got.reflected is None and got.valid.dtype == torch.int32 and got.blocked.dtype == torch.int32
    up = np.array([[0, 0, 1], [0, 0, 0], [0, 0, 1], [0, 0, 1]], np.float32)
    views = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 2]], np.float32)
    for faces in (np.zeros((0, 3), np.int32), np.array([[0, 1, 1]], np.int32)):
        flat = tg._mesh(np.zeros((3, 3), np.float32), faces, up[:3])
        got, rep = mesh.reflect_points(_dev(np.ones((4, 3), np.float32)), _dev(up), _dev(views), _dev(np.full(4, 0.5, np.float32)), flat, sky,
                                       rays=R, mask=_dev(np.array([1, 1, 0, 1], np.uint8)))
        assert (got.visibility == 1).all() and (got.valid == 0).all() and (got.blocked == 0).all() and (got.specular == 0).all()
        assert fr.counters(rep) == (0, 0, 0, 0, 1, 1, 1) and rep["pairs"] == 0 and rep["dims"] == [0, 0, 0]
        assert json.loads(json.dumps(rep)) == rep
    ok, _ = gr.face_points(v, f)
    ok = _dev(ok)
    r1 = torch.full((len(ok),), 0.5, device=DEV)
    for bad in (dict(rays=100), dict(rotations=65), dict(levels=0), dict(levels=65), dict(bias=-1.0), dict(max_distance=float("nan")),
                dict(cube=sky[:5]), dict(cube=-sky), dict(radiosity=torch.zeros((len(v), 2), device=DEV)),
                dict(mask=torch.zeros(len(ok), device=DEV)), dict(directions=np.zeros((4, 64, 3), np.float32))):
        with pytest.raises(ValueError):
            mesh.reflect_points(ok, ok, ok, r1, m, **dict(dict(rays=R), **bad))
    for a, b, c, d in ((ok[:, :2], ok, ok, r1), (ok, ok[:5], ok, r1), (ok, ok, ok[:5], r1), (ok, ok, ok, r1[:5]), (ok, ok, ok, r1.double())):
        with pytest.raises(ValueError):
            mesh.reflect_points(a, b, c, d, m, rays=R)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.reflect_points(ok.cpu(), ok, ok, r1, m, rays=R)


# ---- 4: the compose --------------------------------------------------------------------------------------------------------------
def _planes(N, seed):
    import mesh_distance_ref as dr
    u = lambda k, c: dr.uniform(seed, np.arange(N * c, dtype=np.uint64), k).astype(np.float32).reshape((N, c) if c > 1 else (N,))  # noqa: E731
    nrm = fr.hash_views(np.repeat([[0.0, 0.0, 1.0]], N, 0), seed=seed + 1, below_every=2)  # unit vectors on the whole sphere
    views = fr.hash_views(nrm, seed=seed + 2)
    return nrm, views, u(0, 1), u(1, 3) * np.float32(4.0), u(2, 3), u(3, 1)  # normals, views, roughness, radiance, albedo, metallic


def test_compose_equals_the_restatement_and_the_shade():
    import mesh_render
    import pbr
    from pbr.shade import pbr_shading
    N = 1000
    nrm, views, rough, rad, alb, met = _planes(N, 31)
    rough[:4] = (0.0, 1.0, 0.5, 1.0 / 512)
    mask = (np.arange(N) % 7 != 0).astype(np.uint8)
    vis = _planes(N, 37)[5]
    lut = pbr.get_brdf_lut()
    lut_np = lut.numpy()
    for what, kw_np, kw in (("plain", {}, {}), ("metallic", dict(albedo=alb, metallic=met), dict(albedo=_dev(alb), metallic=_dev(met))),
                            ("masked, visibility", dict(albedo=alb, metallic=met, mask=mask, visibility=vis),
                             dict(albedo=_dev(alb), metallic=_dev(met), mask=_dev(mask), visibility=_dev(vis)))):
        want = fr.compose(nrm, views, rough, rad, lut_np, **kw_np)
        got = mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), _dev(rad), brdf_lut=lut.to(DEV), **kw)
        print("compose, %s: bit patterns that differ %d of %d" % (what, int((_bits(got) != _bits(want)).sum()), want.size))
        assert got.dtype == torch.float32 and np.array_equal(_bits(got), _bits(want)), what
    assert (got.cpu().numpy()[mask == 0] == 0).all() and float(got.max()) > 0
    # the default table is the shade's
    assert torch.equal(mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), _dev(rad)),
                       mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), _dev(rad), brdf_lut=lut.to(DEV)))
    # radiance 1 against the shade under a light whose specular levels are the constant 1: the shade's lookup is then a sum
    # of bilinear and mip weights that add up to 1 within a few float32 roundings, and nothing else differs: 2^-20 relative
    H, W = 25, 40
    light = types.SimpleNamespace(diffuse=torch.ones((6, 16, 16, 3), device=DEV),
                                  specular=[torch.ones((6, r, r, 3), device=DEV) for r in (64, 32, 16, 8)])
    one = torch.ones((N, 3), device=DEV)
    hw = lambda a, c: _dev(a).reshape(H, W, c)  # noqa: E731
    for metallic in (False, True):
        mine = mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), one, _dev(alb), _dev(met) if metallic else None,
                                               brdf_lut=lut.to(DEV)).cpu().numpy().astype(np.float64)
        ref = pbr_shading(light, hw(nrm, 3), hw(views, 3), hw(alb, 3), hw(rough, 1), torch.ones((H, W, 1), device=DEV),
                          metallic=hw(met, 1) if metallic else None, brdf_lut=lut.to(DEV))["specular_rgb"]
        ref = ref.reshape(N, 3).cpu().numpy().astype(np.float64)
        err = float((np.abs(mine - ref) / np.abs(ref)).max())
        print("compose against pbr_shading, metallic %s: largest relative difference %.3g (bound %.3g)" % (metallic, err, 2.0 ** -20))
        assert (ref > 0).all() and err <= 2.0 ** -20
    with pytest.raises(ValueError, match="albedo"):
        mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), _dev(rad), metallic=_dev(met))
    with pytest.raises(ValueError, match="radiance"):
        mesh_render.compose_reflections(_dev(nrm), _dev(views), _dev(rough), _dev(rad)[:5])
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh_render.compose_reflections(torch.from_numpy(nrm), _dev(views), _dev(rough), _dev(rad))


# ---- 5: an image ---------------------------------------------------------------------------------------------------------------
def test_reflection_planes_equal_the_restatement():
    import mesh_distance_ref as dr
    import mesh_render
    IW, IH = tg.IW, tg.IH
    v, f, n = lr.open_box()
    m = tg._mesh(v, f, n, 0.25 + 0.5 * tg._rho(len(v)))
    sky, fine = lr.hash_sky(), lr.hash_sky(16, seed=12)
    cam, cam_np = tg._camera()
    rough = dr.uniform(41, np.arange(IW * IH, dtype=np.uint64), 0).astype(np.float32).reshape(1, IH, IW)
    L = 8
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, seed=6, cube=_dev(sky), bounces=1, light_rays=64, device=DEV) as tracer:
        o = rast(cam)
        cover = o["tri_id"] >= 0
        for cube, rays in ((None, None), (fine, 128)):
            t = tracer.reflections(o["pos"], o["normal"], _dev(rough), cam["viewmatrix"], cam["campos"], cover, levels=L, rays=rays,
                                   cube=None if cube is None else _dev(cube))
            rep = t["report"]
            n_cover = int(cover.sum())
            assert json.loads(json.dumps(rep)) == rep and rep["bounces"] == 1 and rep["rays"] == (rays or R) and rep["levels"] == L
            assert 100 < n_cover < IW * IH and rep["masked"] == IW * IH - n_cover and rep["n"] == IW * IH
            assert tuple(t["specular"].shape) == tuple(t["reflected"].shape) == (3, IH, IW)
            assert tuple(t["visibility"].shape) == (1, IH, IW) and tuple(t["valid"].shape) == tuple(t["blocked"].shape) == (IH, IW)
            assert (t["visibility"][0][~cover] == 1).all() and (t["valid"][~cover] == 0).all() and (t["specular"][:, ~cover] == 0).all()
            assert rep["sky_res"] == (8 if cube is None else 16)
            # the prepared views: numpy float64 on the prepared points, within one float32 ulp
            live = cover.reshape(-1).cpu().numpy()
            want_v = fr.prepare_views(t["points"].cpu().numpy(), cam_np["campos"])[live]
            got_v = t["views"].cpu().numpy().astype(np.float64)[live]
            ulp = np.spacing(np.abs(want_v).astype(np.float32)).astype(np.float64)
            print("views: largest error %.3g ulp" % float((np.abs(got_v - want_v) / ulp).max()))
            assert (np.abs(got_v - want_v) <= ulp).all()
            assert np.array_equal(_bits(t["roughness"]), _bits(rough.reshape(-1)))
            # the restatement fed the prepared arrays
            want = fr.reflect_points(t["points"].cpu().numpy(), t["normals"].cpu().numpy(), t["views"].cpu().numpy(), t["roughness"].cpu().numpy(),
                                     v, f, fr.ggx_table(rays or R, K, L), sky if cube is None else cube, tracer.radiosity[0].cpu().numpy(),
                                     bias=tracer.bias, seed=6, mask=t["mask"].cpu().numpy())
            got = types.SimpleNamespace(specular=t["specular"].reshape(3, -1).t(), reflected=t["reflected"].reshape(3, -1).t(),
                                        visibility=t["visibility"].reshape(-1), valid=t["valid"].reshape(-1), blocked=t["blocked"].reshape(-1))
            _compare("image, cube %s" % (cube is not None), got, rep, want)
            assert rep["front_hits"] > 0 and rep["misses"] > 0 and float(t["reflected"].max()) > 0
        t0 = tracer.reflections(o["pos"], o["normal"], _dev(rough), cam["viewmatrix"], cam["campos"], cover, levels=L, bounces=0)
        assert (t0["reflected"] == 0).all() and t0["report"]["bounces"] == 0 and t0["report"]["radiosity"] is False
        with pytest.raises(ValueError, match="bounces"):
            tracer.reflections(o["pos"], o["normal"], _dev(rough), cam["viewmatrix"], cam["campos"], cover, bounces=2)
        with pytest.raises(ValueError, match="roughness"):
            tracer.reflections(o["pos"], o["normal"], _dev(rough)[:, :5], cam["viewmatrix"], cam["campos"], cover)


def test_raytraced_gbuffer_with_reflections():
    import mesh_render
    import scenes
    m, cam, vd, light = tg._relight_setup()
    gi = scenes.GI_DEFAULTS
    sky = _dev(lr.hash_sky(8, top=2.0))
    keep = lambda b: {k: ({j: y.clone() for j, y in x.items()} if isinstance(x, dict) else  # noqa: E731
                          (x.clone() if isinstance(x, torch.Tensor) else x)) for k, x in b.items()}
    with mesh_render.MeshRasterizer(m, device=DEV) as rast, \
            mesh_render.RaytracedLight(m, rays=R, rotations=K, ao_distance=1.0, bias=0.05, cube=sky, bounces=1, light_rays=64,
                                       device=DEV) as tracer:
        plain = mesh_render.RaytracedGBuffer(mesh_render.MeshGBuffer(gi), tracer)
        off = keep(plain(cam, rast))
        source = mesh_render.RaytracedGBuffer(mesh_render.MeshGBuffer(gi), tracer, reflections=True)
        assert plain.reflections is False and source.reflections is True and source.replayable is False
        on = keep(source(cam, rast))
        new = ["raytraced_reflected", "raytraced_specular", "raytraced_specular_visibility"]
        assert sorted(on) == sorted(off) and sorted(set(on["extra"]) - set(off["extra"])) == new and plain.reflection_report is None
        for k in off:
            if k == "extra":
                assert all(tg._same(on[k][j], off[k][j]) for j in off[k])
            elif isinstance(off[k], torch.Tensor):
                assert tg._same(on[k], off[k]), k
            else:
                assert on[k] == off[k], k
        assert source.report == plain.report
        b = mesh_render.MeshGBuffer(gi)(cam, rast)
        t = tracer.reflections(b["depth_pos"], b["normals_view"], b["roughness_map"], cam["viewmatrix"], cam["campos"], b["mask_u8"],
                               normal_space="view")
        assert torch.equal(on["extra"]["raytraced_specular"], t["specular"]) and torch.equal(on["extra"]["raytraced_reflected"], t["reflected"])
        assert torch.equal(on["extra"]["raytraced_specular_visibility"], t["visibility"]) and source.reflection_report == t["report"]
        covered = b["mask_u8"] != 0
        rep = t["report"]
        print("traced reflections: %d pixels, visibility mean %.4f, misses %d, front %d, back %d, below %d" % (
            int(covered.sum()), float(t["visibility"][0][covered].mean()), rep["misses"], rep["front_hits"], rep["back_hits"],
            rep["below_horizon"]))
        assert rep["masked"] == int((~covered).sum()) and rep["misses"] > 0 and rep["front_hits"] > 0
        assert float(t["specular"].max()) > 0 and float(t["visibility"][0][covered].min()) < 1.0


# ---- 6: the tool ---------------------------------------------------------------------------------------------------------------
def test_render_mesh_reflections(tmp_path):
    import render_mesh
    import scene_io
    import scenes
    import synthetic_dataset
    from PIL import Image
    v, f, n = tg._blob()
    data = synthetic_dataset.write_synthetic_dataset(str(tmp_path / "scene"), n_train=2, n_test=1, size=32)
    out = str(tmp_path / "run")
    os.makedirs(out)
    scene_io.save_mesh_ply(os.path.join(out, "blob.ply"), *tg._mesh(v, f, n, 0.25 + 0.5 * tg._rho(len(v))))
    with open(os.path.join(out, "cfg_args"), "w") as fh:
        fh.write(str(Namespace(sh_degree=3, source_path=data, model_path=out, images="images", resolution=-1,
                               white_background=False, data_device="cuda", eval=True)))
    hdr = str(tmp_path / "sky.npy")
    np.save(hdr, scenes.synthetic_envmap(32, 64, seed=2))
    base = ["-m", out, "--mesh", "blob.ply", "--hdri", hdr, "--split", "train"]
    folder = os.path.join(out, "mesh_train")
    traced = base + ["--lighting", "raytraced", "--bounces", "1", "--light_rays", "64", "--sky_res", "16"]
    # without the flag: the files and the JSON of before
    res0 = render_mesh.render_mesh(traced)
    listing0 = sorted(os.listdir(folder))
    with open(res0["raytraced_vs_screen_json"]) as fh:
        cmp0 = json.load(fh)
    old = ["psnr_%s_bounces_%d" % (k, b) for k in ("baked", "screen") for b in (0, 1)]
    assert sorted(cmp0["average"]) == old and "raytraced_specular" not in res0 and "raytraced" not in res0
    assert sorted(cmp0) == sorted(["mesh", "bounces", "sky_res", "rays", "light_rays", "light", "tracer", "views", "average"])
    assert not any(x.endswith(("_raytraced_specular.png", "_raytraced.png")) for x in listing0)
    # with it: two more PNGs a view, the new keys, everything finite, and the rest of the JSON as it was
    res = render_mesh.render_mesh(traced + ["--reflections", "--reflection_rays", "64", "--roughness_levels", "8", "--reflection_sky_res", "64"])
    assert json.loads(json.dumps(res)) == res and res["files"] == res0["files"]
    with open(res["raytraced_vs_screen_json"]) as fh:
        cmp = json.load(fh)
    key = "psnr_specular_screen_bounces_1"
    print("ray-traced specular against the screen-space shade:", json.dumps(cmp["average"]))
    assert sorted(cmp["average"]) == sorted(old + [key]) and cmp["average"] == res["raytraced_vs_screen"] and len(cmp["views"]) == 2
    assert (cmp["reflection_rays"], cmp["roughness_levels"], cmp["reflection_sky_res"]) == (64, 8, 64)
    rep = cmp["reflections"]
    assert rep["n"] == 32 * 32 and rep["rays"] == 64 and rep["levels"] == 8 and rep["sky_res"] == 64 and rep["bounces"] == 1
    assert rep["misses"] > 0 and rep["misses"] + rep["front_hits"] + rep["back_hits"] + rep["below_horizon"] == 64 * (32 * 32 - rep["masked"] - rep["no_normal"] - rep["no_view"])
    for view, view0 in zip(cmp["views"], cmp0["views"]):
        assert np.isfinite(view[key]) and view[key] > 0 and {k: x for k, x in view.items() if k != key} == view0
    assert {k: x for k, x in cmp.items() if k in cmp0 and k not in ("views", "average")} == {k: x for k, x in cmp0.items() if k not in ("views", "average")}
    assert len(res["raytraced_specular"]) == len(res["raytraced"]) == 2 and res["raytraced_diffuse"] == res0["raytraced_diffuse"]
    for path, tail in [(p, "_raytraced_specular.png") for p in res["raytraced_specular"]] + [(p, "_raytraced.png") for p in res["raytraced"]]:
        img = np.array(Image.open(path))
        assert path.endswith(tail) and img.shape[:2] == (32, 32) and int(img.max()) > 0
    assert sorted(set(os.listdir(folder)) - set(listing0)) == sorted(os.path.basename(p) for p in res["raytraced_specular"] + res["raytraced"])
    with pytest.raises(ValueError, match="reflections needs --lighting raytraced"):
        render_mesh.render_mesh(base + ["--reflections"])
