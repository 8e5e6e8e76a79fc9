"""GPU parity tests: the HIP path (through the C ABI, via the drop-in Python package) against
the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star / SURVEY 8(c)):
  * bit-exact: radii, tiles_touched, point_offsets, depth sort keys, point_list, ranges;
  * n_contrib: bit-exact except pixels where the ulp difference between OCML expf and glibc
    expf flips one of the three threshold tests (alpha < 1/255, T(1-alpha) < 1e-4, power > 0);
    those are counted and bounded (<= 1e-4 of the pixels) and excluded from the max-error check;
  * fp32 planes and gradients: mean per-pixel L1 <= 1e-4 (tolerance stated by north_star).
"""
import os

import numpy as np
import pytest
import torch

import gigs_lib
import scenes
from helpers import GAUSS_KEYS, focal, oracle_forward, random_pix_grads, set_options, small_scene

pytestmark = pytest.mark.gpu

L1_TOL = 1e-4  # north_star: "within 1e-4 per-pixel L1"
DEV = "cuda:0"


def _dgr():
    import diff_gaussian_rasterization as dgr
    return dgr


def tt(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if grad:
        t.requires_grad_(True)
    return t


def settings(dgr, cam, sh_degree, bg=(0, 0, 0), gi=scenes.GI_DEFAULTS, inference=False, argmax_depth=False, debug=False,
             scale_modifier=1.0, prefiltered=False):
    return dgr.GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"],
        tanfovy=cam["tanfovy"], radius=gi["radius"], bias=gi["bias"], thick=gi["thick"], delta=gi["delta"],
        step=gi["step"], start=gi["start"], bg=tt(np.asarray(bg, np.float32)), scale_modifier=scale_modifier,
        viewmatrix=tt(cam["viewmatrix"]), projmatrix=tt(cam["projmatrix"]), sh_degree=sh_degree,
        campos=tt(cam["campos"]), prefiltered=prefiltered, debug=debug, inference=inference, argmax_depth=argmax_depth)


def hip_raw_forward(dgr, sc, cam, bg=(0, 0, 0), colors_precomp=None, cov3D_precomp=None, **kw):
    """_C.rasterize_gaussians + views into the scratch buffers."""
    st = settings(dgr, cam, sc["sh_degree"], bg=bg, **kw)
    e = torch.Tensor([])
    res = dgr._C.rasterize_gaussians(
        st.bg, tt(sc["means3D"]), e if colors_precomp is None else tt(colors_precomp), tt(sc["opacities"]),
        tt(sc["normal"]), tt(sc["albedo"]), tt(sc["roughness"]), tt(sc["metallic"]),
        e if cov3D_precomp is not None else tt(sc["scales"]), e if cov3D_precomp is not None else tt(sc["rotations"]),
        e if cov3D_precomp is None else tt(cov3D_precomp), e if colors_precomp is not None else tt(sc["shs"]),
        st.campos, st.viewmatrix, st.projmatrix, st.scale_modifier, st.tanfovx, st.tanfovy, st.image_height, st.image_width,
        st.sh_degree, st.prefiltered, st.argmax_depth, st.inference, st.debug)
    torch.cuda.synchronize()
    return res


def view(buf, off, dtype, count):
    itemsize = np.dtype(dtype).itemsize
    raw = buf[off:off + count * itemsize].cpu().numpy()
    return raw.view(dtype)


def scratch_views(dgr, res, P, W, H):
    import gigs_lib
    lib = gigs_lib.lib()
    R, geom, binning, img = res[0], res[3], res[4], res[5]
    N, T = W * H, ((W + 15) // 16) * ((H + 15) // 16)
    g = lambda which, dt, n: view(geom, lib.gigs_geom_offset(P, which), dt, n)  # noqa: E731
    out = dict(depths=g(0, np.float32, P), pos_view=g(1, np.float32, 3 * P), means2D=g(2, np.float32, 2 * P),
               cov3D=g(3, np.float32, 6 * P), conic_opacity=g(4, np.float32, 4 * P), rgb=g(5, np.float32, 3 * P),
               clamped=g(6, np.uint8, 3 * P), tiles_touched=g(7, np.uint32, P), point_offsets=g(8, np.uint32, P))
    if R > 0:
        b = lambda which, dt, n: view(binning, lib.gigs_binning_offset(R, which), dt, n)  # noqa: E731
        out.update(keys_unsorted=b(0, np.uint64, R), vals_unsorted=b(1, np.uint32, R), keys=b(2, np.uint64, R),
                   point_list=b(3, np.uint32, R))
    i = lambda which, dt, n: view(img, lib.gigs_image_offset(W, H, which), dt, n)  # noqa: E731
    out.update(final_T=i(0, np.float32, N), n_contrib=i(1, np.uint32, N), ranges=i(2, np.uint32, 2 * T))
    return out


def compare_planes(hip, ref, names, flip_mask=None, tag=""):
    for k in names:
        a, b = hip[k], ref[k]
        nan_a, nan_b = np.isnan(a), np.isnan(b)
        assert np.array_equal(nan_a, nan_b), f"{tag}{k}: NaN pattern differs"
        d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
        assert d.mean() <= L1_TOL, f"{tag}{k}: mean L1 {d.mean():.3e}"
        if flip_mask is not None:
            d = d[:, ~flip_mask]
        scale = max(1.0, np.nanmax(np.abs(b)))
        assert d.max() <= 2e-4 * scale, f"{tag}{k}: max abs {d.max():.3e} (scale {scale:.2f})"


PLANES = ["color", "opacity", "depth", "normal", "normal_view", "pos", "albedo", "roughness", "metallic"]


def hip_planes(res):
    keys = ["color", "radii", "geom", "bin", "img", "opacity", "depth", "normal", "normal_view", "pos", "albedo",
            "roughness", "metallic"]
    return {k: v.cpu().numpy() for k, v in zip(keys, res[1:]) if k not in ("geom", "bin", "img")}


def check_forward(orc, sc, cam, bg=(0.1, 0.3, 0.2), tag="", **kw):
    dgr = _dgr()
    okw = {k: v for k, v in kw.items() if k in ("inference", "argmax_depth", "scale_modifier")}
    extra = {}
    if "colors_precomp" in kw:
        extra.update(shs=None, colors_precomp=kw["colors_precomp"])
    if "cov3D_precomp" in kw:
        extra.update(scales=None, rotations=None, cov3D_precomp=kw["cov3D_precomp"])
    r, ref = oracle_forward(orc, sc, cam, bg=bg, **okw, **extra)
    res = hip_raw_forward(dgr, sc, cam, bg=bg, **kw)
    P, W, H = sc["means3D"].shape[0], cam["image_width"], cam["image_height"]
    assert res[0] == ref["num_rendered"], f"{tag}num_rendered {res[0]} vs {ref['num_rendered']}"
    hp = hip_planes(res)
    np.testing.assert_array_equal(hp["radii"], ref["radii"])
    sv = scratch_views(dgr, res, P, W, H)
    vis = ref["radii"] > 0
    # integer / index state: bit-exact.  The emission-order arrays (point_offsets, unsorted keys / values) exist only on
    # the reference-shaped path (GIGS_BINNING=legacy); the default tile-bucketed path produces the sorted state directly
    import gigs_lib
    legacy = gigs_lib.current().option("binning_legacy") == 1
    for k in ("tiles_touched", "ranges") + (("point_offsets",) if legacy else ()):
        np.testing.assert_array_equal(sv[k], r.state(k), err_msg=tag + k)
    if res[0] > 0:
        for k in (("keys_unsorted", "vals_unsorted") if legacy else ()) + ("keys", "point_list"):
            np.testing.assert_array_equal(sv[k], r.state(k), err_msg=tag + k)
    # per-Gaussian fp32 state: bit-exact too (same IEEE operation sequence, no FMA contraction)
    for k, w in (("depths", 1), ("means2D", 2), ("conic_opacity", 4), ("pos_view", 3)):
        np.testing.assert_array_equal(sv[k].reshape(P, w)[vis], r.state(k).reshape(P, w)[vis], err_msg=tag + k)
    if "cov3D_precomp" not in kw:
        np.testing.assert_array_equal(sv["cov3D"].reshape(P, 6)[vis], r.state("cov3D").reshape(P, 6)[vis])
    if "colors_precomp" not in kw:
        np.testing.assert_array_equal(sv["rgb"].reshape(P, 3)[vis], r.state("rgb").reshape(P, 3)[vis])
        np.testing.assert_array_equal(sv["clamped"].reshape(P, 3)[vis], r.state("clamped").reshape(P, 3)[vis])
    flips = (sv["n_contrib"] != r.state("n_contrib")).reshape(H, W)
    assert flips.mean() <= 1e-4, f"{tag}n_contrib differs on {flips.sum()} pixels"
    compare_planes(hp, ref, PLANES, flip_mask=flips, tag=tag)
    np.testing.assert_allclose(sv["final_T"].reshape(H, W)[~flips], r.state("final_T").reshape(H, W)[~flips], atol=1e-6)
    return r, ref, res, int(flips.sum())


# ------------------------------------------------------------------------------------------
def test_forward_c1_random_cloud(orc):
    """BASELINE config C1: 10k random Gaussians, 400x400, SH degree 0."""
    sc = scenes.random_scene(P=10_000, sh_degree=0, seed=0)
    cam = scenes.orbit_camera(0, 8, 400, 400)
    _, ref, res, nflip = check_forward(orc, sc, cam, bg=(0, 0, 0), tag="C1 ")
    assert res[0] > 50_000


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_forward_sh_degrees_and_ragged_image(orc, deg):
    # image size not a multiple of the 16x16 tile
    sc = scenes.random_scene(P=4000, sh_degree=deg, seed=deg, scale_mu=0.05)
    cam = scenes.orbit_camera(deg, 5, 203, 117)
    check_forward(orc, sc, cam, tag=f"deg{deg} ")


def test_forward_active_degree_below_allocated(orc):
    sc = scenes.random_scene(P=3000, sh_degree=3, seed=4, scale_mu=0.05)
    sc["sh_degree"] = 1  # M = 16 allocated, D = 1 active (gaussian_renderer/__init__.py:81)
    cam = scenes.orbit_camera(2, 5, 160, 96)
    check_forward(orc, sc, cam, tag="D<M ")


def test_forward_surface_scene_flags(orc):
    sc = scenes.surface_scene(P=20_000, sh_degree=2, seed=2, scale_mu=0.02)
    cam = scenes.orbit_camera(1, 6, 256, 192, radius=3.5)
    check_forward(orc, sc, cam, tag="surf ")
    check_forward(orc, sc, cam, inference=True, tag="inference ")
    check_forward(orc, sc, cam, argmax_depth=True, tag="argmax ")


def test_forward_precomputed_colour_and_covariance(orc):
    sc, cam = small_scene(P=2500, sh_degree=0, W=128, H=96, scale_mu=0.05)
    rng = np.random.default_rng(0)
    cols = rng.uniform(0, 1, size=(2500, 3)).astype(np.float32)
    r, _ = oracle_forward(orc, sc, cam)
    cov = r.state("cov3D").reshape(2500, 6).copy()
    check_forward(orc, sc, cam, colors_precomp=cols, tag="colors_precomp ")
    check_forward(orc, sc, cam, cov3D_precomp=cov, tag="cov3D_precomp ")


def test_forward_edge_cases(orc):
    dgr = _dgr()
    cam = scenes.orbit_camera(0, 4, 48, 32)
    # P == 0: outputs stay zero, rendered = 0 (rasterize_points.cu:190-191)
    sc = scenes.random_scene(P=0, sh_degree=0)
    res = hip_raw_forward(dgr, sc, cam)
    assert res[0] == 0 and float(res[1].abs().sum()) == 0
    # nothing visible: every Gaussian behind the camera -> background only, R = 0
    sc = scenes.random_scene(P=100, sh_degree=0)
    sc["means3D"] = (np.asarray(cam["campos"])[None] * 1.5 + 0.01 * sc["means3D"]).astype(np.float32)
    _, ref, res, _ = check_forward(orc, sc, cam, bg=(1.0, 0.5, 0.25), tag="behind ")
    assert res[0] == 0
    # one huge Gaussian covering every tile + a degenerate (zero-scale) one
    sc = scenes.random_scene(P=3, sh_degree=0, seed=1)
    sc["means3D"][:] = 0
    sc["scales"][0] = 5.0
    sc["scales"][1] = 0.0
    check_forward(orc, sc, cam, tag="huge ")
    # bad shape raises like AT_ERROR (rasterize_points.cu:159-161)
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        sc2 = dict(sc)
        sc2["means3D"] = sc["means3D"][:, :2].copy()
        hip_raw_forward(dgr, sc2, cam)


def test_forward_quadrant_cull_is_exact(orc, monkeypatch):
    """The blend kernel skips (Gaussian, 8x8 quadrant) pairs a conservative ellipse/box bound proves empty.
    Needle-shaped, mostly faint Gaussians (opacity around the 1/255 threshold) are the adversarial case:
    parity with the oracle as usual, and switching the cull off must not change a single bit of the
    per-pixel state or of any output plane (same kernel, same expf)."""
    rng = np.random.default_rng(7)
    sc = scenes.random_scene(P=6000, sh_degree=0, seed=7, scale_mu=0.06)
    sc["scales"] = np.ascontiguousarray(
        sc["scales"] * np.exp(rng.uniform(-3.0, 1.5, size=sc["scales"].shape)), dtype=np.float32)
    sc["opacities"] = np.ascontiguousarray(
        np.where(rng.uniform(size=(6000, 1)) < 0.5, rng.uniform(0.002, 0.02, size=(6000, 1)),
                 rng.uniform(0.02, 1.0, size=(6000, 1))), dtype=np.float32)
    cam = scenes.orbit_camera(3, 7, 240, 176)
    dgr = _dgr()
    _, _, res, _ = check_forward(orc, sc, cam, tag="needles ")
    sv = scratch_views(dgr, res, 6000, 240, 176)
    hp = hip_planes(res)
    set_options(monkeypatch, blend_cull=0)
    res0 = hip_raw_forward(dgr, sc, cam, bg=(0.1, 0.3, 0.2))
    sv0 = scratch_views(dgr, res0, 6000, 240, 176)
    hp0 = hip_planes(res0)
    for k in ("n_contrib", "final_T"):
        np.testing.assert_array_equal(sv[k].view(np.uint32), sv0[k].view(np.uint32), err_msg=k)
    for k in PLANES:
        np.testing.assert_array_equal(hp[k].view(np.uint32), hp0[k].view(np.uint32), err_msg=k)


def test_lite_rasterize_matches_full_forward(orc):
    """_C.lite_rasterize_gaussians (colour / opacity / depth "for baking", never called by the reference's own
    Python) returns the full operator's planes bit for bit, in both depth modes."""
    dgr = _dgr()
    sc, cam = small_scene(P=3000, sh_degree=1, W=144, H=96, scale_mu=0.05)
    e = torch.Tensor([])
    for argmax in (False, True):
        st = settings(dgr, cam, sc["sh_degree"], bg=(0.2, 0.1, 0.3), argmax_depth=argmax)
        full = hip_planes(hip_raw_forward(dgr, sc, cam, bg=(0.2, 0.1, 0.3), argmax_depth=argmax))
        R, col, opa, radii, dep = dgr._C.lite_rasterize_gaussians(
            st.bg, tt(sc["means3D"]), e, tt(sc["opacities"]), tt(sc["scales"]), tt(sc["rotations"]), e, tt(sc["shs"]),
            st.campos, st.viewmatrix, st.projmatrix, 1.0, st.tanfovx, st.tanfovy, st.image_height, st.image_width,
            st.sh_degree, False, argmax)
        assert R > 0
        np.testing.assert_array_equal(col.cpu().numpy(), full["color"])
        np.testing.assert_array_equal(opa.cpu().numpy(), full["opacity"])
        np.testing.assert_array_equal(dep.cpu().numpy(), full["depth"])
        np.testing.assert_array_equal(radii.cpu().numpy(), full["radii"])


def test_mark_visible(orc):
    dgr = _dgr()
    sc, cam = small_scene(P=5000, sh_degree=0)
    sc["means3D"] *= 4  # some behind the camera
    st = settings(dgr, cam, 0)
    got = dgr.GaussianRasterizer(st).markVisible(tt(sc["means3D"])).cpu().numpy()
    ref = orc.mark_visible(sc["means3D"], cam["viewmatrix"])
    np.testing.assert_array_equal(got, ref)
    assert 0 < got.sum() < 5000


# ------------------------------------------------------------------------------------------
def _backward_pair(orc, sc, cam, bg, seed, zero=(), scale_modifier=1.0):
    dgr = _dgr()
    H, W = cam["image_height"], cam["image_width"]
    r, ref = oracle_forward(orc, sc, cam, bg=bg, scale_modifier=scale_modifier)
    pg = random_pix_grads(np.random.default_rng(seed), H, W)
    for k in zero:
        pg[k][:] = 0
    want = r.backward(grad_color=pg["color"], grad_opacity=pg["opacity"], grad_depth=pg["depth"],
                      grad_normal=pg["normal"], grad_albedo=pg["albedo"], grad_roughness=pg["roughness"],
                      grad_metallic=pg["metallic"])
    st = settings(dgr, cam, sc["sh_degree"], bg=bg, scale_modifier=scale_modifier)
    t = {k: tt(sc[k], grad=True) for k in GAUSS_KEYS}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    outs = dgr._RasterizeGaussians.apply(t["means3D"], m2d, t["opacities"], t["normal"], t["albedo"], t["roughness"],
                                         t["metallic"], t["shs"], torch.Tensor([]), t["scales"], t["rotations"],
                                         torch.Tensor([]), st)
    color, radii, opacity, depth, normal, albedo, rough, metal, nview, pos = outs
    loss = ((color * tt(pg["color"])).sum() + (opacity * tt(pg["opacity"])).sum() + (depth * tt(pg["depth"])).sum()
            + (normal * tt(pg["normal"])).sum() + (albedo * tt(pg["albedo"])).sum()
            + (rough * tt(pg["roughness"])).sum() + (metal * tt(pg["metallic"])).sum()
            + 0.0 * nview.nan_to_num().sum() + 0.0 * pos.sum())
    loss.backward()
    torch.cuda.synchronize()
    got = dict(means3D=t["means3D"].grad, means2D=m2d.grad, opacity=t["opacities"].grad, normal=t["normal"].grad,
               albedo=t["albedo"].grad, roughness=t["roughness"].grad, metallic=t["metallic"].grad, sh=t["shs"].grad,
               scales=t["scales"].grad, rotations=t["rotations"].grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    return got, want, ref


def _check_grads(got, want, tag=""):
    for k in got:
        a, b = got[k].astype(np.float64), np.asarray(want[k], np.float64).reshape(got[k].shape)
        assert np.isfinite(a).all(), f"{tag}{k}: non-finite gradient"
        peak = max(np.abs(b).max(), 1e-20)
        # per-Gaussian L1 relative to the mean magnitude, and worst entry relative to the peak
        rel_l1 = np.abs(a - b).mean() / max(np.abs(b).mean(), 1e-20)
        rel_max = np.abs(a - b).max() / peak
        assert rel_l1 <= 2e-4, f"{tag}{k}: mean-relative L1 {rel_l1:.3e}"
        assert rel_max <= 2e-3, f"{tag}{k}: peak-relative max {rel_max:.3e}"


@pytest.mark.parametrize("deg,W,H,P", [(0, 64, 48, 400), (2, 203, 117, 3000), (3, 128, 128, 2000)])
def test_backward_matches_oracle(orc, deg, W, H, P):
    sc = scenes.random_scene(P=P, sh_degree=deg, seed=10 + deg, scale_mu=0.06)
    cam = scenes.orbit_camera(deg, 5, W, H)
    got, want, _ = _backward_pair(orc, sc, cam, (0.2, 0.1, 0.4), seed=deg)
    _check_grads(got, want, tag=f"deg{deg} ")
    assert np.abs(want["means3D"]).max() > 0 and np.abs(want["sh"]).max() > 0


def test_backward_stage2_pattern_and_linearity(orc, monkeypatch):
    """Stage-2 training feeds only albedo/roughness/metallic image gradients."""
    sc = scenes.surface_scene(P=8000, sh_degree=2, seed=5, scale_mu=0.03)
    cam = scenes.orbit_camera(0, 4, 160, 128, radius=3.5)
    zero = ("color", "opacity", "depth", "normal")
    got, want, _ = _backward_pair(orc, sc, cam, (0, 0, 0), seed=1, zero=zero)
    for k in ("albedo", "roughness", "metallic"):
        a, b = got[k], np.asarray(want[k]).reshape(got[k].shape)
        assert np.abs(a - b).mean() <= 2e-4 * max(np.abs(b).mean(), 1e-20)
    # detached blend weights: no gradient reaches geometry or colour from these planes
    for k in ("means3D", "scales", "rotations", "opacity", "sh", "means2D"):
        assert np.abs(got[k]).max() == 0.0, k
    # ... which the preprocess backward uses to skip the geometry chain and the SH read of such Gaussians: same
    # result as evaluating everything (GIGS_PRE_BWD_SH_SKIP=0)
    set_options(monkeypatch, pre_bwd_sh_skip=0)
    full, _, _ = _backward_pair(orc, sc, cam, (0, 0, 0), seed=1, zero=zero)
    for k in got:
        if k in ("albedo", "roughness", "metallic"):  # float atomics: equal to rounding
            np.testing.assert_allclose(got[k], full[k], rtol=1e-4, atol=1e-6 * max(np.abs(full[k]).max(), 1e-20))
        else:
            assert np.array_equal(got[k], full[k]), k


def test_backward_colour_gradient_on_part_of_the_image(orc):
    """The preprocess backward reads the SH block of a 256-Gaussian group only if one of its Gaussians
    received a colour gradient: order the cloud along screen x and feed a colour gradient on the left half of
    the image, so that some groups take the reading branch, some the skipping one, and some straddle."""
    sc = scenes.random_scene(P=6000, sh_degree=3, seed=21, scale_mu=0.03)
    cam = scenes.orbit_camera(0, 5, 192, 128)
    pv = np.c_[sc["means3D"], np.ones(len(sc["means3D"]))] @ np.asarray(cam["viewmatrix"], np.float64).reshape(4, 4)
    order = np.argsort(pv[:, 0] / np.maximum(pv[:, 2], 1e-3), kind="stable")  # screen x
    for k in GAUSS_KEYS:
        sc[k] = np.ascontiguousarray(sc[k][order])
    dgr = _dgr()
    H, W = cam["image_height"], cam["image_width"]
    r, _ = oracle_forward(orc, sc, cam, bg=(0.1, 0.2, 0.3))
    pg = random_pix_grads(np.random.default_rng(3), H, W)
    pg["color"][..., W // 3:] = 0
    for k in ("opacity", "depth", "normal"):
        pg[k][:] = 0
    want = r.backward(grad_color=pg["color"], grad_opacity=pg["opacity"], grad_depth=pg["depth"],
                      grad_normal=pg["normal"], grad_albedo=pg["albedo"], grad_roughness=pg["roughness"],
                      grad_metallic=pg["metallic"])
    st = settings(dgr, cam, sc["sh_degree"], bg=(0.1, 0.2, 0.3))
    t = {k: tt(sc[k], grad=True) for k in GAUSS_KEYS}
    m2d = torch.zeros_like(t["means3D"], requires_grad=True)
    outs = dgr._RasterizeGaussians.apply(t["means3D"], m2d, t["opacities"], t["normal"], t["albedo"], t["roughness"],
                                         t["metallic"], t["shs"], torch.Tensor([]), t["scales"], t["rotations"],
                                         torch.Tensor([]), st)
    loss = ((outs[0] * tt(pg["color"])).sum() + (outs[5] * tt(pg["albedo"])).sum()
            + (outs[6] * tt(pg["roughness"])).sum() + (outs[7] * tt(pg["metallic"])).sum())
    loss.backward()
    torch.cuda.synchronize()
    got = dict(means3D=t["means3D"].grad, sh=t["shs"].grad, scales=t["scales"].grad, rotations=t["rotations"].grad,
               opacity=t["opacities"].grad, albedo=t["albedo"].grad)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    _check_grads(got, {k: want[k] for k in got}, tag="partial ")
    per_group = np.abs(got["sh"]).reshape(len(order), -1).max(1)
    groups = [per_group[i:i + 256] for i in range(0, len(order), 256)]
    assert any(g.max() == 0 for g in groups) and any(g.max() > 0 for g in groups)
    assert any(g.max() > 0 and (g == 0).any() for g in groups)


def test_backward_scratch_gradients_c_abi(orc):
    """dL_dconic / dL_ddepth are allocated by the reference binding but not returned
    (rasterize_points.cu:302-303); check them through the raw C-ABI call."""
    dgr = _dgr()
    sc, cam = small_scene(P=800, sh_degree=1, W=96, H=64, scale_mu=0.06)
    H, W = 64, 96
    r, ref = oracle_forward(orc, sc, cam)
    pg = random_pix_grads(np.random.default_rng(3), H, W)
    r.backward(grad_color=pg["color"], grad_opacity=pg["opacity"], grad_depth=pg["depth"], grad_normal=pg["normal"],
               grad_albedo=pg["albedo"], grad_roughness=pg["roughness"], grad_metallic=pg["metallic"])
    res = hip_raw_forward(dgr, sc, cam)
    import gigs_lib
    lib = gigs_lib.lib()
    P = 800
    z = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    outs = dict(m2d=z(P, 3), conic=z(P, 2, 2), ddepth=z(P, 1), dop=z(P, 1), dn=z(P, 3), da=z(P, 3), dr=z(P, 1), dm=z(P, 1),
                dc=z(P, 3), dm3=z(P, 3), dcov=z(P, 6), dsh=z(P, 4, 3), dsc=z(P, 3), drot=z(P, 4))
    g = {k: tt(v) for k, v in pg.items()}
    ins = {k: tt(sc[k]) for k in GAUSS_KEYS}
    vm, pm, cp, bg = tt(cam["viewmatrix"]), tt(cam["projmatrix"]), tt(cam["campos"]), tt(np.zeros(3, np.float32))
    rc = lib.gigs_backward(None, P, 1, 4, res[0], bg.data_ptr(), W, H, ins["means3D"].data_ptr(), ins["shs"].data_ptr(), None,
                           ins["normal"].data_ptr(), ins["albedo"].data_ptr(), ins["roughness"].data_ptr(),
                           ins["metallic"].data_ptr(), ins["scales"].data_ptr(), ins["rotations"].data_ptr(), None,
                           vm.data_ptr(), pm.data_ptr(), cp.data_ptr(), res[2].data_ptr(), 1.0, cam["tanfovx"], cam["tanfovy"],
                           res[3].data_ptr(), res[4].data_ptr(), res[5].data_ptr(), g["depth"].data_ptr(), g["color"].data_ptr(),
                           g["opacity"].data_ptr(), g["normal"].data_ptr(), g["albedo"].data_ptr(), g["roughness"].data_ptr(),
                           g["metallic"].data_ptr(), outs["m2d"].data_ptr(), outs["conic"].data_ptr(), outs["ddepth"].data_ptr(),
                           outs["dop"].data_ptr(), outs["dn"].data_ptr(), outs["da"].data_ptr(), outs["dr"].data_ptr(),
                           outs["dm"].data_ptr(), outs["dc"].data_ptr(), outs["dm3"].data_ptr(), outs["dcov"].data_ptr(),
                           outs["dsh"].data_ptr(), outs["dsc"].data_ptr(), outs["drot"].data_ptr(), 1, None)
    assert rc == 0, lib.gigs_last_error()
    torch.cuda.synchronize()
    for name, got in (("dL_dconic", outs["conic"].cpu().numpy().reshape(-1)), ("dL_ddepth", outs["ddepth"].cpu().numpy().reshape(-1))):
        want = r.state(name)
        assert np.abs(got - want).mean() <= 2e-4 * max(np.abs(want).mean(), 1e-20), name
    # abs-gradient accumulator in means2D.z (backward.cu:618-619)
    assert np.all(outs["m2d"][:, 2].cpu().numpy() >= 0)


# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("march", ["exact", "default"])
def test_gi_passes_match_oracle(orc, march, monkeypatch):
    """SSAO / SSR against the oracle.  GIGS_GI_MARCH=exact reproduces the oracle's pixel choices (only fp sums differ);
    the default march ("proj") spends tolerance and must stay inside a quarter of north_star's
    1e-4 mean L1 with at most 0.2 % of the pixels moved by more than 1e-5 (measured: ~1e-7 / ~1e-4)."""
    set_options(monkeypatch, gi_march="proj" if march == "default" else march)
    l1_tol, moved_tol = (L1_TOL, 1e-3) if march == "exact" else (2.5e-5, 2e-3)
    dgr = _dgr()
    sc = scenes.surface_scene(P=30_000, sh_degree=1, seed=3, scale_mu=0.02)
    cam = scenes.orbit_camera(0, 4, 208, 160, radius=3.5)
    W, H = 208, 160
    fx, fy = focal(cam)
    r, ref = oracle_forward(orc, sc, cam)
    depth_f = orc.median3x3(ref["depth"])
    nd, pos = orc.depth_to_normal(W, H, fx, fy, cam["viewmatrix"], depth_f)
    # filters and depth->normal on identical inputs
    got_df = dgr.filters.median_blur(tt(ref["depth"])[None], (3, 3))[0].cpu().numpy()
    np.testing.assert_array_equal(got_df, depth_f)
    gn, gp = dgr._C.depth_to_normal(W, H, fx, fy, tt(cam["viewmatrix"]), tt(depth_f))
    np.testing.assert_array_equal(gp.cpu().numpy(), pos)
    np.testing.assert_allclose(gn.cpu().numpy(), nd, atol=1e-6)
    assert (nd != 0).any()
    got_bl = dgr.filters.bilateral_blur(tt(nd)[None], (3, 3), 1, (3, 3))[0].cpu().numpy()
    np.testing.assert_allclose(got_bl, orc.bilateral3x3(nd), atol=2e-6)
    posf = orc.median3x3(pos)
    np.testing.assert_array_equal(dgr.filters.median_blur(tt(pos)[None], (3, 3))[0].cpu().numpy(), posf)

    F0 = ((1.0 - ref["metallic"]) * 0.04 + ref["albedo"] * ref["metallic"]).astype(np.float32)
    for gi in (scenes.GI_DEFAULTS, dict(scenes.GI_DEFAULTS, start=64), dict(scenes.GI_DEFAULTS, step=12, start=5, delta=0.125)):
        a = (gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
        occ = orc.ssao(W, H, fx, fy, *a, ref["normal_view"], posf)
        got = dgr._C.SSAO(W, H, fx, fy, *a, tt(ref["normal_view"]), tt(posf)).cpu().numpy()
        d = np.abs(got - occ)
        assert d.mean() <= l1_tol and (d > 1e-5).mean() <= moved_tol, (march, gi, d.mean(), d.max())
        col, abd = orc.ssr(W, H, fx, fy, *a, ref["normal_view"], posf, ref["color"], ref["albedo"], ref["roughness"], ref["metallic"], F0)
        gc, ga = dgr._C.SSR(W, H, fx, fy, *a, tt(ref["normal_view"]), tt(posf), tt(ref["color"]), tt(ref["albedo"]),
                            tt(ref["roughness"]), tt(ref["metallic"]), tt(F0))
        for x, y in ((gc.cpu().numpy(), col), (ga.cpu().numpy(), abd)):
            assert np.array_equal(np.isnan(x), np.isnan(y))
            d = np.abs(np.nan_to_num(x) - np.nan_to_num(y))
            assert d.mean() <= l1_tol and (d > 1e-5).mean() <= moved_tol, (march, gi, d.mean(), d.max())
    assert occ.shape == (1, H, W)


def test_full_operator_matches_oracle_pipeline(orc):
    """GaussianRasterizer.forward 12-tuple == oracle pipeline (…/__init__.py:448-537) and
    Gaussian_SSR backward = grad * abd."""
    dgr = _dgr()
    sc = scenes.surface_scene(P=15_000, sh_degree=2, seed=6, scale_mu=0.025)
    cam = scenes.orbit_camera(2, 6, 176, 144, radius=3.5)
    W, H = 176, 144
    fx, fy = focal(cam)
    gi = scenes.GI_DEFAULTS
    st = settings(dgr, cam, 2)
    t = {k: tt(sc[k]) for k in GAUSS_KEYS}
    out = dgr.GaussianRasterizer(st)(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], t["normal"], t["albedo"],
                                     t["roughness"], t["metallic"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"],
                                     derive_normal=True)
    assert len(out) == 12
    (color, radii, opacity, depth, n_from_d, out_normal, occlusion, albedo, rough, metal, nview, pos_f) = [o.cpu().numpy() for o in out]
    r, ref = oracle_forward(orc, sc, cam)
    depth_f = orc.median3x3(ref["depth"])
    nd, pos = orc.depth_to_normal(W, H, fx, fy, cam["viewmatrix"], depth_f)
    nd = orc.bilateral3x3(nd)
    posf = orc.median3x3(pos)
    occ = orc.ssao(W, H, fx, fy, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"], ref["normal_view"], posf)
    np.testing.assert_array_equal(radii, ref["radii"])
    for a, b, name in ((color, ref["color"], "color"), (depth, ref["depth"], "depth"), (n_from_d, nd, "normal_from_depth"),
                       (pos_f, posf, "depth_pos_filter"), (occlusion, occ, "occlusion"), (albedo, ref["albedo"], "albedo")):
        d = np.abs(np.nan_to_num(a) - np.nan_to_num(b))
        assert d.mean() <= L1_TOL, (name, d.mean())
    # Gaussian_SSR: width before height in the constructor (…/__init__.py:697)
    ssr = dgr.Gaussian_SSR(cam["tanfovx"], cam["tanfovy"], W, H, gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
    alb = out[7].detach().clone().requires_grad_(True)
    rgh = out[8].detach().clone().requires_grad_(True)
    F0 = torch.full_like(alb, 0.04)
    col, abd = ssr(out[10].detach(), out[11].detach(), out[0].detach(), alb, rgh, torch.zeros_like(rgh), F0)
    g = torch.randn_like(col)
    col.nan_to_num().mul(g).sum().backward()
    want = (g * abd).nan_to_num()
    torch.testing.assert_close(alb.grad.nan_to_num(), want)
    assert float(rgh.grad.abs().sum()) == 0


def test_median_backward_routes_gradient(orc):
    dgr = _dgr()
    x = torch.randn(3, 40, 56, device=DEV, requires_grad=True)
    y = dgr.filters.median_blur(x[None], (3, 3))[0]
    g = torch.randn_like(y)
    (y * g).sum().backward()
    # reference semantics: unfold 3x3 (zero pad) + torch.median over the 9 taps
    xr = x.detach().clone().requires_grad_(True)
    patches = torch.nn.functional.unfold(xr[:, None], 3, padding=1).reshape(3, 9, 40, 56)
    yr = patches.median(dim=1).values
    (yr * g).sum().backward()
    torch.testing.assert_close(y.detach(), yr.detach())
    torch.testing.assert_close(x.grad, xr.grad)  # continuous random data: no ties


def test_fast_div2_and_rounding_are_bit_exact():
    """The SSAO/SSR march replaces two IEEE divisions by a shared-reciprocal FMA chain and roundf by
    add-and-truncate; both must be bit-identical to the plain forms (gi_march.h: div2_exact, round_to_int)."""
    import gigs_lib
    lib = gigs_lib.lib()
    rng = np.random.default_rng(0)
    n = 1 << 22
    # projected coordinates / depths as the march sees them, plus wide-exponent and special values
    nx = np.concatenate([rng.normal(0, 3, n // 2), np.ldexp(rng.normal(size=n // 4), rng.integers(-100, 100, n // 4)),
                         rng.uniform(-2000, 2000, n // 4)]).astype(np.float32)
    ny = np.roll(nx, 7) * np.float32(0.73)
    d = np.concatenate([rng.uniform(0.2, 8, n // 2), np.ldexp(rng.normal(size=n // 4), rng.integers(-100, 100, n // 4)),
                        rng.normal(0, 1e-3, n // 4)]).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 3.4e38, 0.5, -0.5, 1.5, 2.5, 8388607.5, -8388607.5,
                        2147483520.0, -2147483648.0, 4e9], np.float32)
    nx[:special.size] = special
    d[special.size:2 * special.size] = special
    tnx, tny, td = tt(nx), tt(ny), tt(d)
    of = torch.zeros(2 * n, device=DEV)
    orf = torch.zeros(2 * n, device=DEV)
    ornd = torch.zeros(2 * n, dtype=torch.int32, device=DEV)
    assert lib.gigs_selftest_div2(n, tnx.data_ptr(), tny.data_ptr(), td.data_ptr(), of.data_ptr(), orf.data_ptr(),
                                  ornd.data_ptr(), None) == 0
    torch.cuda.synchronize()
    a, b = of.cpu().numpy().view(np.uint32), orf.cpu().numpy().view(np.uint32)
    both_nan = np.isnan(of.cpu().numpy()) & np.isnan(orf.cpu().numpy())
    assert np.all((a == b) | both_nan), f"{int(((a != b) & ~both_nan).sum())} quotients differ"
    r = ornd.cpu().numpy().reshape(-1, 2)
    np.testing.assert_array_equal(r[:, 0], r[:, 1])


def test_pixel_rounding_is_exact_for_every_float():
    """gi_march.h (round_pix) rounds projected coordinates with floor(t + (0.5 - 2^-25)) instead of (int)roundf(t); the device sweeps
    all 2^32 floats and counts those where the two would pick a different pixel or a different inside/outside
    decision for an image side below 2^15."""
    import gigs_lib
    lib = gigs_lib.lib()
    bad = torch.ones(1, dtype=torch.int64, device=DEV)
    assert lib.gigs_selftest_round(bad.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert int(bad.item()) == 0


@pytest.mark.parametrize("W,H", [(176, 144), (161, 127), (33, 9)])
def test_fused_derive_normal_is_bit_identical_to_the_four_kernel_chain(W, H, monkeypatch):
    """gigs_derive_normal (one launch) == median3x3 -> depth_to_normal -> bilateral3x3, median3x3 bit for bit, including
    image borders, empty regions (zero depth), NaN depths and sizes that are not a multiple of the tile."""
    dgr = _dgr()
    sc = scenes.surface_scene(P=9_000, sh_degree=1, seed=4, scale_mu=0.03)
    cam = scenes.orbit_camera(1, 5, W, H, radius=3.5)
    t = {k: tt(sc[k]) for k in GAUSS_KEYS}
    outs = []
    for fused in ("0", "1"):
        set_options(monkeypatch, fused_derive=fused)
        st = settings(dgr, cam, 1)
        out = dgr.GaussianRasterizer(st)(t["means3D"], torch.zeros_like(t["means3D"]), t["opacities"], t["normal"],
                                         t["albedo"], t["roughness"], t["metallic"], shs=t["shs"], scales=t["scales"],
                                         rotations=t["rotations"], derive_normal=True)
        outs.append([o.detach().clone() for o in out])
    for i, name in ((4, "normal_from_depth"), (11, "depth_pos_filter"), (6, "occlusion")):
        a, b = outs[0][i], outs[1][i]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    # the stand-alone entry point on a depth plane with holes and NaNs
    import ctypes as C
    import gigs_lib
    lib = gigs_lib.lib()
    g = torch.Generator().manual_seed(W * 1000 + H)
    depth = (torch.rand(1, H, W, generator=g) * 3 + 0.5)
    depth[:, H // 3: H // 3 + 4, W // 4: W // 2] = 0.0
    depth[:, H // 2, W // 2] = float("nan")
    depth = depth.to(DEV)
    vm = tt(cam["viewmatrix"])
    fx, fy = focal(cam)
    df = dgr.filters.median_blur(depth[None], (3, 3))[0]
    n0, p0 = dgr._C.depth_to_normal(W, H, fx, fy, vm, df)
    n0 = dgr.filters.bilateral_blur(n0[None], (3, 3), 1, (3, 3))[0]
    p0 = dgr.filters.median_blur(p0[None], (3, 3))[0]
    n1, p1 = torch.empty_like(n0), torch.empty_like(p0)
    gigs_lib.check(lib.gigs_derive_normal(W, H, float(fx), float(fy), vm.data_ptr(), depth.data_ptr(), 1.0, 3.0, 3.0,
                                          n1.data_ptr(), p1.data_ptr(), torch.cuda.current_stream().cuda_stream),
                   "derive_normal")
    torch.cuda.synchronize()
    assert torch.equal(n0.view(torch.int32), n1.view(torch.int32))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


# ------------------------------------------------------------------------------------------
# binning paths
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["legacy", "bucket", "long_lists"])
def test_binning_paths_match_oracle(orc, mode, monkeypatch):
    """All binning paths -- the reference-shaped scan / duplicate / global radix sort (legacy), the default
    tile-bucketed count / prefix / scatter / per-tile sort, and the latter in its dense-scene configuration (forced here:
    GIGS_LONG_LISTS=1; these scenes have no list long enough to be partitioned, the kernels run empty-handed) -- give the
    oracle's keys, point_list and ranges bit for bit, on a cloud with large footprints (wave-expanded), exact depth ties
    (duplicated Gaussians) and a ragged image."""
    set_options(monkeypatch, binning_legacy=int(mode == "legacy"), long_lists=1 if mode == "long_lists" else -1)
    sc = scenes.random_scene(P=6000, sh_degree=1, seed=21, scale_mu=0.12)
    # exact depth ties inside tiles: the same Gaussian several times (ties must come out in index order)
    for k in GAUSS_KEYS:
        sc[k][3000:3400] = sc[k][100:500]
        sc[k][3400:3800] = sc[k][100:500]
    # ... and a long run of bit-identical depths: one Gaussian 300 times (its tiles see 300 keys that differ in the index only)
    for k in GAUSS_KEYS:
        sc[k][5000:5300] = sc[k][777]
    cam = scenes.orbit_camera(2, 7, 333, 211)
    check_forward(orc, sc, cam, tag=mode + " ")
    sc = scenes.surface_scene(P=40_000, sh_degree=1, seed=5, scale_mu=0.02)
    check_forward(orc, sc, scenes.orbit_camera(1, 5, 400, 304, radius=3.2), tag=mode + " surface ")


def test_async_binning_capacity_and_overflow(orc):
    """gigs_ctx_set_async_binning: no host read-back; with enough capacity the outputs are those of the synchronous call, the
    device counters report R; with too little the overflow flag is raised and nothing is written out of bounds."""
    import gigs_lib
    dgr = _dgr()
    lib = gigs_lib.lib()
    sc = scenes.surface_scene(P=30_000, sh_degree=1, seed=3, scale_mu=0.02)
    cam = scenes.orbit_camera(0, 4, 304, 240, radius=3.5)
    ref = hip_raw_forward(dgr, sc, cam)
    R = ref[0]
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    cap = int(R * 1.3)
    with gigs_lib.use(gigs_lib.current().derive(async_binning=(cap, counters))):
        got = hip_raw_forward(dgr, sc, cam)
    assert got[0] == cap and counters.tolist() == [R, 0]
    for a, b in zip(hip_planes(ref).items(), hip_planes(got).items()):
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=a[0])
    P, W, H = sc["means3D"].shape[0], cam["image_width"], cam["image_height"]
    sa, sb = scratch_views(dgr, ref, P, W, H), scratch_views(dgr, (cap,) + tuple(got[1:]), P, W, H)
    np.testing.assert_array_equal(sa["point_list"], sb["point_list"][:R])
    np.testing.assert_array_equal(sa["ranges"], sb["ranges"])
    # the backward carves the chunk with the capacity it was given
    small = R // 3
    guard = torch.full((1024,), 0x5A, dtype=torch.uint8, device=DEV)
    with gigs_lib.use(gigs_lib.current().derive(async_binning=(small, counters))):
        over = hip_raw_forward(dgr, sc, cam)
    assert over[0] == small and counters.tolist() == [R, R]
    sv = scratch_views(dgr, over, P, W, H)
    assert int(sv["ranges"].max()) <= small and torch.all(guard == 0x5A)
    for k, v in hip_planes(over).items():
        assert np.isfinite(np.nan_to_num(v)).all(), k


@pytest.mark.parametrize("split", ["auto", "off"])
def test_dense_scene_long_lists_sync_and_async(orc, split, monkeypatch):
    """A dense view (mean list 6 000, two tiles near 30 000 keys of which 20 000 share nearly one depth) through the
    tile-bucketed binning with its long lists partitioned by sampled splitters ("auto": the library's own criterion) and
    sorted whole ("off": GIGS_LONG_LISTS=0, the global-memory network), synchronous (the reference's API: R read back) and
    asynchronous (fixed capacity, device counters): keys / point_list / ranges equal the oracle's, the planes equal the
    legacy path's bit for bit, and an undersized capacity raises the flag without writing out of bounds."""
    import gigs_lib
    dgr = _dgr()
    lib = gigs_lib.lib()
    if split == "off":
        set_options(monkeypatch, long_lists=0)
    # ~3 000 instances per tile on average at 96x80 (30 tiles), one screen-filling cluster in front: a very long list
    sc = scenes.surface_scene(P=44_000, sh_degree=1, seed=9, scale_mu=0.08)
    cam = scenes.orbit_camera(1, 5, 96, 80, radius=3.0)
    # the last 20 000 Gaussians: a cluster of small splats on a plane facing the camera, 2 units in front of it -- one
    # tile's worth of screen, (nearly) one depth: they land in ONE (tile, depth bucket) bin whatever the thresholds are
    rng = np.random.default_rng(3)
    fwd = -cam["campos"] / np.linalg.norm(cam["campos"])
    side = np.cross(fwd, [0.0, 0.0, 1.0]); side /= np.linalg.norm(side)
    up = np.cross(side, fwd)
    n_cl = 20_000
    lat = rng.uniform(-0.012, 0.012, size=(n_cl, 2))
    sc["means3D"][-n_cl:] = (cam["campos"] + 2.0 * fwd + lat[:, :1] * side + lat[:, 1:] * up
                             + rng.uniform(-2e-4, 2e-4, size=(n_cl, 1)) * fwd).astype(np.float32)
    sc["scales"][-n_cl:] = 0.002
    sc["opacities"][-n_cl:] = 0.02  # faint: the walk goes through all of them
    check_forward(orc, sc, cam, tag="split " + split + " ")
    got = hip_raw_forward(dgr, sc, cam)
    R = got[0]
    P, W, H = sc["means3D"].shape[0], cam["image_width"], cam["image_height"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    assert R > 2500 * T, (R, T)  # dense by the library's own criterion
    with gigs_lib.options(binning_legacy=1):
        ref = hip_raw_forward(dgr, sc, cam)
    assert ref[0] == R
    sa, sb = scratch_views(dgr, ref, P, W, H), scratch_views(dgr, got, P, W, H)
    for k in ("keys", "point_list", "ranges", "n_contrib"):
        np.testing.assert_array_equal(sa[k], sb[k], err_msg=k)
    for a, b in zip(hip_planes(ref).items(), hip_planes(got).items()):
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=a[0])
    lengths = (sb["ranges"].reshape(T, 2)[:, 1] - sb["ranges"].reshape(T, 2)[:, 0])
    print("dense test: R", R, "mean list", R // T, "longest", int(lengths.max()))
    counters = torch.zeros(2, dtype=torch.int32, device=DEV)
    cap = 2 * R  # what pipeline.WholeStepGraph sizes: the library reads the density off the capacity
    with gigs_lib.use(gigs_lib.current().derive(async_binning=(cap, counters))):
        asy = hip_raw_forward(dgr, sc, cam)
    assert asy[0] == cap and counters.tolist() == [R, 0]
    sc_ = scratch_views(dgr, (cap,) + tuple(asy[1:]), P, W, H)
    np.testing.assert_array_equal(sa["point_list"], sc_["point_list"][:R])
    np.testing.assert_array_equal(sa["keys"], sc_["keys"][:R])
    np.testing.assert_array_equal(sa["ranges"], sc_["ranges"])
    for a, b in zip(hip_planes(ref).items(), hip_planes(asy).items()):
        np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32), err_msg=a[0])
    small = max(65536, R // 3)
    guard = torch.full((1024,), 0x5A, dtype=torch.uint8, device=DEV)
    with gigs_lib.use(gigs_lib.current().derive(async_binning=(small, counters))):
        over = hip_raw_forward(dgr, sc, cam)
    assert over[0] == small and counters.tolist() == [R, R]
    sv = scratch_views(dgr, over, P, W, H)
    assert int(sv["ranges"].max()) <= small and torch.all(guard == 0x5A)


@pytest.mark.parametrize("case", ["c2ish", "ragged", "gi_settings", "blocks32", "blocks64"])
def test_gi_certification_is_exact(case, monkeypatch):
    """The march's conservative coarse-depth certification (LDS min/max table of the z plane) only skips lookups that
    cannot hit: SSAO and SSR outputs are bit-identical with it switched off (GIGS_GI_CERT=0), on smooth and ragged
    views, with empty regions, at several GI settings."""
    import pipeline
    dgr = _dgr()
    if case == "c2ish":
        sc, cam, gis = scenes.surface_scene(P=120_000, sh_degree=1, seed=8, scale_mu=0.012), scenes.orbit_camera(9, 32, 640, 512, radius=3.4), [scenes.GI_DEFAULTS]
    elif case == "ragged":
        sc, cam, gis = scenes.surface_scene(P=50_000, sh_degree=1, seed=2, scale_mu=0.02), scenes.orbit_camera(3, 16, 611, 403, radius=3.2), [scenes.GI_DEFAULTS]
    elif case == "blocks32":  # the table of 16-pixel blocks would exceed its LDS budget: 32-pixel blocks, ragged edges
        sc, cam, gis = scenes.surface_scene(P=60_000, sh_degree=1, seed=5, scale_mu=0.02), scenes.orbit_camera(5, 16, 1621, 1043, radius=3.3), [scenes.GI_DEFAULTS]
    elif case == "blocks64":  # 64-pixel blocks
        sc, cam, gis = scenes.surface_scene(P=60_000, sh_degree=1, seed=6, scale_mu=0.02), scenes.orbit_camera(2, 16, 2891, 1777, radius=3.3), [dict(scenes.GI_DEFAULTS, delta=0.25)]
    else:
        sc, cam = scenes.surface_scene(P=30_000, sh_degree=1, seed=3, scale_mu=0.02), scenes.orbit_camera(0, 4, 208, 160, radius=3.5)
        gis = [dict(scenes.GI_DEFAULTS, radius=1.6, start=4), dict(scenes.GI_DEFAULTS, step=12, start=5, delta=0.125),
               dict(scenes.GI_DEFAULTS, bias=0.2, thick=0.5), dict(scenes.GI_DEFAULTS, start=0)]
    g = {k: tt(sc[k]) for k in GAUSS_KEYS}
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    W, H = cam["image_width"], cam["image_height"]
    fx, fy = focal(cam)
    with torch.no_grad():
        res = pipeline.render(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
        out, _, _ = pipeline.rasterize(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
    raw_nview, posf = out[10].contiguous(), out[11].contiguous()
    F0 = torch.full((3, H, W), 0.04, device=DEV)
    rgb = res["albedo_map"].clamp(0, 1).contiguous()
    hits = 0
    for gi in gis:
        a = (gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
        got = {}
        for cert in ("1", "0"):
            with gigs_lib.options(gi_cert=int(cert)):
                occ = dgr._C.SSAO(W, H, fx, fy, *a, raw_nview, posf)
                col, abd = dgr._C.SSR(W, H, fx, fy, *a, res["out_normal_view"].contiguous(), posf, rgb, res["albedo_map"].contiguous(),
                                      res["roughness_map"].contiguous(), res["metallic_map"].contiguous(), F0)
            got[cert] = (occ.clone(), col.clone(), abd.clone())
        for x, y in zip(got["1"], got["0"]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (case, gi)
        hits += int((got["1"][0] < 1.0).sum())
    assert hits > 0, "no ray of the test views hits anything: the comparison would be vacuous"


def test_gi_long_march_falls_back_to_exact():
    """The projective march reads j / step from a 64-entry table, so a march of more than 60 steps (64 minus the group of
    four) runs the exact march whatever gi_march says: with gi_march = proj, SSAO and SSR are bit-identical to gi_march =
    exact, for a step that is no power of two and for one that is (but too long for the table)."""
    import gigs_lib
    import pipeline
    dgr = _dgr()
    sc = scenes.surface_scene(P=8_000, sh_degree=1, scale_mu=0.03)
    cam = scenes.orbit_camera(0, 4, 96, 64, radius=3.5)
    g = {k: tt(sc[k]) for k in GAUSS_KEYS}
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    W, H = cam["image_width"], cam["image_height"]
    fx, fy = focal(cam)
    with torch.no_grad():
        res = pipeline.render(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
        out, _, _ = pipeline.rasterize(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
    raw_nview, posf = out[10].contiguous(), out[11].contiguous()
    F0 = torch.full((3, H, W), 0.04, device=DEV)
    rgb = res["albedo_map"].clamp(0, 1).contiguous()
    hits = 0
    for gi in (dict(scenes.GI_DEFAULTS, step=72, start=4), dict(scenes.GI_DEFAULTS, step=64, start=0)):
        assert gi["step"] - gi["start"] > 60
        a = (gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
        got = {}
        for march in ("proj", "exact"):
            with gigs_lib.options(gi_march=march):
                occ = dgr._C.SSAO(W, H, fx, fy, *a, raw_nview, posf)
                col, abd = dgr._C.SSR(W, H, fx, fy, *a, res["out_normal_view"].contiguous(), posf, rgb, res["albedo_map"].contiguous(),
                                      res["roughness_map"].contiguous(), res["metallic_map"].contiguous(), F0)
            got[march] = (occ.clone(), col.clone(), abd.clone())
        for name, x, y in zip(("occlusion", "color", "abd"), got["proj"], got["exact"]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (gi, name)
        hits += int((got["proj"][0] < 1.0).sum())
    assert hits > 0, "no ray of the test view hits anything: the comparison would be vacuous"


@pytest.mark.parametrize("march", ["proj", "proj_nocert", "proj_quarters", "exact"])
def test_gi_zero_weight_rays_are_exact(march):
    """The theta = 0 rays of the reference's ray set (forward.cu:679-681, 796-797: 32 of 512 at delta 0.0625, 16 of 144
    at 0.125, 65 of 2080 at 0.03125) have weight cos * sin = 0 and one direction, the normal.  By default they are not
    marched (SSAO) / marched once (SSR, for the NaN a non-finite hit pixel produces: forward.cu:824-826).  Marching all of
    them (gigs_options.gi_zero_rays = 1) must not change a bit of occlusion, colour or abd -- in every march mode, for
    interleaved and contiguous ray splits, with NaN / Inf radiance in the image."""
    import gigs_lib
    import pipeline
    dgr = _dgr()
    sc = scenes.surface_scene(P=40_000, sh_degree=1, seed=11, scale_mu=0.02)
    cam = scenes.orbit_camera(2, 9, 333, 251, radius=3.3)
    g = {k: tt(sc[k]) for k in GAUSS_KEYS}
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    W, H = cam["image_width"], cam["image_height"]
    fx, fy = focal(cam)
    with torch.no_grad():
        res = pipeline.render(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
        out, _, _ = pipeline.rasterize(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
    raw_nview, posf = out[10].contiguous(), out[11].contiguous()
    F0 = torch.full((3, H, W), 0.04, device=DEV)
    rgb = res["albedo_map"].clamp(0, 1).contiguous().clone()
    # non-finite radiance on a band of covered pixels: every ray that hits there turns the pixel's sum into NaN,
    # zero-weight rays included (0 * inf, 0 * nan)
    rgb[0, H // 2 - 6:H // 2 + 6, :] = float("inf")
    rgb[1, :, W // 2 - 5:W // 2 + 5] = float("nan")
    opts = dict(gi_march=march.split("_no")[0].split("_quarters")[0])
    if march == "proj_nocert":
        opts["gi_cert"] = 0
    if march == "proj_quarters":
        opts["gi_interleave"] = 0
    gis = [scenes.GI_DEFAULTS, dict(scenes.GI_DEFAULTS, delta=0.125, start=4, radius=1.2)]
    if march in ("proj", "exact"):
        gis.append(dict(scenes.GI_DEFAULTS, delta=0.03125, start=12))  # 2 080 rays, 65 of weight zero
    hits = nans = 0
    for gi in gis:
        a = (gi["radius"], gi["bias"], gi["thick"], gi["delta"], gi["step"], gi["start"])
        got = {}
        for zero in (0, 1):
            with gigs_lib.options(gi_zero_rays=zero, **opts):
                occ = dgr._C.SSAO(W, H, fx, fy, *a, raw_nview, posf)
                col, abd = dgr._C.SSR(W, H, fx, fy, *a, res["out_normal_view"].contiguous(), posf, rgb, res["albedo_map"].contiguous(),
                                      res["roughness_map"].contiguous(), res["metallic_map"].contiguous(), F0)
            got[zero] = (occ.clone(), col.clone(), abd.clone())
        for name, x, y in zip(("occlusion", "color", "abd"), got[0], got[1]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (march, gi, name)
        hits += int((got[0][0] < 1.0).sum())
        nans += int(torch.isnan(got[0][1]).sum())
    assert hits > 0 and nans > 0, "vacuous: no ray hits / no non-finite radiance was picked up"


def test_two_contexts_on_two_streams_equal_the_serial_runs(orc):
    """the library is re-entrant per stream.  Two contexts with different switches and different
    asynchronous-binning capacities / counters / events drive two views on two streams of one process, their calls
    interleaved and nothing synchronised in between; every output equals the serial, one-context-at-a-time run bit for
    bit (integer state, planes, occlusion, gradients of the deterministic -- atomic-free -- outputs)."""
    import gigs_lib
    dgr = _dgr()
    scA = scenes.surface_scene(P=30_000, sh_degree=1, seed=3, scale_mu=0.02)
    scB = scenes.surface_scene(P=18_000, sh_degree=2, seed=4, scale_mu=0.03)
    camA = scenes.orbit_camera(0, 4, 304, 240, radius=3.5)
    camB = scenes.orbit_camera(1, 5, 251, 333, radius=3.2)
    giA, giB = scenes.GI_DEFAULTS, dict(scenes.GI_DEFAULTS, delta=0.125, start=4)
    RA = hip_raw_forward(dgr, scA, camA)[0]
    RB = hip_raw_forward(dgr, scB, camB)[0]
    cntA, cntB = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    evA, evB = torch.cuda.Event(), torch.cuda.Event()
    evA.record(); evB.record()
    base = gigs_lib.current()
    ctxA = base.derive(async_binning=(int(RA * 1.5), cntA), blend_event=evA, gi_march="exact", blend_cull=0, gi_tile_log2w=4)
    ctxB = base.derive(async_binning=(int(RB * 2.2), cntB), blend_event=evB, gi_march="proj", gi_cert=0, long_lists=1,
                       pre_bwd_sh_skip=0, gi_zero_rays=1)
    assert ctxA.ptr != ctxB.ptr

    def inputs(sc):
        return {k: tt(sc[k], grad=True) for k in GAUSS_KEYS}

    def fwd(ctx, sc, cam, gi, t):
        with gigs_lib.use(ctx):
            st = settings(dgr, cam, sc["sh_degree"], gi=gi)
            return dgr.GaussianRasterizer(st)(t["means3D"], torch.zeros_like(t["means3D"], requires_grad=True), t["opacities"],
                                              t["normal"], t["albedo"], t["roughness"], t["metallic"], shs=t["shs"],
                                              scales=t["scales"], rotations=t["rotations"])

    def bwd(ctx, out):
        with gigs_lib.use(ctx):  # the backward reads its context's switches too (pre_bwd_sh_skip)
            (out[0].sum() * 0.5 + (out[7] * out[7]).sum() + out[3].sum() * 0.1).backward()

    def collect(out, t, cnt):
        torch.cuda.synchronize()
        return ([o.detach().clone() for o in out], {k: v.grad.clone() for k, v in t.items() if v.grad is not None}, cnt.tolist())

    # serial: A completely, then B completely
    tA, tB = inputs(scA), inputs(scB)
    oA = fwd(ctxA, scA, camA, giA, tA); bwd(ctxA, oA); refA = collect(oA, tA, cntA)
    oB = fwd(ctxB, scB, camB, giB, tB); bwd(ctxB, oB); refB = collect(oB, tB, cntB)
    assert refA[2] == [RA, 0] and refB[2] == [RB, 0]
    # interleaved on two streams, no synchronisation between the calls
    cntA.zero_(); cntB.zero_()
    sA, sB = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    tA, tB = inputs(scA), inputs(scB)
    with torch.cuda.stream(sA):
        oA = fwd(ctxA, scA, camA, giA, tA)
    with torch.cuda.stream(sB):
        oB = fwd(ctxB, scB, camB, giB, tB)
    with torch.cuda.stream(sA):
        bwd(ctxA, oA)
    with torch.cuda.stream(sB):
        bwd(ctxB, oB)
    gotA, gotB = collect(oA, tA, cntA), collect(oB, tB, cntB)
    assert evA.query() and evB.query()
    for tag, ref, got in (("A", refA, gotA), ("B", refB, gotB)):
        assert ref[2] == got[2], tag
        for i, (x, y) in enumerate(zip(ref[0], got[0])):
            assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                               y.view(torch.int32) if y.dtype == torch.float32 else y), (tag, "output", i)
        for k in ref[1]:
            # per-Gaussian sums of the blend backward are float atomics over quadrants: equal to rounding, not bit for bit
            np.testing.assert_allclose(got[1][k].cpu().numpy(), ref[1][k].cpu().numpy(), rtol=2e-4,
                                       atol=1e-6 * max(float(ref[1][k].abs().max()), 1e-20), err_msg=tag + " grad " + k)
    # and both equal the default context's synchronous results where the switches are bit-neutral (A: exact march differs)
    with gigs_lib.use(base):
        tB2 = inputs(scB)
        oB2 = fwd(base, scB, camB, giB, tB2)
    torch.cuda.synchronize()
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9):  # colour, radii, opacity, depth, normal, occlusion (cert / zero rays: same bits), materials
        x, y = oB2[i].detach(), gotB[0][i]
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), i


@pytest.mark.parametrize("mode", ["bucket", "long_lists"])
def test_long_runs_of_identical_depths_sort_in_bounded_time(orc, mode, monkeypatch):
    """A tile that holds thousands of bit-identical depths (a cloned Gaussian: 4 500 copies; a second run of 70, just over
    the fix-up's round budget): the LDS sorts order them by index through the bounded fix-up / the complete-key sort
    (csrc/binning.hip::sort_tile_radix) -- keys, point_list and ranges equal the oracle's stable sort bit for bit."""
    set_options(monkeypatch, long_lists=1 if mode == "long_lists" else -1)
    sc = scenes.random_scene(P=9000, sh_degree=1, seed=23, scale_mu=0.05)
    for k in GAUSS_KEYS:
        sc[k][2000:6500] = sc[k][321]
        sc[k][7000:7070] = sc[k][654]
    sc["opacities"][2000:6500] = 0.01  # faint: the walk goes through all of them
    cam = scenes.orbit_camera(1, 6, 160, 128)
    _, _, res, _ = check_forward(orc, sc, cam, tag="identical depths " + mode + " ")
    assert res[0] > 4500


def test_backward_runs_with_the_context_and_sink_of_its_forward(monkeypatch):
    """autograd executes backward nodes on its own device thread, where the per-thread current library context and the
    per-thread scopes of the operator module are not the caller's.  The node carries both from its forward
    (gigs_lib.with_forward_context): gigs_backward receives the context the forward ran with -- even when backward() is
    called after the `with` block has ended -- and writes into the gradient sink that was active at the forward."""
    dgr = _dgr()
    lib = gigs_lib.lib()
    sc, cam = small_scene(P=1500, sh_degree=1, W=96, H=64, scale_mu=0.06)
    seen = []
    real = lib.gigs_backward

    def spy(ctx_ptr, *a):
        seen.append(ctx_ptr)
        return real(ctx_ptr, *a)
    monkeypatch.setattr(lib, "gigs_backward", spy)
    ctx = gigs_lib.current().derive(pre_bwd_sh_skip=0, gi_march="exact")
    assert ctx.ptr != gigs_lib.current().ptr
    t = {k: tt(sc[k], grad=True) for k in GAUSS_KEYS}
    sink = {"means3D": torch.empty_like(t["means3D"]), "albedo": torch.empty_like(t["albedo"])}
    st = settings(dgr, cam, 1)
    with gigs_lib.use(ctx), dgr.grad_sink(sink):
        out = dgr.GaussianRasterizer(st)(t["means3D"], torch.zeros_like(t["means3D"], requires_grad=True), t["opacities"], t["normal"],
                                         t["albedo"], t["roughness"], t["metallic"], shs=t["shs"], scales=t["scales"],
                                         rotations=t["rotations"])
    assert gigs_lib.current().ptr != ctx.ptr
    (out[0].sum() + out[7].sum()).backward()   # outside both scopes, on autograd's thread
    torch.cuda.synchronize()
    assert seen == [ctx.ptr], (seen, ctx.ptr)
    # AccumulateGrad may clone a gradient that something else references: compare values with the sink's
    assert torch.equal(t["means3D"].grad, sink["means3D"]) and torch.equal(t["albedo"].grad, sink["albedo"])
    assert float(sink["albedo"].abs().sum()) > 0


@pytest.mark.parametrize("case", ["default", "ragged_delta", "nan_radiance"])
def test_ssr_hit_list_gather_equals_the_march(case):
    """gigs_ssr_hits / gigs_ssr_apply (frozen-geometry reuse): the hit list recorded by the march -- count per (pixel, wave),
    exclusive prefix, fill -- and the gather over it reproduce gigs_ssr_ex bit for bit, also for other radiance than the one
    the list was recorded with (the hits depend on normals and positions only: forward.cu:796-829), on ragged images, other
    ray sets, with NaN / Inf radiance, and with a capacity that is too small (entries beyond it dropped, total reported)."""
    import ctypes as C

    import pipeline
    dgr = _dgr()
    lib = gigs_lib.lib()
    if case == "ragged_delta":
        sc, cam = scenes.surface_scene(P=30_000, sh_degree=1, seed=7, scale_mu=0.02), scenes.orbit_camera(2, 9, 333, 251, radius=3.3)
        gi = dict(scenes.GI_DEFAULTS, delta=0.125, start=4, radius=1.2)
    else:
        sc, cam = scenes.surface_scene(P=40_000, sh_degree=1, seed=11, scale_mu=0.02), scenes.orbit_camera(1, 7, 320, 240, radius=3.4)
        gi = scenes.GI_DEFAULTS
    g = {k: tt(sc[k]) for k in GAUSS_KEYS}
    camt = {k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    W, H = cam["image_width"], cam["image_height"]
    N = W * H
    fx, fy = focal(cam)
    with torch.no_grad():
        res = pipeline.render(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
        out, _, _ = pipeline.rasterize(camt, g, 1, torch.zeros(3, device=DEV), dict(scenes.GI_DEFAULTS, start=16))
    nrm, posf = res["out_normal_view"].contiguous(), out[11].contiguous()
    alb, rough, metal = res["albedo_map"].contiguous(), res["roughness_map"].contiguous(), res["metallic_map"].contiguous()
    F0 = torch.full((3, H, W), 0.04, device=DEV)
    rgb1 = alb.clamp(0, 1).clone()
    if case == "nan_radiance":
        rgb1[0, H // 2 - 5:H // 2 + 5, :] = float("inf")
        rgb1[2, :, W // 2 - 4:W // 2 + 4] = float("nan")
    torch.manual_seed(3)
    rgb2 = torch.rand(3, H, W, device=DEV)
    a = (W, H, float(fx), float(fy), float(gi["radius"]), float(gi["bias"]), float(gi["thick"]), float(gi["delta"]), int(gi["step"]), int(gi["start"]))
    s = torch.cuda.current_stream().cuda_stream
    scratch = torch.empty(int(lib.gigs_gi_scratch_bytes(W, H)) or 1, dtype=torch.uint8, device=DEV)
    new3 = lambda: torch.empty(3, H, W, device=DEV)  # noqa: E731

    def march(rgb):
        col, abd = new3(), new3()
        gigs_lib.check(lib.gigs_ssr_ex(None, *a, nrm.data_ptr(), posf.data_ptr(), rgb.data_ptr(), alb.data_ptr(), rough.data_ptr(),
                                       metal.data_ptr(), F0.data_ptr(), col.data_ptr(), abd.data_ptr(), scratch.data_ptr(), s), "ssr_ex")
        return col, abd

    counts = torch.zeros(4 * N, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(4 * N + 1, dtype=torch.int32, device=DEV)
    c1, a1 = new3(), new3()
    gigs_lib.check(lib.gigs_ssr_hits(None, *a, nrm.data_ptr(), posf.data_ptr(), rgb1.data_ptr(), alb.data_ptr(), rough.data_ptr(),
                                     metal.data_ptr(), F0.data_ptr(), c1.data_ptr(), a1.data_ptr(), 1, counts.data_ptr(), None, None, 0,
                                     scratch.data_ptr(), s), "ssr_hits count")
    torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
    total = int(offsets[-1])
    assert total > 1000, "no ray of the test view hits anything"
    entries = torch.full((total, 2), -1, dtype=torch.int32, device=DEV)
    c2, a2 = new3(), new3()
    gigs_lib.check(lib.gigs_ssr_hits(None, *a, nrm.data_ptr(), posf.data_ptr(), rgb1.data_ptr(), alb.data_ptr(), rough.data_ptr(),
                                     metal.data_ptr(), F0.data_ptr(), c2.data_ptr(), a2.data_ptr(), 2, None, offsets.data_ptr(),
                                     entries.data_ptr(), total, scratch.data_ptr(), s), "ssr_hits fill")
    assert int((entries < 0).sum()) == 0 and int(entries[:, 0].max()) < N  # every slot written, hit pixels inside the image
    ref1 = march(rgb1)
    for x, y in ((c1, ref1[0]), (a1, ref1[1]), (c2, ref1[0]), (a2, ref1[1])):  # the recording passes give the march's outputs
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for rgb in (rgb1, rgb2):
        col, abd = new3(), new3()
        gigs_lib.check(lib.gigs_ssr_apply(W, H, float(gi["delta"]), offsets.data_ptr(), entries.data_ptr(), nrm.data_ptr(), posf.data_ptr(),
                                          rgb.data_ptr(), alb.data_ptr(), metal.data_ptr(), F0.data_ptr(), col.data_ptr(), abd.data_ptr(), s),
                       "ssr_apply")
        want = march(rgb)
        assert torch.equal(col.view(torch.int32), want[0].view(torch.int32)) and torch.equal(abd.view(torch.int32), want[1].view(torch.int32))
    if case == "nan_radiance":
        assert int(torch.isnan(ref1[0]).sum()) > 0
    # too small a buffer: nothing is written beyond it
    cap = total // 3
    guard = torch.full((total, 2), -7, dtype=torch.int32, device=DEV)
    gigs_lib.check(lib.gigs_ssr_hits(None, *a, nrm.data_ptr(), posf.data_ptr(), rgb1.data_ptr(), alb.data_ptr(), rough.data_ptr(),
                                     metal.data_ptr(), F0.data_ptr(), c2.data_ptr(), a2.data_ptr(), 2, None, offsets.data_ptr(),
                                     guard.data_ptr(), cap, scratch.data_ptr(), s), "ssr_hits fill (small)")
    torch.cuda.synchronize()
    assert int((guard[cap:] != -7).sum()) == 0 and torch.equal(guard[:cap], entries[:cap])
    # recorded by the default march only
    with gigs_lib.options(gi_march="exact") as cx:
        rc = lib.gigs_ssr_hits(cx.ptr, *a, nrm.data_ptr(), posf.data_ptr(), rgb1.data_ptr(), alb.data_ptr(), rough.data_ptr(), metal.data_ptr(),
                               F0.data_ptr(), c2.data_ptr(), a2.data_ptr(), 1, counts.data_ptr(), None, None, 0, scratch.data_ptr(), s)
    assert rc < 0 and b"default march" in lib.gigs_last_error()


def test_reused_tile_lists_equal_a_full_forward_and_are_guarded(orc):
    """gigs_ctx_set_reuse_binning (dgr.view_cache): a forward that reuses the tile lists of an earlier forward of the same
    view and geometry -- preprocess + blend only -- gives that forward's planes bit for bit, with other material attributes
    the planes of a complete forward of THOSE; and lists made for another Gaussian count are not blended at all (every tile
    empty: background), instead of dereferencing stale indices."""
    dgr = _dgr()
    sc = scenes.surface_scene(P=20_000, sh_degree=1, seed=13, scale_mu=0.025)
    cam = scenes.orbit_camera(1, 5, 251, 203, radius=3.4)
    bg = (0.2, 0.4, 0.1)
    full = hip_raw_forward(dgr, sc, cam, bg=bg)
    R = full[0]
    slot = dgr.ViewSlot(DEV)
    with dgr.AsyncBinning(int(1.5 * R), DEV):
        with dgr.view_cache(slot, "record"):
            rec = hip_raw_forward(dgr, sc, cam, bg=bg)
        with dgr.view_cache(slot, "replay"):
            rep = hip_raw_forward(dgr, sc, cam, bg=bg)
        sc2 = dict(sc, albedo=np.ascontiguousarray(1.0 - sc["albedo"]), roughness=np.ascontiguousarray(sc["roughness"] * 0.5))
        with dgr.view_cache(slot, "replay"):
            rep2 = hip_raw_forward(dgr, sc2, cam, bg=bg)
        # another cloud (fewer Gaussians) against the same lists: guarded
        sc3 = scenes.surface_scene(P=12_000, sh_degree=1, seed=14, scale_mu=0.025)
        with dgr.view_cache(slot, "replay"):
            bad = hip_raw_forward(dgr, sc3, cam, bg=bg)
    want2 = hip_planes(hip_raw_forward(dgr, sc2, cam, bg=bg))
    for name, a, b in (("record", hip_planes(full), hip_planes(rec)), ("replay", hip_planes(full), hip_planes(rep)),
                       ("replay, other materials", want2, hip_planes(rep2))):
        for k in PLANES + ["radii"]:
            x, y = a[k], b[k]
            np.testing.assert_array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                          y.view(np.uint32) if y.dtype == np.float32 else y, err_msg=name + " " + k)
    hb = hip_planes(bad)
    assert np.all(hb["opacity"] == 0.0) and np.all(hb["albedo"] == 0.0)
    for c in range(3):
        assert np.all(hb["color"][c] == np.float32(bg[c]))
