"""The sparse forward of a light's fine GGX levels (csrc/shade.hip spec_tap_census_kernel, csrc/light_filter.hip
specular_apply_multi_fwd_sparse_kernel, pbr.renderutils.ops.SparseFineLevels, pipeline.Stage2Step(sparse_light=True)).

The light is the smallest chain with two fine levels below a coarse one, 64 / 32 / 16, and the G-buffer is 48 x 64 pixels
drawn from the generators of shade_cases.py: seam and corner directions of both fine levels on every face, in both roles of
the level blend, roughnesses in every level pair and on both sides of the knots, grazing, back-facing and head-on normals,
zero normals, pixels outside the mask and fillers.  Every pixel keeps shade_cases' float64 decision margin, so the float64
reference (oracle/torch_pbr_ref.shade) and the kernels take the same cube face, taps and level pair.

What is asked (no bound is measured from the code under test):
  * a listed texel has the dense launch's bits, for the 8-, 16- and 64-lane groupings; a texel that is not listed is not
    written (its poison is still there);
  * the marked set contains every (level, texel) the float64 shade samples for the pixels that mark -- every pixel, or
    the pixels of the entry point's optional mask -- and holds at most 8 entries per such pixel;
  * with the fine levels poisoned with NaN before the fill, gigs_shade_fwd_ex and gigs_shade_bwd_ex give, in every plane
    and at every pixel, inside the G-buffer's mask or not, the bits they give with the dense levels, without a NaN.  The
    one exception is not the sparse path's: the light's gradient textures are summed with float atomics by the shade
    backward, two runs on the same DENSE levels do not reproduce them bit for bit, and where those two runs differ the
    sparse run is held to 4 x their deviation (the bound of tests/test_gpu_spec_sparse.py).  A census restricted to an
    empty mask lists nothing and writes nothing;
  * a level whose capacity is below its count takes the dense body (every texel, dense bits), the other one stays listed,
    and `state` says so;
  * the graphed Stage2Step gives the loss and render bits of the same stepper with sparse_light=False; its gradients are
    held to the sparse backward's bounds (tests/test_gpu_spec_sparse.py: bit identity where two dense runs are bit
    identical, else 4 x their run-to-run deviation; the light's gradient 4 x max(that deviation, one ulp of its peak)); a
    second call on another view, with the fine levels poisoned with NaN in between, does the same.
"""
import types

import numpy as np
import pytest
import torch

import shade_cases as sc
from oracle import torch_pbr_ref as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RES = sc.SPEC_RES3
ROUGH = [0.08, 0.5, 1.0]  # CubemapLight._build's roughness per level of a three-level chain
H, W = 48, 64
LANES = {8: dict(spec_max8=1 << 30, spec_max16=1 << 30), 16: dict(spec_max8=0, spec_max16=1 << 30),
         64: dict(spec_max8=0, spec_max16=0)}


@pytest.fixture(autouse=True)
def _every_level_may_be_listed(monkeypatch):
    """The shipped capacities (a tenth and a quarter of a level's texels) are speed thresholds: 48 x 64 pixels read three
    quarters of a 32^2 level.  Here both fine levels must take the listed path, so the capacity is the level; the overflow test sets
    its own."""
    from pbr.renderutils import ops
    monkeypatch.setattr(ops.SparseFineLevels, "CAPACITY", 1.0)


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _generators():
    gens = []
    L = len(RES)
    for level in (0, 1):
        for face in range(6):
            for kind in range(sc.SEAM_KINDS):
                for role in (0, 1):
                    gens.append(sc._specular_seam(RES, level, face, kind, role))
    for lo, hi in ((0.0, 0.07), (0.09, 0.49), (0.51, 0.99), (1.0, 1.05)):  # below the first knot, the two pairs, above the last
        gens += [sc._at_roughness(lambda rng, lo=lo, hi=hi: rng.uniform(lo, hi), "pair")] * 60
    gens += [sc._perpendicular] * 40 + [sc._back_facing] * 40 + [sc._head_on] * 20 + [sc._zero_normal] * 10
    gens += [sc._masked_out] * 200 + [sc._interior(f) for f in range(6)] * 10
    assert len(gens) < H * W  # the rest are fillers (a tenth of them outside the mask)
    return gens


@pytest.fixture(scope="module")
def scene():
    """The G-buffer, the light's mips (the filter's inputs) and the float64 decisions, built once."""
    light = sc.make_light(RES, seed=28)
    margin = lambda g: sc._margin(g, light, [(False, False, False)])  # noqa: E731
    order = np.random.default_rng(5).permutation(H * W)
    g, tags = sc._build_image(_generators(), H, W, 2028, margin, order=order)
    det = tp.shade_with_grads(g, light[0], light[1], sc.lut_np(), {})["details"]
    grads = sc._planes(np.random.default_rng(9), H, W)
    return types.SimpleNamespace(g=g, tags=tags, diffuse=light[0], mips=[tt(m) for m in light[1]], details=det, grads=grads)


def gbuffer(scene, mask):
    g = dict(scene.g)
    if mask == "full":
        g["mask"] = np.ones_like(g["mask"])
    elif mask == "empty":
        g["mask"] = np.zeros_like(g["mask"])
    return g


def dense_levels(scene):
    from pbr.renderutils import ops
    with torch.no_grad():
        return ops.specular_cubemap_levels(scene.mips, ROUGH)


def sparse_levels(scene, g, caps=None, poison=float("nan"), census_mask=False):
    """-> (levels, the SparseFineLevels, marked texel lists per fine level): primed dense, built again, the fine levels
    poisoned, then filled for the G-buffer `g`."""
    from pbr.renderutils import ops
    sp = ops.SparseFineLevels()
    with torch.no_grad():
        ops.specular_cubemap_levels(scene.mips, ROUGH, sparse=sp)
        assert sp.pending is None  # the first build through the object is dense
        lv = ops.specular_cubemap_levels(scene.mips, ROUGH, sparse=sp)
    assert sp.pending is not None and len(sp.out) == 2 and lv[0] is sp.out[0] and lv[1] is sp.out[1]
    for t in sp.out + sp.wsum:
        t.fill_(poison)
    if caps is not None:
        sp.caps = tuple(caps)  # the list buffer keeps its (larger) size
    # every pixel marks, as the shade samples for every pixel; census_mask: only the pixels of g's mask
    assert sp.fill(H, W, tt(g["view_dirs"]), tt(g["roughness"]), normals=tt(g["normals"]),
                   mask=tt(g["mask"].astype(np.uint8)) if census_mask else None)
    rep = sp.report()
    lists, off = [], 0
    host = sp.lists.cpu().numpy()
    for (listed, n), cap in zip(rep, sp.caps):
        lists.append(np.sort(host[off:off + min(n, cap)]) if listed else None)
        off += cap
    for t in sp.needed:
        assert not t.any(), "the list census clears the marks for the next call"
    return lv, sp, rep, lists


def reference_taps(scene, inside):
    """{level: set of texels} the float64 shade samples for the pixels `inside` [H,W]"""
    d = scene.details
    l0, l1 = d["l0"].numpy(), d["l1"].numpy()
    want = {0: set(), 1: set()}
    for lvl in want:
        idx = d["spec"][lvl]["idx"].numpy()
        use = inside & ((l0 == lvl) | ((l1 == lvl) & (l1 != l0)))
        taps = idx[use]
        want[lvl] = set(int(i) for i in taps[taps >= 0])
    return want


@pytest.mark.parametrize("lanes", sorted(LANES))
def test_listed_texels_have_the_dense_bits(scene, lanes):
    import gigs_lib
    with gigs_lib.options(**LANES[lanes]):
        dense = dense_levels(scene)
        lv, sp, rep, lists = sparse_levels(scene, scene.g)
    print("lanes", lanes, "fine levels (listed, texels marked):", rep)
    assert not any(torch.isnan(x).any() for x in dense)
    np.testing.assert_array_equal(bits(lv[2]), bits(dense[2]))  # the coarse level is the dense launch's
    for i in (0, 1):
        assert rep[i][0] and 0 < rep[i][1] <= sp.caps[i] and len(lists[i]) == rep[i][1] == len(set(lists[i]))
        got, want = bits(lv[i]).reshape(-1, 3), bits(dense[i]).reshape(-1, 3)
        np.testing.assert_array_equal(got[lists[i]], want[lists[i]])
        rest = np.ones(len(got), bool)
        rest[lists[i]] = False
        assert rest.any() and np.isnan(lv[i].cpu().numpy().reshape(-1, 3)[rest]).all(), "a texel outside the list was written"
        assert not np.isnan(sp.wsum[i].cpu().numpy().reshape(-1)[lists[i]]).any()
        assert np.isnan(sp.wsum[i].cpu().numpy().reshape(-1)[rest]).all()


@pytest.mark.parametrize("census_mask", [False, True])
def test_marked_set_covers_what_the_float64_shade_samples(scene, census_mask):
    _, sp, rep, lists = sparse_levels(scene, scene.g, census_mask=census_mask)
    inside = scene.g["mask"][..., 0] if census_mask else np.ones((H, W), bool)
    want = reference_taps(scene, inside)
    total = 0
    for lvl in (0, 1):
        got = set(int(i) for i in lists[lvl])
        print("census mask", census_mask, "level", RES[lvl], "marked", len(got), "sampled by the reference", len(want[lvl]),
              "of", 6 * RES[lvl] ** 2)
        assert want[lvl] and want[lvl] <= got, sorted(want[lvl] - got)[:8]
        total += len(got)
    assert total <= 8 * int(inside.sum())


@pytest.mark.parametrize("mask", ["full", "partial", "empty"])
def test_poisoned_fine_levels_never_reach_the_shade(scene, mask):
    import test_gpu_shade_f64 as f64
    g = gbuffer(scene, mask)
    dense = dense_levels(scene)
    lv, sp, rep, lists = sparse_levels(scene, g, census_mask=(mask == "empty"))
    if mask == "empty":
        assert rep == [(True, 0), (True, 0)], rep
        for t in sp.out + sp.wsum:
            assert torch.isnan(t).all(), "an empty list must write nothing"
        return
    diffuse = scene.diffuse
    outs = []
    for levels in (dense, lv):
        case = sc.Case("fwd_sparse_" + mask, g, scene.tags, (diffuse, [x.cpu().numpy() for x in levels]), {},
                       grads=scene.grads, spec_res=RES)
        outs.append((f64.hip_forward(case), f64.hip_backward(case)))
    (fd, bd), (fs, bs) = outs
    bd2 = f64.hip_backward(case.__class__("fwd_dense_again", g, scene.tags, (diffuse, [x.cpu().numpy() for x in dense]), {},
                                          grads=scene.grads, spec_res=RES))
    for name, a, b, c in [(k, fs[k], fd[k], None) for k in fd] + [(k, bs[k], bd[k], bd2[k]) for k in bd]:
        assert not np.isnan(a).any(), name
        if c is None or np.array_equal(bits(b), bits(c)):
            np.testing.assert_array_equal(bits(a), bits(b), err_msg=name)
        else:
            # a light gradient: the shade backward sums it with float atomics, two runs on the DENSE levels differ
            # themselves; held to the sparse backward's bound (tests/test_gpu_spec_sparse.py), 4 x that deviation
            assert name in ("diffuse", "spec64", "spec32", "spec16"), name
            noise, dev = float(np.abs(b - c).max()), float(np.abs(a - b).max())
            print(f"{mask} {name}: dense-dense {noise:.3e}, sparse-dense {dev:.3e}")
            assert dev <= 4.0 * noise, (name, dev, noise)


def test_a_level_over_its_capacity_is_filtered_densely(scene):
    dense = dense_levels(scene)
    _, _, rep0, _ = sparse_levels(scene, scene.g)
    need0 = rep0[0][1]
    lv, sp, rep, lists = sparse_levels(scene, scene.g, caps=(need0 - 1, 6 * RES[1] ** 2))
    assert rep == [(False, need0), (True, rep0[1][1])], rep
    np.testing.assert_array_equal(bits(lv[0]), bits(dense[0]))  # the dense body: every texel, dense bits
    got, want = bits(lv[1]).reshape(-1, 3), bits(dense[1]).reshape(-1, 3)
    np.testing.assert_array_equal(got[lists[1]], want[lists[1]])
    rest = np.ones(len(got), bool)
    rest[lists[1]] = False
    assert np.isnan(lv[1].cpu().numpy().reshape(-1, 3)[rest]).all()


def test_graphed_stepper_matches_the_dense_build_on_two_views():
    import pbr
    import pipeline
    import scenes
    from helpers import GAUSS_KEYS
    scn = dict(scenes.surface_scene(P=4000, sh_degree=2, seed=21, scale_mu=0.03))
    rough = np.full_like(scn["roughness"], 0.9)
    rough[::3] = 0.1   # both fine levels are sampled
    rough[1::3] = 0.3
    scn["roughness"] = rough
    Hs = Ws = 128
    cams = [scenes.orbit_camera(i, 6, Ws, Hs, radius=3.5) for i in (0, 2)]
    camts = [{k: (tt(v) if isinstance(v, np.ndarray) else v) for k, v in c.items()} for c in cams]
    torch.manual_seed(3)
    gt = torch.rand(3, Hs, Ws, device=DEV) * 0.5
    lut = pbr.get_brdf_lut().to(DEV)
    rays = pipeline.canonical_rays(cams[0], DEV)
    vds = [pipeline.view_dirs_for(c, rays, DEV) for c in camts]

    def run(sparse):
        torch.manual_seed(6)
        light = pbr.CubemapLight(base_res=64, device=DEV)
        g = {k: tt(scn[k]).requires_grad_(True) for k in GAUSS_KEYS}
        st = pipeline.Stage2Step(light, lut, scenes.GI_DEFAULTS, 2, fused=True, graphs=True, sparse_light=sparse)
        res, reports = [], []
        for ci in (0, 1):
            for t in list(g.values()) + [light.base]:
                t.grad = None
            o = st(camts[ci], g, gt, vds[ci])
            torch.cuda.synchronize()
            assert st.whole is not None and st.whole.recaptures == 1
            outs = {k: g[k].grad.clone() for k in GAUSS_KEYS if g[k].grad is not None}
            outs["loss"] = torch.tensor([float(o["loss"])], dtype=torch.float64)
            outs["render_rgb"] = o["render_rgb"].clone()
            res.append((outs, light.base.grad.cpu().numpy().astype(np.float64)))
            sp = st.whole.inner.sparse
            assert (sp is not None) == sparse
            if sparse:
                reports.append(sp.report())
                for t in sp.out + sp.wsum:  # whatever the next view does not list must not be read
                    t.fill_(float("nan"))
                torch.cuda.synchronize()
        st.close()
        return res, reports

    d1, _ = run(False)
    d2, _ = run(False)
    s1, reports = run(True)
    print("fine levels (listed, texels marked) per view:", reports)
    assert all(listed and n > 0 for rep in reports for listed, n in rep), reports
    assert reports[0] != reports[1], "the two views should need different texels"
    for view in (0, 1):
        (a_, la), (b_, lb), (c_, lc) = s1[view], d1[view], d2[view]
        for k in sorted(b_, key=lambda k: k not in ("loss", "render_rgb")):
            a, b, c = (x[k].cpu().numpy() for x in (a_, b_, c_))
            assert not np.isnan(a).any(), (view, k)
            if k in ("loss", "render_rgb") or np.array_equal(bits(b), bits(c)):
                np.testing.assert_array_equal(bits(a), bits(b), err_msg="view %d %s" % (view, k))
            else:
                noise_k, dev_k = float(np.abs(b - c).max()), float(np.abs(a - b).max())
                print(f"view {view} {k}: dense-dense {noise_k:.3e}, sparse-dense {dev_k:.3e}")
                assert dev_k <= 4.0 * noise_k, (view, k, dev_k, noise_k)
        noise = float(np.abs(lc - lb).max())
        floor = float(np.spacing(np.float32(np.abs(lb).max())))
        dev = float(np.abs(la - lb).max())
        print(f"view {view} light gradient: peak {np.abs(lb).max():.3e} sparse-dense {dev:.3e} dense-dense {noise:.3e} floor {floor:.3e}")
        assert not np.isnan(la).any() and dev <= 4.0 * max(noise, floor), (view, dev, noise, floor)
