"""LPIPS-VGG on the GPU (gigs_lpips_vgg through the drop-in lpips package) against the float64 restatement in
tests/lpips_ref.py with seeded He-initialised weights: raw taps, values, exact identities (zero distance, symmetry, batch
invariance, repeatability), the interface, graph capture, and the three evaluators' opt-in LPIPS."""
import numpy as np
import pytest
import torch

import lpips_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def weights():
    return lpips_ref.random_weights(seed=11)


@pytest.fixture(scope="module")
def fn(weights):
    import lpips
    _, _, whole = lpips_ref.state_dicts(*weights)
    return lpips.LPIPS(net="vgg", state_dict=whole).to(DEV)


def _images(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, H, W), generator=g)


def _close(got, ref, rtol=1e-5, floor=1e-7):
    got, ref = float(got), float(ref)
    assert abs(got - ref) <= max(rtol * abs(ref), floor), (got, ref, abs(got - ref) / max(abs(ref), 1e-300))


@pytest.mark.parametrize("H,W", [(64, 48), (100, 75)])
@pytest.mark.parametrize("n", [1, 3])
def test_taps_match_float64(fn, weights, n, H, W):
    a, b = _images(n, H, W, seed=n * 1000 + H), _images(n, H, W, seed=n * 1000 + H + 1)
    taps = _tap_buffers(n, H, W)
    fn.record(a.to(DEV), b.to(DEV), taps=taps)
    _check_taps(taps, n, (a, b), weights, None)


@pytest.mark.parametrize("H,W", [(64, 48), (100, 75)])
def test_value_matches_float64(fn, weights, H, W):
    a, b = _images(3, H, W, seed=21), _images(3, H, W, seed=22)
    noise = torch.randn((3, 3, H, W), generator=torch.Generator().manual_seed(23))
    near = a + 0.01 * noise
    for x, y in ((a, b), (a, near)):
        ref, terms = lpips_ref.lpips(x, y, *weights)
        rec = fn.record(x.to(DEV), y.to(DEV)).cpu()
        for i in range(3):
            _close(rec[i, 0], ref[i])
            for l in range(5):
                _close(rec[i, 1 + l], terms[l][i])
    ref_near, _ = lpips_ref.lpips(a, near, *weights)
    ref_far, _ = lpips_ref.lpips(a, b, *weights)
    assert float(ref_near.max()) < 0.1 * float(ref_far.min())


def test_full_size_256(fn, weights):
    a, b = _images(1, 256, 256, seed=31), _images(1, 256, 256, seed=32)
    ref, _ = lpips_ref.lpips(a, b, *weights)
    got = fn(a.to(DEV), b.to(DEV))
    assert got.shape == (1, 1, 1, 1) and got.dtype == torch.float32 and not got.requires_grad
    _close(got.double().cpu().reshape(()), ref[0])


def _conv_tiles(n, H, W):
    """The cout tile width gigs_lpips_vgg picks for each MFMA conv (conv1_2 .. conv5_3), restating its dispatch
    (lpips.hip): 64 for Cout = 64 and for grids under 512 workgroups of 128-wide tiles, else 128."""
    out, cout = [], (64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
    levels = (0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
    for co, lv in zip(cout, levels):
        P = 2 * n * (H >> lv) * (W >> lv)
        ptiles = (P + 127) // 128
        out.append(64 if co == 64 or ptiles * (co // 128) < 512 else 128)
    return out


def _check_taps(taps, n, imgs, weights, device):
    ws, bs, _ = weights
    for k, img in enumerate(imgs):
        ref = lpips_ref.taps(img, ws, bs, device=device)
        for l in range(5):
            got = taps[5 * k + l].double()
            r = ref[l].to(got.device)
            scale = float(r.abs().max())
            assert scale > 0
            err = float((got - r).abs().max())
            assert err <= 1e-5 * scale, (k, l, err, scale)


def _tap_buffers(n, H, W):
    shapes = [(64, H, W), (128, H // 2, W // 2), (256, H // 4, W // 4), (512, H // 8, W // 8), (512, H // 16, W // 16)]
    return [torch.full((n, *s), float("nan"), device=DEV) for s in shapes + shapes]


def test_wide_tiles_at_800_match_float64(fn, weights):
    """800x800 (the reference's novel-view size): 128-wide cout tiles at levels 1-3 (Cin 64 .. 512), 64-wide at level 4;
    raw taps and the value against float64 computed on the GPU."""
    tiles = _conv_tiles(1, 800, 800)
    assert tiles[1:9] == [128] * 8 and tiles[9:] == [64] * 3
    a, b = _images(1, 800, 800, seed=71), _images(1, 800, 800, seed=72)
    taps = _tap_buffers(1, 800, 800)
    rec = fn.record(a.to(DEV), b.to(DEV), taps=taps).cpu()
    _check_taps(taps, 1, (a, b), weights, DEV)
    del taps
    ref, terms = lpips_ref.lpips(a, b, *weights, device=DEV)
    _close(rec[0, 0], ref[0])
    for l in range(5):
        _close(rec[0, 1 + l], terms[l][0])


def test_batch_crossing_the_tile_switch(fn, weights):
    """192x192: a batch of 4 runs conv2_x with 128-wide tiles, one image alone with 64-wide tiles.  The batch's taps match
    float64 and each image's record has the same bits as that image alone."""
    assert 128 in _conv_tiles(4, 192, 192) and 128 not in _conv_tiles(1, 192, 192)
    a, b = _images(4, 192, 192, seed=81), _images(4, 192, 192, seed=82)
    taps = _tap_buffers(4, 192, 192)
    rec = fn.record(a.to(DEV), b.to(DEV), taps=taps).cpu()
    _check_taps(taps, 4, (a, b), weights, DEV)
    for i in range(4):
        assert torch.equal(fn.record(a[i].to(DEV), b[i].to(DEV)).cpu()[0], rec[i]), i


def test_exact_identities(fn):
    a, b = _images(4, 72, 88, seed=41).to(DEV), _images(4, 72, 88, seed=42).to(DEV)
    assert torch.equal(fn.record(a, a)[:, 0].cpu(), torch.zeros(4, dtype=torch.float64))
    assert torch.equal(fn.record(a, a).cpu(), torch.zeros((4, 6), dtype=torch.float64))
    ab, ba = fn.record(a, b).cpu(), fn.record(b, a).cpu()
    assert torch.equal(ab, ba)
    assert bool((ab[:, 0] > 0).all())
    for i in range(4):  # image i of the batch == that image alone
        assert torch.equal(fn.record(a[i], b[i]).cpu()[0], ab[i]), i
    assert torch.equal(fn.record(a, b).cpu(), ab)  # two calls
    big0, big1 = _images(1, 800, 800, seed=43).to(DEV), _images(1, 800, 800, seed=44).to(DEV)
    r1 = fn.record(big0, big1).cpu()
    r2 = fn.record(big0, big1).cpu()
    assert torch.equal(r1, r2) and float(r1[0, 0]) > 0


def test_interface(fn):
    import lpips
    a, b = _images(2, 40, 52, seed=51).to(DEV), _images(2, 40, 52, seed=52).to(DEV)
    one = fn(a[0], b[0])
    assert one.shape == (1, 1, 1, 1) and one.dtype == torch.float32
    both = fn(a, b)
    assert both.shape == (2, 1, 1, 1) and torch.equal(both[0], one[0])
    assert torch.equal(fn(a, b, normalize=True), fn(2 * a - 1, 2 * b - 1))
    val, layers = fn(a, b, retPerLayer=True)
    assert torch.equal(val, both) and len(layers) == 5
    tot = layers[0].double()
    for x in layers[1:]:
        tot = tot + x.double()
    assert torch.allclose(tot, val.double(), rtol=1e-6, atol=0)
    for H, W in ((15, 40), (40, 15), (8, 8)):
        x = _images(1, H, W, seed=53).to(DEV)
        with pytest.raises(ValueError):
            fn(x, x)
    assert lpips.LPIPS is type(fn)


def test_graph_capture_matches_eager(fn):
    a, b = _images(2, 96, 80, seed=61).to(DEV), _images(2, 96, 80, seed=62).to(DEV)
    c, d = _images(2, 96, 80, seed=63).to(DEV), _images(2, 96, 80, seed=64).to(DEV)
    eager = fn.record(a, b).clone()
    eager_cd = fn.record(c, d).clone()
    assert not torch.equal(eager[:, 0].float(), eager_cd[:, 0].float())
    sa, sb = a.clone(), b.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn.record(sa, sb)  # warm-up: the scratch exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(sa, sb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(2).cpu(), eager[:, 0].float().cpu())
    sa.copy_(c)  # a different pair: the replay recomputes from its inputs
    sb.copy_(d)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(2).cpu(), eager_cd[:, 0].float().cpu())
    del graph
    torch.cuda.synchronize()


def _tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_novel_view_evaluator_lpips(fn):
    import evaluate
    import pipeline
    import relight
    import scenes
    from oracle import stage2_ref
    W, H = 176, 144
    sc = scenes.surface_scene(P=9000, sh_degree=2, seed=4, scale_mu=0.03)
    gi = scenes.GI_DEFAULTS
    light = relight.make_light(_tt(scenes.synthetic_envmap(128, 256, seed=5)), res=64)
    g = {k: _tt(sc[k]) for k in stage2_ref.KEYS}
    rng = np.random.default_rng(1)
    alpha = _tt((rng.uniform(size=(1, H, W)) > 0.1).astype(np.float32))
    gt = _tt(rng.uniform(size=(3, H, W)).astype(np.float32))
    plain = evaluate.NovelViewEvaluator(light, gi, 2, graphs=False)
    evs = {m: evaluate.NovelViewEvaluator(light, gi, 2, graphs=(m == "graphed"), lpips=fn) for m in ("eager", "graphed")}
    want = {m: [] for m in evs}
    for view in (1, 5, 1):
        cam = scenes.orbit_camera(view, 8, W, H, radius=3.5)
        cam_t = {k: (_tt(v) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
        vd = pipeline.view_dirs_for(cam_t, pipeline.canonical_rays(cam, DEV), DEV)
        plain(cam_t, g, vd, gt, alpha)
        gt_c = (gt * alpha).clamp(0, 1)
        for m, ev in evs.items():
            pbr = ev(cam_t, g, vd, gt, alpha)["pbr"].clone()
            want[m].append(float(fn(gt_c, pbr).reshape(())))
    assert set(plain.results()) == {"psnr_avg", "ssim_avg", "n_views"}
    for m, ev in evs.items():
        r = ev.results()
        assert set(r) == {"psnr_avg", "ssim_avg", "n_views", "lpips_avg"}
        assert r["n_views"] == 3 and r["lpips_avg"] > 0
        assert r["lpips_avg"] == pytest.approx(sum(want[m]) / 3, rel=1e-12, abs=0), m
        lp = ev.lpips_records()
        assert lp.shape == (3, 6) and torch.allclose(lp[0], lp[2], rtol=1e-5, atol=0)
        assert r["psnr_avg"] == pytest.approx(plain.results()["psnr_avg"], rel=1e-6)
    assert evs["eager"].results()["lpips_avg"] == pytest.approx(evs["graphed"].results()["lpips_avg"], rel=1e-4)
    evs["graphed"].close()


def test_relight_evaluator_and_albedo_metrics_lpips(fn):
    import torch.nn.functional as F
    import evaluate
    import relight
    K, H, W = 3, 64, 80
    gen = torch.Generator(device="cpu").manual_seed(3)
    pred = (torch.rand((2, K, 3, H, W), generator=gen) * 1.2 - 0.1).to(DEV)
    gt = torch.rand((2, K, 3, 2 * H, 2 * W), generator=gen).to(DEV)
    names = ["a", "b", "c"]
    plain = relight.RelightEvaluator(names)
    ev = relight.RelightEvaluator(names, lpips=fn)
    for v in range(2):
        plain.add(pred[v], gt[v])
        ev.add(pred[v], gt[v])
    res, res0 = ev.results(), plain.results()
    for k, name in enumerate(names):
        assert set(res0[name]) == {"psnr_avg", "ssim_avg", "n_views"}
        assert set(res[name]) == {"psnr_avg", "ssim_avg", "n_views", "lpips_avg"}
        assert res[name]["psnr_avg"] == res0[name]["psnr_avg"] and res[name]["ssim_avg"] == res0[name]["ssim_avg"]
        vals = []
        for v in range(2):
            q = relight.quantize_8bit(pred[v, k])
            g = F.interpolate(gt[v, k][None], size=(H, W), mode="bilinear", align_corners=False)[0]
            vals.append(float(fn(g, q).reshape(())))
        assert res[name]["lpips_avg"] == pytest.approx(sum(vals) / 2, rel=1e-12, abs=0), name
    assert res["a"]["lpips_avg"] != res["b"]["lpips_avg"]

    # albedo_metrics: lpips(gt, pred * ratio)
    rng = np.random.default_rng(7)
    gts = [_tt(rng.uniform(0.1, 0.9, size=(48, 56, 3)).astype(np.float32)) for _ in range(3)]
    preds = [_tt(rng.uniform(0.1, 0.9, size=(48, 56, 3)).astype(np.float32)) for _ in range(3)]
    masks = [_tt(rng.uniform(size=(48, 56)) > 0.3) for _ in range(3)]
    r0 = evaluate.albedo_metrics(gts, preds, masks)
    r1 = evaluate.albedo_metrics(gts, preds, masks, lpips=fn)
    assert set(r0) == {"albedo_psnr", "albedo_ssim", "roughmse"}
    assert set(r1) == set(r0) | {"albedo_lpips"} and all(r1[k] == r0[k] for k in r0)
    ratio = evaluate.albedo_ratio(gts, preds, masks)
    vals = [float(fn(gt.permute(2, 0, 1), pr.permute(2, 0, 1) * ratio[:, None, None]).reshape(()))
            for gt, pr in zip(gts, preds)]
    assert r1["albedo_lpips"] == pytest.approx(sum(vals) / 3, rel=1e-12, abs=0) and r1["albedo_lpips"] > 0
