"""CPU: the evaluation module's public surface (gi-gs_amd/evaluate.py, CubemapLight.export_envmap) and the pure
torch reduction albedo_ratio against render.py's expression."""
import inspect

import numpy as np
import pytest
import torch


def test_export_envmap_signature_and_missing_cv2():
    from pbr import CubemapLight
    sig = inspect.signature(CubemapLight.export_envmap)
    assert list(sig.parameters) == ["self", "filename", "res", "return_img"]
    assert sig.parameters["filename"].default is None and sig.parameters["res"].default == [512, 1024]
    assert sig.parameters["return_img"].default is False
    try:
        import cv2  # noqa: F401
    except ImportError:
        light = CubemapLight(base_res=16, device="cpu")
        with pytest.raises(ImportError, match="cv2"):
            light.export_envmap("envmap.exr")


def test_evaluator_surface():
    import evaluate
    assert evaluate.PLANES == ("pbr", "DIR", "indirect", "albedo", "roughness", "metallic", "occlusion", "normal",
                               "from_depth")
    params = list(inspect.signature(evaluate.NovelViewEvaluator.__init__).parameters)
    assert params[:8] == ["self", "light", "gi", "sh_degree", "metallic", "tone", "gamma", "graphs"]
    assert list(inspect.signature(evaluate.NovelViewEvaluator.__call__).parameters) == [
        "self", "cam", "g", "view_dirs", "gt_image", "alpha_mask"]
    assert "LPIPS" in evaluate.__doc__ or "lpips" in evaluate.__doc__


def test_metrics_scratch_covers_both_entries():
    import gigs_lib
    lib = gigs_lib.lib()
    n = lib.gigs_image_metrics_scratch_bytes(3, 800, 800)
    assert n >= 4 * 3 * 25 * 25 * 8 and n >= 1024 * 8
    assert lib.gigs_image_metrics_scratch_bytes(0, 8, 8) == 0


@pytest.mark.parametrize("views,even", [(3, False), (2, True)])
def test_albedo_ratio_is_torch_lower_median(views, even):
    import evaluate
    rng = np.random.default_rng(5)
    gts, preds, masks = [], [], []
    total = 0
    for v in range(views):
        H, W = 9 + v, 7
        gt = torch.from_numpy(rng.integers(0, 4, size=(H, W, 3)).astype(np.float32) / 4)  # many ties
        pred = torch.from_numpy(rng.integers(0, 3, size=(H, W, 3)).astype(np.float32) / 2)  # zeros hit the clamp
        m = torch.from_numpy(rng.uniform(size=(H, W)) > 0.3)
        gts.append(gt), preds.append(pred), masks.append(m)
        total += int(m.sum())
    if even != (total % 2 == 0):
        masks[0].view(-1)[int(torch.nonzero(masks[0].view(-1))[0])] = False
        total -= 1
    assert (total % 2 == 0) == even
    got = evaluate.albedo_ratio(gts, preds, masks)
    g = torch.cat([a[m] for a, m in zip(gts, masks)], dim=0)
    p = torch.cat([a[m] for a, m in zip(preds, masks)], dim=0)
    want, _ = (g / p.clamp(min=1e-6)).median(dim=0)
    assert got.shape == (3,) and torch.equal(got, want)
    # the lower median: for an even count it is the smaller of the two middle values
    srt = (g / p.clamp(min=1e-6)).sort(dim=0).values
    assert torch.equal(got, srt[(srt.shape[0] - 1) // 2])
