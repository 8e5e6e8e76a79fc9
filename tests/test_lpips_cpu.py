"""CPU: the drop-in lpips package's weight loading (three state-dict layouts, shapes, missing files without a download)
and option checks, and self-checks of the float64 restatement the GPU tests pin the kernels against."""
import os
import urllib.request

import pytest
import torch

import lpips_ref


def _lpips():
    import lpips
    return lpips


def test_state_dict_layouts_map_to_the_same_tensors(tmp_path):
    lp = _lpips()
    ws, bs, lin = lpips_ref.random_weights(seed=3)
    tv, linf, whole = lpips_ref.state_dicts(ws, bs, lin)

    for sd in (tv, whole):
        w2, b2 = lp.vgg_weights(sd)
        assert len(w2) == 13 and len(b2) == 13
        for a, b, (co, ci) in zip(w2, ws, lpips_ref.VGG_CHANNELS):
            assert a.shape == (co, ci, 3, 3) and a.dtype == torch.float32 and torch.equal(a, b)
        for a, b in zip(b2, bs):
            assert torch.equal(a, b)
    for sd in (linf, whole):
        l2 = lp.lin_weights(sd)
        assert [t.shape[0] for t in l2] == [64, 128, 256, 512, 512]
        for a, b in zip(l2, lin):
            assert torch.equal(a, b)

    # files: torchvision checkpoint + lin file, and a whole state dict given as a file or a dict
    torch.save(tv, tmp_path / "vgg16.pth")
    torch.save(linf, tmp_path / "vgg.pth")
    torch.save(whole, tmp_path / "whole.pth")
    for got in (lp.load_weights(vgg_path=str(tmp_path / "vgg16.pth"), model_path=str(tmp_path / "vgg.pth")),
                lp.load_weights(state_dict=str(tmp_path / "whole.pth")), lp.load_weights(state_dict=whole)):
        for xs, ys in zip(got, (ws, bs, lin)):
            assert len(xs) == len(ys) and all(torch.equal(x, y) for x, y in zip(xs, ys))


def test_wrong_shapes_and_missing_keys_are_rejected():
    lp = _lpips()
    ws, bs, lin = lpips_ref.random_weights(seed=4)
    tv, linf, whole = lpips_ref.state_dicts(ws, bs, lin)
    bad = dict(tv)
    bad["features.7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(ValueError, match="features.7.weight"):
        lp.vgg_weights(bad)
    bad = dict(whole)
    bad["lin2.model.1.weight"] = torch.zeros(1, 128, 1, 1)
    with pytest.raises(ValueError, match="lin2"):
        lp.lin_weights(bad)
    bad = dict(tv)
    del bad["features.28.bias"]
    with pytest.raises(KeyError):
        lp.vgg_weights(bad)
    with pytest.raises(KeyError, match="lin4"):
        lp.lin_weights({k: v for k, v in linf.items() if not k.startswith("lin4")})


def test_missing_weights_raise_without_a_download(tmp_path, monkeypatch):
    lp = _lpips()

    def no_download(*a, **k):
        raise AssertionError("lpips attempted a download")

    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", no_download)
    monkeypatch.setattr(torch.hub, "download_url_to_file", no_download)
    monkeypatch.setattr(urllib.request, "urlopen", no_download)
    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path / "hub"))
    want = os.path.join(str(tmp_path / "hub"), "checkpoints", "vgg16-397923af.pth")
    with pytest.raises(FileNotFoundError, match="vgg16-397923af.pth") as ex:
        lp.LPIPS(net="vgg")
    assert want in str(ex.value)
    # the VGG file present, the lin file missing
    ws, bs, lin = lpips_ref.random_weights(seed=5)
    tv, _, _ = lpips_ref.state_dicts(ws, bs, lin)
    os.makedirs(os.path.dirname(want))
    torch.save(tv, want)
    with pytest.raises(FileNotFoundError, match="nowhere.pth"):
        lp.LPIPS(net="vgg", model_path=str(tmp_path / "nowhere.pth"))
    with pytest.raises(FileNotFoundError, match="whole.pth"):
        lp.LPIPS(net="vgg", state_dict=str(tmp_path / "whole.pth"))


def test_unsupported_options_raise():
    lp = _lpips()
    ws, bs, lin = lpips_ref.random_weights(seed=6)
    _, _, whole = lpips_ref.state_dicts(ws, bs, lin)
    for kw in (dict(net="alex"), dict(net="squeeze"), dict(spatial=True), dict(version="0.0"), dict(lpips=False)):
        with pytest.raises(NotImplementedError):
            lp.LPIPS(**{"net": "vgg", "state_dict": whole, **kw})


def test_restatement_self_checks():
    ws, bs, lin = lpips_ref.random_weights(seed=7)
    g = torch.Generator().manual_seed(1)
    a = torch.rand((2, 3, 100, 75), generator=g)
    b = torch.rand((2, 3, 100, 75), generator=g)
    t = lpips_ref.taps(a, ws, bs)
    assert [tuple(x.shape[1:]) for x in t] == [(64, 100, 75), (128, 50, 37), (256, 25, 18), (512, 12, 9), (512, 6, 4)]
    assert all(float(x.abs().max()) > 0 for x in t)
    zero, terms0 = lpips_ref.lpips(a, a, ws, bs, lin)
    assert torch.equal(zero, torch.zeros(2, dtype=torch.float64)) and all(torch.equal(x, zero) for x in terms0)
    ab, terms_ab = lpips_ref.lpips(a, b, ws, bs, lin)
    ba, terms_ba = lpips_ref.lpips(b, a, ws, bs, lin)
    assert torch.allclose(ab, ba, rtol=1e-14, atol=0) and bool((ab > 0).all())
    total = terms_ab[0]
    for x in terms_ab[1:]:
        total = total + x
    assert torch.equal(total, ab)
    # normalize=True is the call on 2x - 1
    n1, _ = lpips_ref.lpips(a, b, ws, bs, lin, normalize=True)
    n2, _ = lpips_ref.lpips(2 * a.double() - 1, 2 * b.double() - 1, ws, bs, lin)
    assert torch.allclose(n1, n2, rtol=1e-14, atol=0)


def test_restatement_matmul_conv_equals_conv2d():
    """The GPU tests run the float64 restatement through nine shifted matrix products (taps(device=...)); on the CPU that
    path equals the conv2d one to float64 rounding."""
    ws, bs, lin = lpips_ref.random_weights(seed=8)
    g = torch.Generator().manual_seed(2)
    a = torch.rand((2, 3, 48, 37), generator=g)
    b = torch.rand((2, 3, 48, 37), generator=g)
    for x, y in zip(lpips_ref.taps(a, ws, bs), lpips_ref.taps(a, ws, bs, device="cpu")):
        assert x.shape == y.shape and float((x - y).abs().max()) <= 1e-12 * float(x.abs().max())
    v0, _ = lpips_ref.lpips(a, b, ws, bs, lin)
    v1, _ = lpips_ref.lpips(a, b, ws, bs, lin, device="cpu")
    assert torch.allclose(v0, v1, rtol=1e-12, atol=0)
