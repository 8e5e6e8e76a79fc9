"""CPU: the K-light relighting entry points are declared and exported, the 8-bit quantiser of RelightEvaluator matches
torchvision.utils.save_image's formula, and MultiRelighter refuses mismatched lights before any GPU work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gigs_ssr_multi", "gigs_shade_fwd_multi")


def test_multi_light_entries_declared_and_exported():
    import gigs_lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gigs_hip.h")).read(), flags=re.S)
    lib = ctypes.CDLL(gigs_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in gigs_lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert re.search(r"#define GIGS_MAX_LIGHTS 16\b", open(os.path.join(ROOT, "include", "gigs_hip.h")).read())
    import relight
    assert relight.MAX_LIGHTS == 16


def _save_image_roundtrip(x: np.ndarray) -> np.ndarray:
    """torchvision.utils.save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8), in float32; the PNG read / 255."""
    y = np.clip(x.astype(np.float32) * np.float32(255) + np.float32(0.5), 0, 255)
    return (y.astype(np.uint8).astype(np.float32) / np.float32(255)).astype(np.float32)


def test_quantize_8bit_matches_save_image():
    import relight
    rng = np.random.default_rng(0)
    ties = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)  # (k + 0.5) / 255: 0.5-ties after * 255
    exact = np.arange(256, dtype=np.float32) / np.float32(255)
    out_of_range = np.array([-1.0, -0.002, -0.0, 1.0, 1.0001, 1.002, 7.0, 1e30, -1e30, np.inf, -np.inf], np.float32)
    x = np.concatenate([ties, exact, np.nextafter(ties, np.float32(0)), np.nextafter(ties, np.float32(1)), out_of_range,
                        rng.uniform(-0.2, 1.2, 5000).astype(np.float32)])
    got = relight.quantize_8bit(torch.from_numpy(x)).numpy()
    want = _save_image_roundtrip(x)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
    assert got.min() == 0.0 and got.max() == 1.0


def test_multi_relighter_rejects_mismatched_lights_on_cpu():
    import relight
    from pbr import CubemapLight
    a, b = CubemapLight(base_res=16, device="cpu"), CubemapLight(base_res=32, device="cpu")
    with pytest.raises(ValueError, match="resolution"):
        relight.MultiRelighter([a, b], {}, 2)
    with pytest.raises(ValueError):
        relight.MultiRelighter([], {}, 2)
    with pytest.raises(ValueError):
        relight.MultiRelighter([a] * 17, {}, 2)
    assert not hasattr(a, "specular") and not hasattr(b, "specular")  # no mips were built


def _planes(seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand((3, 5, 7), generator=gen), torch.rand((1, 5, 7), generator=gen), torch.rand((1, 5, 7), generator=gen)


def test_gbuffer_from_planes_refuses_cpu_tensors():
    import relight
    a, r, m = _planes()
    three = torch.zeros(3, 5, 7)
    planes = dict(depth_map=r, normal_map=three, occlusion_map=r, albedo_map=a, roughness_map=r, metallic_map=m,
                  out_normal_view=three, depth_pos=three)
    scratch = relight.Scratch()
    with pytest.raises(RuntimeError, match="no CPU path"):
        relight.gbuffer_from_planes(planes, torch.eye(4), False, scratch)
    assert not scratch  # refused before anything was allocated


@pytest.mark.parametrize("metallic", [False, True])
def test_fused_f0_is_the_reference_branch_written_out(metallic):
    """relight.py:236-240 in the spelling of the fused paths: metallic=False -> F0 = 0.04 + albedo * metallic_map and the
    metallic map; metallic=True -> the 0.04 / zero-plane pair."""
    import relight
    a, r, m = _planes(1)
    F0, metallic_in = relight.fused_f0(a, r, m, metallic)
    assert F0.shape == a.shape and metallic_in.shape == r.shape and F0.dtype == metallic_in.dtype == torch.float32
    if metallic:
        assert torch.equal(F0, torch.full((3, 5, 7), 0.04)) and torch.equal(metallic_in, torch.zeros(1, 5, 7))
    else:
        assert torch.equal(F0, torch.addcmul(torch.full_like(a, 0.04), a, m)) and metallic_in is m
        assert float((F0 - 0.04).abs().max()) > 0.1
