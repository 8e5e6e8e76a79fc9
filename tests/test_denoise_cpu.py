"""CPU: the a-trous denoiser -- the four symbols' place in the C ABI, the properties of the numpy restatement
(tests/denoise_ref.py) that the definition promises, and what denoise.atrous refuses before any launch."""
import math
import os
import re

import numpy as np
import pytest

import denoise_ref as dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_symbols_are_declared_bound_and_built():
    import build
    import gigs_lib
    with open(os.path.join(ROOT, "include", "gigs_hip.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "gi-gs_amd", "csrc", "denoise.hip")) as fh:
        src = fh.read()
    assert "denoise.hip" in build.SOURCES and "Denoising ray-traced planes" in header
    for symbol, n_args in (("gigs_denoise_pack", 13), ("gigs_denoise_variance", 13), ("gigs_denoise_atrous", 16), ("gigs_denoise_unpack", 9)):
        proto = re.search(r"int %s\(([^;]*)\);" % symbol, header)
        assert proto is not None
        assert len(gigs_lib.SIGNATURES[symbol][1]) == len(proto.group(1).split(",")) == n_args
        assert re.sub(r"\s+", " ", proto.group(1)) in re.sub(r"\s+", " ", src)
    assert re.search(r"#define GIGS_DENOISE_MAX_CHANNELS 16\b", header) and re.search(r"#define GIGS_DENOISE_MAX_STEP 16\b", header)
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    for name in ("exp", "pow", "sqrt", "fmax", "fmin", "atomic"):  # + - * / only, max as a comparison, no atomics
        assert not re.search(r"\b_*%s\w*\s*\(" % name, code), name


def _signal(C, H, W, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (C, H, W)).astype(F)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_a_constant_signal_returns_its_own_bits_and_variance_zero(n):
    H, W = 23, 31
    p, nr, mask, _ = dn.crease_guide(H, W)
    mask[::7] = 0
    x = np.empty((7, H, W), F)
    x[:] = np.array([0.3, 1.7, 0.1, 0.7, 12.5, 1e-3, 0.9], F)[:, None, None]
    rough = np.linspace(0.1, 0.9, H * W).astype(F)
    for groups, r in (([1, 3, 3], None), ([3, 3, 1], rough), (None, None)):
        for sigma_l in (4.0, 0.0):
            got, var = dn.atrous(x, p, nr, mask, groups, n, plane_distance=0.5, sigma_l=sigma_l, roughness=r)
            assert got.dtype == var.dtype == F and np.array_equal(_bits(got), _bits(x)) and not var.any()
            assert var.shape == (7 if groups is None else 3, H, W)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_an_edge_of_the_geometry_is_not_crossed(n):
    """Signals 0 and 1 on two half-planes that lie more than plane_distance apart (the depth step) or meet at 90 degrees (the
    crease): a weight across the edge is exactly 0, so both stay exactly 0 and 1 -- with the signal weight off, so that the
    geometry alone does it, and with it on."""
    H, W = 37, 29
    p, nr, mask, region = dn.crease_guide(H, W, step_height=3.0)
    assert all((region == k).sum() > 100 for k in (0, 1, 2))
    for values in ((0.0, 1.0, 0.0), (1.0, 0.0, 1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)):  # floor, lowered floor, wall
        x = np.array(values, F)[region][None]
        for sigma_l in (0.0, 4.0):
            got, var = dn.atrous(x, p, nr, mask, None, n, plane_distance=2.0, sigma_l=sigma_l)
            assert np.array_equal(_bits(got), _bits(x)), (values, sigma_l)
            assert not var.any()
    # closer than plane_distance the step IS crossed: the assertion above is not vacuous
    x = (region == 1).astype(F)[None]
    got, _ = dn.atrous(x, p, nr, mask, None, n, plane_distance=4.0, sigma_l=0.0)
    assert not np.array_equal(got, x)


def _b3_float64(x, n):
    """n iterations of the separable a-trous B3 convolution in float64, periodic: only pixels further than 2 (2^n - 1) from the
    border are compared."""
    h = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    x = x.astype(np.float64)
    for i in range(n):
        s = 1 << i
        x = sum(h[k] * np.roll(x, -(k - 2) * s, axis=0) for k in range(5))
        x = sum(h[k] * np.roll(x, -(k - 2) * s, axis=1) for k in range(5))
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_flat_plane_without_signal_weight_is_the_b3_convolution(n):
    """On a flat plane every g = 1 and with sigma_l = 0 every l = 1, so w = h[dy] h[dx] exactly and Wsum = 1 exactly (its
    partial sums are multiples of 2^-8).  An iteration then rounds, for a signal in [0, 1]: 25 differences and 25 products
    (each below 1 in magnitude, half an ulp(1) = 2^-24 each at most), 24 additions of partial sums below 1, one division by 1
    (exact) and one final sum: 76 roundings of at most 2^-24.  The filter is convex, so the error of the earlier iterations
    passes through with a gain of at most 1: |error| <= 76 n 2^-24."""
    H = W = 72
    x = _signal(1, H, W, seed=n)
    p, nr, mask = dn.flat_guide(H, W)
    got, _ = dn.atrous(x, p, nr, mask, None, n, plane_distance=1.0, sigma_l=0.0)
    want = _b3_float64(x[0], n)
    m = 2 * ((1 << n) - 1)
    assert m < H // 2
    err = np.abs(got[0].astype(np.float64) - want)[m:H - m, m:W - m]
    bound = 76 * n * 2.0 ** -24
    print("n=%d: %d interior pixels, largest error %.3g = %.1f ulp(1), bound %.3g" % (n, err.size, err.max(), err.max() * 2.0 ** 23, bound))
    assert err.size >= 144 and float(err.max()) <= bound


def test_noise_variance_drops_by_the_b3_factor():
    """One iteration on i.i.d. Gaussian noise over a flat plane, signal weight off: the output's variance is
    (sum h^2)^2 = (70/256)^2 = 0.0748 times the input's.  252 x 252 = 63504 interior pixels; the output is correlated over the
    5 x 5 footprint, so the sample variance has some 63504 / 9 independent terms and a relative standard error of
    sqrt(2 x 9 / 63504) = 1.7 %: the bound is 4 standard errors, 7 %.  The variance PLANE obeys the same law exactly in the mean
    (V = sum w^2 var_q is linear), up to the border and float32 rounding: 0.5 %."""
    H = W = 256
    x = np.random.default_rng(5).normal(0.5, 0.1, (1, H, W)).astype(F)
    p, nr, mask = dn.flat_guide(H, W)
    prm = dn.parameters(1.0, 32, 0.0)
    guide = dn._Guide(p, nr, None, np.ones((H, W), bool), prm)
    var0 = dn.variance(x, [1], guide)
    got, var1 = dn.step(x, var0, [1], guide, 1)
    inner = (slice(None), slice(2, H - 2), slice(2, W - 2))
    ratio = float(got[inner].astype(np.float64).var() / x[inner].astype(np.float64).var())
    factor = (70.0 / 256.0) ** 2
    inner4 = (slice(None), slice(4, H - 4), slice(4, W - 4))
    plane = float(var1[inner].astype(np.float64).mean() / var0[inner4].astype(np.float64).mean())
    print("variance ratio %.5f, plane ratio %.5f, (70/256)^2 = %.5f" % (ratio, plane, factor))
    assert abs(ratio / factor - 1.0) < 0.07 and abs(plane / factor - 1.0) < 0.005
    # and the 5 x 5 estimate of launch A sees the noise: its mean is the input's variance times 24/25 (m is the window's own mean)
    assert abs(float(var0[inner].mean()) / (0.01 * 24.0 / 25.0) - 1.0) < 0.03


def test_pixels_that_are_not_live_pass_through_and_weigh_nothing():
    H, W = 19, 21
    p, nr, mask, _ = dn.crease_guide(H, W)
    x = _signal(4, H, W, seed=2)
    rough = np.full(H * W, 0.5, F)
    dead = np.zeros(H * W, bool)
    mask = mask.copy()
    mask[::5] = 0
    dead[::5] = True
    p, nr, rough = p.copy(), nr.copy(), rough.copy()
    for i, (arr, col) in enumerate(((p, 1), (nr, 2), (rough, None))):
        q = 3 * W + 4 + 2 * i
        if col is None:
            arr[q] = np.inf
        else:
            arr[q, col] = np.nan
        dead[q] = True
    x.reshape(4, -1)[2, 6 * W + 7] = np.nan
    dead[6 * W + 7] = True
    assert np.array_equal(dn.live_pixels(x, p, nr, mask, rough).reshape(-1), ~dead)
    got, var = dn.atrous(x, p, nr, mask, [1, 3], 3, plane_distance=1.5, roughness=rough)
    d2 = dead.reshape(H, W)
    assert np.array_equal(_bits(got[:, d2]), _bits(x[:, d2])) and not var[:, d2].any()
    assert np.isfinite(got[:, ~d2]).all() and np.isfinite(var).all() and not np.array_equal(got[:, ~d2], x[:, ~d2])
    # other values in the dead pixels, finite or not, change no bit anywhere else
    y = x.copy()
    y[:, d2] = np.array([1e30, -7.0, np.inf, 0.0], F)[:, None]
    got2, var2 = dn.atrous(y, p, nr, mask, [1, 3], 3, plane_distance=1.5, roughness=rough)
    assert np.array_equal(_bits(got2[:, ~d2]), _bits(got[:, ~d2])) and np.array_equal(_bits(var2), _bits(var))
    # a normal without length is live but weighs nothing and is left as it is
    nr[9 * W + 9] = 0.0
    got3, var3 = dn.atrous(x, p, nr, mask, [1, 3], 2, plane_distance=1.5, roughness=rough)
    assert np.array_equal(_bits(got3[:, 9, 9]), _bits(x[:, 9, 9])) and not var3[:, 9, 9].any()


def test_what_is_refused():
    import torch
    import denoise
    hp = denoise.host_parameters(0.5, 32, 4.0, 0.25)
    assert hp == dict(e=5, inv_plane2=4.0, sigma_l2=16.0, eps=float(np.float32(1e-10)), inv_rough2=16.0)
    ref = dn.parameters(0.5, 32, 4.0, 0.25)
    assert all(float(ref[k]) == hp[k] for k in hp) and float(dn.EPS) == denoise.EPS
    off = denoise.host_parameters(0.3, 1, 0.0, None)
    assert off["e"] == 0 and off["sigma_l2"] == 0.0 and off["eps"] == math.inf and off["inv_rough2"] is None
    assert off["inv_plane2"] == float(np.float32(1.0 / 0.09)) == float(dn.parameters(0.3, 1, 0.0)["inv_plane2"])
    assert [denoise.record_floats(c, g) for c, g in ((1, 1), (7, 3), (11, 5), (16, 16), (3, 1))] == [4, 12, 16, 32, 4]
    for bad in (dict(plane_distance=0.0), dict(plane_distance=-1.0), dict(plane_distance=float("nan")), dict(plane_distance=float("inf")),
                dict(plane_distance=1e-30), dict(normal_power=0), dict(normal_power=3), dict(normal_power=256), dict(normal_power=2.0),
                dict(sigma_l=-1.0), dict(sigma_l=float("nan")), dict(sigma_l=1e30), dict(roughness_sigma=0.0), dict(roughness_sigma=1e-30)):
        with pytest.raises(ValueError, match="denoise.atrous"):
            denoise.host_parameters(**dict(dict(plane_distance=0.5, normal_power=32, sigma_l=4.0, roughness_sigma=0.25), **bad))
    p, nr, mask = dn.flat_guide(4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        denoise.atrous(torch.zeros((1, 4, 5)), torch.from_numpy(p), torch.from_numpy(nr), torch.from_numpy(mask))
    with pytest.raises(RuntimeError, match="no CPU path"):
        denoise.atrous(np.zeros((1, 4, 5), F), p, nr, mask)
