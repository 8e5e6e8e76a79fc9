"""Denoising ray-traced planes: a variance-guided, edge-avoiding a-trous wavelet filter (csrc/denoise.hip) over the planes the
per-pixel tracers return (mesh_render.RaytracedLight.planes / .reflections / .shadows), guided by their prepared points and
normals.

    atrous(signal, points, normals, mask, groups, iterations, ...) -> (filtered [C,H,W], variance [G,H,W], report)

include/gigs_hip.h, "Denoising ray-traced planes", states the arithmetic (float32, + - * / only, polynomial edge-stopping
functions of compact support) and tests/denoise_ref.py restates it in numpy bit for bit.  One call filters at most
MAX_CHANNELS channels; more is the caller's loop.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

import gigs_lib

_lib = gigs_lib.lib()

MAX_CHANNELS = 16  # GIGS_DENOISE_MAX_CHANNELS
MAX_ITERATIONS = 5  # steps 1 .. GIGS_DENOISE_MAX_STEP = 16
GUIDE_FLOATS = 8
EPS = float(np.float32(1e-10))  # the eps of r = 1 / (sigma_l2 var + eps): far below the variance of any estimate of 64 rays
# The shipped defaults ("Denoising ray-traced planes", records how they were chosen).
ITERATIONS = 4
NORMAL_POWER = 32
SIGMA_L = 4.0
ROUGHNESS_SIGMA = 0.25
PLANE_FRACTION = 0.02  # plane_distance = None: this share of the largest extent of the live points


def record_floats(channels: int, n_groups: int) -> int:
    """The floats of a pixel's signal record: the C values, the G variances, padded to whole float4s."""
    return 4 * ((channels + n_groups + 3) // 4)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def host_parameters(plane_distance: float, normal_power: int, sigma_l: float, roughness_sigma: Optional[float]) -> Dict:
    """The numbers the launches take, made on the host: e with normal_power = 2^e, inv_plane2 = float32(1 / plane_distance^2),
    sigma_l2 = float32(sigma_l^2) and eps (sigma_l = 0: 0 and +inf, the signal weight off), inv_rough2 =
    float32(1 / roughness_sigma^2) or None.  Raises ValueError on what the library would refuse."""
    what = "denoise.atrous"
    if isinstance(normal_power, bool) or not isinstance(normal_power, (int, np.integer)) or int(normal_power) not in [1 << e for e in range(8)]:
        raise ValueError("%s: normal_power is a power of two in [1, 128], got %r" % (what, normal_power))

    def positive(v, name):
        v = float(v)
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError("%s: %s must be positive and finite, got %r" % (what, name, v))
        with np.errstate(over="ignore"):
            inv = float(np.float32(1.0 / (v * v))) if v * v > 0.0 else math.inf
        if not math.isfinite(inv):
            raise ValueError("%s: 1 / %s^2 is not a finite float32" % (what, name))
        return inv

    sigma_l = float(sigma_l)
    with np.errstate(over="ignore"):
        square = float(np.float32(sigma_l * sigma_l)) if math.isfinite(sigma_l) else math.inf
    if not (sigma_l >= 0.0 and math.isfinite(square)):
        raise ValueError("%s: sigma_l must be >= 0 with a finite float32 square (0: the signal weight is off), got %r" % (what, sigma_l))
    out = dict(e=int(normal_power).bit_length() - 1, inv_plane2=positive(plane_distance, "plane_distance"),
               sigma_l2=square, eps=EPS if sigma_l > 0.0 else math.inf, inv_rough2=None)
    if roughness_sigma is not None:
        out["inv_rough2"] = positive(roughness_sigma, "roughness_sigma")
    return out


@torch.no_grad()
def atrous(signal, points, normals, mask, groups: Optional[Sequence[int]] = None, iterations: int = ITERATIONS,
           plane_distance: Optional[float] = None, normal_power: int = NORMAL_POWER, sigma_l: float = SIGMA_L, roughness=None,
           roughness_sigma: float = ROUGHNESS_SIGMA) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """(filtered [C,H,W] float32, variance [G,H,W] float32, report): `iterations` steps (1 .. 5, step 2^i) of the a-trous filter
    of include/gigs_hip.h, "Denoising ray-traced planes", after one launch that estimates each group's variance in the 5 x 5
    window.
      signal      [C,H,W] float32 on a CUDA/HIP device, 1 <= C <= 16
      points, normals [H W,3] float32, mask [H W] uint8 or bool: the prepared arrays the tracers return, on signal's device
      groups      channel counts, each 1 or 3, summing to C: the channels of a group share one weight, computed from their
                  sum.  None: one group per channel
      plane_distance  a tap further than this from the centre's tangent plane weighs nothing.  None: PLANE_FRACTION of the
                  largest extent of the live pixels' bounding box (a device reduction and a read-back)
      normal_power  a power of two in [1, 128]: the exponent of the normals' cosine
      sigma_l     the signal weight reaches 0 at |y_q - y_p| = sigma_l sqrt(var_p); 0 turns it off
      roughness   [H W] float32 or None: a further guide (glossy planes), its weight 0 at a difference of roughness_sigma
    A pixel that is not live (masked, or a non-finite guide or signal value) keeps its bits and has variance 0.  The report
    (JSON-serialisable) carries the live count, the parameters and the launches."""
    what = "denoise.atrous"
    if not isinstance(signal, torch.Tensor) or not signal.is_cuda:
        raise RuntimeError("%s: signal must be a CUDA/HIP tensor: gigs-hip has no CPU path" % what)
    if signal.dim() != 3 or signal.dtype != torch.float32:
        raise ValueError("%s: signal is a [C,H,W] float32 tensor" % what)
    dev = signal.device
    Cn, H, W = (int(x) for x in signal.shape)
    if not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError("%s: 1 to %d channels a call, got %d" % (what, MAX_CHANNELS, Cn))
    N = H * W
    if N > 0x7FFFFFFF:
        raise ValueError("%s: at most 2^31 - 1 pixels" % what)

    def arr(t, name, shape, dtypes=(torch.float32,)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype not in dtypes or tuple(t.shape) != shape:
            raise ValueError("%s: %s must be a %s %s tensor on the signal's device" % (
                what, name, list(shape), " or ".join(str(d).replace("torch.", "") for d in dtypes)))
        return t.detach().contiguous()

    points, normals = arr(points, "points", (N, 3)), arr(normals, "normals", (N, 3))
    mask = arr(mask, "mask", (N,), (torch.uint8, torch.bool)).to(torch.uint8)
    rough = None if roughness is None else arr(roughness, "roughness", (N,))
    groups = [1] * Cn if groups is None else list(groups)
    if (not groups or any(isinstance(g, bool) or not isinstance(g, (int, np.integer)) or int(g) not in (1, 3) for g in groups)
            or sum(int(g) for g in groups) != Cn):
        raise ValueError("%s: groups are channel counts of 1 or 3 that sum to %d, got %r" % (what, Cn, groups))
    groups = [int(g) for g in groups]
    G = len(groups)
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError("%s: iterations lie in [1, %d], got %r" % (what, MAX_ITERATIONS, iterations))
    iterations = int(iterations)
    signal = signal.detach().contiguous()
    # refuse before any launch; a plane_distance of None is made from the packed guide below
    host_parameters(1.0 if plane_distance is None else plane_distance, normal_power, sigma_l, None if rough is None else roughness_sigma)
    filtered, variance = torch.empty_like(signal), torch.zeros((G, H, W), dtype=torch.float32, device=dev)
    report = dict(width=W, height=H, channels=Cn, groups=groups, iterations=iterations, steps=[1 << i for i in range(iterations)],
                  plane_distance=None if plane_distance is None else float(plane_distance), normal_power=int(normal_power),
                  sigma_l=float(sigma_l), roughness_sigma=None if rough is None else float(roughness_sigma), live=0, launches=[])
    if N == 0:
        return filtered, variance, report
    S = record_floats(Cn, G)
    sizes = (C.c_int * G)(*groups)
    guide = torch.empty((N, GUIDE_FLOATS), dtype=torch.float32, device=dev)
    a, b = (torch.empty((N, S), dtype=torch.float32, device=dev) for _ in range(2))
    with torch.cuda.device(dev):
        s = _stream()
        gigs_lib.check(_lib.gigs_denoise_pack(W, H, Cn, G, sizes, _p(signal), _p(points), _p(normals), _p(mask), _p(rough), _p(guide),
                                              _p(a), s), "denoise_pack")
        live = guide[:, GUIDE_FLOATS - 1] != 0
        report["live"] = int(live.sum())
        if plane_distance is None:
            plane_distance = 1.0  # no live point, or all in one place: nothing to weigh
            if report["live"] > 0:
                pts = guide[live, :3]
                extent = PLANE_FRACTION * float((pts.max(0).values - pts.min(0).values).max())
                plane_distance = extent if extent > 0.0 else 1.0
            report["plane_distance"] = plane_distance
        hp = host_parameters(plane_distance, normal_power, sigma_l, None if rough is None else roughness_sigma)
        use_rough, inv_rough2 = (0, 0.0) if rough is None else (1, hp["inv_rough2"])
        gigs_lib.check(_lib.gigs_denoise_variance(W, H, Cn, G, sizes, hp["e"], hp["inv_plane2"], use_rough, inv_rough2, _p(guide), _p(a),
                                                  _p(b), s), "denoise_variance")
        report["launches"] += ["pack", "variance"]
        a, b = b, a
        for step in report["steps"]:
            gigs_lib.check(_lib.gigs_denoise_atrous(W, H, Cn, G, sizes, step, hp["e"], hp["inv_plane2"], use_rough, inv_rough2,
                                                    hp["sigma_l2"], hp["eps"], _p(guide), _p(a), _p(b), s), "denoise_atrous")
            report["launches"].append("atrous:%d" % step)
            a, b = b, a
        gigs_lib.check(_lib.gigs_denoise_unpack(W, H, Cn, G, sizes, _p(a), _p(filtered), _p(variance), s), "denoise_unpack")
        report["launches"].append("unpack")
    return filtered, variance, report
