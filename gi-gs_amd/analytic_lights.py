"""Analytic lights: point and directional lamps over any G-buffer, with ray-traced shadows against a mesh.

    lights = load_lights("lights.json")                     # or parse_lights([...])
    vis, lit, report = mesh.shadow_points(points, normals, mesh, lights, samples=16)
    diffuse, specular = shade_lights(points, normals, albedo, roughness, metallic, campos, lights, visibility=vis)
    relighter = AnalyticRelighter(lights, MeshGBuffer(gi), tracer=RaytracedLight(mesh))

A lights file is a JSON list of objects:

    {"kind": "point",       "position":  [x, y, z], "color": [r, g, b], "intensity": I, "radius": r}
    {"kind": "directional", "direction": [x, y, z], "color": [r, g, b], "intensity": I, "angle": degrees}

`direction` is the direction the light TRAVELS in (a sun overhead: [0, 0, -1]); it is normalised here in float64.  `color`
defaults to white, `intensity` to 1; `radius` (the sphere a point light's shadow samples lie on) and `angle` (the half-angle
of a directional light's cone of shadow samples, below 90 degrees) default to 0, the hard shadow.  The radiance of a light is
color x intensity: a point light delivers it divided by the squared distance, a directional light as it is.  The extent
only softens the shadow: the shade evaluates every light at its centre.

The device halves are csrc/mesh_shadow.hip and csrc/shade_lights.hip; include/gigs_hip.h, "Shadows of analytic lights" and
"Shading under analytic lights", states the packed row and every expression."""
from __future__ import annotations

import json
import math
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

import gigs_lib
import mesh as mesh_ops
from pipeline import linear_to_srgb

MAX_LIGHTS = 16  # GIGS_MAX_LIGHTS
LIGHT_ROW = 8    # GIGS_LIGHT_ROW
KINDS = ("point", "directional")
_FIELDS = {"point": ("kind", "position", "color", "intensity", "radius"),
           "directional": ("kind", "direction", "color", "intensity", "angle")}


class AnalyticLight(NamedTuple):
    kind: str                            # "point" or "directional"
    vector: Tuple[float, float, float]   # point: the position; directional: the unit direction the light travels in
    color: Tuple[float, float, float]
    intensity: float
    extent: float                        # point: the radius; directional: the half-angle in degrees


def _vec3(entry, field: str, i: int, default=None):
    x = entry.get(field, default)
    if (not isinstance(x, (list, tuple)) or len(x) != 3
            or not all(isinstance(c, (int, float)) and not isinstance(c, bool) and math.isfinite(c) for c in x)):
        raise ValueError("lights[%d]: %s must be three finite numbers, got %r" % (i, field, x))
    return tuple(float(c) for c in x)


def _number(entry, field: str, i: int, default: float, hi: float = math.inf):
    x = entry.get(field, default)
    if not isinstance(x, (int, float)) or isinstance(x, bool) or not (0 <= x < hi) or not math.isfinite(x):
        raise ValueError("lights[%d]: %s must be a finite number in [0, %g), got %r" % (i, field, hi, x))
    return float(x)


def parse_lights(entries) -> Tuple[AnalyticLight, ...]:
    """The lights of a decoded JSON list (see the module's text) -> a tuple of AnalyticLight.  A malformed entry raises a
    ValueError that names its index and field."""
    if not isinstance(entries, (list, tuple)) or not 1 <= len(entries) <= MAX_LIGHTS:
        raise ValueError("lights: a list of 1 to %d lights is needed, got %s" % (
            MAX_LIGHTS, "%d" % len(entries) if isinstance(entries, (list, tuple)) else type(entries).__name__))
    out = []
    for i, e in enumerate(entries):
        if isinstance(e, AnalyticLight):  # checked as its entry and kept as it is: parsing twice changes no bit
            parse_lights([light_entry(e)])
            out.append(e)
            continue
        if not isinstance(e, dict):
            raise ValueError("lights[%d]: an object is needed, got %s" % (i, type(e).__name__))
        kind = e.get("kind")
        if kind not in KINDS:
            raise ValueError("lights[%d]: kind must be one of %s, got %r" % (i, ", ".join(KINDS), kind))
        unknown = sorted(set(e) - set(_FIELDS[kind]))
        if unknown:
            raise ValueError("lights[%d]: a %s light has no field %s" % (i, kind, ", ".join(unknown)))
        color = _vec3(e, "color", i, [1.0, 1.0, 1.0])
        if min(color) < 0:
            raise ValueError("lights[%d]: color must not be negative, got %r" % (i, list(color)))
        intensity = _number(e, "intensity", i, 1.0)
        if kind == "point":
            vector, extent = _vec3(e, "position", i), _number(e, "radius", i, 0.0)
        else:
            d = np.asarray(_vec3(e, "direction", i), np.float64)
            length = float(np.sqrt((d * d).sum()))
            if not length > 0:
                raise ValueError("lights[%d]: direction must not be zero" % i)
            vector, extent = tuple(float(c) for c in d / length), _number(e, "angle", i, 0.0, 90.0)
        out.append(AnalyticLight(kind, vector, color, intensity, extent))
    return tuple(out)


def load_lights(path: str) -> Tuple[AnalyticLight, ...]:
    with open(path) as fh:
        try:
            entries = json.load(fh)
        except json.JSONDecodeError as err:
            raise ValueError("lights: %s is not JSON: %s" % (path, err))
    return parse_lights(entries)


def light_entry(light: AnalyticLight) -> Dict:
    """The JSON object parse_lights reads `light` back from."""
    where, extent = ("position", "radius") if light.kind == "point" else ("direction", "angle")
    return {"kind": light.kind, where: list(light.vector), "color": list(light.color), "intensity": light.intensity,
            extent: light.extent}


def pack(lights: Sequence[AnalyticLight]) -> Tuple[np.ndarray, np.ndarray]:
    """(rows [L,8] float32, radiance [L,3] float32): the device's light rows (include/gigs_hip.h, "Shadows of analytic
    lights", 1) -- kind, the position or the direction normalised in float64, the radius or tan(angle) -- and
    color x intensity."""
    lights = parse_lights(list(lights))
    rows = np.zeros((len(lights), LIGHT_ROW), np.float32)
    radiance = np.zeros((len(lights), 3), np.float32)
    for i, light in enumerate(lights):
        v = np.asarray(light.vector, np.float64)
        if light.kind == "directional":
            v = v / np.sqrt((v * v).sum())
        rows[i, 0] = KINDS.index(light.kind)
        rows[i, 1:4] = v
        rows[i, 4] = light.extent if light.kind == "point" else math.tan(math.radians(light.extent))
        radiance[i] = np.asarray(light.color, np.float64) * light.intensity
    if not (np.isfinite(rows).all() and np.isfinite(radiance).all()):
        raise ValueError("lights: a packed value leaves the float32 range")
    return rows, radiance


def light_rows(lights, what: str = "lights") -> np.ndarray:
    """[L,8] float32 rows from a sequence of AnalyticLight (pack) or from rows packed before, checked: 1 <= L <= 16, every
    entry finite, kind 0 or 1, extent >= 0."""
    if isinstance(lights, torch.Tensor):
        lights = lights.detach().cpu().numpy()
    if isinstance(lights, np.ndarray):
        rows = np.ascontiguousarray(lights, np.float32)
        if rows.ndim != 2 or rows.shape[1] != LIGHT_ROW or not 1 <= rows.shape[0] <= MAX_LIGHTS:
            raise ValueError("%s: light rows must be [L,%d] with 1 <= L <= %d, got %s" % (what, LIGHT_ROW, MAX_LIGHTS, rows.shape,))
        if not (np.isfinite(rows).all() and np.isin(rows[:, 0], (0.0, 1.0)).all() and (rows[:, 4] >= 0).all()):
            raise ValueError("%s: light rows must be finite with kind 0 or 1 and an extent >= 0" % what)
        return rows
    return pack(lights)[0]


def _uniform(seed: int, i, k: int):
    """u(i, k) in [0, 1): mix64((seed 2^32 + i) 4 + k) >> 11, times 2^-53, the project's counter hash."""
    with np.errstate(over="ignore"):
        x = ((np.uint64(seed) << np.uint64(32)) + np.asarray(i, np.uint64)) * np.uint64(4) + np.uint64(k)
    return (mesh_ops._mix64(x) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


OFFSET_SEED = 0x5AD0


def ball_offsets(samples: int = 1, rotations: int = 16) -> np.ndarray:
    """[rotations, samples, 3] float32: points of the unit ball, a pure function of the two arguments.  samples == 1 gives
    zeros: the one sample is the light's centre.  Otherwise point (k, s) has the hash-uniform direction z = 1 - 2 u0,
    azimuth 2 pi u1 and the radius u2^(1/3) of a uniform ball, u = the counter hash of k samples + s, scaled by 1 - 2^-20 so
    that the float32 rounding leaves every norm <= 1."""
    S, K = int(samples), int(rotations)
    if S < 1 or S > mesh_ops.SHADOW_MAX_SAMPLES or K < 1 or K > mesh_ops.SHADOW_MAX_ROTATIONS:
        raise ValueError("ball_offsets: samples in [1, %d] and rotations in [1, %d] are needed, got %d and %d" % (
            mesh_ops.SHADOW_MAX_SAMPLES, mesh_ops.SHADOW_MAX_ROTATIONS, S, K))
    if S == 1:
        return np.zeros((K, 1, 3), np.float32)
    i = np.arange(K * S, dtype=np.uint64)
    z = 1.0 - 2.0 * _uniform(OFFSET_SEED, i, 0)
    phi = 2.0 * np.pi * _uniform(OFFSET_SEED, i, 1)
    r = np.cbrt(_uniform(OFFSET_SEED, i, 2)) * (1.0 - 2.0 ** -20)
    s = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    return (r[:, None] * np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)).astype(np.float32).reshape(K, S, 3)


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _array(x, dev, shape, what: str, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != shape:
        raise ValueError("%s: %s must be a %s float32 tensor" % (what, name, list(shape)))
    if x.device != dev:
        raise RuntimeError("%s: %s must live on the points' device: gigs-hip has no CPU path" % (what, name))
    return x.detach().contiguous()


@torch.no_grad()
def shade_lights(points, normals, albedo, roughness, metallic, campos, lights, visibility=None, mask=None):
    """(diffuse [N,3], specular [N,3]) float32, linear radiance: the points under the analytic `lights` (a sequence of
    AnalyticLight), Lambert plus GGX (gigs_shade_lights; include/gigs_hip.h, "Shading under analytic lights").  points,
    normals, albedo [N,3], roughness [N], metallic [N] or None (0), campos [3]: float32 tensors on one CUDA/HIP device;
    visibility [N,L] float32 (mesh.shadow_points') or None (1); mask [N] uint8 or bool or None.  A masked point and one with
    no unit normal get zeros."""
    what = "shade_lights"
    rows, radiance = pack(lights)
    L = int(rows.shape[0])
    if not isinstance(points, torch.Tensor) or not points.is_cuda:
        raise RuntimeError("%s: points must be a CUDA/HIP tensor: gigs-hip has no CPU path" % what)
    dev = points.device
    if points.dim() != 2:
        raise ValueError("%s: points must be [N,3]" % what)
    N = int(points.shape[0])
    points = _array(points, dev, (N, 3), what, "points")
    normals = _array(normals, dev, (N, 3), what, "normals")
    albedo = _array(albedo, dev, (N, 3), what, "albedo")
    roughness = _array(roughness, dev, (N,), what, "roughness")
    metallic = None if metallic is None else _array(metallic, dev, (N,), what, "metallic")
    campos = _array(torch.as_tensor(campos, dtype=torch.float32).to(dev), dev, (3,), what, "campos")
    visibility = None if visibility is None else _array(visibility, dev, (N, L), what, "visibility")
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.uint8, torch.bool)
                or tuple(mask.shape) != (N,)):
            raise ValueError("%s: mask must be a [%d] uint8 or bool tensor on the points' device" % (what, N))
        mask = mask.detach().to(torch.uint8).contiguous()
    diffuse = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    specular = torch.zeros((N, 3), dtype=torch.float32, device=dev)
    if N == 0:
        return diffuse, specular
    with torch.cuda.device(dev):
        d_rows, d_radiance = torch.from_numpy(rows).to(dev), torch.from_numpy(radiance).to(dev)
        gigs_lib.check(gigs_lib.lib().gigs_shade_lights(
            N, _p(points), _p(normals), _p(mask), _p(albedo), _p(roughness), _p(metallic), _p(campos), L, _p(d_rows),
            _p(d_radiance), _p(visibility), _p(diffuse), _p(specular), torch.cuda.current_stream().cuda_stream), "shade_lights")
    return diffuse, specular


class AnalyticRelighter:
    """A view of any G-buffer source (relight.SplatGBuffer, mesh_render.MeshGBuffer, mesh_render.RaytracedGBuffer) under
    analytic lights: relighter(cam, scene) takes the source's depth_pos, normals_view, mask_u8, albedo_map, roughness_map
    (and metallic_map when the source is metallic), prepares world points with the tracer's transform, traces the shadows
    against `tracer` (a mesh_render.RaytracedLight; None: no shadows, visibility 1) and shades.  -> {lights_diffuse,
    lights_specular [3,H,W] linear, lights_rgb [3,H,W] = clamp(diffuse + specular, 0, 1), through linear_to_srgb when `gamma`,
    shadow [L,H,W], report}; an uncovered pixel is 0 in the three images and 1 in shadow.  A traced view replays no
    hipGraph.  denoise=n > 0 filters each light's visibility plane with n a-trous iterations (denoise.atrous, one channel per
    light, the tracer's plane_distance()) before the shade; report["denoise"] lists the filter's reports.  0 changes no bit."""
    replayable = False

    def __init__(self, lights, source, tracer=None, samples: int = 1, gamma: bool = True, denoise: int = 0):
        import mesh_render
        self.lights = parse_lights(list(lights))
        self.source, self.tracer, self.samples, self.gamma = source, tracer, int(samples), bool(gamma)
        if tracer is not None and not isinstance(tracer, mesh_render.RaytracedLight):
            raise TypeError("AnalyticRelighter: the tracer is a mesh_render.RaytracedLight or None")
        if not 1 <= self.samples <= mesh_ops.SHADOW_MAX_SAMPLES:
            raise ValueError("AnalyticRelighter: samples must lie in [1, %d], got %d" % (mesh_ops.SHADOW_MAX_SAMPLES, self.samples))
        self.denoise = mesh_render.denoise_iterations("AnalyticRelighter", denoise)
        if self.denoise and tracer is None:
            raise ValueError("AnalyticRelighter: denoise filters traced shadows: it needs a tracer")
        self.report = None

    @torch.no_grad()
    def __call__(self, cam: Dict, scene) -> Dict:
        import denoise as denoise_ops
        import mesh_render
        b = self.source(cam, scene)
        pos, mask = b["depth_pos"], b["mask_u8"]
        _, H, W = pos.shape
        L = len(self.lights)
        if self.tracer is not None:
            visibility, points, normals, m, report = self.tracer.shadows(pos, b["normals_view"], cam["viewmatrix"], mask, self.lights,
                                                                         self.samples, normal_space="view")
            report = dict(report, shadows=True)
            if self.denoise:  # one channel per light, each with its own weight; at most MAX_CHANNELS lights a call
                reports = []
                for l0 in range(0, L, denoise_ops.MAX_CHANNELS):
                    chunk = visibility[l0:l0 + denoise_ops.MAX_CHANNELS]
                    chunk, _, rep = denoise_ops.atrous(chunk, points, normals, m, None, self.denoise,
                                                       plane_distance=self.tracer.plane_distance())
                    visibility[l0:l0 + denoise_ops.MAX_CHANNELS] = chunk
                    reports.append(rep)
                report["denoise"] = reports
            flat = visibility.reshape(L, H * W).t().contiguous()
        else:
            points, normals, m = mesh_render.prepare_points(pos, b["normals_view"], cam["viewmatrix"], mask, "view", pos.device)
            flat, visibility = None, torch.ones((L, H, W), dtype=torch.float32, device=pos.device)
            report = dict(n=H * W, lights=L, shadows=False)
        metallic = b["metallic_map"].reshape(H * W) if getattr(self.source, "metallic", False) else None
        campos = torch.as_tensor(cam["campos"], dtype=torch.float32).to(points.device).reshape(3)
        diffuse, specular = shade_lights(points, normals, b["albedo_map"].reshape(3, H * W).t().contiguous(),
                                         b["roughness_map"].reshape(H * W).contiguous(),
                                         None if metallic is None else metallic.contiguous(), campos, self.lights, flat, m)
        plane3 = lambda x: x.t().reshape(3, H, W).contiguous()  # noqa: E731
        rgb = (plane3(diffuse) + plane3(specular)).clamp_(0.0, 1.0)
        if self.gamma:
            rgb = linear_to_srgb(rgb)
        self.report = report
        return dict(lights_diffuse=plane3(diffuse), lights_specular=plane3(specular), lights_rgb=rgb, shadow=visibility,
                    points=points, normals=normals, mask=m, report=report)
