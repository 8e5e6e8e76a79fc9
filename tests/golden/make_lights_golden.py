"""Generates tests/golden/lights_bsdf.npz (run where the reference is checked out; the reference never travels).

REFERENCE-PINNED values of the analytic BSDF: the reference's own pbr/renderutils/bsdf.py `bsdf_pbr` (pure torch, CPU)
evaluated in FLOAT64 on seeded float32 inputs -- 2048 points x 4 lights, normals over the whole sphere, roughness at 0, at 1
and below min_roughness, metallic over [0, 1], grazing and back-facing lights -- as gigs_shade_lights defines its call:
kd = albedo, arm = (0, roughness, metallic), light_pos = p + wi, min_roughness = 0.08, BSDF = 0.  The same call in FLOAT32
gives ref32_err, the largest error of a float32 evaluation of these formulas against float64, relative to
max(|want|, 1e-3): the GPU test allows the kernel 4 x that.  Only inputs and outputs are stored.

    python tests/golden/make_lights_golden.py <the reference's root>
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
N, FLOOR, BAND, BAND_CAP, EPS = 2048, 1e-3, 1e-5, 0.01, 1e-4

# [kind, x, y, z, extent, 0, 0, 0]: two point lights outside the points' cube, two directional ones (unit travel directions)
LIGHT_ROWS = np.array([[0, 0.5, 0.3, 2.5, 0, 0, 0, 0], [0, -2.0, 1.0, 0.5, 0, 0, 0, 0],
                       [1, 0.0, 0.0, -1.0, 0, 0, 0, 0], [1, 0.6, -0.48, 0.64, 0, 0, 0, 0]], np.float32)
CAMPOS = np.array([0.3, -0.2, 3.5], np.float32)


def incident(points, rows, dtype):
    """wi [N,L,3] of the header's "Shading under analytic lights", 3, in `dtype` -> torch."""
    p, r = torch.from_numpy(points).to(dtype), torch.from_numpy(rows).to(dtype)
    out = []
    for l in range(len(rows)):
        if float(r[l, 0]) == 0:
            v = r[l, 1:4][None, :] - p
            out.append(v / torch.sqrt((v * v).sum(-1, keepdim=True)))
        else:
            out.append((-r[l, 1:4])[None, :].expand(len(p), 3))
    return torch.stack(out, 1)


def excluded(points, normals, rows, campos):
    """[N,L] bool: the pairs the frontfacing step makes ill-conditioned -- float64 n.wo or n.wi within BAND of
    specular_epsilon, or |n.wi| < BAND."""
    p, n = torch.from_numpy(points).double(), torch.from_numpy(normals).double()
    wo = torch.nn.functional.normalize(torch.from_numpy(campos).double()[None, :] - p, dim=-1)
    wi = incident(points, rows, torch.float64)
    n_wo = (n * wo).sum(-1)[:, None]
    n_wi = (n[:, None, :] * wi).sum(-1)
    return (((n_wo - EPS).abs() < BAND) | ((n_wi - EPS).abs() < BAND) | (n_wi.abs() < BAND)).numpy()


def inputs():
    rng = np.random.default_rng(20251)
    points = rng.uniform(-1, 1, size=(N, 3)).astype(np.float32)
    nrm = rng.normal(size=(N, 3))
    # a quarter of the normals graze one of the lights: n = the unit vector across wi, tilted by a sine in +-[1e-3, 0.05]
    wi = incident(points, LIGHT_ROWS, torch.float64).numpy()
    k = np.arange(N // 4)
    w = wi[k, k % 4]
    across = np.cross(w, rng.normal(size=(len(k), 3)))
    across /= np.linalg.norm(across, axis=1, keepdims=True)
    tilt = rng.uniform(1e-3, 0.05, size=len(k)) * rng.choice([-1.0, 1.0], size=len(k))
    nrm[k] = across * np.sqrt(1 - tilt ** 2)[:, None] + w * tilt[:, None]
    normals = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    roughness = rng.uniform(0, 1, size=N).astype(np.float32)
    roughness[0::16] = 0.0
    roughness[1::16] = 1.0
    roughness[2::16] = rng.uniform(0.0, 0.08, size=len(roughness[2::16])).astype(np.float32)
    metallic = rng.uniform(0, 1, size=N).astype(np.float32)
    metallic[3::32], metallic[4::32] = 0.0, 1.0
    albedo = rng.uniform(0.02, 1, size=(N, 3)).astype(np.float32)
    return points, normals, albedo, roughness, metallic


def evaluate(bsdf_pbr, points, normals, albedo, roughness, metallic, dtype):
    """bsdf_pbr per light -> [N,L,3] in `dtype`."""
    t = lambda x: torch.from_numpy(x).to(dtype)  # noqa: E731
    p, n, kd = t(points), t(normals), t(albedo)
    arm = torch.stack([torch.zeros(N, dtype=dtype), t(roughness), t(metallic)], -1)
    wi = incident(points, LIGHT_ROWS, dtype)
    view = t(CAMPOS)[None, :].expand(N, 3)
    return torch.stack([bsdf_pbr(kd, arm, p, n, view, p + wi[:, l], 0.08, 0) for l in range(LIGHT_ROWS.shape[0])], 1)


def main(reference):
    import importlib.util
    # the module alone, by its path: the package around it imports what the BSDF does not need
    spec = importlib.util.spec_from_file_location("reference_bsdf", os.path.join(reference, "pbr", "renderutils", "bsdf.py"))
    bsdf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bsdf)
    bsdf_pbr = bsdf.bsdf_pbr

    points, normals, albedo, roughness, metallic = inputs()
    want = evaluate(bsdf_pbr, points, normals, albedo, roughness, metallic, torch.float64).numpy()
    got32 = evaluate(bsdf_pbr, points, normals, albedo, roughness, metallic, torch.float32).numpy().astype(np.float64)
    out = excluded(points, normals, LIGHT_ROWS, CAMPOS)
    share = float(out.mean())
    assert share <= BAND_CAP, "the band leaves out %.3f of the pairs" % share
    err = np.abs(got32 - want) / np.maximum(np.abs(want), FLOOR)
    ref32_err = float(err[~out].max())
    assert np.isfinite(want).all() and (want >= 0).all() and (want[~out] > 0).any()
    np.savez_compressed(os.path.join(HERE, "lights_bsdf.npz"), points=points, normals=normals, albedo=albedo, roughness=roughness,
                        metallic=metallic, campos=CAMPOS, light_rows=LIGHT_ROWS, want=want, ref32_err=np.float64(ref32_err),
                        floor=np.float64(FLOOR), band=np.float64(BAND), band_cap=np.float64(BAND_CAP))
    lit = (want > 0).any(-1)
    print("wrote lights_bsdf.npz: %d points x %d lights, %d pairs in the band (%.4f), %d pairs lit, largest f %.4g, ref32_err %.4g" % (
        N, LIGHT_ROWS.shape[0], int(out.sum()), share, int(lit.sum()), float(want.max()), ref32_err))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ["GIGS_REFERENCE"])
