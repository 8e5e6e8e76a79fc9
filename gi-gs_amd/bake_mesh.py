"""Bakes ambient occlusion into a mesh PLY: mesh.bake_occlusion casts --rays cosine-distributed rays from every vertex and
stores the open share of its hemisphere (1 = open) as one more vertex property.

    python gi-gs_amd/bake_mesh.py IN.ply -o OUT.ply [--rays 256] [--distance D] [--bias B] [--seed S] [--rotations 16]
                                  [--light a.hdr [--bounces 1] [--sky_res 32] [--light_rays 256]]
    bake_mesh(args) -> {...}                                                                        (API)

Reads with scene_io.read_mesh_ply (an occlusion channel already in the file is replaced) and writes with
scene_io.save_mesh_ply(..., occlusion=...), so the colour makes one more trip through the PLY's 8 bits, as in clean_mesh.py.
Prints the report as JSON: mesh.bake_occlusion's (hits_total, no_normal, rays, rotations, seed, max_distance, bias and the
grid), the mean and a ten-bin histogram of the baked values, the sizes, the paths and the time.  --distance defaults to
0.1 of the longest axis of the mesh's grid and --bias to 1e-3 of the distance: conventions, not measurements.

--light a.hdr (or .npy [H,W,3]) bakes light as well: mesh.bake_light under that map's cube pooled to --sky_res texels an edge,
--light_rays rays per vertex traced without a distance limit, --bounces diffuse inter-reflections, with --bias, --seed and
--rotations as above.  The per-vertex irradiance goes into the PLY as irradiance_r / _g / _b after the occlusion, and the
report gains `light`: misses, front_hits, back_hits, no_normal, the mean irradiance of every pass and the time.  Without
--light the file and the report are what they were.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from argparse import Namespace
from typing import Dict, List, Optional

if __package__ in (None, ""):  # run as a script: make the package's modules importable
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Occlusion baking parameters")
    p.add_argument("input", type=str, help="a PLY written by extract_mesh.py, clean_mesh.py or simplify_mesh.py")
    p.add_argument("-o", "--output", type=str, required=True)
    p.add_argument("--rays", type=int, default=256, help="rays per vertex, a multiple of 64 in [64, 1024]")
    p.add_argument("--distance", type=float, default=None, help="how far an occluder counts")
    p.add_argument("--bias", type=float, default=None, help="the origin's offset along the normal")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--rotations", type=int, default=16, help="turns of the direction table about the normal, in [1, 64]")
    p.add_argument("--light", type=str, default=None, help="an environment map (.hdr or .npy) to bake light under")
    p.add_argument("--bounces", type=int, default=1, help="diffuse inter-reflections of the light bake")
    p.add_argument("--sky_res", type=int, default=32, help="texels an edge of the sky cube the light bake looks up")
    p.add_argument("--light_rays", type=int, default=256, help="rays per vertex of the light bake, a multiple of 64 in [64, 1024]")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def load_sky(path: str, res: int, dev):
    """The environment map at `path` (.hdr or .npy [H,W,3]) as the [6,res,res,3] sky of mesh.gather_light: the map's 256^2 cube
    (relight.latlong_to_cubemap, what a light's base holds), pooled by mesh.sky_cube."""
    import torch

    import image_writer
    import mesh
    import relight
    return mesh.sky_cube(relight.latlong_to_cubemap(torch.from_numpy(image_writer.load_latlong(path)).to(dev), [256, 256]), res)


def bake_mesh(args) -> Dict:
    """`args`: a Namespace from parse_args or an argv list."""
    import torch

    import mesh
    import mesh_render
    import scene_io
    if not isinstance(args, Namespace):
        args = parse_args(list(args))
    if not torch.cuda.is_available():
        raise RuntimeError("bake_mesh needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    m = mesh_render.device_mesh(args.input, dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    occlusion, report = mesh.bake_occlusion(m, rays=args.rays, max_distance=args.distance, bias=args.bias, seed=args.seed,
                                            rotations=args.rotations)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    irradiance, light = None, None
    if getattr(args, "light", None):
        irradiance, light = mesh.bake_light(m, load_sky(args.light, args.sky_res, dev), rays=args.light_rays, bounces=args.bounces, bias=args.bias, seed=args.seed,
                                            rotations=args.rotations)
        torch.cuda.synchronize()
        light = dict(light, map=args.light, light_s=round(time.perf_counter() - t1, 4))
    scene_io.save_mesh_ply(args.output, *m, occlusion=occlusion, irradiance=irradiance)
    V = int(occlusion.shape[0])
    hist = torch.histc(occlusion, bins=10, min=0.0, max=1.0).cpu().tolist() if V else [0.0] * 10
    return dict(report, input=args.input, path=args.output, vertices=V, faces=int(m.faces.shape[0]),
                mean=float(occlusion.double().mean().item()) if V else 1.0, histogram=[int(x) for x in hist],
                bake_s=round(t1 - t0, 4), **(dict(light=light) if light is not None else {}))


def main(argv=None) -> int:
    print(json.dumps(bake_mesh(parse_args(argv))))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
