"""How far two mesh PLYs are apart: mesh.distance samples both surfaces and finds, for every sample, the closest triangle
of the other mesh.

    python gi-gs_amd/compare_mesh.py A.ply B.ply [--samples N] [--seed S] [--tau T ...] [--max_distance D] [-o report.json]
    compare_mesh(args) -> {...}                                                                   (API)

Prints the report as JSON: per direction (a_to_b, b_to_a) n, far, mean, rms, median, max; chamfer (the mean of the two
means), hausdorff (the larger max); per --tau the precision (the share of A's samples within T of B), the recall (B's
within T of A) and their F-score; the faces skipped as unusable, both grids, and the two paths.  --max_distance caps the
search: a sample farther than D from the other mesh counts with D (and as `far`), and no sample walks the whole grid.
Reads with scene_io.read_mesh_ply, as clean_mesh.py and simplify_mesh.py do.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from argparse import Namespace
from typing import Dict, List, Optional

if __package__ in (None, ""):  # run as a script: make the package's modules importable
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Mesh comparison parameters")
    p.add_argument("a", type=str, help="a PLY written by extract_mesh.py, clean_mesh.py, simplify_mesh.py or bake_mesh.py (an occlusion channel is "
                                      "read and dropped)")
    p.add_argument("b", type=str, help="the PLY to compare it with")
    p.add_argument("--samples", type=int, default=100000, help="surface samples per mesh")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--tau", type=float, nargs="*", default=[], help="distance thresholds of the F-score")
    p.add_argument("--max_distance", type=float, default=None, help="cap the search and the distances at D")
    p.add_argument("-o", "--output", type=str, default=None, help="also write the report here")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def compare_mesh(args) -> Dict:
    """`args`: a Namespace from parse_args or an argv list."""
    import torch

    import mesh
    import mesh_render
    if not isinstance(args, Namespace):
        args = parse_args(list(args))
    if not torch.cuda.is_available():
        raise RuntimeError("compare_mesh needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    report = mesh.distance(mesh_render.device_mesh(args.a, dev), mesh_render.device_mesh(args.b, dev), samples=args.samples,
                           seed=args.seed, taus=args.tau, max_distance=args.max_distance)
    report = dict(report, a=args.a, b=args.b)
    if args.output:
        with open(args.output, "w") as f:
            json.dump(report, f)
    return report


def main(argv=None) -> int:
    print(json.dumps(compare_mesh(parse_args(argv))))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
