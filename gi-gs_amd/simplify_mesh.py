"""A mesh PLY already on disk (extract_mesh.py's) with fewer faces: mesh.simplify puts one vertex into every occupied cell
of a uniform grid, placed by the plane quadrics of the faces that touch the cell, and drops the faces that collapse.

    python gi-gs_amd/simplify_mesh.py IN.ply -o OUT.ply (--cell X | --cell_edges R) [--keep_largest K] [--min_faces M]
                                      [--distance N]                                              (CLI)
    simplify_mesh(args) -> {...}                                                                  (API)

--cell is the cell size in world units; --cell_edges R makes it R times the median edge length of the valid faces
(mesh.median_edge, computed on the device), so R is roughly the factor by which edges grow.  The grid starts at the
minimum of the vertices.  --keep_largest / --min_faces run mesh.clean AFTER the simplification (clustering can join what
were separate components, and cleaning first would spend the labelling on faces that go anyway).  Reads with
scene_io.read_mesh_ply and writes with scene_io.save_mesh_ply, as clean_mesh.py does.  Prints the report as JSON:
mesh.simplify's, the clean's if it ran, and the times.  --distance N adds `distance`: mesh.distance of the input against
the output with N surface samples each (Chamfer, Hausdorff, one-sided means); the PLY written is the same with and without.
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
    p = argparse.ArgumentParser(description="Mesh simplification parameters")
    p.add_argument("input", type=str, help="a PLY written by extract_mesh.py (an occlusion channel of bake_mesh.py is read and dropped)")
    p.add_argument("-o", "--output", type=str, required=True)
    size = p.add_mutually_exclusive_group(required=True)
    size.add_argument("--cell", type=float, default=None, help="cell size in world units")
    size.add_argument("--cell_edges", type=float, default=None, help="cell size in median edge lengths")
    p.add_argument("--keep_largest", type=int, default=0, help="afterwards keep the components with at least as many faces as the K-th largest")
    p.add_argument("--min_faces", type=int, default=0, help="afterwards drop the components with fewer faces")
    p.add_argument("--distance", type=int, default=0, help="report mesh.distance of the input against the output, N samples each")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def simplify_mesh(args) -> Dict:
    """`args`: a Namespace from parse_args or an argv list."""
    import torch

    import mesh
    import mesh_render
    import scene_io
    if not isinstance(args, Namespace):
        args = parse_args(list(args))
    if not torch.cuda.is_available():
        raise RuntimeError("simplify_mesh needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    m = mesh_render.device_mesh(args.input, dev)
    extra = {}
    cell = args.cell
    if cell is None:
        edge = mesh.median_edge(m)
        if not edge > 0:
            raise ValueError("simplify_mesh: --cell_edges needs a valid face with a positive edge length")
        cell, extra["median_edge"] = args.cell_edges * edge, edge
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out, report = mesh.simplify(m, cell)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    extra["simplify_s"] = round(t1 - t0, 4)
    if args.keep_largest > 0 or args.min_faces > 0:
        out, cleaned = mesh.clean(out, args.keep_largest, args.min_faces)
        torch.cuda.synchronize()
        extra.update(components=cleaned["components"], components_kept=cleaned["components_kept"],
                     faces_removed=cleaned["faces_removed"], clean_s=round(time.perf_counter() - t1, 4))
        report = dict(report, vertices=int(out.vertices.shape[0]), faces=int(out.faces.shape[0]))
    if args.distance > 0:  # a: the input, b: what is written
        extra["distance"] = mesh.distance(m, out, samples=args.distance)
    scene_io.save_mesh_ply(args.output, *out)
    return dict(report, path=args.output, **extra)


def main(argv=None) -> int:
    print(json.dumps(simplify_mesh(parse_args(argv))))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
