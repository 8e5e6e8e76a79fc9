"""A trained scene on disk as a triangle mesh with its recovered materials (mesh.py): the views of a split are rendered,
their depth and material planes fused into a truncated signed distance volume, and the zero level set written as a PLY
(scene_io.save_mesh_ply: position, world normal, albedo as colour, roughness, metallic per vertex).

    python gi-gs_amd/extract_mesh.py -m <out> --checkpoint <out>/chkpntN.pth [--grid 256] [--bounds x0 y0 z0 x1 y1 z1]
                                     [--trunc_voxels 4] [--min_weight 2] [--opacity_min 0.5] [--no_carve]
                                     [--split train] [--keep_largest K] [--min_faces M] [--simplify R]
                                     [--bake_occlusion RAYS] [--ao_distance D] [--texture B]
                                     [--bake_light a.hdr [--bounces 1] [--sky_res 32] [--light_rays 256]]
                                     -o mesh.ply                                                           (CLI)
    extract_mesh(args) -> {...}                                                                            (API)

The scene path, the SH degree and the resolution come from <out>/cfg_args as in render_scene.py, command-line values
first.  --grid is the number of samples along the longest axis of the box; without --bounds the box is
mesh.auto_bounds of the Gaussians.  A relative -o lands in <out>.  Prints the counts of views, samples, vertices and
faces and the time of each phase.  --keep_largest K and --min_faces M (both 0: the raw level set, as before) run
mesh.clean on the extracted mesh: the connected components of fewer faces than max(M, the K-th largest, 1) are dropped,
and the result gains components, components_kept, faces_removed and clean_s.  --simplify R (0: off, as before) then runs
mesh.simplify with cells of R voxels that start at the volume's corner, so that a cell holds R^3 voxels of the fusion
grid: the face count falls by about R^2 while the volume keeps its resolution.  The result gains clusters,
faces_collapsed, faces_duplicate and simplify_s.  --bake_occlusion RAYS (0: off, as before, byte for byte) runs
mesh.bake_occlusion with RAYS rays per vertex (a multiple of 64) on the mesh that is written -- after cleaning and
simplifying -- and the PLY gains `property float occlusion` (1 = open); --ao_distance D is its max_distance (default: 0.1 of
the longest axis of the mesh's grid).  The result gains occlusion (the bake's report) and bake_s.  --texture B (0: off, as
before, byte for byte; needs --simplify R and an -o that ends in .obj) writes the simplified mesh as OBJ + MTL + PNG instead
of a PLY: mesh.bake_atlas stores the materials of the level set BEFORE the simplification in an atlas of charts of B texels
over the simplified mesh (texture_mesh.py's files), and --bake_occlusion then bakes that unsimplified mesh, whose occlusion
becomes the first channel of the ORM image.  The result gains texture (the atlas's report), files and texture_s.
--bake_light a.hdr (or .npy; off by default, and then every byte is what it was) runs mesh.bake_light under that map with
--bounces, --sky_res and --light_rays as bake_mesh.py --light does (bias, seed and rotations are the bake's defaults here:
this tool has no flags for them), on the mesh the occlusion is baked on: the PLY gains irradiance_r / _g / _b, or, with --texture, the
atlas gains a light-map written as <name>_lightmap.hdr.  The result gains light (the bake's report) and light_s.
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
    import render_scene
    p = argparse.ArgumentParser(description="Mesh extraction parameters")
    render_scene.add_model_arguments(p)
    p.add_argument("--checkpoint", type=str, default=None, help="The path to the checkpoint to load.")
    for k, v in render_scene.GI_FLAGS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    p.add_argument("--grid", type=int, default=256, help="samples along the longest axis of the box")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    p.add_argument("--trunc_voxels", type=float, default=4.0, help="truncation distance in voxels")
    p.add_argument("--min_weight", type=float, default=2.0, help="views a sample needs to take part in the mesh")
    p.add_argument("--opacity_min", type=float, default=0.5, help="pixels below this opacity are background")
    p.add_argument("--no_carve", action="store_true", help="background pixels leave their samples alone")
    p.add_argument("--split", choices=("train", "test"), default="train")
    p.add_argument("--keep_largest", type=int, default=0, help="keep the components with at least as many faces as the K-th largest")
    p.add_argument("--min_faces", type=int, default=0, help="drop the components with fewer faces")
    p.add_argument("--simplify", type=float, default=0.0, help="cluster the vertices in cells of this many voxels (0: off)")
    p.add_argument("--bake_occlusion", type=int, default=0, help="rays per vertex of the occlusion bake, a multiple of 64 (0: off)")
    p.add_argument("--ao_distance", type=float, default=None, help="how far an occluder counts (default: 0.1 of the longest axis)")
    p.add_argument("--texture", type=int, default=0, help="texels along a chart of the texture atlas; needs --simplify and a .obj output (0: off)")
    p.add_argument("--bake_light", type=str, default=None, help="an environment map (.hdr or .npy) to bake light under (default: off)")
    p.add_argument("--bounces", type=int, default=1, help="diffuse inter-reflections of the light bake")
    p.add_argument("--sky_res", type=int, default=32, help="texels an edge of the sky cube the light bake looks up")
    p.add_argument("--light_rays", type=int, default=256, help="rays per vertex of the light bake, a multiple of 64 in [64, 1024]")
    p.add_argument("-o", "--output", type=str, default="mesh.ply")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def extract_mesh(args) -> Dict:
    """`args`: a Namespace from parse_args, a dict of overrides or an argv list."""
    import torch

    import dataset_readers as dr
    import mesh
    import pipeline
    import render_scene
    import scene_io
    args = render_scene.combine_args(render_scene.as_namespace(args, parse_args))
    if not torch.cuda.is_available():
        raise RuntimeError("extract_mesh needs the GPU")
    if args.texture != 0 and not (args.texture >= 3 and args.simplify > 0 and args.output.endswith(".obj")):
        raise ValueError("extract_mesh: --texture B needs B >= 3, --simplify R and an output that ends in .obj")
    dev = torch.device("cuda", torch.cuda.current_device())
    args.source_path = os.path.abspath(args.source_path)
    sync = torch.cuda.synchronize
    t0 = time.perf_counter()
    g, sh_degree, _, cams = render_scene.load_trained(args, dev)
    infos = cams[args.split]
    if not infos:
        raise ValueError("extract_mesh: the %s split has no views" % args.split)
    t1 = time.perf_counter()
    try:
        if args.bounds is not None:
            lo, hi = args.bounds[:3], args.bounds[3:]
        else:
            lo, hi = mesh.auto_bounds(g)
        voxel, dims = mesh.grid_for_bounds(lo, hi, args.grid)
        vol = mesh.TSDFVolume(lo, voxel, dims, args.trunc_voxels * voxel, opacity_min=args.opacity_min,
                              carve=not args.no_carve, device=dev)
        gi = {k: getattr(args, k) for k in render_scene.GI_FLAGS}
        views = [dr.camera_from_info(ci, args.resolution, device=dev) for ci in infos]
        sync()
        t2 = time.perf_counter()
        mesh.fuse_views(g, sh_degree, views, gi, vol)
        sync()
        t3 = time.perf_counter()
        m = vol.extract(args.min_weight)
        sync()
        t4 = time.perf_counter()
        report = None
        if args.keep_largest > 0 or args.min_faces > 0:
            m, report = mesh.clean(m, args.keep_largest, args.min_faces)
            sync()
        t4c = time.perf_counter()
        simplified = None
        level_set = m  # what --texture reads the materials from
        if args.simplify > 0:
            m, simplified = mesh.simplify(m, args.simplify * voxel, origin=vol.lo)
            sync()
        t4s = time.perf_counter()
        occlusion = baked = None
        if args.bake_occlusion > 0:
            occlusion, baked = mesh.bake_occlusion(level_set if args.texture else m, rays=args.bake_occlusion,
                                                   max_distance=args.ao_distance)
            sync()
        t4b = time.perf_counter()
        irradiance = lit = None
        if getattr(args, "bake_light", None):
            import bake_mesh
            irradiance, lit = mesh.bake_light(level_set if args.texture else m, bake_mesh.load_sky(args.bake_light, args.sky_res, dev),
                                              rays=args.light_rays, bounces=args.bounces)
            lit["map"] = args.bake_light
            sync()
        t4l = time.perf_counter()
        path = args.output if os.path.isabs(args.output) else os.path.join(args.model_path, args.output)
        textured = files = None
        if args.texture:
            import texture_mesh
            atlas, textured = mesh.bake_atlas(m, level_set, block=args.texture, occlusion=occlusion, extra=irradiance)
            sync()
            t4t = time.perf_counter()
            files = texture_mesh.save_textured_mesh(path, m, atlas, lightmap=irradiance is not None)
        else:
            t4t = t4l
            scene_io.save_mesh_ply(path, *m, occlusion=occlusion, irradiance=irradiance)
        t5 = time.perf_counter()
    finally:
        pipeline._collect_idle()
    res = dict(path=path, views=len(views), samples=vol.n_samples, dims=list(dims), voxel=voxel,
               lo=[float(v) for v in lo], hi=[float(v) for v in hi], vertices=int(m.vertices.shape[0]),
               faces=int(m.faces.shape[0]), load_s=round(t1 - t0, 4), cameras_s=round(t2 - t1, 4),
               fuse_s=round(t3 - t2, 4), extract_s=round(t4 - t3, 4), write_s=round(t5 - t4t, 4))
    if report is not None:
        res.update(components=report["components"], components_kept=report["components_kept"],
                   faces_removed=report["faces_removed"], clean_s=round(t4c - t4, 4))
    if simplified is not None:
        res.update(clusters=simplified["clusters"], faces_collapsed=simplified["faces_collapsed"],
                   faces_duplicate=simplified["faces_duplicate"], simplify_s=round(t4s - t4c, 4))
    if baked is not None:
        res.update(occlusion=baked, bake_s=round(t4b - t4s, 4))
    if textured is not None:
        res.update(texture=textured, files=files, texture_s=round(t4t - t4l, 4))
    if lit is not None:
        res.update(light=lit, light_s=round(t4l - t4b, 4))
    return res


def main(argv=None) -> int:
    res = extract_mesh(parse_args(argv))
    print("views %d, samples %d (%d x %d x %d), vertices %d, faces %d" % (res["views"], res["samples"], *res["dims"],
                                                                        res["vertices"], res["faces"]))
    print("load %.3f s, cameras %.3f s, render + fuse %.3f s, extract %.3f s, write %.3f s" % (
        res["load_s"], res["cameras_s"], res["fuse_s"], res["extract_s"], res["write_s"]))
    if "components" in res:
        print("clean %.3f s: %d of %d components kept, %d faces removed" % (res["clean_s"], res["components_kept"],
                                                                          res["components"], res["faces_removed"]))
    if "clusters" in res:
        print("simplify %.3f s: %d clusters, %d faces collapsed, %d duplicates" % (res["simplify_s"], res["clusters"],
                                                                                  res["faces_collapsed"], res["faces_duplicate"]))
    if "occlusion" in res:
        print("bake %.3f s: %d rays per vertex, %d hits, %d vertices without a normal" % (
            res["bake_s"], res["occlusion"]["rays"], res["occlusion"]["hits_total"], res["occlusion"]["no_normal"]))
    if "texture" in res:
        print("texture %.3f s: %d x %d texels, %d baked" % (res["texture_s"], res["texture"]["width"], res["texture"]["height"],
                                                          res["texture"]["baked"]))
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
