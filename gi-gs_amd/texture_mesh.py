"""A mesh PLY already on disk (extract_mesh.py's) as a light mesh with textures: the heavy mesh's recovered materials are
baked into an atlas over a simplification of it (mesh.bake_atlas) and written as OBJ + MTL + PNG, the form DCC tools and
engines read.

    python gi-gs_amd/texture_mesh.py SRC.ply -o OUT.obj (--target LOW.ply | --cell_edges R | --cell X) [--block 8]
                                     [--width W] [--bake_occlusion RAYS] [--max_distance D] [--samples N]
                                     [--light a.hdr [--bounces 1] [--sky_res 32] [--light_rays 256]]             (CLI)
    texture_mesh(args) -> {...}                                                                                   (API)

The light mesh is --target, or SRC simplified by mesh.simplify with cells of --cell world units or --cell_edges median
edge lengths (simplify_mesh.py's options).  Every face of it gets a chart of --block texels in an atlas --width wide
(mesh.atlas_layout), and every texel the albedo, occlusion, roughness, metallic and normal of SRC at the closest point of
SRC's surface.  SRC's occlusion is the PLY's channel if it has one, else mesh.bake_occlusion with --bake_occlusion rays, else
1.  --max_distance leaves texels farther than D from SRC unbaked.  Written: OUT.obj and OUT.mtl (scene_io.save_mesh_obj),
OUT_albedo.png, OUT_orm.png (occlusion, roughness, metallic), OUT_roughness.png, OUT_metallic.png and OUT_normal.png (the
world normal n / |n| / 2 + 1/2, a zero normal as 1/2), through image_writer.  Prints the report as JSON: mesh.bake_atlas's
(`atlas`), the simplification's if it ran (`simplify`), the files and the times.

--light a.hdr (or .npy) adds a light-map: mesh.bake_light on SRC under that map (bake_mesh.py's options), carried through the
same atlas launch (bake_atlas's `extra`) and written as OUT_lightmap.hdr, linear irradiance, with the host Radiance writer; the
report names it under `files` and gains `light`, the bake's report.  Without --light every file is what it was.

--samples N adds `samples`, the number the textures exist for: at N surface samples of the light mesh
(mesh.sample_surface), per channel group, the RMS difference to SRC's attributes at the closest point of SRC
(mesh.transfer_attributes) of (a) `atlas_rms`: the atlas looked up at the sample (mesh.sample_atlas), and (b)
`vertex_rms`: the light mesh's own per-vertex attributes interpolated at the sample -- what a PLY of the light mesh shows.
Normals are compared as unit vectors.  The light mesh's own occlusion is --target's channel if it has one, else SRC's
transferred to its vertices.
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

GROUPS = (("albedo", 0, 3), ("occlusion", 3, 4), ("roughness", 4, 5), ("metallic", 5, 6), ("normal", 6, 9))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Mesh texturing parameters")
    p.add_argument("input", type=str, help="the heavy mesh: a PLY written by extract_mesh.py or bake_mesh.py")
    p.add_argument("-o", "--output", type=str, required=True, help="the .obj to write; the .mtl and the PNGs land beside it")
    light = p.add_mutually_exclusive_group(required=True)
    light.add_argument("--target", type=str, default=None, help="the light mesh, a PLY; default: simplify the input")
    light.add_argument("--cell", type=float, default=None, help="simplify with cells of this size in world units")
    light.add_argument("--cell_edges", type=float, default=None, help="simplify with cells of this many median edge lengths")
    p.add_argument("--block", type=int, default=8, help="texels along a chart's edge (>= 3)")
    p.add_argument("--width", type=int, default=None, help="atlas width in texels (default: the smallest power of two)")
    p.add_argument("--bake_occlusion", type=int, default=0, help="rays per vertex if the input has no occlusion channel (0: occlusion 1)")
    p.add_argument("--max_distance", type=float, default=None, help="texels farther than this from the input stay unbaked")
    p.add_argument("--samples", type=int, default=0, help="report the material error of the atlas and of the light mesh's vertices at N samples")
    p.add_argument("--light", type=str, default=None, help="an environment map (.hdr or .npy): bake a light-map under it")
    p.add_argument("--bounces", type=int, default=1, help="diffuse inter-reflections of the light bake")
    p.add_argument("--sky_res", type=int, default=32, help="texels an edge of the sky cube the light bake looks up")
    p.add_argument("--light_rays", type=int, default=256, help="rays per vertex of the light bake, a multiple of 64 in [64, 1024]")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def normal_image(normal):
    """[3,H,W] world normals as interpolated -> n / |n| / 2 + 1/2, a zero (or non-finite) normal as 1/2."""
    import torch
    length = normal.double().pow(2).sum(0, keepdim=True).sqrt()
    unit = torch.where((length > 0) & torch.isfinite(length), normal.double() / length, torch.zeros_like(normal, dtype=torch.float64))
    return (unit * 0.5 + 0.5).float()


def save_textured_mesh(path: str, m, atlas, lightmap: bool = False) -> Dict[str, str]:
    """Writes the light mesh `m` (a mesh.Mesh) with `atlas` (a mesh.Atlas over it) as PATH (.obj), its .mtl and the five PNGs
    beside it.  -> {obj, mtl, albedo, orm, roughness, metallic, normal}: the paths written.  `lightmap`: atlas.extra [3,H,W]
    (linear irradiance) goes to STEM_lightmap.hdr as well, and the result names it."""
    import image_writer
    import scene_io
    if atlas.layout.height < 1:
        raise ValueError("save_textured_mesh: the mesh has no face to texture")
    names = scene_io.obj_texture_names(path)
    folder = os.path.dirname(path)
    files = {k: os.path.join(folder, v) for k, v in names.items()}
    scene_io.save_mesh_obj(path, m.vertices, m.faces, atlas.uvs, normals=m.normals, textures=names)
    with image_writer.ImageWriter(workers=5, slots=1) as writer:
        writer.submit([image_writer.Image(files["albedo"], atlas.albedo), image_writer.Image(files["orm"], atlas.orm),
                       image_writer.Image(files["roughness"], atlas.orm[1:2]), image_writer.Image(files["metallic"], atlas.orm[2:3]),
                       image_writer.Image(files["normal"], normal_image(atlas.normal))])
    out = dict(files, obj=path, mtl=os.path.splitext(path)[0] + ".mtl")
    if lightmap:
        if atlas.extra is None or atlas.extra.shape[0] != 3:
            raise ValueError("save_textured_mesh: a light-map needs an atlas with three extra channels")
        out["lightmap"] = os.path.splitext(path)[0] + "_lightmap.hdr"
        image_writer.write_hdr(out["lightmap"], atlas.extra.permute(1, 2, 0).contiguous().cpu().numpy())
    return out


def _unit(n):
    import torch
    length = n.pow(2).sum(1, keepdim=True).sqrt()
    return torch.where(length > 0, n / length, torch.zeros_like(n))


def material_error(dst, dst_occlusion, src, src_occlusion, atlas, n: int, seed: int = 0, grid=None) -> Dict:
    """The `samples` report: per channel group atlas_rms and vertex_rms against src at n surface samples of dst."""
    import torch

    import mesh
    points, face, bary = mesh.sample_surface(dst, n, seed)
    values = torch.cat((src.albedo, src_occlusion[:, None], src.roughness[:, None], src.metallic[:, None], src.normals), 1)
    want, near, _, _, _ = mesh.transfer_attributes(points, src, values, grid=grid)
    planes = torch.cat((atlas.albedo, atlas.orm, atlas.normal), 0)
    looked = mesh.sample_atlas(planes, atlas.layout, face, bary)
    own = torch.cat((dst.albedo, dst_occlusion[:, None], dst.roughness[:, None], dst.metallic[:, None], dst.normals), 1).double()
    idx = dst.faces[face.long()].long()
    w1, w2 = bary[:, 0:1].double(), bary[:, 1:2].double()
    interpolated = ((1.0 - w1) - w2) * own[idx[:, 0]] + w1 * own[idx[:, 1]] + w2 * own[idx[:, 2]]
    ok = near >= 0
    want = want.double()
    out = dict(n=int(points.shape[0]), compared=int(ok.sum().item()), seed=seed)
    for name, a, b in GROUPS:
        ref, x, y = want[ok, a:b], looked[ok, a:b], interpolated[ok, a:b]
        if name == "normal":
            ref, x, y = _unit(ref), _unit(x), _unit(y)
        rms = lambda d: float(d.pow(2).mean().sqrt().item()) if d.numel() else 0.0  # noqa: E731
        out[name] = dict(atlas_rms=rms(x - ref), vertex_rms=rms(y - ref))
    return out


def texture_mesh(args) -> Dict:
    """`args`: a Namespace from parse_args or an argv list."""
    import torch

    import mesh
    import mesh_render
    import scene_io
    if not isinstance(args, Namespace):
        args = parse_args(list(args))
    if not torch.cuda.is_available():
        raise RuntimeError("texture_mesh needs the GPU")
    if not args.output.endswith(".obj"):
        raise ValueError("texture_mesh: the output must end in .obj, got %r" % args.output)
    dev = torch.device("cuda", torch.cuda.current_device())
    sync = torch.cuda.synchronize

    def load(path):
        read = scene_io.read_mesh_ply(path)
        occ = torch.from_numpy(read["occlusion"]).to(dev) if "occlusion" in read else None
        return mesh_render.device_mesh(read, dev), occ

    src, src_occ = load(args.input)
    res: Dict = dict(input=args.input)
    times: Dict = {}
    grid = mesh.triangle_grid(src)
    if src_occ is not None:
        res["occlusion"] = "channel"
    elif args.bake_occlusion > 0:
        sync()
        t0 = time.perf_counter()
        src_occ, baked = mesh.bake_occlusion(src, rays=args.bake_occlusion, grid=grid)
        sync()
        times["bake_occlusion_s"] = round(time.perf_counter() - t0, 4)
        res["occlusion"], res["bake_occlusion"] = "baked", baked
    else:
        res["occlusion"] = "none"
    dst_occ = None
    if args.target is not None:
        dst, dst_occ = load(args.target)
        res["target"] = args.target
    else:
        cell = args.cell
        if cell is None:
            edge = mesh.median_edge(src)
            if not edge > 0:
                raise ValueError("texture_mesh: --cell_edges needs a valid face with a positive edge length")
            cell, res["median_edge"] = args.cell_edges * edge, edge
        sync()
        t0 = time.perf_counter()
        dst, res["simplify"] = mesh.simplify(src, cell)
        sync()
        times["simplify_s"] = round(time.perf_counter() - t0, 4)
    irradiance = None
    if getattr(args, "light", None):
        import bake_mesh
        sync()
        t0 = time.perf_counter()
        irradiance, res["light"] = mesh.bake_light(src, bake_mesh.load_sky(args.light, args.sky_res, dev), rays=args.light_rays,
                                                   bounces=args.bounces, grid=grid)
        sync()
        times["bake_light_s"] = round(time.perf_counter() - t0, 4)
        res["light"]["map"] = args.light
    sync()
    t0 = time.perf_counter()
    atlas, res["atlas"] = mesh.bake_atlas(dst, src, block=args.block, width=args.width, occlusion=src_occ,
                                          max_distance=args.max_distance, grid=grid, extra=irradiance)
    sync()
    t1 = time.perf_counter()
    res["files"] = save_textured_mesh(args.output, dst, atlas, lightmap=irradiance is not None)
    times.update(bake_atlas_s=round(t1 - t0, 4), write_s=round(time.perf_counter() - t1, 4))
    if args.samples > 0:
        ones = torch.ones(int(src.vertices.shape[0]), dtype=torch.float32, device=dev)
        so = src_occ if src_occ is not None else ones
        if dst_occ is None:  # the light mesh's own: the source's, transferred to its vertices
            dst_occ = mesh.transfer_attributes(dst.vertices, src, so, grid=grid)[0][:, 0] if src_occ is not None else \
                torch.ones(int(dst.vertices.shape[0]), dtype=torch.float32, device=dev)
        res["samples"] = material_error(dst, dst_occ, src, so, atlas, args.samples, grid=grid)
    return dict(res, path=args.output, vertices=int(dst.vertices.shape[0]), faces=int(dst.faces.shape[0]), **times)


def main(argv=None) -> int:
    print(json.dumps(texture_mesh(parse_args(argv))))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
