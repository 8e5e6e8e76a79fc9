"""A trained scene under new environment maps, on disk: the reference's relight.py (and relight_eval.py with --gt_dir)
over relight.TurntableRelighter, relight.RelightEvaluator and image_writer.ImageWriter.

    python gi-gs_amd/relight_scene.py -m <out> --checkpoint <out>/chkpntN.pth --hdri a.hdr [b.hdr ...]
                                      [--metallic --tone --gamma --skip_train --skip_test --gt_dir DIR --lpips_weights DIR]
                                      [--rotations N [--rotation_axis x y z]]
                                      [--occluder mesh.ply [--ao_rays 64 --ao_distance D --ray_bias B
                                       --occluder_mode replace|multiply]]
                                      [--lights lights.json [--shadow_samples S]] [--denoise N]
    relight_scene(args) -> {split: {...}}

Flags and defaults are relight.py's (:340-356), with --hdri taking one or more maps (Radiance .hdr or .npy [H,W,3]): all
maps of a view go through one TurntableRelighter call (one G-buffer and one march per view, any number of lights).
<light> is the map's file name up to the first dot (:286).  --rotations N (a turntable) relights every map under N equal
right-handed steps of a full turn about the light's up axis (+y of the map's frame, or --rotation_axis), the identity
first: the lights are then <light>_r000 .. _r<N-1>, and --gt_dir is refused (no dataset has ground truth for rotated
maps).  Per split it writes (`planned_paths` is the table):

    <out>/<split>/envmap_relight_<light>.png                                       relight.py:142-145
    <out>/<split>/ours_<iter>/relight/<image_name>_<light>.png                     :249-251
    <out>/<split>/ours_<iter>/relight/<image_name>_<light>_occlusion.png           :184-186
    <out>/<split>/ours_<iter>/relight/<light>.json                                 with --gt_dir: relight_eval.py:68-85

The albedo ratio is read from <out>/test/ours_<iter>/pbr/albedo_ratio.json (:203-210) when that file exists; without it
the albedo is not scaled (the reference fails there).  With --gt_dir the ground truth of view <image_name> under <light>
is <gt_dir>/<light>/<image_name>.png; each view feeds RelightEvaluator, and <light>.json holds psnr_avg, ssim_avg (and
lpips_avg with --lpips_weights) over the split's views -- relight_eval.py's metrics without its fixed view list r_0010 ..
and its 400 x 400 resize target (the ground truth is resized to the prediction's size).

--occluder mesh.ply (the scene's extracted mesh; a relative path is looked up in <out>) ray-traces the occlusion of every
view's pixels against that mesh in place of SSAO (mesh_render.RaytracedGBuffer over relight.SplatGBuffer: --ao_rays rays a
pixel, a multiple of 64, within --ao_distance, started --ray_bias off the surface; both default as mesh.bake_occlusion's), so
geometry the view does not see occludes too; --occluder_mode multiply shades with the product of both.  The occlusion PNG is
then that plane, and the split's result holds the last view's tracer report as `occluder`.  --denoise N (1 to 5, needs
--occluder) filters the traced occlusion -- and the shadow planes of --lights -- with N iterations of denoise.atrous before they
are used; the result then holds the filter's report as `occluder_denoise`, and lights_report.json gains "denoise".

--lights lights.json also renders every view under the point and directional lights of that file (analytic_lights.py states
its format): <image_name>_lights.png, analytic_lights.AnalyticRelighter's lights_rgb over the splats' G-buffer, beside the
relit images.  With --occluder the lights cast ray-traced shadows against that mesh (--shadow_samples S samples a light, 1:
hard shadows; --ray_bias as above) and <image_name>_shadow_<l>.png is the visibility of light l; without it they are
unshadowed, no shadow image is written, and lights_report.json -- the lights' echo and every view's counters, in the same
folder -- says so.  Without --lights nothing of this runs.

Deviation: the reference writes <split>/envmap_relight.png, which every light of relight_all.bash overwrites; here the
file carries the light's name.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from argparse import Namespace
from typing import Dict, List, Optional, Sequence

if __package__ in (None, ""):  # run as a script: make the package's modules importable
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import render_scene as rs  # noqa: E402

OCCLUDER_MODES = ("replace", "multiply")  # mesh_render.RAYTRACED_MODES, without its imports


def rotated_names(names: Sequence[str], rotations: int) -> List[str]:
    """The light names of a run: the maps' own, or <light>_r000 .. per map with --rotations N."""
    if rotations <= 0:
        return list(names)
    return ["%s_r%03d" % (n, k) for n in names for k in range(rotations)]


def light_name(path: str) -> str:
    return os.path.basename(path).split(".")[0]  # relight.py:286


# ---- file names (pure) ----------------------------------------------------------------------------------------------------
def view_paths(out: str, split: str, iteration: int, image_name: str, lights: Sequence[str]) -> List[str]:
    base = os.path.join(rs.split_dir(out, split, iteration), "relight")
    files = []
    for light in lights:
        files.append(os.path.join(base, "%s_%s.png" % (image_name, light)))
        files.append(os.path.join(base, "%s_%s_occlusion.png" % (image_name, light)))
    return files


def planned_paths(out: str, split: str, iteration: int, image_names: Sequence[str], lights: Sequence[str],
                  with_metrics: bool = False) -> List[str]:
    """Every file relight_scene writes for a split."""
    files = [os.path.join(out, split, "envmap_relight_%s.png" % light) for light in lights]
    for name in image_names:
        files.extend(view_paths(out, split, iteration, name, lights))
    if with_metrics:
        files.extend(os.path.join(rs.split_dir(out, split, iteration), "relight", light + ".json") for light in lights)
    return files


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Testing script parameters")
    rs.add_model_arguments(p)
    for k in ("skip_train", "skip_test", "quiet", "tone", "gamma", "metallic"):
        p.add_argument("--" + k, action="store_true")
    p.add_argument("--hdri", type=str, nargs="+", default=None, help="The environment maps for relighting (.hdr or .npy).")
    p.add_argument("--checkpoint", type=str, default=None, help="The path to the checkpoint to load.")
    for k, v in rs.GI_FLAGS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    p.add_argument("--gt_dir", type=str, default=None, help="ground truth: <gt_dir>/<light>/<image_name>.png")
    p.add_argument("--lpips_weights", type=str, default=None, help="directory with vgg16-397923af.pth and vgg.pth")
    p.add_argument("--rotations", type=int, default=0, help="relight every map under N equal turns about its up axis")
    p.add_argument("--rotation_axis", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                   help="axis of --rotations in the map's frame (default 0 1 0)")
    p.add_argument("--workers", type=int, default=12, help="PNG encoder threads (at most 16)")
    p.add_argument("--occluder", type=str, default=None, help="a mesh PLY: ray-trace the occlusion against it in place of SSAO")
    p.add_argument("--ao_rays", type=int, default=64, help="occlusion rays per pixel, a multiple of 64 in [64, 1024]")
    p.add_argument("--ao_distance", type=float, default=None, help="how far an occluder counts (default: mesh.bake_occlusion's)")
    p.add_argument("--ray_bias", type=float, default=None, help="the rays' start off the surface (default: 1e-3 ao_distance)")
    p.add_argument("--occluder_mode", choices=OCCLUDER_MODES, default="replace",
                   help="shade with the traced occlusion, or with its product with SSAO")
    p.add_argument("--lights", type=str, default=None, help="a JSON list of point and directional lights: also render under them")
    p.add_argument("--shadow_samples", type=int, default=1, help="shadow samples per light in [1, 64] (needs --occluder)")
    p.add_argument("--denoise", type=int, default=0,
                   help="a-trous iterations (1 to 5) over the traced occlusion and shadow planes (needs --occluder)")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def check_occluder(args: Namespace) -> bool:
    """Whether --occluder is given; refuses the tracer's flags without it and values outside their ranges."""
    rays, mode = int(getattr(args, "ao_rays", 64)), getattr(args, "occluder_mode", "replace")
    distance, bias = getattr(args, "ao_distance", None), getattr(args, "ray_bias", None)
    n = getattr(args, "denoise", 0) or 0
    if not 0 <= int(n) <= 5:
        raise ValueError("--denoise: 1 to 5 a-trous iterations (0: off), got %r" % (n,))
    if not getattr(args, "occluder", None):
        if rays != 64 or distance is not None or bias is not None or mode != "replace":
            raise ValueError("--ao_rays, --ao_distance, --ray_bias and --occluder_mode need --occluder")
        if int(n):
            raise ValueError("--denoise needs --occluder: it filters ray-traced planes")
        return False
    if mode not in OCCLUDER_MODES:
        raise ValueError("--occluder_mode: one of %s, got %r" % (", ".join(OCCLUDER_MODES), mode))
    if rays < 64 or rays > 1024 or rays % 64 != 0:
        raise ValueError("--ao_rays: a multiple of 64 in [64, 1024], got %d" % rays)
    for name, x in (("--ao_distance", distance), ("--ray_bias", bias)):
        if x is not None and not (0.0 <= float(x) < float("inf")):
            raise ValueError("%s: finite and >= 0, got %r" % (name, x))
    return True


def check_lights(args: Namespace) -> bool:
    """Whether --lights is given; refuses --shadow_samples without it or without --occluder, and a count outside [1, 64]."""
    samples = int(getattr(args, "shadow_samples", 1))
    if not getattr(args, "lights", None):
        if samples != 1:
            raise ValueError("--shadow_samples needs --lights")
        return False
    if samples != 1 and not getattr(args, "occluder", None):
        raise ValueError("--shadow_samples needs --occluder: without a mesh the lights are unshadowed")
    if samples < 1 or samples > 64:
        raise ValueError("--shadow_samples: a count in [1, 64], got %d" % samples)
    return True


def lights_split(args: Namespace, split: str, infos, g, sh_degree: int, iteration: int, dev) -> Dict:
    """--lights: the files and the report described in the module docstring, for one split."""
    import torch

    import analytic_lights
    import dataset_readers as dr
    import image_writer
    import relight
    import render_mesh
    out = args.model_path
    lights = analytic_lights.load_lights(args.lights)
    base = os.path.join(rs.split_dir(out, split, iteration), "relight")
    os.makedirs(base, exist_ok=True)
    gi = {k: getattr(args, k) for k in rs.GI_FLAGS}
    shadows, S = bool(getattr(args, "occluder", None)), int(args.shadow_samples)
    n_denoise = int(getattr(args, "denoise", 0) or 0) if shadows else 0
    views, files = [], []
    with image_writer.ImageWriter(workers=args.workers) as wr, torch.no_grad():
        tracer = None
        if shadows:
            import mesh_render
            path = args.occluder if os.path.isabs(args.occluder) or os.path.exists(args.occluder) else os.path.join(out, args.occluder)
            tracer = mesh_render.RaytracedLight(path, bias=args.ray_bias, device=dev)
        try:
            relighter = analytic_lights.AnalyticRelighter(lights, relight.SplatGBuffer(gi, sh_degree, args.metallic), tracer, S, gamma=True,
                                                          denoise=n_denoise)
            for ci in infos:
                c = dr.camera_from_info(ci, args.resolution, device=dev)
                o = relighter(c, g)
                paths = render_mesh.lights_paths(base, ci.image_name, len(lights), shadows)
                images = [image_writer.Image(paths["lights"], o["lights_rgb"])]
                images += [image_writer.Image(p, o["shadow"][l:l + 1], bias=0.0) for l, p in enumerate(paths["shadow"])]
                wr.submit(images)
                files += [paths["lights"]] + paths["shadow"]
                views.append(dict(o["report"], image_name=ci.image_name))
        finally:
            if tracer is not None:
                tracer.close()
    path = os.path.join(base, "lights_report.json")
    render_mesh.write_lights_report(path, lights, shadows, S, views, occluder=getattr(args, "occluder", None),
                                    **(dict(denoise=n_denoise) if n_denoise else {}))
    return dict(report_json=path, files=files, shadows=shadows, views=views)


def check_rotations(args: Namespace) -> int:
    """--rotations as a count (0 = none); refuses a negative count and --rotations together with --gt_dir."""
    n = int(getattr(args, "rotations", 0) or 0)
    if n < 0:
        raise ValueError("--rotations: a count of turns, got %d" % n)
    if n > 0 and getattr(args, "gt_dir", None):
        raise ValueError("--rotations with --gt_dir: there is no ground truth for rotated maps")
    return n


def _read_gt(path: str, dev):
    import numpy as np
    import torch
    from PIL import Image
    arr = np.array(Image.open(path))[..., :3]
    return torch.from_numpy(arr).to(dev).permute(2, 0, 1) / 255.0  # relight_eval.py:52-53


def relight_split(args: Namespace, split: str, infos, g, sh_degree: int, lights, names: List[str], iteration: int, dev,
                  ratio, lp=None) -> Dict:
    import torch

    import dataset_readers as dr
    import image_writer
    import pbr
    import pipeline
    import relight
    out = args.model_path
    image_names = [ci.image_name for ci in infos]
    for path in planned_paths(out, split, iteration, image_names, names):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    gi = {k: getattr(args, k) for k in rs.GI_FLAGS}
    lut = pbr.get_brdf_lut().to(dev)
    res: Dict = {"n_views": len(infos), "lights": list(names)}
    MAX_LIGHTS = relight.MAX_LIGHTS
    t0 = time.perf_counter()
    with image_writer.ImageWriter(workers=args.workers) as wr, torch.no_grad():
        tracer = source = None
        if getattr(args, "occluder", None):  # without it the relighter builds its own SplatGBuffer, as before
            import mesh_render
            path = args.occluder if os.path.isabs(args.occluder) or os.path.exists(args.occluder) else os.path.join(out, args.occluder)
            tracer = mesh_render.RaytracedLight(path, rays=args.ao_rays, ao_distance=args.ao_distance, bias=args.ray_bias, device=dev)
            source = mesh_render.RaytracedGBuffer(relight.SplatGBuffer(gi, sh_degree, args.metallic), tracer, args.occluder_mode,
                                                  denoise=int(getattr(args, "denoise", 0) or 0))
        tr = relight.TurntableRelighter(lights, gi, sh_degree, metallic=args.metallic, tone=args.tone, gamma=args.gamma,
                                        brdf_lut=lut, source=source)  # build_mips per light (:141)
        ev = relight.RelightEvaluator(names, device=dev, lpips=lp) if args.gt_dir else None
        try:
            for first in range(0, len(lights), MAX_LIGHTS):  # one batch of files per MAX_LIGHTS lights
                wr.submit([(os.path.join(out, split, "envmap_relight_%s.png" % n),
                            light.export_envmap(return_img=True).permute(2, 0, 1).clamp(min=0.0, max=1.0))
                           for n, light in zip(names[first:first + MAX_LIGHTS], lights[first:first + MAX_LIGHTS])])
            rays = None
            for ci in infos:
                c = dr.camera_from_info(ci, args.resolution, device=dev)
                if rays is None:
                    rays = pipeline.canonical_rays(c, dev)
                o = tr(c, g, pipeline.view_dirs_for(c, rays, dev), alpha_mask=c["gt_alpha_mask"], albedo_ratio=ratio)
                paths = view_paths(out, split, iteration, ci.image_name, names)
                images = []
                for k in range(len(lights)):
                    images.append((paths[2 * k], o["render_rgb"][k]))
                    images.append((paths[2 * k + 1], o["occlusion"]))
                for first in range(0, len(images), 2 * MAX_LIGHTS):
                    wr.submit(images[first:first + 2 * MAX_LIGHTS])
                if ev is not None:
                    gt = [_read_gt(os.path.join(args.gt_dir, n, ci.image_name + ".png"), dev) for n in names]
                    ev.add(o["render_rgb"], torch.stack(gt))
            if ev is not None:
                for n, m in ev.results().items():
                    m = {k: v for k, v in m.items() if k != "n_views"}
                    path = os.path.join(rs.split_dir(out, split, iteration), "relight", n + ".json")
                    with open(path, "w") as f:
                        json.dump(m, f, indent=4)
                    res.setdefault("metrics", {})[n] = m
        finally:
            tr.close()
            if tracer is not None:
                res["occluder"] = source.report
                if source.denoise:
                    res["occluder_denoise"] = source.denoise_report
                tracer.close()
    res.update(files=wr.files, png_bytes=wr.bytes_written, submit_blocked_s=round(wr.blocked_s, 4),
               total_s=round(time.perf_counter() - t0, 4))
    return res


def relight_scene(args) -> Dict[str, Dict]:
    """relight.py's launch (:254-334) for every map of --hdri.  `args`: a Namespace from parse_args, a dict of overrides
    or an argv list."""
    import torch

    import image_writer
    import pipeline
    import relight
    args = rs.as_namespace(args, parse_args)
    n_rot = check_rotations(args)  # before anything is read
    check_occluder(args)
    with_lights = check_lights(args)
    args = rs.combine_args(args)
    if not args.hdri:
        raise ValueError("--hdri: at least one environment map is required")
    if not torch.cuda.is_available():
        raise RuntimeError("relight_scene needs the GPU")
    hdris = [args.hdri] if isinstance(args.hdri, str) else list(args.hdri)
    names = [light_name(p) for p in hdris]
    if len(set(names)) != len(names):
        raise ValueError("--hdri: two maps share the light name %s" % sorted(n for n in names if names.count(n) > 1)[0])
    dev = torch.device("cuda", torch.cuda.current_device())
    args.source_path = os.path.abspath(args.source_path)
    g, sh_degree, ck, cams = rs.load_trained(args, dev)
    iteration = int(ck["iteration"])
    maps = [torch.from_numpy(image_writer.load_latlong(p)).to(dev) for p in hdris]
    if n_rot:
        turns = relight.yaw_rotations(n_rot, args.rotation_axis or (0.0, 1.0, 0.0))
        lights = [light for m in maps for light in relight.rotated_lights(m, turns, res=256)]
        names = rotated_names(names, n_rot)
    else:
        lights = [relight.make_light(m, res=256) for m in maps]
    ratio = None
    ratio_path = os.path.join(rs.split_dir(args.model_path, "test", iteration), "pbr", "albedo_ratio.json")
    if os.path.exists(ratio_path):
        with open(ratio_path) as f:
            ratio = tuple(float(v) for v in json.load(f)["three_channel_ratio"])
    lp = rs.load_lpips(args)
    results: Dict[str, Dict] = {}
    try:
        for split, skip in (("train", args.skip_train), ("test", args.skip_test)):
            if not skip and cams[split]:
                results[split] = relight_split(args, split, cams[split], g, sh_degree, lights, names, iteration, dev, ratio, lp)
                results[split]["albedo_ratio"] = ratio
                if with_lights:
                    results[split]["analytic_lights"] = lights_split(args, split, cams[split], g, sh_degree, iteration, dev)
        return results
    finally:
        pipeline._collect_idle()


def main(argv=None) -> int:
    args = parse_args(argv)
    print("Rendering " + (args.model_path or os.path.dirname(os.path.abspath(args.checkpoint or "."))))
    print(json.dumps(relight_scene(args)))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
