"""Novel views of a trained scene on disk: the reference's render.py (render_set's pbr branch, eval_brdf) over
evaluate.NovelViewEvaluator and image_writer.ImageWriter.

    python gi-gs_amd/render_scene.py -m <out> --checkpoint <out>/chkpntN.pth --pbr [--metallic --indirect --tone --gamma
                                     --skip_train --skip_test --brdf_eval --lpips_weights DIR]            (CLI)
    render_scene(args) -> {split: {...}}                                                                  (API)

Flags and defaults are render.py's (:638-686); the scene path, the SH degree, --eval, --white_background and the
resolution come from <out>/cfg_args (get_combined_args), command-line values first.  Per split it writes what render_set
writes, under the same names (`planned_paths` is the table):

    <out>/<split>/envmap.png, unscaled_envmap.png, envmap.hdr                                    render.py:143-156
    <out>/<split>/ours_<iter>/pbr/<image_name>{,_DIR,_indirect,_albedo,_roughness,_metallic,_brdf,_diffuse,_specular,
                                               _occlusion}.png                                   :361-377
    <out>/<split>/ours_<iter>/normal/<idx:05d>_{normal,from_depth}.png                           :258-261, :363
    <out>/<split>/ours_<iter>/depth/<image_name>_depth.png                                       :376
    <out>/<split>/ours_<iter>/pbr/<last image_name>_NVS.json                                     :383-395

<iter> is the checkpoint's iteration.  View v + 1 is rendered while the writer's threads encode view v: the evaluator's
planes are the static outputs of its graph, and the writer's pack launch consumes them on the same stream before the
next replay overwrites them.  --brdf_eval (:496-634) reads the *_albedo.png files of an earlier run back and writes
albedo_ratio.json, albedo_metrics.json and <image_name>_albedo_{val,srgb,val_gt}.png per frame.

Deviations: the environment map is saved as Radiance envmap.hdr (the reference writes envmap.exr through OpenCV);
<image_name>_occlusion.png is an RGB file with three equal channels (ToPILImage makes a one-channel file of the same
values); lpips_avg is in *_NVS.json only with --lpips_weights; without --pbr only the from_depth normals are written,
as in the reference; --indirect is accepted and changes nothing, as in the reference (:248-252); cfg_args is parsed as
a literal Namespace(...) expression, not evaluated.  Not reproduced: envmap_test.png (:158-168 reads an absolute path on
the authors' machine), the viridis depth image (:233-234, computed and never saved), the empty renders/ gt/ pc/ folders.
eval_brdf looks for the ground-truth albedo of a frame at <scene>/<file_path>_albedo.png (Synthetic4Relight),
<scene>/<file_path with rgba -> albedo>.png (TensoIR) or <scene>/albedo/<image_name>*.png (:526-553) and takes the mask
from that file's alpha channel, else from the frame's own image; albedo_metrics.json also holds the masked MSE the
reference only prints.
"""
from __future__ import annotations

import argparse
import ast
import glob
import json
import os
import sys
import time
from argparse import Namespace
from typing import Dict, List, Optional, Sequence

if __package__ in (None, ""):  # run as a script: make the package's modules importable
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PBR_SUFFIXES = ("", "_DIR", "_indirect", "_albedo", "_roughness", "_metallic", "_brdf", "_diffuse", "_specular", "_occlusion")
# suffix -> the evaluator's plane (brdf: three planes side by side)
PBR_PLANES = {"": "pbr", "_DIR": "DIR", "_indirect": "indirect", "_albedo": "albedo", "_roughness": "roughness",
              "_metallic": "metallic", "_brdf": ("albedo", "roughness", "metallic"), "_diffuse": "diffuse",
              "_specular": "specular", "_occlusion": "occlusion"}
GI_FLAGS = dict(radius=0.8, bias=0.01, thick=0.05, delta=0.0625, step=16, start=8)


# ---- file names (pure) ----------------------------------------------------------------------------------------------------
def split_dir(out: str, split: str, iteration: int) -> str:
    return os.path.join(out, split, "ours_%d" % iteration)


def view_paths(out: str, split: str, iteration: int, idx: int, image_name: str, pbr: bool = True) -> Dict[str, str]:
    """{key: path} of one view's images: the PBR_SUFFIXES keys, "normal", "from_depth", "depth" (13 files with pbr)."""
    base = split_dir(out, split, iteration)
    paths = {"from_depth": os.path.join(base, "normal", "%05d_from_depth.png" % idx)}
    if pbr:
        for s in PBR_SUFFIXES:
            paths[s] = os.path.join(base, "pbr", image_name + s + ".png")
        paths["normal"] = os.path.join(base, "normal", "%05d_normal.png" % idx)
        paths["depth"] = os.path.join(base, "depth", image_name + "_depth.png")
    return paths


def planned_paths(out: str, split: str, iteration: int, image_names: Sequence[str], pbr: bool = True) -> List[str]:
    """Every file render_scene writes for a split, in writing order."""
    files = [os.path.join(out, split, n) for n in ("envmap.hdr", "envmap.png", "unscaled_envmap.png")]
    for idx, name in enumerate(image_names):
        files.extend(view_paths(out, split, iteration, idx, name, pbr).values())
    if pbr and image_names:
        files.append(os.path.join(split_dir(out, split, iteration), "pbr", image_names[-1] + "_NVS.json"))
    return files


# ---- arguments ------------------------------------------------------------------------------------------------------------
def add_model_arguments(p: argparse.ArgumentParser) -> None:
    """ModelParams(parser, sentinel=True) (arguments/__init__.py:21-40): every default is None, so that cfg_args shows
    through where the command line says nothing."""
    import trainer
    for k, v in trainer.MODEL_PARAMS.items():
        short = k.startswith("_")
        k = k.lstrip("_")
        names = ["--" + k] + (["-" + k[0]] if short else [])
        if isinstance(v, bool):
            p.add_argument(*names, default=None, action="store_true")
        else:
            p.add_argument(*names, default=None, type=type(v))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Testing script parameters")
    add_model_arguments(p)
    for k in ("skip_train", "skip_test", "quiet", "pbr", "tone", "gamma", "metallic", "indirect", "brdf_eval"):
        p.add_argument("--" + k, action="store_true")
    p.add_argument("--checkpoint", type=str, default=None, help="The path to the checkpoint to load.")
    for k, v in GI_FLAGS.items():
        p.add_argument("--" + k, type=type(v), default=v)
    p.add_argument("--lpips_weights", type=str, default=None,
                   help="directory with vgg16-397923af.pth and vgg.pth: adds lpips_avg / albedo_lpips")
    p.add_argument("--workers", type=int, default=12, help="PNG encoder threads (at most 16)")
    return p


def read_cfg_args(path: str) -> Dict:
    """<out>/cfg_args (prepare_output_and_logger, train.py:532-545) is the repr of a Namespace: its keyword arguments,
    each a Python literal, as a dict."""
    with open(path) as f:
        tree = ast.parse(f.read().strip(), mode="eval").body
    if not (isinstance(tree, ast.Call) and getattr(tree.func, "id", None) == "Namespace" and not tree.args):
        raise ValueError(f"{path}: not a Namespace(...) expression")
    return {kw.arg: ast.literal_eval(kw.value) for kw in tree.keywords}


def combine_args(args: Namespace) -> Namespace:
    """get_combined_args (arguments/__init__.py:101-120): <model_path>/cfg_args under the command line's values."""
    import trainer
    if not args.checkpoint:
        raise ValueError("--checkpoint is required")
    model_path = args.model_path or os.path.dirname(os.path.abspath(args.checkpoint))
    merged = {k.lstrip("_"): v for k, v in trainer.MODEL_PARAMS.items()}
    cfg_path = os.path.join(model_path, "cfg_args")
    if os.path.exists(cfg_path):
        merged.update(read_cfg_args(cfg_path))
    merged.update({k: v for k, v in vars(args).items() if v is not None or k not in merged})
    merged["model_path"] = model_path
    if not merged.get("source_path"):
        raise ValueError(f"no scene path: {cfg_path} is missing and -s was not given")
    return Namespace(**merged)


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    return build_parser().parse_args(argv)


def as_namespace(args, parser_fn) -> Namespace:
    if isinstance(args, (list, tuple)):
        return parser_fn(list(args))
    if isinstance(args, dict):
        d = vars(parser_fn([]))
        d.update(args)
        return Namespace(**d)
    return args


# ---- the scene ------------------------------------------------------------------------------------------------------------
def load_trained(args: Namespace, dev):
    """(Gaussian tensors, SH degree, checkpoint dict, {split: [CameraInfo]}) of a combined argument set."""
    import torch

    import pipeline
    import scene_io
    import trainer
    ck = scene_io.load_checkpoint(args.checkpoint)
    sc = scene_io.load_scene(args.checkpoint)
    g = {k: torch.from_numpy(sc[k]).to(dev) for k in pipeline.RASTER_KEYS}
    info = trainer._read_scene(args)  # Scene(dataset, gaussians, shuffle=False)
    return g, int(ck["gaussians"][0]), ck, {"train": info["train_cameras"], "test": info["test_cameras"]}


def load_lpips(args):
    if not getattr(args, "lpips_weights", None):
        return None
    import lpips
    return lpips.LPIPS(vgg_path=os.path.join(args.lpips_weights, "vgg16-397923af.pth"),
                       model_path=os.path.join(args.lpips_weights, "vgg.pth"))


def view_images(paths: Dict[str, str], planes: Dict) -> List:
    """One view's planes (NovelViewEvaluator with extra_planes) as the writer's images, render.py:361-377's conversions:
    save_image's rounding everywhere, ToPILImage's truncation for occlusion, min-max normalisation for depth."""
    import image_writer
    images = []
    for key, path in paths.items():
        if key == "depth":
            images.append(image_writer.Image(path, planes["depth"], normalize=True))
        elif key in ("normal", "from_depth"):
            images.append(image_writer.Image(path, planes[key]))
        else:
            src = PBR_PLANES[key]
            src = [planes[n] for n in src] if isinstance(src, tuple) else planes[src]
            images.append(image_writer.Image(path, src, bias=0.0 if key == "_occlusion" else 0.5))
    return images


def render_split(args: Namespace, split: str, infos, g, sh_degree: int, light, iteration: int, dev, lp=None) -> Dict:
    import torch

    import dataset_readers as dr
    import evaluate
    import image_writer
    import pbr
    import pipeline
    out = args.model_path
    names = [ci.image_name for ci in infos]
    for path in planned_paths(out, split, iteration, names, args.pbr):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    gi = {k: getattr(args, k) for k in GI_FLAGS}
    ev = evaluate.NovelViewEvaluator(light, gi, sh_degree, metallic=args.metallic, tone=args.tone, gamma=args.gamma,
                                     brdf_lut=pbr.get_brdf_lut().to(dev), lpips=lp, extra_planes=True)  # build_mips (:142)
    res: Dict = {"n_views": len(infos)}
    t0 = time.perf_counter()
    try:
        with image_writer.ImageWriter(workers=args.workers) as wr, torch.no_grad():
            envmap = light.export_envmap(return_img=True)  # [H,W,3]
            image_writer.write_hdr(os.path.join(out, split, "envmap.hdr"), envmap.clamp(min=0.0).cpu().numpy())
            env = envmap.permute(2, 0, 1)
            wr.submit([(os.path.join(out, split, "envmap.png"), env / env.max()),
                       (os.path.join(out, split, "unscaled_envmap.png"), env)])
            rays = None
            for idx, ci in enumerate(infos):
                c = dr.camera_from_info(ci, args.resolution, device=dev)
                if rays is None:
                    rays = pipeline.canonical_rays(c, dev)
                planes = ev(c, g, pipeline.view_dirs_for(c, rays, dev), c["original_image"], c["gt_alpha_mask"])
                wr.submit(view_images(view_paths(out, split, iteration, idx, ci.image_name, args.pbr), planes))
        res.update(files=wr.files + 1, png_bytes=wr.bytes_written, submit_blocked_s=round(wr.blocked_s, 4),
                   total_s=round(time.perf_counter() - t0, 4))
        if args.pbr and infos:
            r = ev.results()
            nvs = {k: r[k] for k in ("psnr_avg", "ssim_avg", "lpips_avg") if k in r}
            path = os.path.join(split_dir(out, split, iteration), "pbr", names[-1] + "_NVS.json")
            with open(path, "w") as f:
                json.dump(nvs, f, indent=4)
            res.update(nvs, nvs_json=path)
    finally:
        ev.close()
    return res


# ---- eval_brdf (render.py:496-634) ----------------------------------------------------------------------------------------
def _gt_albedo_path(root: str, file_path: str, image_name: str) -> str:
    tried = [os.path.join(root, file_path + "_albedo.png")]
    if "rgba" in file_path:
        tried.append(os.path.join(root, file_path.replace("rgba", "albedo") + ".png"))
    pattern = os.path.join(root, "albedo", image_name + "*.png")
    for p in tried + sorted(glob.glob(pattern)):
        if os.path.exists(p):
            return p
    raise FileNotFoundError("eval_brdf: no ground-truth albedo for %s (tried %s, %s)" % (file_path, ", ".join(tried), pattern))


def eval_brdf(args: Namespace, split: str, iteration: int, dev, lp=None) -> Dict:
    import numpy as np
    import torch
    from PIL import Image

    import evaluate
    import image_writer
    import pipeline
    root = args.source_path
    with open(os.path.join(root, "transforms_%s.json" % split)) as f:
        frames = json.load(f)["frames"]
    pbr_dir = os.path.join(split_dir(args.model_path, split, iteration), "pbr")
    gts, preds, masks, names = [], [], [], []
    for frame in frames:
        name = os.path.splitext(os.path.basename(frame["file_path"]))[0]
        pred = np.array(Image.open(os.path.join(pbr_dir, name + "_albedo.png")))[..., :3].copy()
        size = (pred.shape[1], pred.shape[0])
        gt_arr = np.array(Image.open(_gt_albedo_path(root, frame["file_path"], name)).resize(size))
        if gt_arr.ndim == 3 and gt_arr.shape[2] == 4:
            mask = gt_arr[..., 3] > 0
        else:
            view = Image.open(os.path.join(root, os.environ.get("DATA_SUBDIR", ""), os.path.basename(frame["file_path"]) + ".png"))
            mask = np.array(view.resize(size))[..., 3] > 0
        gt = gt_arr[..., :3].copy()
        gt[~mask] = 0
        pred[~mask] = 0
        gts.append(pipeline.srgb_to_linear(torch.from_numpy(gt).to(dev) / 255.0))
        preds.append(torch.from_numpy(pred).to(dev) / 255.0)
        masks.append(torch.from_numpy(mask).to(dev))
        names.append(name)
    ratio = evaluate.albedo_ratio(gts, preds, masks)
    with open(os.path.join(pbr_dir, "albedo_ratio.json"), "w") as f:
        json.dump({"three_channel_ratio": ratio.cpu().tolist()}, f, indent=4)
    metrics = evaluate.albedo_metrics(gts, preds, masks, ratio=ratio, lpips=lp)
    with image_writer.ImageWriter(workers=args.workers) as wr:
        for name, gt, pred in zip(names, gts, preds):
            scaled = (pred * ratio).permute(2, 0, 1)
            wr.submit([(os.path.join(pbr_dir, name + "_albedo_val.png"), scaled),
                       (os.path.join(pbr_dir, name + "_albedo_srgb.png"), pipeline.linear_to_srgb(scaled)),
                       (os.path.join(pbr_dir, name + "_albedo_val_gt.png"), gt.permute(2, 0, 1))])
    with open(os.path.join(pbr_dir, "albedo_metrics.json"), "w") as f:
        json.dump(metrics, f, indent=4)
    return dict(metrics, three_channel_ratio=ratio.cpu().tolist())


# ---- entry points ---------------------------------------------------------------------------------------------------------
def render_scene(args) -> Dict[str, Dict]:
    """render.py's launch (:398-486).  `args`: a Namespace from parse_args, a dict of overrides or an argv list."""
    import torch

    import pbr
    import pipeline
    args = combine_args(as_namespace(args, parse_args))
    if not torch.cuda.is_available():
        raise RuntimeError("render_scene needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    args.source_path = os.path.abspath(args.source_path)
    g, sh_degree, ck, cams = load_trained(args, dev)
    iteration = int(ck["iteration"])
    lp = load_lpips(args)
    results: Dict[str, Dict] = {}
    try:
        splits = [s for s, skip in (("train", args.skip_train), ("test", args.skip_test)) if not skip]
        if args.brdf_eval:
            for split in splits:
                if cams[split]:
                    results[split] = eval_brdf(args, split, iteration, dev, lp)
            return results
        if not ck.get("cubemap"):
            raise ValueError(f"{args.checkpoint}: the checkpoint holds no cubemap")
        light = pbr.CubemapLight(base_res=256, device=dev)
        light.load_state_dict({k: v.to(dev) for k, v in ck["cubemap"].items()})
        light.eval()
        for split in splits:
            if cams[split]:
                results[split] = render_split(args, split, cams[split], g, sh_degree, light, iteration, dev, lp)
        return results
    finally:
        pipeline._collect_idle()


def main(argv=None) -> int:
    args = parse_args(argv)
    print("Rendering " + (args.model_path or os.path.dirname(os.path.abspath(args.checkpoint or "."))))
    print(json.dumps(render_scene(args)))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
