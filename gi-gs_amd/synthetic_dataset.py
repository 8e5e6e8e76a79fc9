"""A small NeRF-synthetic style dataset rendered by this package, for the trainer's tests and tools/train_scene_bench.py.

A teacher scene (scenes.surface_scene, SH 0) is shaded by the stage-2 path (evaluate.NovelViewEvaluator: render.py's pbr
branch) under scenes.synthetic_envmap and written as RGBA PNGs -- alpha = the rasterizer's opacity plane -- beside
transforms_{train,test}.json.  The images sit in the scene folder under their base names, where the reader looks for them
(scene/dataset_readers.py:246-248).  Needs the GPU."""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

FOVX = 0.69


def _c2w(eye, target=(0.0, 0.0, -0.2), up=(0.0, 0.0, 1.0)):
    """Blender camera-to-world (the camera looks down its -Z, Y up)."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def write_synthetic_dataset(root: str, n_train: int = 24, n_test: int = 8, seed: int = 0, size: int = 128,
                            points: int = 4000) -> str:
    """Writes the dataset into `root` (created) and returns it."""
    from PIL import Image

    import activations
    import dataset_readers as dr
    import evaluate
    import pipeline
    import relight
    import scenes
    import train_iteration as ti
    dev = torch.device("cuda:0")
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(seed)
    frames = {"train": [], "test": []}
    for split, n in (("train", n_train), ("test", n_test)):
        for i in range(n):
            a = 2 * math.pi * (i + (0.5 if split == "test" else 0.0)) / n
            el = 0.35 + 0.25 * rng.random()
            eye = (3.2 * math.cos(a) * math.cos(el), 3.2 * math.sin(a) * math.cos(el), 3.2 * math.sin(el))
            frames[split].append({"file_path": "./%s/%s_%d" % (split, split, i), "transform_matrix": _c2w(eye).tolist()})
        with open(os.path.join(root, "transforms_%s.json" % split), "w") as f:
            json.dump({"camera_angle_x": FOVX, "frames": frames[split]}, f)
    sc = scenes.surface_scene(P=points, sh_degree=0, seed=seed + 3, scale_mu=0.05)
    raw = ti.raw_from_scene(sc, dev)
    with torch.no_grad():
        g = activations.activate(raw)
    env = torch.from_numpy(scenes.synthetic_envmap(128, 256)).to(dev) * 0.5
    light = relight.make_light(env, res=64)
    gi = dict(scenes.GI_DEFAULTS, start=64)
    ev = evaluate.NovelViewEvaluator(light, gi, 0, metallic=True, graphs=False)
    for split in ("train", "test"):
        cams = dr.cameras_from_transforms(os.path.join(root, "transforms_%s.json" % split), size, size)
        for i, c in enumerate(cams):
            c = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
            with torch.no_grad():
                alpha = pipeline.render(c, g, 0, torch.zeros(3, device=dev), gi, inference=True)["opacity_map"].clamp(0, 1)
            rays = pipeline.canonical_rays(c, dev)
            planes = ev(c, g, pipeline.view_dirs_for(c, rays, dev), torch.zeros(3, size, size, device=dev), alpha)
            rgba = torch.cat([planes["pbr"].clamp(0, 1), alpha], 0).permute(1, 2, 0).cpu().numpy()
            Image.fromarray((rgba * 255 + 0.5).astype(np.uint8), "RGBA").save(os.path.join(root, "%s_%d.png" % (split, i)))
    ev.close()
    del light, ev, g, raw
    torch.cuda.synchronize()
    return root
