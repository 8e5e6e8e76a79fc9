"""End-to-end scene training: train.py's two-stage schedule (:171-527) over the graphed iterations.

    python gi-gs_amd/trainer.py -s <scene> -m <out> [--eval --indirect --metallic ...]      (CLI)
    train_scene(args) -> TrainResult                                                          (API)

The pieces and where the schedule puts them:

    scene reading, cameras_extent          Scene (scene/__init__.py:30-110): dataset_readers (transforms_train.json or
                                           sparse/0), getNerfppNorm radius = cameras_extent = spatial_lr_scale
    init_from_cloud                        GaussianModel.create_from_pcd (scene/gaussian_model.py:272-317), distCUDA2 = knn.hip
    ten Adam groups + the light's          training_setup (:318-346), train.py:212-216 (one FusedAdam each, kept for the run)
    iterations 1..N                        train.py:236-527:
      SH ramp                                :241-242  every sh_up_interval (1000) iterations, before the render
      view order                             :245-249  shuffled train list (Scene, random.seed), stack.pop(randint(0, n-1))
      stage 1 / stage 2                      :255-420  Stage1Trainer (bg white with -w) / Stage2Trainer (black background)
      densification statistics               :494-498  a node of the captured stage-1 backward (gigs_densify_stats_guarded)
      densify_and_prune / reset_opacity      :500-514  densify.py, BEFORE the optimizer step, so that ...
      optimizer step                         :517-523  ... a densify iteration updates no Gaussian group, a reset alone
                                                       skips opacity (the new nn.Parameters carry no gradient); the light
                                                       steps from iteration pbr_iteration on; nothing steps at the last one
      update_learning_rate                   scene/gaussian_model.py:386-395 (its early return: xyz and albedo only)
      test reports                           training_report (:553-818): L1 / PSNR on the test cameras and five train
                                             cameras, as JSON lines in <out>/metrics.jsonl
      checkpoints                            :466-490 chkpnt{N}.pth (scene_io), <out>/cfg_args (prepare_output_and_logger)

Documented deviations: a checkpoint holds the state after iteration N's update (the reference saves before the densify
and the step of N, which its resume at N + 1 then never applies); likewise a test report at iteration N renders the model
after N's densify and update (training_report runs before them, train.py:440-460: its "iteration 1" report shows the
initial model) -- the graphed iteration carries its update, and replaying it without would change the arithmetic of the
stage-2 step; --start_checkpoint also restores the cubemap and the light optimizer (commented out at train.py:226-233); the initial cloud of a Blender scene is drawn from
numpy.random.RandomState(seed) (np.random.seed(seed) + np.random.random, as safe_state + readNerfSyntheticInfo do) and
not cached as points3d.ply; densification inside stage 2 (densify_until_iter > pbr_iteration + 1) is rejected up front.
"""
from __future__ import annotations

import argparse
import json
import os
import random
import sys
import time
from argparse import Namespace
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

if __package__ in (None, ""):  # run as a script: make the package's modules importable
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dataset_readers as dr  # noqa: E402

# arguments/__init__.py:50-99: the three parameter groups (name -> default; a leading "_" gives a one-letter shorthand)
MODEL_PARAMS = dict(sh_degree=3, _source_path="", _model_path="", _images="images", _resolution=-1,
                    _white_background=False, data_device="cuda", eval=False)
PIPELINE_PARAMS = dict(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
OPTIMIZATION_PARAMS = dict(iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016,
                           position_lr_delay_mult=0.01, position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05,
                           BRDF_lr=0.005, scaling_lr=0.005, rotation_lr=0.001, percent_dense=0.01, lambda_dssim=0.2,
                           densification_interval=100, opacity_reset_interval=3000, densify_from_iter=500,
                           densify_until_iter=15_000, densify_grad_threshold=0.0002, random_background=False)
# train.py:827-860
_REPORT_ITERS = [7_000, 30000, 32_000, 33000, 34000, 35000, 36000, 37000, 38000, 39000]
TRAIN_FLAGS = dict(ip="127.0.0.1", port=6009, debug_from=-1, detect_anomaly=False, test_iterations=_REPORT_ITERS,
                   save_iterations=_REPORT_ITERS, quiet=False, checkpoint_iterations=[30_000], start_checkpoint=None,
                   pbr_iteration=30_000, normal_tv=5.0, brdf_tv=1.0, env_tv=0.01, radius=0.8, bias=0.01, thick=0.05,
                   delta=0.0625, step=16, start=8, degree=3, tone=False, gamma=False, metallic=False, indirect=False)
# flags of this trainer (reference behaviour by default)
NEW_FLAGS = dict(hdri=None, init_points=100_000, sh_up_interval=1000, seed=0, lpips_weights=None)
IGNORED_FLAGS = ("ip", "port", "debug_from", "detect_anomaly")
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "normal", "albedo", "roughness", "metallic", "scaling", "rotation")


def _add_group(parser: argparse.ArgumentParser, name: str, params: Dict) -> None:
    """ParamGroup.__init__ (arguments/__init__.py:21-40)."""
    group = parser.add_argument_group(name)
    for key, value in params.items():
        short = key.startswith("_")
        key = key.lstrip("_")
        names = ["--" + key] + (["-" + key[0:1]] if short else [])
        if isinstance(value, bool):
            group.add_argument(*names, default=value, action="store_true")
        else:
            group.add_argument(*names, default=value, type=type(value))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Training script parameters")
    _add_group(p, "Loading Parameters", MODEL_PARAMS)
    _add_group(p, "Optimization Parameters", OPTIMIZATION_PARAMS)
    _add_group(p, "Pipeline Parameters", PIPELINE_PARAMS)
    for k in ("ip",):
        p.add_argument("--" + k, type=str, default=TRAIN_FLAGS[k])
    p.add_argument("--port", type=int, default=TRAIN_FLAGS["port"])
    p.add_argument("--debug_from", type=int, default=TRAIN_FLAGS["debug_from"])
    p.add_argument("--detect_anomaly", action="store_true", default=False)
    for k in ("test_iterations", "save_iterations", "checkpoint_iterations"):
        p.add_argument("--" + k, nargs="+", type=int, default=list(TRAIN_FLAGS[k]))
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--start_checkpoint", type=str, default=None)
    p.add_argument("--pbr_iteration", type=int, default=TRAIN_FLAGS["pbr_iteration"])
    for k in ("normal_tv", "brdf_tv", "env_tv", "radius", "bias", "thick", "delta"):
        p.add_argument("--" + k, type=float, default=TRAIN_FLAGS[k])
    for k in ("step", "start", "degree"):
        p.add_argument("--" + k, type=int, default=TRAIN_FLAGS[k])
    for k in ("tone", "gamma", "metallic", "indirect"):
        p.add_argument("--" + k, action="store_true")
    p.add_argument("--hdri", type=str, default=None, help="latitude-longitude HDR map (.npy [H,W,3] float32 or Radiance .hdr) for the initial light")
    p.add_argument("--init_points", type=int, default=NEW_FLAGS["init_points"], help="random initial points of a Blender scene")
    p.add_argument("--sh_up_interval", type=int, default=NEW_FLAGS["sh_up_interval"])
    p.add_argument("--seed", type=int, default=NEW_FLAGS["seed"])
    p.add_argument("--lpips_weights", type=str, default=None,
                   help="directory with vgg16-397923af.pth and vgg.pth: adds LPIPS-VGG to the test reports")
    return p


def parse_args(argv: Optional[List[str]] = None) -> Namespace:
    """train.py:828-866: the three iteration lists get `iterations` appended."""
    args = build_parser().parse_args(argv)
    for k in ("test_iterations", "save_iterations", "checkpoint_iterations"):
        getattr(args, k).append(args.iterations)
    return args


def validate(args: Namespace) -> None:
    if args.random_background:
        raise ValueError("--random_background is not supported by this trainer (the captured stage-1 iteration bakes its "
                         "background in)")
    if args.densify_until_iter > args.pbr_iteration + 1:
        raise ValueError("densify_until_iter (%d) > pbr_iteration + 1 (%d): densification inside stage 2 is not supported (the "
                         "graphed stage-2 iteration declares only material gradients, so it has no viewspace statistics)"
                         % (args.densify_until_iter, args.pbr_iteration + 1))


# ---- the schedule (host only) -----------------------------------------------------------------------------------------
def lr_functions(args: Namespace, spatial_lr_scale: float):
    """training_setup (scene/gaussian_model.py:347-358): the xyz and BRDF schedulers."""
    xyz = dr.get_expon_lr_func(args.position_lr_init * spatial_lr_scale, args.position_lr_final * spatial_lr_scale,
                               lr_delay_mult=args.position_lr_delay_mult, max_steps=args.position_lr_max_steps)
    brdf = dr.get_expon_lr_func(args.opacity_lr, args.BRDF_lr, lr_delay_mult=args.position_lr_delay_mult, max_steps=10000)
    return xyz, brdf


def initial_lrs(args: Namespace, spatial_lr_scale: float) -> Dict[str, float]:
    """training_setup (scene/gaussian_model.py:325-344)."""
    o = args.opacity_lr
    return dict(xyz=args.position_lr_init * spatial_lr_scale, f_dc=args.feature_lr, f_rest=args.feature_lr / 20.0, opacity=o,
                normal=o, albedo=o, roughness=o, metallic=o, scaling=args.scaling_lr, rotation=args.rotation_lr)


def schedule(iteration: int, args: Namespace) -> Dict:
    """What train.py does at `iteration` besides the render: {sh_up, stage, stats, densify, size_threshold, reset,
    update (the Gaussian groups the optimizer step moves), light_step, lr_update}."""
    densify_win = iteration < args.densify_until_iter                                                  # :493
    densify = densify_win and iteration > args.densify_from_iter and iteration % args.densification_interval == 0  # :500-503
    reset = densify_win and (iteration % args.opacity_reset_interval == 0 or
                             (args.white_background and iteration == args.densify_from_iter))         # :509-512
    step = iteration < args.iterations                                                                  # :517
    if not step or densify:
        update = ()
    elif reset:
        update = tuple(g for g in GROUPS if g != "opacity")
    else:
        update = GROUPS
    return dict(sh_up=iteration % args.sh_up_interval == 0, stage=1 if iteration <= args.pbr_iteration else 2,
                stats=densify_win, densify=densify,
                size_threshold=(20 if iteration > args.opacity_reset_interval else None) if densify else None,  # :505
                reset=reset, update=update, light_step=step and iteration >= args.pbr_iteration, lr_update=step)


def learning_rates(iteration: int, lrs: Dict[str, float], xyz_fn, brdf_fn) -> Dict[str, float]:
    """update_learning_rate(iteration) (scene/gaussian_model.py:386-395): the loop returns at the albedo group, so xyz
    follows its schedule, albedo BRDF_scheduler(iteration - 30000), roughness and metallic keep theirs."""
    out = dict(lrs)
    out["xyz"] = float(xyz_fn(iteration))
    out["albedo"] = float(brdf_fn(iteration - 30000))
    return out


def shuffled_train_order(n_views: int, rng: random.Random) -> List[int]:
    """Scene.__init__ (scene/__init__.py:96-97): random.shuffle of the training cameras."""
    order = list(range(n_views))
    rng.shuffle(order)
    return order


def view_sequence(order: List[int], n_iters: int, rng: random.Random) -> List[int]:
    """train.py:245-249: the stack is refilled when empty and a random entry popped."""
    out, stack = [], None
    for _ in range(n_iters):
        if not stack:
            stack = list(order)
        out.append(stack.pop(rng.randint(0, len(stack) - 1)))
    return out


# ---- model init --------------------------------------------------------------------------------------------------------
def init_from_cloud(points: np.ndarray, colors: np.ndarray, max_sh_degree: int, device="cuda", dist2=None):
    """GaussianModel.create_from_pcd (scene/gaussian_model.py:272-317) -> {name: nn.Parameter} under the reference's names;
    scales from distCUDA2 (csrc/knn.hip).  `dist2` replaces distCUDA2 (the CPU tests pass the oracle's)."""
    import torch
    if dist2 is None:
        from simple_knn._C import distCUDA2 as dist2
    pts = torch.tensor(np.asarray(points), dtype=torch.float32, device=device)
    col = (torch.tensor(np.asarray(colors), dtype=torch.float32, device=device) - 0.5) / 0.28209479177387814  # RGB2SH
    P, K = pts.shape[0], (max_sh_degree + 1) ** 2
    features = torch.zeros((P, 3, K), dtype=torch.float32, device=device)
    features[:, :3, 0] = col
    d2 = torch.clamp_min(dist2(pts), 0.0000001)
    scales = torch.log(torch.sqrt(d2))[..., None].repeat(1, 3)
    rots = torch.zeros((P, 4), device=device)
    rots[:, 0] = 1
    opac = torch.full((P, 1), 0.1, dtype=torch.float32, device=device)
    opac = torch.log(opac / (1 - opac))                                          # inverse_sigmoid
    normal = torch.zeros((P, 3), dtype=torch.float32, device=device)
    normal[..., 2] = 1.0
    ones = lambda c: torch.ones((P, c), dtype=torch.float32, device=device)  # noqa: E731
    t = dict(xyz=pts, f_dc=features[:, :, 0:1].transpose(1, 2).contiguous(), f_rest=features[:, :, 1:].transpose(1, 2).contiguous(),
             opacity=opac, normal=normal, albedo=ones(3), roughness=ones(1), metallic=ones(1), scaling=scales, rotation=rots)
    return {k: torch.nn.Parameter(v.contiguous().requires_grad_(True)) for k, v in t.items()}


@dataclass
class TrainResult:
    final_metrics: Dict = field(default_factory=dict)   # the last test report ({"test": {...}, "train": {...}})
    iterations: int = 0                                 # the last iteration run
    points: List = field(default_factory=list)          # [(iteration, P)] whenever P changed (and at the start)
    losses: List = field(default_factory=list)          # [(iteration, loss)] every 10 iterations
    reports: List = field(default_factory=list)         # every test report
    paths: List[str] = field(default_factory=list)      # files written
    recaptures: int = 0
    timings: Dict = field(default_factory=dict)
    start: Dict = field(default_factory=dict)           # where the run began: {"iteration", "sh_degree", "P", "resumed"}


@dataclass
class Restored:
    """What restore_checkpoint rebuilt from a chkpnt{N}.pth (the trainer starts at iteration + 1 from exactly this)."""
    iteration: int
    active_sh_degree: int
    raw: Dict            # {name: nn.Parameter} on the device
    optimizer: object    # FusedAdam over `raw`, state loaded
    stats: object        # densify.DensifyState
    spatial_lr_scale: float


def restore_checkpoint(path: str, device, light, light_optimizer) -> Restored:
    """train.py:223-234 (GaussianModel.restore, scene/gaussian_model.py:151-176): the Gaussians, the densification
    statistics, the optimizer state and the active SH degree; unlike the reference (whose lines are commented out) also the
    cubemap and the light optimizer when the checkpoint holds them -- loaded into `light` / `light_optimizer` in place."""
    import torch

    import densify
    import optim
    import scene_io
    ckpt = scene_io.load_checkpoint(path)
    active_sh, params, stats_d, opt_state, spatial_lr_scale = scene_io.restore(ckpt["gaussians"])
    raw = {k: torch.nn.Parameter(params[k].detach().to(device).float().contiguous()) for k in GROUPS}
    optimizer = optim.FusedAdam([{"params": [raw[k]], "lr": 0.0, "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
    optimizer.load_state_dict(opt_state)
    stats = densify.DensifyState(0, device)
    for k, v in stats_d.items():
        setattr(stats, k, v.detach().to(device).float().contiguous())
    if ckpt.get("cubemap"):
        light.load_state_dict({k: v.to(device) for k, v in ckpt["cubemap"].items()})
    if ckpt.get("light_optimizer"):
        light_optimizer.load_state_dict(ckpt["light_optimizer"])
    return Restored(int(ckpt["iteration"]), int(active_sh), raw, optimizer, stats, float(spatial_lr_scale))


def _as_namespace(args) -> Namespace:
    if isinstance(args, (list, tuple)):
        return parse_args(list(args))
    if isinstance(args, dict):
        args = Namespace(**args)
    d = vars(parse_args(["-s", "x"]))  # every default
    for k in ("test_iterations", "save_iterations", "checkpoint_iterations"):
        d[k] = d[k][:-1]
    d.update(vars(args))
    return Namespace(**d)


def _read_scene(args):
    src = args.source_path
    if os.path.exists(os.path.join(src, "sparse")):
        info = dr.readColmapSceneInfo(src, args.images, args.eval)
    elif os.path.exists(os.path.join(src, "transforms_train.json")):
        info = dr.readNerfSyntheticInfo(src, args.white_background, args.eval)
        info["point_cloud"] = None
    else:
        raise FileNotFoundError(f"{src}: neither sparse/0 nor transforms_train.json (Scene, scene/__init__.py:47-56)")
    return info


def _light(args, dev, opacity_lr):
    import optim
    import torch
    from pbr import CubemapLight
    if args.hdri:
        import image_writer
        import relight
        light = relight.make_light(torch.from_numpy(image_writer.load_latlong(args.hdri)).to(dev), res=256)
        light.train()
    else:
        light = CubemapLight(base_res=256, device=dev)                      # train.py:210-212 without the private HDRI
    light_opt = optim.FusedAdam([{"name": "cubemap", "params": list(light.parameters()), "lr": opacity_lr}], lr=opacity_lr)
    return light, light_opt


def train_scene(args, graphs: bool = True) -> TrainResult:
    """Runs train.py's schedule; `args`: a Namespace from parse_args, a dict of overrides or an argv list.  graphs=False
    runs the steppers' eager formulation instead of the captured one (the rasterizer launched op by op, the statistics,
    densification and Adam as eager launches): the comparison row of tools/train_scene_bench.py."""
    import contextlib

    import torch
    args = _as_namespace(args)
    validate(args)
    if not torch.cuda.is_available():
        raise RuntimeError("train_scene needs the GPU")
    dev = torch.device("cuda", torch.cuda.current_device())
    trainers = []
    try:
        with contextlib.ExitStack() as files:  # metrics.jsonl is closed however the run ends
            return _train(args, dev, trainers, files, graphs)
    finally:
        for tr in trainers:
            tr.close()
        trainers.clear()
        import pipeline
        pipeline._collect_idle()


def _train(args, dev, trainers, files, graphs=True) -> TrainResult:
    import torch

    import activations
    import densify
    import evaluate
    import losses
    import optim
    import pbr
    import pipeline
    import scene_io
    import train_iteration as ti

    t_start = time.perf_counter()
    res = TrainResult()
    out_dir = args.model_path or os.path.join("output", "run")
    os.makedirs(out_dir, exist_ok=True)
    # safe_state (utils/general_utils.py:125-150)
    rng = random.Random(args.seed)
    np_rng = np.random.RandomState(args.seed)
    torch.manual_seed(args.seed)
    gen = torch.Generator(device=dev).manual_seed(args.seed)

    args.source_path = os.path.abspath(args.source_path)
    info = _read_scene(args)
    extent = float(info["nerf_normalization"]["radius"])
    cloud = info.get("point_cloud") or dr.random_init_cloud(args.init_points, rng=np_rng)
    train_infos = [info["train_cameras"][i] for i in shuffled_train_order(len(info["train_cameras"]), rng)]
    test_infos = info["test_cameras"]
    cams = [dr.camera_from_info(c, args.resolution, device=dev) for c in train_infos]
    test_cams = [dr.camera_from_info(c, args.resolution, device=dev) for c in test_infos]
    # cfg_args (prepare_output_and_logger, train.py:532-545): the ModelParams group, as render.py / relight.py read it
    cfg = Namespace(**{k.lstrip("_"): getattr(args, k.lstrip("_")) for k in MODEL_PARAMS})
    cfg.sh_degree = args.degree
    cfg_path = os.path.join(out_dir, "cfg_args")
    with open(cfg_path, "w") as f:
        f.write(str(cfg))
    res.paths.append(cfg_path)
    metrics_path = os.path.join(out_dir, "metrics.jsonl")
    mlog = files.enter_context(open(metrics_path, "w"))
    res.paths.append(metrics_path)

    def log(rec):
        mlog.write(json.dumps(rec) + "\n")
        mlog.flush()

    max_sh = args.degree
    bg1 = torch.tensor([1.0, 1.0, 1.0] if args.white_background else [0.0, 0.0, 0.0], device=dev)
    bg2 = torch.zeros(3, device=dev)

    def compose(c, bg):  # train.py:314
        return (c["original_image"] * c["gt_alpha_mask"] + bg[:, None, None] * (1.0 - c["gt_alpha_mask"])).clamp(0.0, 1.0).contiguous()

    gts = [compose(c, bg1) for c in cams]
    first_iter, active_sh = 0, 0
    light, light_opt = _light(args, dev, args.opacity_lr)
    spatial_lr_scale = extent
    if args.start_checkpoint:
        rs = restore_checkpoint(args.start_checkpoint, dev, light, light_opt)
        first_iter, active_sh, raw, optimizer, stats, spatial_lr_scale = (
            rs.iteration, rs.active_sh_degree, rs.raw, rs.optimizer, rs.stats, rs.spatial_lr_scale)
        del rs
    else:
        raw = init_from_cloud(cloud["points"], cloud["colors"], max_sh, dev)
        lrs0 = initial_lrs(args, spatial_lr_scale)
        optimizer = optim.FusedAdam([{"params": [raw[k]], "lr": lrs0[k], "name": k} for k in GROUPS], lr=0.0, eps=1e-15)
        stats = densify.DensifyState(raw["xyz"].shape[0], dev)
    res.start = dict(iteration=first_iter, sh_degree=active_sh, P=int(raw["xyz"].shape[0]), resumed=bool(args.start_checkpoint))
    xyz_fn, brdf_fn = lr_functions(args, spatial_lr_scale)
    gi = dict(radius=args.radius, bias=args.bias, thick=args.thick, delta=args.delta, step=args.step, start=args.start)
    lut = pbr.get_brdf_lut().to(dev)
    lp = None
    if args.lpips_weights:
        import lpips
        lp = lpips.LPIPS(vgg_path=os.path.join(args.lpips_weights, "vgg16-397923af.pth"),
                         model_path=os.path.join(args.lpips_weights, "vgg.pth"))

    s1 = ti.Stage1Trainer(raw, gi, active_sh, lambda_dssim=args.lambda_dssim, normal_loss_weight=1.0,
                          normal_tv_weight=args.normal_tv, graphs=graphs, bg=bg1, densify_state=stats, optimizer=optimizer)
    trainers.append(s1)
    s2, gts2, vds = None, None, None
    report_views = [(5 + 5 * i) % len(cams) for i in range(5)]  # training_report: range(5, 30, 5)
    # the pops of iterations first_iter+1..N: the stack starts empty, as after the reference's resume
    seq = view_sequence(list(range(len(cams))), args.iterations - first_iter, rng)
    res.points.append((first_iter, int(raw["xyz"].shape[0])))
    tick = {"stage1_densify_window": [0, 0.0], "stage1_after_window": [0, 0.0], "stage2": [0, 0.0]}
    cur_phase = [None, 0.0]  # (phase, its start time less the reports and checkpoints inside it)

    def report(iteration, stage):
        rec = {"iteration": iteration, "stage": stage}
        with torch.no_grad():
            g = activations.activate(s1.raw if s2 is None else s2.raw)
        for name, views in (("test", list(range(len(test_cams)))), ("train", report_views)):
            vc = test_cams if name == "test" else cams
            if not views:
                continue
            l1s = []
            if stage == 1:  # training_report: the colour render, clamped, against the ground truth over the background
                rows, lps = [], []
                for v in views:
                    c = vc[v]
                    with torch.no_grad():
                        img = pipeline.render(c, g, active_sh, bg1, gi, inference=True)["render"].clamp(0.0, 1.0)
                        gt = compose(c, bg1)
                        l1s.append(losses.l1_loss(img, gt))
                        rows.append(evaluate.image_metrics(img, gt))
                        if lp is not None:
                            lps.append(lp(gt, img).reshape(()))
                entry = {"l1": float(torch.stack(l1s).mean()), "psnr": float(torch.stack([r[3] for r in rows]).mean()),
                         "n_views": len(views)}
                if lp is not None:
                    entry["lpips"] = float(torch.stack(lps).double().mean())
            else:  # the PBR render (NovelViewEvaluator: render.py's pbr branch and its metrics)
                ev = evaluate.NovelViewEvaluator(light, gi, active_sh, metallic=args.metallic, tone=args.tone,
                                                 gamma=args.gamma, graphs=False, brdf_lut=lut, lpips=lp)
                rays = pipeline.canonical_rays(vc[views[0]], dev)
                for v in views:
                    c = vc[v]
                    planes = ev(c, g, pipeline.view_dirs_for(c, rays, dev), c["original_image"], c["gt_alpha_mask"])
                    with torch.no_grad():
                        l1s.append(losses.l1_loss(planes["pbr"], compose(c, bg2)))
                r = ev.results()
                entry = {"l1": float(torch.stack(l1s).mean()), "psnr": r["psnr_avg"], "n_views": r["n_views"]}
                if lp is not None:
                    entry["lpips"] = r["lpips_avg"]
                ev.close()
            if lp is None:
                entry["lpips"] = None
                entry["lpips_note"] = "skipped: no --lpips_weights"
            rec[name] = entry
        rec["P"] = int(g["means3D"].shape[0])
        del g
        log(dict(rec, kind="report"))
        res.reports.append(rec)
        res.final_metrics = rec

    iteration = first_iter
    for iteration in range(first_iter + 1, args.iterations + 1):
        sch = schedule(iteration, args)
        if sch["sh_up"] and active_sh < max_sh:                                      # train.py:241-242
            active_sh += 1
            (s1 if s2 is None else s2).set_sh_degree(active_sh)
        v = seq[iteration - first_iter - 1]
        if s2 is None and not sch["stats"] and s1.densify_state is not None:
            s1.set_densify_state(None)  # the window has closed (train.py:493): the statistics stay as they are
        phase = "stage2" if sch["stage"] == 2 else ("stage1_densify_window" if sch["stats"] else "stage1_after_window")
        if phase != cur_phase[0]:
            # phases are timed on the device's clock: drain the queue at the boundary (three times per run)
            torch.cuda.synchronize()
            now = time.perf_counter()
            if cur_phase[0] is not None:
                tick[cur_phase[0]][1] += now - cur_phase[1]
            cur_phase[:] = [phase, now]
        if sch["stage"] == 1:
            tr = s1
            out = s1.iteration(cams[v], gts[v], update=sch["update"] == GROUPS)
            if sch["light_step"]:
                # iteration == pbr_iteration: light_optimizer.step() finds no gradient, the clamp still runs (train.py:520-523)
                with torch.no_grad():
                    light.clamp_(min=0.0)
        else:
            if s2 is None:                                                           # the stage switch
                s1.close()
                gts = None
                gts2 = [compose(c, bg2) for c in cams]
                rays = pipeline.canonical_rays(cams[0], dev)
                vds = [pipeline.view_dirs_for(c, rays, dev) for c in cams]
                s2 = ti.Stage2Trainer(s1.raw, light, lut, gi, active_sh, brdf_tv_weight=args.brdf_tv,
                                      env_tv_weight=args.env_tv, metallic=args.metallic, indirect=args.indirect,
                                      gamma=args.gamma, tone=args.tone, optimizer=optimizer, light_optimizer=light_opt,
                                      graphs=graphs)
                trainers.append(s2)
            tr = s2
            full = sch["update"] == GROUPS and sch["light_step"]
            out = s2.iteration(cams[v], gts2[v], vds[v], update=full)
            if not full and sch["light_step"]:
                s2.light_step()
        if sch["densify"] or sch["reset"]:
            raw_now = tr.raw
            new_stats = None
            if sch["densify"]:                                                       # train.py:500-507
                _, new_stats = densify.densify_and_prune(optimizer, stats, args.densify_grad_threshold, 0.05,
                                                         extent, sch["size_threshold"], percent_dense=args.percent_dense,
                                                         generator=gen)
            if sch["reset"]:                                                         # train.py:509-512
                densify.reset_opacity(optimizer)
            if sch["update"]:  # a reset alone: the nine groups that still hold gradients step (train.py:517-519)
                optimizer.step()
            for p in raw_now.values():
                p.grad = None
            by_name = {gr["name"]: gr["params"][0] for gr in optimizer.param_groups}
            tr.replace_parameters({k: by_name[k] for k in GROUPS}, densify_state=new_stats)
            if new_stats is not None:
                stats = new_stats
                res.points.append((iteration, int(by_name["xyz"].shape[0])))
        elif sch["update"] != GROUPS:
            for p in tr.raw.values():  # the last iteration: no step, nothing kept
                p.grad = None
        if sch["lr_update"]:                                                         # train.py:519
            lr = learning_rates(iteration, {}, xyz_fn, brdf_fn)
            tr.set_lr("xyz", lr["xyz"])
            tr.set_lr("albedo", lr["albedo"])
        tick[phase][0] += 1
        if iteration % 10 == 0:                                                      # train.py:429-431
            loss = float(out["loss"])
            res.losses.append((iteration, loss))
            log({"kind": "loss", "iteration": iteration, "loss": loss, "stage": sch["stage"]})
        del out
        if iteration in args.test_iterations or iteration in args.checkpoint_iterations or iteration in args.save_iterations:
            torch.cuda.synchronize()  # reports and checkpoints are not part of a phase's time
            t_out = time.perf_counter()
        if iteration in args.test_iterations:
            report(iteration, sch["stage"])
        if iteration in args.checkpoint_iterations or iteration in args.save_iterations:
            path = os.path.join(out_dir, "chkpnt%d.pth" % iteration)
            cur = tr.raw
            scene_io.save_checkpoint(path, scene_io.capture(active_sh, cur, stats, optimizer, spatial_lr_scale),
                                     light.state_dict(), light_opt.state_dict(), iteration)
            res.paths.append(path)
        if iteration in args.test_iterations or iteration in args.checkpoint_iterations or iteration in args.save_iterations:
            torch.cuda.synchronize()
            cur_phase[1] += time.perf_counter() - t_out
    torch.cuda.synchronize()
    if cur_phase[0] is not None:
        tick[cur_phase[0]][1] += time.perf_counter() - cur_phase[1]
    res.iterations = iteration
    res.recaptures = sum(w.recaptures for t in trainers for w in t.stepper._wholes.values())
    res.timings = {k: {"iterations": n, "seconds": round(s, 3)} for k, (n, s) in tick.items()}
    res.timings["total_s"] = round(time.perf_counter() - t_start, 3)
    return res


def main(argv=None) -> int:
    args = parse_args(argv)
    validate(args)
    if not args.model_path:
        args.model_path = os.path.join("output", "run")
    print("Optimizing " + args.model_path)
    r = train_scene(args)
    print(json.dumps({"iterations": r.iterations, "final": r.final_metrics, "points": r.points[-1] if r.points else None,
                      "paths": r.paths}))
    return 0


if __name__ == "__main__":
    import importlib
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    importlib.import_module("gi-gs_amd")
    sys.exit(main())
