"""A COMPLETE stage-2 ("PBR + indirect") training iteration of the reference's train.py (:247-523) on the fast path.

    activations of the ten raw parameter groups      scene/gaussian_model.py:178-263      (gigs_activate_fwd/_bwd)
    rasterizer + in-op filters + SSAO                gaussian_renderer/__init__.py:30-220 (gigs_forward, ...)
    build_mips, pbr_shading, Gaussian_SSR, L1, lamb   train.py:293-402                     (the fused stage-2 node)
    masked BRDF TV + envmap TV                        train.py:387-420                     (gigs_tv_loss_*, gigs_cube_texture_*)
    loss.backward()
    Adam over the ten Gaussian groups + the light     train.py:517-522; gaussian_model.py:325-346 (gigs_adam_step_dyn)
    cubemap.clamp_(min=0)                             train.py:522

`Stage2Trainer` holds the optimizer's tensors and runs that sequence through `pipeline.Stage2Step`; with graphs=True
the whole iteration replays from three hipGraphs (forward, backward, update; `pipeline.WholeStepGraph`).  Dataset
loading, densification (every 100 iterations: densify.py) and logging are outside.

The reference picks the masked or the unmasked BRDF TV with a host read (`(normal_mask == 0).sum() > 0`,
train.py:388); the two are the same expression when the mask is all ones (the products with 1.0 are exact), so
the masked form is used unconditionally and nothing is read back.
"""
from __future__ import annotations

import time
from typing import Dict, Optional

import numpy as np
import torch

import activations
import losses
import optim
import pipeline

# arguments/__init__.py:79-89 (OptimizationParams) as scene/gaussian_model.py:325-346 assigns them
DEFAULT_LRS = dict(xyz=1.6e-4, f_dc=2.5e-3, f_rest=2.5e-3 / 20.0, opacity=0.05, normal=0.05, albedo=0.05, roughness=0.05,
                   metallic=0.05, scaling=5e-3, rotation=1e-3)
RAW_KEYS = ("xyz", "f_dc", "f_rest", "opacity", "normal", "albedo", "roughness", "metallic", "scaling", "rotation")


def _logit(x):
    x = np.clip(x, 1e-6, 1.0 - 1e-6)
    return np.log(x / (1.0 - x))


def raw_from_scene(sc: Dict[str, np.ndarray], device) -> Dict[str, torch.nn.Parameter]:
    """Pre-activation parameters whose activations reproduce the post-activation arrays of `sc` (scenes.*_scene)."""
    t = lambda x: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device))  # noqa: E731
    return dict(xyz=t(sc["means3D"]), f_dc=t(sc["shs"][:, :1]), f_rest=t(sc["shs"][:, 1:]), opacity=t(_logit(sc["opacities"])),
                normal=t(sc["normal"]), albedo=t(_logit(sc["albedo"])), roughness=t(_logit(sc["roughness"])),
                metallic=t(_logit(sc["metallic"])), scaling=t(np.log(sc["scales"])), rotation=t(sc["rotations"]))


class Stage2Regularizer:
    """train.py:387-420 minus the lamb term (which the fused stage-2 node already carries): the masked TV of
    [albedo, remapped roughness, metallic] weighted by the ground-truth image's edges, and the TV of the panorama
    sampled from the light's base cubemap."""

    def __init__(self, light, envmap_dirs: Optional[torch.Tensor] = None, brdf_tv_weight: float = 1.0,
                 env_tv_weight: float = 0.01):
        self.light, self.brdf_tv_weight, self.env_tv_weight = light, float(brdf_tv_weight), float(env_tv_weight)
        self.envmap_dirs = envmap_dirs if envmap_dirs is not None else losses.get_envmap_dirs(device=light.base.device)

    def __call__(self, maps: Dict[str, torch.Tensor]) -> torch.Tensor:
        # the envmap term's nodes are created first: autograd walks later nodes first, so the BRDF term's backward -- whose
        # gradients the rasterizer's backward waits for -- runs ahead of the panorama lookup's (the values do not change)
        env = losses.env_tv_loss(self.light.base, self.envmap_dirs) if self.env_tv_weight != 0.0 else None
        mask = losses.nonzero_mask(maps["normal_map"])                  # gaussian_renderer/__init__.py:158
        rough = maps["roughness_map"] * (1.0 - 0.04) + 0.04             # train.py:297-298
        brdf = torch.cat([maps["albedo_map"], rough, maps["metallic_map"]], dim=0)
        loss = self.brdf_tv_weight * losses.get_masked_tv_loss(mask, maps["gt_image"], brdf)
        if env is not None:
            loss = loss + self.env_tv_weight * env
        return loss


class Stage2Trainer:
    """The optimizer's tensors + one `iteration(cam, gt_image, view_dirs)` call per training step.

    raw: {"xyz", "f_dc", "f_rest", "opacity", "normal", "albedo", "roughness", "metallic", "scaling", "rotation"}
    (leaf tensors; the reference's names, scene/gaussian_model.py:325-346).  `before_update` (e.g. a dp.GradSlab
    all-reduce + wait) runs between the backward and the update on every formulation."""

    def __init__(self, raw: Dict[str, torch.Tensor], light, brdf_lut: torch.Tensor, gi: Dict, sh_degree: int,
                 lrs: Optional[Dict[str, float]] = None, light_lr: float = 0.05, graphs: bool = True, glue: str = "hip",
                 brdf_tv_weight: float = 1.0, env_tv_weight: float = 0.01, before_update=None, metallic: bool = True,
                 geometry_cache: bool = False, materials_only: bool = True, indirect: bool = True, gamma: bool = False,
                 tone: bool = False, optimizer=None, light_optimizer=None):
        """geometry_cache: reuse, per view, what frozen geometry makes constant -- tile lists, occlusion plane (pipeline.
        GeometryCache; graphs only).  Same updates as without it (tested); a secondary figure, never the headline metric.
        materials_only (graphs only): a stage-2 iteration's loss reaches albedo / roughness / metallic and the light, every
        other gradient is an exact zero -- DECLARED here, so those zeros are neither written by the rasterizer's backward,
        nor pushed through the activations' backward, nor read by Adam (which updates the groups with g = 0: same
        arithmetic), and CHECKED on the device by every backward (gigs_ctx_set_materials_only): a violation raises at
        the next iteration.  Same updates as without it (tested).
        optimizer / light_optimizer: existing optimizers to step instead of fresh ones -- the reference keeps ONE Adam across
        the stage switch (train.py:186, 517-520), so a stage-1 trainer's `optimizer` (moments and step counts) is handed on
        here; it must hold `raw`'s tensors under the reference's group names.  indirect / gamma / tone: train.py's flags
        (the defaults are the ones this trainer has always used)."""
        if glue not in ("hip", "torch"):
            raise ValueError("glue must be 'hip' or 'torch'")
        self.raw, self.light = raw, light
        lrs = dict(DEFAULT_LRS, **(lrs or {}))
        Opt = optim.FusedAdam if glue == "hip" else torch.optim.Adam
        if optimizer is not None:
            _check_holds(optimizer, raw)
            self.optimizer = optimizer
        else:
            groups = [{"params": [raw[k]], "lr": lrs[k], "name": k} for k in RAW_KEYS]
            self.optimizer = Opt(groups, lr=0.0, eps=1e-15)                               # gaussian_model.py:346
        if light_optimizer is not None:
            self.light_optimizer = light_optimizer
        else:
            self.light_optimizer = Opt([{"name": "cubemap", "params": list(light.parameters()), "lr": light_lr}], lr=light_lr)
        self.regularizer = Stage2Regularizer(light, brdf_tv_weight=brdf_tv_weight, env_tv_weight=env_tv_weight)
        self.stepper = pipeline.Stage2Step(
            light, brdf_lut, gi, sh_degree, metallic=metallic, indirect=indirect, gamma=gamma, tone=tone,
            graphs=graphs and glue == "hip", fused=glue == "hip",
            prepare=activations.activate if glue == "hip" else activations.activate_torch, regularizer=self.regularizer,
            optimizers=[self.optimizer, self.light_optimizer], post_update=lambda: light.clamp_(min=0.0),
            before_update=before_update, geometry_cache=geometry_cache and graphs and glue == "hip",
            materials_only=materials_only and graphs and glue == "hip")

    def set_lr(self, name: str, lr: float) -> None:
        """update_learning_rate (scene/gaussian_model.py:349-355): takes effect at the next iteration, graphs included
        (the captured Adam launch reads its step sizes from a table refreshed every step)."""
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                group["lr"] = lr

    def iteration(self, cam: Dict, gt_image: torch.Tensor, view_dirs: torch.Tensor, update: bool = True) -> Dict[str, torch.Tensor]:
        """update=False: forward and backward from the same graphs, no Adam (Gaussians or light) and no clamp; the gradients
        are left in `.grad` (the light's included: `light_step()` applies it)."""
        return self.stepper(cam, self.raw, gt_image, view_dirs, update=update)

    def light_step(self) -> None:
        """The light's half of the update after an `update=False` iteration: light_optimizer.step(), zero_grad(set_to_none),
        cubemap.clamp_(min=0) (train.py:520-523)."""
        self.light_optimizer.step()
        for p in self.light.parameters():
            p.grad = None
        with torch.no_grad():
            self.light.clamp_(min=0.0)

    def set_sh_degree(self, sh_degree: int) -> None:
        """The active SH degree (oneupSHdegree, train.py:241-242): the stepper re-captures at the next iteration."""
        self.stepper.set_sh_degree(sh_degree)

    def close(self) -> None:
        """Deterministic teardown of the stepper's hipGraphs (synchronise, release, synchronise): call it when the trainer
        is done -- a trainer references its stepper and the stepper the trainer's bound methods, so without it the graph
        execs would live until a cyclic-GC pass.  `with Stage2Trainer(...) as tr:` closes on exit."""
        self.stepper.close()
        from pbr import texture
        texture.release_plans(self.regularizer.envmap_dirs)  # the envmap TV's cached gather plan goes with the trainer

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def replace_parameters(self, raw: Dict[str, torch.Tensor], densify_state=None) -> None:
        """After densification / pruning / opacity reset (densify.py on `self.optimizer`, as the reference's
        GaussianModel methods do, scene/gaussian_model.py:580-931): the optimizer's groups hold NEW tensor objects and
        moments; hand the new dictionary over.  The next iteration re-captures the graphs (once) around them.
        densify_state: attach / replace the statistics the iterations update (needs materials_only=False: the declared
        stage-2 gradient set has no viewspace gradient)."""
        if densify_state is not None and self.stepper.materials_only:
            raise ValueError("replace_parameters: densification statistics need materials_only=False")
        missing = [k for k in RAW_KEYS if k not in raw]
        if missing:
            raise KeyError("replace_parameters: missing " + ", ".join(missing))
        held = {id(g["params"][0]) for g in self.optimizer.param_groups}
        if any(id(raw[k]) not in held for k in RAW_KEYS):
            raise ValueError("replace_parameters: the tensors must be the ones the optimizer's groups hold")
        self.stepper.close()  # the graphs around the old tensors are released here, with the device idle
        self.raw = {k: raw[k] for k in RAW_KEYS}
        if densify_state is not None:
            self.stepper.densify_state = densify_state
        if getattr(self, "_dp_args", None) is not None:  # the gradient slab follows the new tensors
            timing = self.slab.timing
            _attach_slab(self, *self._dp_args, light=self.light)
            self.slab.timing = timing

    # the tensors a stage-2 iteration's loss reaches (train.py:330-420): everything else gets exact zeros
    STAGE2_TRAINABLE = ("albedo", "roughness", "metallic", "cubemap")

    def grad_buffers(self, names=STAGE2_TRAINABLE) -> Dict[str, torch.Tensor]:
        """The gradient tensors the NEXT update will read, by name ("cubemap" = light.base): the whole-step graphs' static
        buffers once they are captured (the captured Adam launch reads exactly these addresses), `.grad` otherwise.  Valid
        inside `before_update` (after the backward, before the update)."""
        leaves = dict(self.raw, cubemap=self.light.base)
        wsg = self.stepper.whole
        if wsg is not None and wsg.gf is not None:
            params = wsg._params(self.raw)
            by_id = {id(p): g for p, g in zip(params, wsg.grads)}
            return {n: by_id[id(leaves[n])] for n in names if by_id.get(id(leaves[n])) is not None}
        return {n: leaves[n].grad for n in names if leaves[n].grad is not None}

    def data_parallel(self, group=None, names=STAGE2_TRAINABLE, average: bool = False, force: bool = False):
        """View-parallel training: every rank runs `iteration` on its own view; between the backward and the
        update the gradients of `names` are summed over the ranks -- ONE collective on the communication stream, over one
        contiguous stretch of a dp.GradSlab that holds every raw gradient and the light's (the slab is ordered so that
        `names` are adjacent, at its end).  On the graph path the backward writes the raw gradients straight into the slab
        (activations.grad_sink; the rasterizer's grad_sink for xyz; the light's is copied in by a node of the backward graph)
        and the captured Adam launch reads the slab's views, so nothing is packed or unpacked per step; the eager path packs
        `.grad` once.  Identically initialised ranks take identical updates.  A stage-2 iteration reaches only the default
        `names` (every other gradient is an exact zero on every rank); pass every raw name for stage-1 style losses.
        `force` issues the collective with a single rank too (a one-GPU RCCL rehearsal).  Returns the slab
        (`.timing = True` + `.comm_stats()` for measurements)."""
        return _attach_slab(self, group, names, average, force, light=self.light)


def _check_holds(optimizer, raw) -> None:
    held = {g.get("name"): g["params"] for g in optimizer.param_groups}
    if any(k not in held or len(held[k]) != 1 or held[k][0] is not raw[k] for k in RAW_KEYS):
        raise ValueError("optimizer: its groups must hold raw's tensors under the reference's names")


def _attach_slab(trainer, group, names, average, force, light=None):
    import dp
    raw = trainer.raw
    leaves = dict(raw)
    if light is not None:
        leaves["cubemap"] = light.base
    unknown = [n for n in names if n not in leaves]
    if unknown:
        raise KeyError("data_parallel: unknown parameter name(s) " + ", ".join(unknown))
    order = [k for k in leaves if k not in names] + [k for k in leaves if k in names]  # the reduced stretch last: one piece
    slab = dp.GradSlab([leaves[k] for k in order], group)
    only = [i for i, k in enumerate(order) if k in names]
    trainer.slab, trainer.slab_order = slab, order
    trainer._dp_args = (group, tuple(names), average, force)
    stepper = trainer.stepper
    stepper.grad_slab = {k: v for k, v in zip(order, slab.views)}
    stepper.grad_slab_reduced = set(names)  # what the collective covers (pipeline.WholeStepGraph._into_slab)

    def hook():
        wsg = stepper.whole
        packed = wsg is not None and wsg.gf is not None  # the captured backward has written the views
        slab.allreduce_async(average=average, force=force, only=None if len(only) == len(order) else only, packed=packed)
        slab.wait()
    stepper.before_update = hook
    stepper.close()  # graphs captured before this call hand their gradients out elsewhere
    return slab


class Stage1Trainer:
    """The same for stage 1 (`iteration <= pbr_iteration`, train.py:266-331, 517-520): activations -> rasterizer (+ in-op
    filters + SSAO, computed as in the reference although stage 1 does not read it) -> fused G-buffer post-processing ->
    0.8 L1 + 0.2 D-SSIM + masked normal L1 + normal TV -> backward -> Adam over the ten Gaussian groups; three hipGraphs
    with graphs=True.  `gi` with start >= step (the README's --start 64) skips the march: same losses and gradients."""

    def __init__(self, raw: Dict[str, torch.Tensor], gi: Dict, sh_degree: int, lrs: Optional[Dict[str, float]] = None,
                 lambda_dssim: float = 0.2, normal_loss_weight: float = 1.0, normal_tv_weight: float = 1.0, graphs: bool = True,
                 before_update=None, compute_occlusion: bool = True, bg: Optional[torch.Tensor] = None, densify_state=None,
                 optimizer=None):
        """compute_occlusion=False: the operator's SSAO march is switched off for these iterations (start = step in the raster
        settings, what the README's --start 64 does): stage 1 neither reads occlusion_map nor differentiates through it, so
        losses, gradients and updates are unchanged (tested) while the iteration loses its largest kernel.  The default keeps
        the reference's work.
        bg: background colour (white with -w; black by default).  densify_state: a densify.DensifyState updated by every
        iteration (a node of the captured backward on the graph path).  optimizer: an existing FusedAdam over `raw` (e.g.
        restored from a checkpoint) instead of a fresh one."""
        self.raw = raw
        if not compute_occlusion:
            gi = dict(gi, start=gi["step"])
        lrs = dict(DEFAULT_LRS, **(lrs or {}))
        if optimizer is not None:
            _check_holds(optimizer, raw)
            self.optimizer = optimizer
        else:
            self.optimizer = optim.FusedAdam([{"params": [raw[k]], "lr": lrs[k], "name": k} for k in RAW_KEYS], lr=0.0, eps=1e-15)
        self.stepper = pipeline.Stage1Step(gi, sh_degree, lambda_dssim, normal_loss_weight, normal_tv_weight, graphs=graphs,
                                           prepare=activations.activate, optimizers=[self.optimizer], before_update=before_update,
                                           bg=bg, densify_state=densify_state)

    def set_lr(self, name: str, lr: float) -> None:
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                group["lr"] = lr

    def iteration(self, cam: Dict, gt_image: torch.Tensor, update: bool = True) -> Dict[str, torch.Tensor]:
        """update=False: forward, backward and statistics from the same graphs without the Adam step (a densify iteration,
        train.py:493-520); the gradients are left in `.grad`."""
        return self.stepper(cam, self.raw, gt_image, update=update)

    def set_sh_degree(self, sh_degree: int) -> None:
        """The active SH degree (oneupSHdegree, train.py:241-242): the stepper re-captures at the next iteration."""
        self.stepper.set_sh_degree(sh_degree)

    @property
    def densify_state(self):
        return self.stepper.densify_state

    def set_densify_state(self, state) -> None:
        """Attach, replace or (None) detach the statistics; the next iteration re-captures."""
        self.stepper.close()
        self.stepper.densify_state = state

    def close(self) -> None:
        """Deterministic teardown of the stepper's hipGraphs (synchronise, release, synchronise): call it when the trainer
        is done -- a trainer references its stepper and the stepper the trainer's bound methods, so without it the graph
        execs would live until a cyclic-GC pass.  `with Stage1Trainer(...) as tr:` closes on exit."""
        self.stepper.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def data_parallel(self, group=None, names=RAW_KEYS, average: bool = False, force: bool = False):
        """As Stage2Trainer.data_parallel; a stage-1 loss reaches every Gaussian group, so the whole slab is one collective."""
        return _attach_slab(self, group, names, average, force)

    def replace_parameters(self, raw: Dict[str, torch.Tensor], densify_state=None) -> None:
        """As Stage2Trainer.replace_parameters; densify_state attaches / replaces the statistics (densify_and_prune returns a
        new one sized for the new set)."""
        held = {id(g["params"][0]) for g in self.optimizer.param_groups}
        if any(k not in raw or id(raw[k]) not in held for k in RAW_KEYS):
            raise ValueError("replace_parameters: pass the tensors the optimizer's groups hold, under the reference's names")
        self.stepper.close()
        self.raw = {k: raw[k] for k in RAW_KEYS}
        if densify_state is not None:
            self.stepper.densify_state = densify_state
        if getattr(self, "_dp_args", None) is not None:
            timing = self.slab.timing
            _attach_slab(self, *self._dp_args)
            self.slab.timing = timing


def _dp_timed(run, steps, warmup, slab):
    """`steps` iterations between two (barrier + synchronize) brackets; with a process group the maximum over the ranks."""
    import torch.distributed as dist
    on = dist.is_available() and dist.is_initialized()
    for i in range(warmup):
        run(i)
    if slab is not None:
        torch.cuda.synchronize()
        slab.comm_stats()  # drop the warm-up collectives' events
    if on:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        out = run(warmup + i)
    if on:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if on:
        t = torch.tensor([dt], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return dt / steps, out


def _dp_fields(slab, world, P):
    if slab is None:
        return {}
    comm = slab.comm_stats() or {}
    comm["floats_per_gaussian"] = round(comm.get("bytes", 0) / 4 / max(P, 1), 2)
    return {"data_parallel": {"ranks": world, "views_per_iteration": world, "comm": comm,
                              "how": "ONE all-reduce of a contiguous stretch of the gradient slab on the communication stream, "
                                     "between the backward graph and the captured Adam (which reads the slab's views)"}}


def bench_stage1_iteration(sc, gi, sh_degree, cams_t, gt_image, steps=40, warmup=5, compute_occlusion=True,
                           data_parallel=False, force=False, rank=0, world=1) -> Dict:
    """bench.py's `iteration_stage1` field.  data_parallel: every rank trains on its own view and EVERY raw gradient is
    summed over the ranks (a stage-1 loss reaches every Gaussian group) before the update."""
    import dp
    raw = raw_from_scene(sc, gt_image.device)
    tr = Stage1Trainer(raw, gi, sh_degree, graphs=True, compute_occlusion=compute_occlusion)
    slab = None
    if data_parallel:
        slab = tr.data_parallel(force=force)
        slab.timing = True
    n = len(cams_t)
    dt, out = _dp_timed(lambda i: tr.iteration(cams_t[dp.view_for(i, rank, world, n)], gt_image), steps, warmup, slab)
    formulation = "3 hipGraphs (fwd, bwd, update)" if tr.stepper.whole is not None else "eager"
    final_loss = float(out["loss"])
    del out
    extra = _dp_fields(slab, world, raw["xyz"].shape[0])
    tr.close()
    return {"iterations_per_s": round(world / dt, 2), "ms_per_iteration": round(1e3 * dt, 3), "steps": steps, "final_loss": final_loss, **extra,
            "what": "activations + rasterizer + in-op filters + SSAO + G-buffer post-processing + L1 + D-SSIM + masked normal L1 + "
                    "normal TV + backward (colour and normal gradients: the blend backward's full chain) + Adam (train.py:266-331, 517-520)",
            "formulation": formulation}


def bench_iteration(sc, light, brdf_lut, gi, sh_degree, cams_t, view_dirs, gt_image, steps=40, warmup=5,
                    data_parallel=False, force=False, rank=0, world=1, geometry_cache=False) -> Dict:
    """bench.py's `iteration` field: complete iterations/s of the C-config workload on the fast path (three hipGraphs).
    data_parallel: Stage2Trainer.data_parallel() -- every rank trains on its own view, the stage-2 gradient set (materials
    and light) is summed over the ranks before the update; `iterations_per_s` then counts views (ranks x iterations)."""
    import dp
    dev = gt_image.device
    raw = raw_from_scene(sc, dev)
    base0 = light.base.detach().clone()
    tr = Stage2Trainer(raw, light, brdf_lut, gi, sh_degree, graphs=True, geometry_cache=geometry_cache)
    slab = None
    if data_parallel:
        slab = tr.data_parallel(force=force)
        slab.timing = True
    n = len(cams_t)
    if geometry_cache:
        # a training set that is revisited: eight views, every one recorded once during the warm-up
        n = min(n, 8)
        warmup = max(warmup, 2 * n + 4)  # every view recorded, then replayed once with its hit list recorded: three captures

    def run(i):
        v = dp.view_for(i, rank, world, n)
        return tr.iteration(cams_t[v], gt_image, view_dirs[v])
    dt, out = _dp_timed(run, steps, warmup, slab)
    whole = tr.stepper.whole is not None
    final_loss = float(out["loss"])
    del out
    extra = _dp_fields(slab, world, raw["xyz"].shape[0])
    if geometry_cache and tr.stepper.geom_cache is not None:
        c = tr.stepper.geom_cache
        extra["geometry_cache"] = dict(c.stats, views=n, bytes_per_view=int(sum(v.numel() * v.element_size() for v in next(iter(c.entries.values())).values())) if c.entries else 0,
                                       what="per view: tile lists (ranges, tile order, point list), the occlusion plane and the hit "
                                            "list of the indirect-light march are reused while the optimizer reports no change of a "
                                            "geometry bit (gigs_adam_step_watch): no binning, no SSAO march, SSR = a gather at the "
                                            "recorded hits; preprocess, blend, normal derivation, shade, loss, backward and update "
                                            "run every iteration")
    wsg = tr.stepper.whole
    if wsg is not None and wsg.go is not None and wsg.adam is not None and not geometry_cache and not data_parallel:
        # the update graph alone (Adam on the ten Gaussian groups and the light, clamp): an HBM-streaming launch -- parameter and
        # both moments read and rewritten, the gradient read where one exists -- against the 8 TB/s peak
        nbytes = sum(p.numel() * 4 * (6 + (1 if gr is not None else 0)) for _, _, p, gr in wsg.adam.entries)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(3):
            wsg.go.replay()
        a.record()
        for _ in range(10):
            wsg.go.replay()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b) / 10
        extra["update"] = dict(ms=round(ms, 4), adam_bytes=int(nbytes), achieved_GBs=round(nbytes / ms / 1e6, 1), hbm_peak_GBs=8000.0,
                               hbm_frac=round(nbytes / ms / 1e6 / 8000.0, 4),
                               groups_without_gradient_tensor=sum(1 for e in wsg.adam.entries if e[3] is None),
                               what="the third hipGraph replayed alone: gigs_adam_step_guarded on every group (a group whose "
                                    "gradient is a declared zero has no gradient tensor: g = 0) + clamp of the light")
    tr.close()
    with torch.no_grad():
        light.base.copy_(base0)  # bench.py's light is shared with the legs that follow
    return {"iterations_per_s": round(world / dt, 2), "ms_per_iteration": round(1e3 * dt, 3), "steps": steps,
            "final_loss": final_loss, **extra,
            "what": "activations + rasterizer + SSAO + build_mips + shade + SSR + L1 + lamb + masked BRDF TV + envmap TV + "
                    "backward + Adam (10 Gaussian groups + light) + clamp (train.py:247-523 without data loading / densification)",
            "formulation": "3 hipGraphs (fwd, bwd, update)" if whole else "eager rasterizer (dense scene / fallback), fused glue"}
