"""GPU: the end-to-end trainer (gi-gs_amd/trainer.py) and the stepper options it needs -- densification statistics inside
the captured stage-1 iteration, iterations without the Gaussian update, one Adam across the stage switch, resume.

Every module run renders its own NeRF-synthetic style dataset into tmp_path (gi-gs_amd/synthetic_dataset.py: a teacher
scene shaded by this package's stage-2 path under scenes.synthetic_envmap, RGBA PNGs + transforms_{train,test}.json)."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

def make_dataset(root, **kw):
    import synthetic_dataset
    return synthetic_dataset.write_synthetic_dataset(root, **kw)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    import importlib
    importlib.import_module("gi-gs_amd")
    return make_dataset(str(tmp_path_factory.mktemp("scene")))


def _args(src, out, **kw):
    import trainer
    argv = ["-s", src, "-m", out, "--eval", "--indirect", "--metallic", "--start", "64", "--init_points", "6000",
            "--iterations", "1200", "--pbr_iteration", "900", "--densify_from_iter", "200", "--densify_until_iter", "800",
            "--densification_interval", "100", "--opacity_reset_interval", "600", "--sh_up_interval", "300",
            "--test_iterations", "1", "--save_iterations", "600", "--checkpoint_iterations", "1000"]
    args = trainer.parse_args(argv)
    for k, v in kw.items():
        setattr(args, k, v)
    return args


@pytest.fixture(scope="module")
def full_run(dataset, tmp_path_factory):
    import trainer
    out = str(tmp_path_factory.mktemp("run"))
    return trainer.train_scene(_args(dataset, out)), out


def test_end_to_end_run(full_run):
    import dataset_readers as dr
    import evaluate
    import pbr
    import pipeline
    import scene_io
    import scenes
    res, out = full_run
    assert res.iterations == 1200
    Ps = [p for _, p in res.points]
    assert len(set(Ps)) > 1, "densification never changed P"
    assert all(math.isfinite(loss) for _, loss in res.losses) and len(res.losses) == 120
    first, last = res.reports[0], res.reports[-1]
    assert first["iteration"] == 1 and last["iteration"] == 1200 and last["stage"] == 2
    gain = last["test"]["psnr"] - first["test"]["psnr"]
    assert gain > 8.0, (first["test"], last["test"])  # measured: 10.87 -> 23.71 dB (End-to-end training)
    for name in ("metrics.jsonl", "cfg_args", "chkpnt600.pth", "chkpnt1000.pth", "chkpnt1200.pth"):
        assert os.path.exists(os.path.join(out, name)), name
    with open(os.path.join(out, "metrics.jsonl")) as f:
        recs = [json.loads(line) for line in f]
    assert sum(r["kind"] == "report" for r in recs) == 2
    # the last checkpoint re-rendered through the evaluator gives the PSNR the trainer reported
    dev = torch.device("cuda:0")
    sc = scene_io.load_scene(os.path.join(out, "chkpnt1200.pth"))
    ck = scene_io.load_checkpoint(os.path.join(out, "chkpnt1200.pth"))
    light = pbr.CubemapLight(base_res=256, device=dev)
    light.load_state_dict({k: v.to(dev) for k, v in ck["cubemap"].items()})
    g = {k: torch.from_numpy(sc[k]).to(dev) for k in pipeline.RASTER_KEYS}
    info = dr.readNerfSyntheticInfo(scenes_path(out), False, True)
    ev = evaluate.NovelViewEvaluator(light, dict(scenes.GI_DEFAULTS, start=64), int(ck["gaussians"][0]), metallic=True)
    for ci in info["test_cameras"]:
        c = dr.camera_from_info(ci, device=dev)
        rays = pipeline.canonical_rays(c, dev)
        ev(c, g, pipeline.view_dirs_for(c, rays, dev), c["original_image"], c["gt_alpha_mask"])
    psnr = ev.results()["psnr_avg"]
    ev.close()
    assert abs(psnr - last["test"]["psnr"]) < 1e-3, (psnr, last["test"]["psnr"])
    print("test PSNR: iteration 1 %.3f dB, iteration 1200 %.3f dB; P %s" % (first["test"]["psnr"], last["test"]["psnr"], Ps))


def scenes_path(out):
    with open(os.path.join(out, "cfg_args")) as f:
        from argparse import Namespace  # noqa: F401  (cfg_args is a Namespace repr, as render.py reads it)
        return eval(f.read()).source_path


def _views(src, n, dev):
    import dataset_readers as dr
    info = dr.readNerfSyntheticInfo(src, False, True)
    cams = [dr.camera_from_info(c, device=dev) for c in info["train_cameras"][:n]]
    gts = [(c["original_image"] * c["gt_alpha_mask"]).contiguous() for c in cams]
    return cams, gts


def _raw(P, dev, seed=0):
    import dataset_readers as dr
    import trainer
    cloud = dr.random_init_cloud(P, rng=np.random.RandomState(seed))
    raw = trainer.init_from_cloud(cloud["points"] * 0.6, cloud["colors"], 1, dev)
    with torch.no_grad():
        raw["opacity"].fill_(1.0)
    return raw


def test_graphed_statistics_equal_eager(dataset):
    import densify
    import train_iteration as ti
    dev = torch.device("cuda:0")
    cams, gts = _views(dataset, 6, dev)
    gi = dict(__import__("scenes").GI_DEFAULTS, start=64)
    states = []
    for graphs in (True, False):
        raw = _raw(5000, dev)
        st = densify.DensifyState(raw["xyz"].shape[0], dev)
        tr = ti.Stage1Trainer(raw, gi, 1, graphs=graphs, densify_state=st)
        for i in range(20):  # no update: both runs see the same parameters, so radii and counts agree exactly
            tr.iteration(cams[i % 6], gts[i % 6], update=False)
            for p in tr.raw.values():
                p.grad = None
        torch.cuda.synchronize()
        if graphs:
            assert tr.stepper.whole is not None and tr.stepper.whole.gf is not None
        tr.close()
        states.append(st)
    a, b = states
    assert torch.equal(a.denom, b.denom) and float(a.denom.max()) > 0
    assert torch.equal(a.max_radii2D, b.max_radii2D)
    for x, y in ((a.xyz_gradient_accum, b.xyz_gradient_accum), (a.xyz_gradient_accum_abs, b.xyz_gradient_accum_abs)):
        torch.testing.assert_close(x, y, rtol=1e-3, atol=1e-7)


def test_densify_iteration_skips_update_and_reset_matches_torch_adam(dataset):
    import densify
    import train_iteration as ti
    dev = torch.device("cuda:0")
    cams, gts = _views(dataset, 4, dev)
    gi = dict(__import__("scenes").GI_DEFAULTS, start=64)
    raw = _raw(5000, dev)
    st = densify.DensifyState(raw["xyz"].shape[0], dev)
    tr = ti.Stage1Trainer(raw, gi, 1, graphs=True, densify_state=st)
    for i in range(5):
        tr.iteration(cams[i % 4], gts[i % 4])
    before = {k: v.detach().clone() for k, v in tr.raw.items()}
    moments = {k: {m: tr.optimizer.state[v][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k, v in tr.raw.items()}
    steps = {k: int(tr.optimizer.state[v]["step"]) for k, v in tr.raw.items()}
    tr.iteration(cams[1], gts[1], update=False)
    torch.cuda.synchronize()
    for k, v in tr.raw.items():  # nothing moved: no Adam in this iteration
        assert torch.equal(v.detach(), before[k]), k
        assert int(tr.optimizer.state[v]["step"]) == steps[k]
        assert torch.equal(tr.optimizer.state[v]["exp_avg"], moments[k]["exp_avg"]), k
        assert v.grad is not None
    grads = {k: v.grad.clone() for k, v in tr.raw.items()}
    # opacity reset alone: nine groups step with this iteration's gradients, opacity is only reset
    ref = {k: torch.nn.Parameter(before[k].clone()) for k in tr.raw}
    ref_opt = torch.optim.Adam([{"params": [ref[k]], "lr": g["lr"], "name": k} for k, g in
                                zip(tr.raw, tr.optimizer.param_groups)], lr=0.0, eps=1e-15)
    for k in tr.raw:
        ref_opt.state[ref[k]] = {"step": torch.tensor(float(steps[k])), "exp_avg": moments[k]["exp_avg"].clone(),
                                 "exp_avg_sq": moments[k]["exp_avg_sq"].clone()}
    new_opacity = densify.reset_opacity(tr.optimizer)
    tr.optimizer.step()
    for k in tr.raw:
        ref[k].grad = None if k == "opacity" else grads[k]
    ref_opt.step()
    for k, v in tr.raw.items():
        if k == "opacity":
            assert torch.equal(v.detach(), before[k])  # the old tensor: untouched; the group now holds the reset one
            assert new_opacity.grad is None and float(torch.sigmoid(new_opacity.detach()).max()) <= 0.01 + 1e-6
            continue
        torch.testing.assert_close(v.detach(), ref[k].detach(), rtol=1e-5, atol=1e-7)
        assert int(tr.optimizer.state[v]["step"]) == steps[k] + 1
    # a densify iteration: every row densify wrote is a copy of a pre-iteration row (nothing was updated in between); only
    # the positions and scales of new rows are re-sampled
    for p in tr.raw.values():
        p.grad = None
    tr.replace_parameters({g["name"]: g["params"][0] for g in tr.optimizer.param_groups})
    old = {k: v.detach().clone() for k, v in tr.raw.items()}
    tr.iteration(cams[2], gts[2], update=False)
    new, st2 = densify.densify_and_prune(tr.optimizer, tr.densify_state, 0.0002, 0.0, 3.0, None)
    assert new["xyz"].shape[0] > old["xyz"].shape[0]
    for k in ("f_dc", "opacity", "normal", "albedo", "rotation"):
        a, b = new[k].detach().reshape(new[k].shape[0], -1), old[k].reshape(old[k].shape[0], -1)
        for i in range(0, a.shape[0], 1024):  # every new row equals some old row, bit for bit
            assert bool((a[i:i + 1024, None, :] == b[None, :, :]).all(-1).any(1).all()), k
    tr.replace_parameters(new, densify_state=st2)
    tr.close()


def test_stage_switch_keeps_adam_state(dataset, tmp_path):
    import trainer
    args = _args(dataset, str(tmp_path), iterations=60, pbr_iteration=30, densify_until_iter=20, densify_from_iter=500,
                 test_iterations=[], save_iterations=[], checkpoint_iterations=[30, 31], init_points=3000)
    trainer.train_scene(args)
    import scene_io
    a = scene_io.load_checkpoint(os.path.join(str(tmp_path), "chkpnt30.pth"))
    b = scene_io.load_checkpoint(os.path.join(str(tmp_path), "chkpnt31.pth"))
    sa, sb = a["gaussians"][16]["state"], b["gaussians"][16]["state"]
    assert sorted(sa) == sorted(sb) and len(sa) == 10
    for i in sa:
        assert int(sb[i]["step"]) == int(sa[i]["step"]) + 1  # carried across, not restarted at 1
    # the stage-2 step moved the material moments from where stage 1 left them
    assert not torch.equal(sa[5]["exp_avg"], sb[5]["exp_avg"])
    # the light steps from pbr_iteration on, but at pbr_iteration (stage 1) it has no gradient: its first step is at 31
    assert len(a["light_optimizer"]["state"]) == 0 and int(b["light_optimizer"]["state"][0]["step"]) == 1


@pytest.mark.parametrize("at", [600, 1000])  # inside the stage-1 densify window / in stage 2
def test_resume_restores_state(dataset, full_run, tmp_path, at):
    import optim
    import pbr
    import scene_io
    import trainer
    res, out = full_run
    ck = os.path.join(out, "chkpnt%d.pth" % at)
    saved = scene_io.load_checkpoint(ck)
    g = saved["gaussians"]
    dev = torch.device("cuda:0")
    # what train_scene restores from (it calls restore_checkpoint), compared with the file bit for bit
    light = pbr.CubemapLight(base_res=256, device=dev)
    light_opt = optim.FusedAdam([{"name": "cubemap", "params": list(light.parameters()), "lr": 0.05}], lr=0.05)
    rs = trainer.restore_checkpoint(ck, dev, light, light_opt)
    assert rs.iteration == at and rs.active_sh_degree == g[0] == (3 if at == 1000 else 2)
    again = scene_io.capture(rs.active_sh_degree, rs.raw, rs.stats, rs.optimizer, rs.spatial_lr_scale)
    for k, (x, y) in enumerate(zip(again[1:16], g[1:16])):  # ten parameter tensors, max_radii2D and the four statistics
        assert x.is_cuda and torch.equal(x.detach().cpu(), y), k
    assert again[17] == g[17]
    got, want = again[16], g[16]
    assert [pg["lr"] for pg in got["param_groups"]] == [pg["lr"] for pg in want["param_groups"]]
    assert sorted(got["state"]) == sorted(want["state"]) and len(want["state"]) == 10
    for i, st in want["state"].items():
        assert int(got["state"][i]["step"]) == int(st["step"])
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(got["state"][i][m].cpu(), st[m]), (i, m)
    for k, v in saved["cubemap"].items():
        assert torch.equal(light.state_dict()[k].cpu(), v), k
    lo = light_opt.state_dict()
    assert sorted(lo["state"]) == sorted(saved["light_optimizer"]["state"])
    for i, st in saved["light_optimizer"]["state"].items():  # empty at 600: the light has not stepped in stage 1
        assert int(lo["state"][i]["step"]) == int(st["step"])
        for m in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(lo["state"][i][m].cpu(), st[m]), (i, m)
    assert (at == 1000) == bool(saved["light_optimizer"]["state"])
    del rs, light, light_opt, again
    # the resumed run starts from that state and reaches the end
    r2 = trainer.train_scene(_args(dataset, str(tmp_path), start_checkpoint=ck, test_iterations=[1200], checkpoint_iterations=[],
                                   save_iterations=[]))
    assert r2.start == dict(iteration=at, sh_degree=g[0], P=int(g[1].shape[0]), resumed=True)
    assert r2.iterations == 1200 and len(r2.losses) == (1200 - at) // 10
    assert all(math.isfinite(loss) for _, loss in r2.losses)
    if at == 600:  # the restored statistics, re-attached to the captured backward, drive the densify at 700
        assert len({p for _, p in r2.points}) > 1
    print("resume at %d: final test PSNR %.3f dB (uninterrupted %.3f)" % (at, r2.final_metrics["test"]["psnr"],
                                                                          res.final_metrics["test"]["psnr"]))
    assert abs(r2.final_metrics["test"]["psnr"] - res.final_metrics["test"]["psnr"]) < 0.5


def test_memory_returns_after_train_scene(dataset, tmp_path):
    import trainer
    kw = dict(iterations=40, pbr_iteration=20, densify_until_iter=15, densify_from_iter=5, densification_interval=10,
              test_iterations=[40], save_iterations=[], checkpoint_iterations=[], init_points=3000)
    trainer.train_scene(_args(dataset, str(tmp_path / "a"), **kw))  # process-wide caches (tables, LUTs) settle
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    trainer.train_scene(_args(dataset, str(tmp_path / "b"), **kw))
    torch.cuda.synchronize()
    assert abs(torch.cuda.memory_allocated() - m0) <= 1 << 20, (m0, torch.cuda.memory_allocated())
