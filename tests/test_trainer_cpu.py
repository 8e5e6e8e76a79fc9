"""CPU: the host side of gi-gs_amd/trainer.py -- train.py's schedule, view order, command line and initialisation --
against tests/golden/ref_train_schedule.npz (make_train_schedule_golden.py) and restatements of the reference."""
import importlib
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
importlib.import_module("gi-gs_amd")
import trainer  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "ref_train_schedule.npz"))


def _args(settings):
    a = trainer.parse_args(["-s", "scene"])
    for k, v in settings.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("tag", ["readme", "short"])
def test_schedule_matches_reference(tag):
    st = json.loads(str(GOLD[f"{tag}_settings_json"]))
    a = _args(st)
    xyz_fn, brdf_fn = trainer.lr_functions(a, st["spatial_lr_scale"])
    lrs0 = trainer.initial_lrs(a, st["spatial_lr_scale"])
    N = GOLD[f"{tag}_lrs"].shape[0]
    got = {k: np.zeros(N, np.int64) for k in ("sh_up", "stage", "stats", "densify", "size_threshold", "reset", "light_step",
                                                "lr_update")}
    update = np.zeros((N, 10), np.uint8)
    lrs = np.zeros((N, 10))
    for i in range(1, N + 1):
        s = trainer.schedule(i, a)
        for k in got:
            v = s[k]
            got[k][i - 1] = (-1 if v is None else v) if k == "size_threshold" else int(v)
        update[i - 1] = [g in s["update"] for g in trainer.GROUPS]
        lr = trainer.learning_rates(i, lrs0, xyz_fn, brdf_fn)
        lrs[i - 1] = [lr[g] for g in trainer.GROUPS]
    for k, v in got.items():
        np.testing.assert_array_equal(v, GOLD[f"{tag}_{k}"], err_msg=k)
    np.testing.assert_array_equal(update, GOLD[f"{tag}_update"])
    np.testing.assert_array_equal(lrs, GOLD[f"{tag}_lrs"])
    assert got["densify"].sum() > 0 and got["reset"].sum() > 0


def test_view_order_is_the_reference_stack_pop():
    n, iters = 24, 500
    # restated from scene/__init__.py:96-97 and train.py:245-249 after safe_state's random.seed(0)
    random.seed(0)
    cams = list(range(n))
    random.shuffle(cams)
    want, stack = [], None
    for _ in range(iters):
        if not stack:
            stack = cams.copy()
        want.append(stack.pop(random.randint(0, len(stack) - 1)))
    rng = random.Random(0)
    order = trainer.shuffled_train_order(n, rng)
    seq = trainer.view_sequence(list(range(n)), iters, rng)
    assert [order[i] for i in seq] == want


def test_cli_defaults_equal_reference_parameter_groups():
    ref = json.loads(str(GOLD["arg_defaults_json"]))
    a = vars(trainer.parse_args(["-s", ""]))
    for k, v in ref.items():
        assert k in a, k
        assert a[k] == v and type(a[k]) is type(v), (k, a[k], v)
    # train.py's own flags keep their names and defaults; ignored ones parse
    b = trainer.parse_args(["-s", "x", "-m", "o", "-w", "-r", "2", "--ip", "1.2.3.4", "--port", "1", "--detect_anomaly",
                            "--debug_from", "3", "--iterations", "50"])
    assert b.white_background and b.resolution == 2 and b.model_path == "o"
    assert b.pbr_iteration == 30000 and b.normal_tv == 5.0 and b.start == 8 and b.degree == 3
    assert b.test_iterations[-1] == 50 and b.checkpoint_iterations == [30000, 50]
    assert b.init_points == 100_000 and b.sh_up_interval == 1000 and b.seed == 0 and b.hdri is None


def test_rejected_settings():
    with pytest.raises(ValueError, match="random_background"):
        trainer.validate(trainer.parse_args(["-s", "x", "--random_background"]))
    with pytest.raises(ValueError, match="stage 2"):
        trainer.validate(trainer.parse_args(["-s", "x", "--pbr_iteration", "1000", "--densify_until_iter", "1002"]))
    trainer.validate(trainer.parse_args(["-s", "x", "--pbr_iteration", "1000", "--densify_until_iter", "1001"]))


def test_init_from_cloud_matches_create_from_pcd():
    from oracle import knn_ref
    rng = np.random.RandomState(3)
    pts = rng.random((1000, 3)) * 2.6 - 1.3
    cols = rng.random((1000, 3))
    raw = trainer.init_from_cloud(pts, cols, 3, device="cpu",
                                  dist2=lambda p: torch.from_numpy(knn_ref.dist2_brute(p.numpy())))
    # scene/gaussian_model.py:272-317 restated in numpy
    sh = (cols.astype(np.float32) - 0.5) / 0.28209479177387814
    d2 = np.maximum(knn_ref.dist2_brute(pts.astype(np.float32)), 1e-7)
    want = dict(xyz=pts.astype(np.float32), f_dc=sh[:, None, :], f_rest=np.zeros((1000, 15, 3)),
                opacity=np.full((1000, 1), np.log(0.1 / 0.9)), normal=np.tile([0.0, 0.0, 1.0], (1000, 1)),
                albedo=np.ones((1000, 3)), roughness=np.ones((1000, 1)), metallic=np.ones((1000, 1)),
                scaling=np.repeat(np.log(np.sqrt(d2))[:, None], 3, 1), rotation=np.tile([1.0, 0, 0, 0], (1000, 1)))
    assert list(raw) == list(trainer.GROUPS)
    for k, v in want.items():
        t = raw[k]
        assert isinstance(t, torch.nn.Parameter) and t.dtype == torch.float32 and t.is_contiguous(), k
        np.testing.assert_allclose(t.detach().numpy(), v, rtol=1e-6, atol=1e-6, err_msg=k)
