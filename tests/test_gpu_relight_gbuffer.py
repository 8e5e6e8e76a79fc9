"""The two seams of relight.py on the GPU: one G-buffer (relight.SplatGBuffer) serves every relighter's from_gbuffer and
is left as it was, and a mesh source (mesh_render.MeshGBuffer) in the plain relight.Relighter is mesh_render.MeshRelighter.
Everything is compared bit for bit: the launches are the same, only who issues them differs."""
import pytest
import torch

import scenes
from test_gpu_mesh_render import _relight_setup
from test_gpu_relight_multi import _case, bits_equal, cam_t, view_dirs

pytestmark = pytest.mark.gpu
LIT = ("render_rgb", "render_direct", "IRR")


def _tensors(b):
    return {k: v for k, v in b.items() if isinstance(v, torch.Tensor)}


def test_one_gbuffer_serves_every_relighter():
    """test_gpu_relight_multi.py's small case (176x144, 9000 Gaussians, 64^2 lights), K = 3."""
    import relight
    _, cam, _, lights, g = _case(3)
    gi = scenes.GI_DEFAULTS
    c, vd = cam_t(cam), view_dirs(cam)
    b = relight.SplatGBuffer(gi, 2)(c, g)
    keys, extra = list(b), dict(b["extra"])
    ptrs = {k: v.data_ptr() for k, v in _tensors(b).items()}
    held = {k: v.clone() for k, v in _tensors(b).items()}
    assert extra == {} and len(ptrs) == 13
    turntable = relight.TurntableRelighter(lights, gi, 2)
    for rl in [relight.Relighter(light, gi, 2) for light in lights] + [relight.MultiRelighter(lights, gi, 2), turntable]:
        got = rl.from_gbuffer(c, b, vd)
        if rl is turntable:
            assert turntable.last_hits is not None and turntable.last_hits > 0
        got = {k: got[k].clone() for k in LIT}
        want = rl(c, g, vd)
        for k in LIT:
            assert bits_equal(got[k], want[k]), (type(rl).__name__, k)  # the same bits: NaNs in the same places
        assert float(want["IRR"].nan_to_num().abs().max()) > 0 and float(want["render_rgb"].nan_to_num().max()) > 0
        rl.close()
    # nothing downstream wrote into the G-buffer or replaced a plane of it
    assert list(b) == keys and b["extra"] == extra
    assert {k: v.data_ptr() for k, v in _tensors(b).items()} == ptrs
    for k, v in held.items():
        assert torch.equal(b[k].view(torch.uint8), v.view(torch.uint8)), k


def test_a_mesh_source_in_the_plain_relighter():
    import mesh_render
    import relight
    rast, cam, vd, lights = _relight_setup()
    gi = scenes.GI_DEFAULTS
    want = {k: (v.clone() if isinstance(v, torch.Tensor) else v)
            for k, v in mesh_render.MeshRelighter(lights[0], gi)(cam, rast, vd).items()}
    got = relight.Relighter(lights[0], gi, 0, source=mesh_render.MeshGBuffer(gi))(cam, rast, vd)
    assert list(got) == list(want) and got["radii"] is None and want["radii"] is None
    for k in ("tri_id", "opacity_map", "albedo_map", "roughness_map", "metallic_map"):
        assert k in got, k
    for k, w in want.items():
        if w is not None:
            assert got[k].dtype == w.dtype and torch.equal(got[k].contiguous().view(torch.uint8),
                                                           w.contiguous().view(torch.uint8)), k
    assert int((got["tri_id"] >= 0).sum()) > 2000 and float(got["render_rgb"].nan_to_num().max()) > 0.2
