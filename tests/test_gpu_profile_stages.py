"""GPU: the profile session's accounting.  The translation units that time the stages of a training iteration (api,
light_filter, cube_texture, shade, stage2, image_loss, adam, activations) and knn are exercised by three small cases,
and the {stage name: launches} dictionary of each has to equal the one recorded in tests/golden/profile_stages.json -- recorded once with the library as it was before the stage ids moved into
csrc/gigs_internal.h, so a stage that is re-labelled, lost or counted twice by a host-side change shows here.

Recording (GIGS_LIB = the library whose accounting is the reference):

    GIGS_LIB=/path/to/libgigs_hip.so python tests/test_gpu_profile_stages.py OUT.json
"""
import json
import math
import os

import numpy as np
import pytest
import torch  # ahead of gigs_lib, as in every GPU test module: libgigs_hip.so is loaded after torch

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "profile_stages.json")
DEV = "cuda:0"


def _second_call_profile(call):
    """{name: (ms, launches)} of the second of two calls: the first one builds what is built once (tables, plans)."""
    import gigs_lib
    call()
    torch.cuda.synchronize()
    with gigs_lib.profile() as prof:
        call()
    return prof.stages


def _stage2_inputs():
    import pbr
    import pipeline
    from helpers import small_scene
    sc, cam = small_scene(P=300, W=64, H=48)
    camt = {k: (torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    torch.manual_seed(5)
    light = pbr.CubemapLight(base_res=64, device=DEV)  # the smallest light with a level between its ends (pbr/light.py)
    gt = torch.rand(3, 48, 64, device=DEV)
    vd = pipeline.view_dirs_for(camt, pipeline.canonical_rays(cam, DEV), DEV)
    return sc, camt, light, pbr.get_brdf_lut().to(DEV), gt, vd


def case_stage2_step():
    """(a) one eager fused stage-2 step: rasterizer, SSAO / SSR, G-buffer post, light chain, shade, loss, both directions"""
    import pipeline
    import scenes
    from helpers import GAUSS_KEYS
    sc, camt, light, lut, gt, vd = _stage2_inputs()
    g = {k: torch.from_numpy(np.ascontiguousarray(sc[k])).to(DEV).requires_grad_(True) for k in GAUSS_KEYS}
    step = pipeline.Stage2Step(light, lut, scenes.GI_DEFAULTS, sc["sh_degree"], fused=True, graphs=False, metallic=True)

    def call():
        for t in list(g.values()) + [light.base]:
            t.grad = None
        step(camt, g, gt, vd)
    return _second_call_profile(call)


def case_stage2_iteration():
    """(b) one eager stage-2 training iteration: (a) plus activations, regularisers and the Adam steps"""
    import scenes
    import train_iteration
    sc, camt, light, lut, gt, vd = _stage2_inputs()
    raw = train_iteration.raw_from_scene(sc, DEV)
    with train_iteration.Stage2Trainer(raw, light, lut, scenes.GI_DEFAULTS, sc["sh_degree"], graphs=False) as tr:
        return _second_call_profile(lambda: tr.iteration(camt, gt, vd))


def case_dist2():
    """(c) simple_knn's distCUDA2"""
    from simple_knn._C import distCUDA2
    pts = torch.from_numpy(np.random.default_rng(7).normal(size=(300, 3)).astype(np.float32)).to(DEV)
    return _second_call_profile(lambda: distCUDA2(pts))


CASES = {"stage2_step": case_stage2_step, "stage2_iteration": case_stage2_iteration, "dist2": case_dist2}


@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_launches_match_the_recorded_accounting(case):
    stages = CASES[case]()
    expected = json.load(open(GOLDEN))["launches"][case]
    assert expected, "an empty record checks nothing"
    assert {name: n for name, (_, n) in stages.items()} == expected
    for name, (ms, _) in stages.items():
        assert math.isfinite(ms) and ms > 0.0, (name, ms)


def _record(path):
    import ctypes as C
    import gigs_lib
    gl = gigs_lib.lib()
    count = gl.gigs_profile_end((C.c_float * 1)(), (C.c_int * 1)(), 0)
    rec = {"library": "parent of the commit that added csrc/gigs_internal.h",
           "stages": [gl.gigs_profile_stage_name(i).decode() for i in range(count)],
           "launches": {name: {k: n for k, (_, n) in fn().items()} for name, fn in sorted(CASES.items())}}
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "gi-gs_amd")]
    _record(sys.argv[1])
