"""CPU: the register budget of the default screen-space marches as hipcc reports it.  gi.hip is compiled device-only with
gi-gs_amd/build.py's compiler and flags plus -Rpass-analysis=kernel-resource-usage, and the remarks of the two kernels the
training step launches -- ssr_kernel<(gigs::March)3, 0, 1> and ssao_kernel<(gigs::March)3>, the certified projective march
-- are held to what DESIGN.md section 5 (GI, item 7) states: six waves per SIMD each, at most 80 VGPRs, no scratch.  Compiler
remarks only: no instruction stream is read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSR = "ssr_kernelILNS_5MarchE3ELi0ELi1EEE"  # ssr_kernel<(gigs::March)3, 0, 1>
SSAO = "ssao_kernelILNS_5MarchE3EEE"        # ssao_kernel<(gigs::March)3>


def _load_build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("gigs_build", os.path.join(ROOT, "gi-gs_amd", "build.py"))
    bld = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bld)
    return bld


def _remarks(log):
    """{function name: {vgpr, scratch, occ}} as tools/kernel_resources.py reads them"""
    keys = (("vgpr", r" VGPRs"), ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"))
    out = {}
    for block in re.split(r"(?=remark: [^\n]*Function Name:)", log):
        m = re.search(r"Function Name: (\S+)", block)
        if not m:
            continue
        vals = {name: re.search(k + r": (\d+)", block) for name, k in keys}
        if all(vals.values()):
            out[m.group(1)] = {name: int(v.group(1)) for name, v in vals.items()}
    return out


def test_default_marches_run_six_waves_per_simd(tmp_path):
    bld = _load_build()
    if not (os.path.exists(bld.HIPCC) or shutil.which(bld.HIPCC)):
        pytest.skip("no hipcc")
    assert "--offload-arch=gfx950" in bld.FLAGS and "gi.hip" in bld.SOURCES
    cmd = [bld.HIPCC, *bld.FLAGS, "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
           os.path.join(bld.CSRC, "gi.hip"), "-o", str(tmp_path / "gi.out")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = _remarks(r.stderr)
    ssr = [v for k, v in found.items() if SSR in k]
    ssao = [v for k, v in found.items() if SSAO in k]
    assert len(ssr) == 1 and len(ssao) == 1, sorted(found)
    print("ssr_kernel<kProjCert, 0, 1>:", ssr[0], " ssao_kernel<kProjCert>:", ssao[0])
    assert ssr[0]["occ"] == 6 and ssr[0]["vgpr"] <= 80 and ssr[0]["scratch"] == 0, ssr[0]
    assert ssao[0]["occ"] == 6 and ssao[0]["vgpr"] <= 80 and ssao[0]["scratch"] == 0, ssao[0]
