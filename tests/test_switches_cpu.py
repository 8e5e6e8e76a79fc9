"""CPU: the Python-side A/B switches (gigs_lib.SWITCHES) live in the library context beside the gigs_options -- defaults
from the environment once, scoped per thread by options() / derive(), carried into a backward by with_forward_context --
and no module of the package reads the environment for them.  The library is loaded as in test_cabi.py; no GPU call."""
import os
import re
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gi-gs_amd")

NAMES = ("step_graph", "light_prefetch", "mip_chain", "spec_multi", "spec_prescaled", "cube_bwd_gather", "ssr_hit_list",
         "declared_grads", "split_sh", "fused_derive", "stage2_gather", "shade_post_fused")

CHILD = """
import os, sys
sys.path.insert(0, %r)
import gigs_lib
c = gigs_lib.current()
first = [n for n in gigs_lib.SWITCHES if not c.switch(n)]
for var in gigs_lib.SWITCHES.values():
    os.environ[var] = "0"
os.environ["GIGS_STEP_GRAPH"] = "1"
again = [n for n in gigs_lib.SWITCHES if not gigs_lib.current().switch(n)]
fresh = [n for n, on in zip(gigs_lib.SWITCHES, gigs_lib.default_switches()) if not on]
print("off:", ",".join(first), "|", ",".join(again), "|", ",".join(fresh))
""" % PKG


def _child(**env_vars):
    import gigs_lib
    env = {k: v for k, v in os.environ.items() if k not in gigs_lib.SWITCHES.values()}
    env.update(env_vars)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("off:")][-1]
    return [sorted(filter(None, part.strip().split(","))) for part in line[4:].split("|")]


def test_the_table_names_the_twelve_switches():
    import gigs_lib
    assert tuple(gigs_lib.SWITCHES) == NAMES
    assert gigs_lib.SWITCHES["declared_grads"] == "GIGS_MATERIALS_ONLY"
    assert all(v == "GIGS_" + k.upper() for k, v in gigs_lib.SWITCHES.items() if k != "declared_grads")
    assert not set(gigs_lib.SWITCHES) & set(gigs_lib.OPTION_NAMES)


def test_defaults_come_from_the_environment_once():
    """A switch is on iff its variable is unset or equals "1"; later writes to os.environ change nothing."""
    first, again, fresh = _child()
    assert first == [] and again == [] and fresh == []
    first, again, fresh = _child(GIGS_STEP_GRAPH="0", GIGS_MIP_CHAIN="yes")
    assert first == ["mip_chain", "step_graph"] and again == first and fresh == first


def test_scoping_interning_and_unknown_names():
    import gigs_lib
    base = gigs_lib.current()
    assert base.switches == gigs_lib.default_switches()
    on = base.switch("stage2_gather")
    with gigs_lib.options(stage2_gather=0, gi_march="exact") as c1:
        assert gigs_lib.current() is c1 and not c1.switch("stage2_gather") and c1.option("gi_march") == 0
        with gigs_lib.options(stage2_gather=1, split_sh=0) as c2:
            assert c2.switch("stage2_gather") and not c2.switch("split_sh") and c2.option("gi_march") == 0
        assert gigs_lib.current() is c1
        assert gigs_lib.current().derive(gi_march="exact", stage2_gather=False) is c1  # equal settings, same object
        assert c1.derive(stage2_gather=on, gi_march=base.option("gi_march")) is base
    assert gigs_lib.current() is base and base.switch("stage2_gather") == on
    for bad in ("stage2_gathr", "GIGS_STAGE2_GATHER", "materials_only_grads"):
        with pytest.raises(ValueError, match="stage2_gather") as e:  # the message names the valid ones
            base.derive(**{bad: 0})
        assert "gi_march" in str(e.value)
        with pytest.raises(ValueError):
            gigs_lib.options(**{bad: 0})
    with pytest.raises(ValueError):
        base.switch("nonsense")


def test_another_thread_sees_the_defaults():
    import gigs_lib
    seen = {}

    def worker():
        seen["switches"] = gigs_lib.current().switches
        seen["march"] = gigs_lib.current().option("gi_march")

    flipped = {n: int(not on) for n, on in zip(gigs_lib.SWITCHES, gigs_lib.default_switches())}
    with gigs_lib.options(gi_march="exact", **flipped) as c:
        assert c.switches == tuple(not on for on in gigs_lib.default_switches())
        t = threading.Thread(target=worker)
        t.start()
        t.join()
    assert seen["switches"] == gigs_lib.default_switches() and seen["march"] == gigs_lib.default_options()[
        gigs_lib.OPTION_NAMES.index("gi_march")]


def test_backward_runs_under_its_forwards_switches():
    import torch

    import gigs_lib
    seen = []

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.lib_ctx = gigs_lib.current()
            return x * 2.0

        @staticmethod
        @gigs_lib.with_forward_context
        def backward(ctx, g):
            seen.append(gigs_lib.current().switch("stage2_gather"))
            return g * 2.0

    x = torch.ones(3, requires_grad=True)
    with gigs_lib.options(stage2_gather=1):  # the surroundings of the backward: on, whatever the environment says
        with gigs_lib.options(stage2_gather=0):
            y = Probe.apply(x).sum()
        assert gigs_lib.current().switch("stage2_gather")
        y.backward()
    assert seen == [False] and torch.equal(x.grad, torch.full((3,), 2.0))


def _package_sources():
    for dirpath, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith(".py"):
                path = os.path.join(dirpath, f)
                yield os.path.relpath(path, PKG), open(path).read()


def test_no_module_reads_the_environment_for_a_switch():
    """The Python twin of test_cabi.py::test_no_launch_path_reads_the_environment: os.environ / os.getenv appear only in
    gigs_lib.py (library path, the switches' defaults) and build.py, and on the lines of the reference's DATA_SUBDIR and
    the table capacity GIGS_SPEC_TABLE_MAX_GB; every `.switch("...")` names a key of SWITCHES, and every key is read."""
    import gigs_lib
    read = set()
    for rel, txt in _package_sources():
        for no, line in enumerate(txt.splitlines(), 1):
            if rel not in ("gigs_lib.py", "build.py") and re.search(r"\b(environ|getenv|putenv)\b", line):
                assert "DATA_SUBDIR" in line or "GIGS_SPEC_TABLE_MAX_GB" in line, f"{rel}:{no}: {line.strip()}"
        if rel == "gigs_lib.py":
            continue
        calls = len(re.findall(r"\.switch\(", txt))
        literals = re.findall(r"""\.switch\(\s*["']([^"']*)["']\s*\)""", txt)
        assert calls == len(literals), f"{rel}: a .switch() call without a literal name"
        for name in literals:
            assert name in gigs_lib.SWITCHES, f"{rel}: unknown switch {name!r}"
        read.update(literals)
    assert read == set(gigs_lib.SWITCHES), sorted(set(gigs_lib.SWITCHES) - read)
