"""CPU tests (no GPU) of the net the screen-space GI kernels are checked with (tests/gi_cases.py, oracle/gi_ref.py): every march
case enters its branches with enough DECIDED rays, holds few undecided ones and hits enough; the C oracle -- an independent
fp32 statement of the same lines -- agrees with the float64 restatement on every pixel of occlusion, colour and abd within the
a-priori summation bound, pixels that hold undecided rays included, with an identical pattern of
non-finite values; A6, the median and the bilateral filter agree per pixel within the recorded figures, early-outs as exact
zeros; the committed figures are what the generator produces; and the net has teeth: each of sixteen deliberate errors of the
restatement moves a decided ray's outcome or a pixel by more than ten times its bound on the case that owns the branch."""
import os
import sys

import numpy as np
import pytest

import gi_cases as gc
from oracle import gi_ref as gr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_gi_f64_bounds as gen  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return gc.load_bounds()


@pytest.fixture(scope="module")
def references():
    memo = {}

    def get(name):
        if name not in memo:
            case, m = gc.build(name)
            memo[name] = (case, gc.reference(case, m))
        return memo[name]

    return get


def test_ray_table_is_the_oracles_ray_set(orc):
    """the table's size is the oracle's loop count, the zero-weight rays stand behind the live ones, the weights' fp32 sum in
    loop order is SSAO's nrSamples"""
    for delta, n, dead in ((0.0625, 512, 32), (0.125, 144, 16), (0.03125, 2080, 65)):
        t = gr.ray_table(delta)
        a, b = orc.gi_ray_counts(delta)
        assert (t["n"], t["n_dead"], t["n_live"]) == (a * b, dead, n - dead) == (n, dead, n - dead)
        assert np.all(t["w"][t["n_live"]:] == 0) and np.all(t["w"][:t["n_live"]] != 0)
        assert np.all(np.diff(t["loop_index"][:t["n_live"]]) > 0)
        s = np.float32(0)
        for w in t["w"][np.argsort(t["loop_index"])]:
            s = np.float32(s + np.float32(w))
        assert float(s) == t["sum_w"]


def test_cases_cover_the_settings_and_sizes():
    cases = [gc.build(n)[0] for n in gc.MARCH_CASES]
    sizes = {(c.W, c.H) for c in cases}
    assert {(1, 1), (5, 3), (37, 29), (48, 40), (64, 64), (80, 64)} <= sizes
    rays = {gr.ray_table(c.gi["delta"])["n"]: c for c in cases}
    assert set(rays) == {144, 512, 2080}
    assert all(c.W * c.H <= 15 for c in cases if gr.ray_table(c.gi["delta"])["n"] == 2080)
    assert any(c.gi == gc.GI_DEFAULTS for c in cases)
    assert any(c.gi["step"] == 12 for c in cases) and any(c.gi["step"] - c.gi["start"] > 60 for c in cases)
    assert any(c.gi["bias"] == 0 and c.gi["thick"] == 0 for c in cases) and any(c.gi["start"] == 0 for c in cases)
    big = [c for c in cases if (c.W, c.H) == (80, 64)]
    assert big and all(gr.ray_table(c.gi["delta"])["n"] == 144 for c in big)


@pytest.mark.parametrize("name", gc.MARCH_CASES)
def test_march_populations_and_the_c_oracle(orc, references, recorded, name):
    case, ref = references(name)
    pop = gc.check_populations(case, ref)  # branches, the undecided caps, the hit share
    print(name, f"{case.W} x {case.H}, {gr.ray_table(case.gi['delta'])['n']} rays:",
          {k: (round(v, 5) if isinstance(v, float) else v) for k, v in pop.items() if v})
    rec = recorded["march"][name]
    assert {k: pop[k] for k in gen.POP_KEYS} == rec["populations"], "regenerate the bounds"
    occ, col, abd = gc.oracle_march(orc, case)
    for k, got, b in (("occlusion", occ, "occ"), ("color", col, "color"), ("abd", abd, "abd")):
        e = gc.plane_errors(got, ref[b], ref[b + "_bound"])  # every pixel, the pixels that hold undecided rays included
        print(f"  {name}.{k}: C oracle worst |d| {e['worst_abs']:.3e}, {e['worst_ratio']:.3f} of the bound")
        assert e["violations"] == 0 and e["pattern"] == 0, (name, k, e)
        assert e["worst_abs"] <= rec["oracle_worst_abs"][k] and e["worst_ratio"] <= max(rec["oracle_worst_over_bound"][k], 1e-12)
    fr = ref["fresnel"]
    print(f"  {name}: Fresnel clamp arguments at least {np.nanmin(fr['ndv_dist'][ref['finite']]) if ref['finite'].any() else 0:.2e} / "
          f"{np.nanmin(fr['arg_dist'][ref['finite']]) if ref['finite'].any() else 0:.2e} from their thresholds")
    # the non-finite population: the oracle's conventions, value for value
    bad = ~ref["finite"]
    for got, want in ((occ, ref["occ"]), (col, ref["color"]), (abd, ref["abd"])):
        np.testing.assert_array_equal(np.asarray(got)[..., bad], np.asarray(want)[..., bad].astype(np.float32))
    # exact zeros / ones where no ray hit
    none = ref["finite"] & ~(ref["march"]["outcome"] == gr.HIT).any(1)
    assert np.all(occ[none] == 1.0) and np.all(col[:, none] == 0.0) and np.all(abd[:, none] == 0.0)
    if case.gi["start"] == 0 and case.gi["bias"] > 0:  # every ray hits its own pixel: fully occluded, to the bound
        assert np.all(occ[ref["finite"]] <= ref["occ_bound"][ref["finite"]])


def test_committed_bounds_are_the_generators(orc, recorded):
    orc.set_threads(1)
    try:
        fresh = gen.generate(orc, device=recorded.get("device"))
    finally:
        orc.set_threads(min(8, orc.max_threads()))

    def same(a, b, path):
        if isinstance(a, dict):
            assert set(a) == set(b), path
            for k in a:
                same(a[k], b[k], path + "/" + str(k))
        elif isinstance(a, float) and path.split("/")[1] != "device":
            assert abs(a - b) <= 0.02 * abs(b), (path, a, b)  # float64 sums may differ in the last digits between vector units
        else:
            assert a == b, (path, a, b)

    same(fresh, recorded, "")
    assert set(recorded["march"]) == set(gc.MARCH_CASES)


# mutation -> the march case that owns its branch
TEETH = [("lt_for_le", "equal_5x3"), ("bias_thick_swapped", "room_37x29"), ("continue_on_leaving", "room_37x29"),
         ("start_plus_1", "room_37x29"), ("step_minus_1_end", "room_37x29"), ("floor_for_round", "room_37x29"),
         ("w_for_w_minus_1", "room_37x29"), ("no_1e-7", "micro_37x29"), ("scale_once", "room_37x29"),
         ("radius_over_step_minus_1", "room_37x29"), ("weight_cos", "room_37x29"), ("ssr_over_sum_w", "room_37x29"),
         ("ssao_over_count", "room_37x29"), ("kd_without_metallic", "room_37x29"),
         ("lt_for_le", "start0_37x29"), ("start_plus_1", "step12_37x29"), ("step_minus_1_end", "long_5x3")]


def test_every_mutation_is_listed():
    assert {m for m, _ in TEETH} | {"a6_pad_1", "a6_centre_only"} == set(gr.MUTATIONS)


@pytest.mark.parametrize("mutation,name", TEETH)
def test_wrong_march_is_told_apart(references, mutation, name):
    """a march with one deliberate error moves a DECIDED ray's outcome, or a pixel by more than ten times its bound"""
    case, ref = references(name)
    wrong = gc.reference(case, mut=mutation)
    m0, m1 = ref["march"], wrong["march"]
    moved = ref["decided"] & ((m0["outcome"] != m1["outcome"]) | (m0["hit_pix"] != m1["hit_pix"]))
    fin = ref["finite"]
    worst = 0.0
    for k in ("occ", "color", "abd"):
        with np.errstate(all="ignore"):
            d = np.abs(np.asarray(wrong[k]) - np.asarray(ref[k]))[..., fin]
            b = np.asarray(ref[k + "_bound"])[..., fin]
            ok = np.isfinite(d) & (b > 0)
            worst = max(worst, float((d[ok] / b[ok]).max()) if ok.any() else 0.0)
    print(f"{mutation} on {name}: {int(moved.sum())} decided rays moved, worst pixel {worst:.3g} x its bound")
    if mutation == "lt_for_le" and name == "start0_37x29":
        assert not moved.any() and worst == 0.0  # bias > 0: the strict test decides the same -- only the equality window tells
        return
    assert moved.any() or worst > 10.0, (mutation, name)
    if mutation in ("weight_cos", "ssr_over_sum_w", "ssao_over_count", "kd_without_metallic"):
        assert not moved.any() and worst > 10.0  # errors of the sums, not of the march


# ---- A6, median, bilateral -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.normal_cases()))
def test_depth_to_normal_early_outs_and_the_c_oracle(orc, recorded, name):
    c = gc.normal_cases()[name]
    n64, p64, early, dist = gr.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], c["depth"])
    n32, p32 = orc.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], c["depth"])
    rec = recorded["normal"][name]
    assert {k: int((early == i).sum()) for i, k in enumerate(gr.EARLY)} == rec["early"]
    print(name, rec["early"], "closest depth to 0.01:", float(np.nanmin(dist)))
    for k, got, want in (("normal", n32, n64), ("depth_pos", p32, p64)):
        e = gc.plane_errors(got, want, np.full(want.shape, rec["comparator_worst"][k]))
        assert e["violations"] == 0 and e["pattern"] == 0, (name, k, e)
    assert np.all(n32[:, early != 0] == 0) and np.all(p32[:, early == 1] == 0)  # early-outs: exact zeros
    if name == "pad_45x38":
        assert rec["early"]["depth"] == 14 and rec["early"]["pad"] >= 12 * 25  # every pad position entered, on both sides
        assert early[4 + 7 * 4, 4 + 7 * 4] != 2 and early[4 + 7 * 4, 4 + 7 * 5] == 2  # exactly 0.01 passes, one ulp below does not
        for mut in ("a6_pad_1", "a6_centre_only"):
            _, _, e2, _ = gr.depth_to_normal(c["W"], c["H"], c["f"], c["f"], c["viewmatrix"], c["depth"], mut=mut)
            assert int((e2 != early).sum()) >= 32, mut
    if min(c["W"], c["H"]) < 3:
        assert rec["early"]["border"] == c["W"] * c["H"]


@pytest.mark.parametrize("name", list(gc.filter_cases()))
def test_filters_and_the_c_oracle(orc, recorded, name):
    x = gc.filter_cases()[name]
    rec = recorded["filters"][name]["comparator_worst"]
    med, tap, tied = gr.median3x3(x)
    np.testing.assert_array_equal(orc.median3x3(x), med.astype(np.float32))  # a selection: exact, NaNs included
    assert rec["median"] == 0.0
    if name == "distinct_37x29":
        assert not tied[:, 1:-1, 1:-1].any() and len(np.unique(tap[~tied])) == 9  # ties only among the padding's zeros; every tap chosen
    if name == "ties_11x13":
        assert tied.mean() > 0.5
    if name == "nan_10x9":
        assert int(np.isnan(med).sum()) == 9
    if "bilateral" in rec:
        b64 = gr.bilateral3x3(x)
        e = gc.plane_errors(orc.bilateral3x3(x), b64, np.full(b64.shape, rec["bilateral"]))
        assert e["violations"] == 0 and e["pattern"] == 0, (name, e)
        if name == "const_9x7":
            assert np.abs(b64 - 0.375).max() < 1e-15
