"""Shared cases for the per-Gaussian float64 checks of the rasterizer's backward (tests/test_backward_f64_cpu.py,
tests/test_gpu_backward_f64.py, tests/golden/make_backward_f64_bounds.py).  A plain module, numpy only.

A case is (scene, camera, background, pixel-gradient planes, options), built deterministically, and it DECLARES the minimum
population of every branch of the backward kernels it is there for (`Case.needs`); `populations()` measures them from the
bookkeeping of the float64 restatement (oracle/torch_ref.py) and `check_populations()` fails when a case has silently
stopped entering one of its branches.  The image is 72 x 40: the last tile column and the last tile row are half outside.

The metric (`row_errors`): for a gradient tensor and every Gaussian row i,  e_i = |got_i - ref_i|_inf / (|ref_i|_inf + m)
with m the median of |ref_j|_inf over the rows with a non-zero reference -- a per-row error with a typical-magnitude floor
that never looks at the tensor's peak.  Where the reference is an exact zero the result has to be one.
"""
import json
import os
import time

import numpy as np

import scenes

W, H = 72, 40
GX, GY = 5, 3
FOVX = 0.9
BG = (0.3, 0.1, 0.6)
MIN_MARGIN = 1e-4       # smallest relative distance of any (pixel, instance) decision to its threshold
BOUND_FACTOR = 4.0      # the HIP kernel may be this many times as far from float64 as the fp32 oracle is
BOUND_CAP = 1e-4        # no raised bound may exceed this
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backward_f64_bounds.json")

# result name (oracle.Rasterizer.backward / grad_sink) -> key of torch_ref.render_with_grads
TENSORS = dict(means3D="d_means3D", means2D="d_means2D", opacity="d_opacities", normal="d_normal", albedo="d_albedo",
               roughness="d_roughness", metallic="d_metallic", sh="d_shs", scales="d_scales", rotations="d_rotations",
               colors="d_colors", cov3D="d_cov3D")
PLANES = (("color", 3), ("opacity", 1), ("depth", 1), ("normal", 3), ("albedo", 3), ("roughness", 1), ("metallic", 1))
LIST_LENGTHS = {(0, 0): 1, (1, 0): 63, (2, 0): 64, (3, 0): 65, (0, 1): 127, (1, 1): 128, (2, 1): 129, (3, 1): 200}
RAGGED_TILES = {(4, 0): 5, (4, 1): 6, (4, 2): 4, (0, 2): 7, (2, 2): 5}  # half outside the image: x >= 72 or y >= 40


def camera():
    return scenes.look_at_camera((2.0, -3.0, 1.5), (0.0, 0.0, 0.0), W, H, FOVX)


class _Builder:
    """Places Gaussians by pixel position, view depth and footprint in pixels."""

    def __init__(self, cam, seed, sh_degree):
        self.cam, self.rng, self.deg = cam, np.random.default_rng(seed), sh_degree
        self.inv = np.linalg.inv(np.asarray(cam["viewmatrix"], np.float64))
        self.fx = W / (2.0 * cam["tanfovx"])
        self.rows, self.depth_slot = [], 0

    def world(self, px, py, z):
        xv = ((2.0 * px + 1.0) / W - 1.0) * self.cam["tanfovx"] * z
        yv = ((2.0 * py + 1.0) / H - 1.0) * self.cam["tanfovy"] * z
        return (np.array([xv, yv, z, 1.0]) @ self.inv)[:3]

    def add(self, px, py, z, sigma_px, opacity, qnorm=1.0, tag="", clamp_channels=0):
        rng = self.rng
        z = z + 1e-3 * self.depth_slot  # distinct depths: the sort order does not hang on a tie
        self.depth_slot += 1
        sig = np.broadcast_to(np.asarray(sigma_px, np.float64), (3,)) * z / self.fx
        q = rng.normal(size=4)
        q *= qnorm / np.linalg.norm(q)
        M = (self.deg + 1) ** 2
        rgb = rng.uniform(0.15, 0.95, size=3)
        rgb[:clamp_channels] = -0.35  # below zero whatever the view-dependent part adds: clamped at 0
        sh = np.zeros((M, 3))
        sh[0] = scenes.rgb2sh(rng.permutation(rgb))
        sh[1:] = rng.normal(0.0, 0.08, size=(M - 1, 3))
        nrm = rng.normal(size=3)
        self.rows.append(dict(means3D=self.world(px, py, z), scales=sig, rotations=q, opacities=[opacity], shs=sh,
                              normal=nrm / np.linalg.norm(nrm), albedo=rng.uniform(0.05, 0.95, 3),
                              roughness=[rng.uniform(0.05, 0.95)], metallic=[rng.uniform(0.05, 0.95)], tag=tag))

    def scene(self, shuffle):
        rows = self.rows
        if shuffle:
            rows = [rows[i] for i in self.rng.permutation(len(rows))]
        sc = {k: np.ascontiguousarray(np.stack([np.asarray(r[k], np.float64) for r in rows]), dtype=np.float32)
              for k in ("means3D", "scales", "rotations", "opacities", "shs", "normal", "albedo", "roughness", "metallic")}
        sc["sh_degree"] = self.deg
        return sc, [r["tag"] for r in rows]


def _list_geometry(seed):
    """Small Gaussians (3-sigma footprint inside one 16x16 tile) that give chosen tiles lists of exactly the lengths of
    LIST_LENGTHS: the backward walk's prologue (1), one chunk (63 / 64), the second in flight (65 / 127 / 128), the steady
    state and a short last chunk (129, 200); a few more sit in the visible half of the ragged tiles and reach the border."""
    b = _Builder(camera(), seed, 3)
    rng = b.rng
    for (tx, ty), n in LIST_LENGTHS.items():
        for k in range(n):
            px, py = 16 * tx + rng.uniform(3.2, 12.8), 16 * ty + rng.uniform(3.2, 12.8)
            op = rng.uniform(0.2, 0.9) if n < 100 else rng.uniform(0.04, 0.22)
            b.add(px, py, 3.0, rng.uniform(0.25, 0.5, size=3), op, tag="list", clamp_channels=(k % 4 if n >= 63 and k < 24 else 0))
    for (tx, ty), n in RAGGED_TILES.items():
        for k in range(n):
            px = 16 * tx + (rng.uniform(3.2, 6.6) if tx == GX - 1 else rng.uniform(3.2, 12.8))
            py = 16 * ty + (rng.uniform(3.2, 6.6) if ty == GY - 1 else rng.uniform(3.2, 12.8))
            b.add(px, py, 3.0, rng.uniform(0.25, 0.5, size=3), rng.uniform(0.3, 0.9), tag="ragged")
    return b.scene(shuffle=True)


def _rich_geometry(seed, sh_degree=3):
    """Everything the list cases keep out: an opaque stack that terminates pixels in front of further instances, opacities
    above the 0.99 cap centred on pixels, centres beyond 1.3 tan(fov) in x, in y and in both with the footprint on screen,
    needles, Gaussians far below the +0.3 low-pass, quaternions of norm 0.5 .. 2, and culled Gaussians (behind the 0.2 near
    plane; empty tile rectangle) interleaved with the visible ones inside one 256-Gaussian block."""
    b = _Builder(camera(), seed, sh_degree)
    rng = b.rng
    for k in range(12):
        b.add(24.3 + rng.uniform(-0.2, 0.2), 12.4 + rng.uniform(-0.2, 0.2), 2.0, 3.0, 0.97, tag="stack")
    for k in range(3):
        b.add(24.3 + rng.uniform(-0.6, 0.6), 12.4 + rng.uniform(-0.6, 0.6), 2.6, 0.3, 0.5, tag="behind")
    for k in range(10):
        px, py = 40 + 3 * (k % 5) + rng.uniform(-0.03, 0.03), 24 + 5 * (k // 5) + rng.uniform(-0.03, 0.03)
        b.add(px, py, 2.2, 1.0, (1.0 if k % 2 else 0.995), qnorm=rng.uniform(0.8, 1.25), tag="cap", clamp_channels=k % 4)
        # ... and right behind it a small one that sees the world through the capped pixel: T = 0.01 there, not 1 - alpha
        b.add(px + rng.uniform(-0.1, 0.1), py + rng.uniform(-0.1, 0.1), 2.25, 0.3, 0.6, tag="undercap")
    for px, py, tag in ((86, 18, "fov_x"), (-15, 25, "fov_x"), (30, 52, "fov_y"), (50, -12, "fov_y"), (86, 52, "fov_xy"),
                        (-15, -12, "fov_xy")):
        b.add(px + rng.uniform(-0.5, 0.5), py + rng.uniform(-0.5, 0.5), 1.0, rng.uniform(9.0, 11.0, size=3), 0.5, tag=tag)
    for k in range(8):
        b.add(rng.uniform(8, 64), rng.uniform(6, 34), 2.4, (1.2, 0.012, 0.4), rng.uniform(0.3, 0.9),
              qnorm=rng.uniform(0.7, 1.2), tag="needle")
    for k in range(10):
        b.add(rng.uniform(4, 68), rng.uniform(4, 36), 2.3, 0.02, rng.uniform(0.4, 0.95), qnorm=rng.uniform(0.5, 2.0), tag="tiny")
    for k in range(10):
        b.add(rng.uniform(10, 60), rng.uniform(5, 35), (0.1 if k % 2 else -1.0), 1.0, 0.8, tag="near")
    for k in range(10):
        b.add(300 + 10 * k, 200.0, 2.5, 0.5, 0.8, tag="norect")
    for k in range(60):
        b.add(rng.uniform(-2, 74), rng.uniform(-2, 42), 2.5, rng.uniform(0.6, 2.5, size=3), rng.uniform(0.1, 0.95),
              qnorm=rng.uniform(0.5, 2.0), tag="filler", clamp_channels=(k % 4 if k < 12 else 0))
    return b.scene(shuffle=True)


def _dense_planes(rng):
    return {k: rng.normal(size=(c, H, W)).astype(np.float32) for k, c in PLANES}


QUADRANT_KINDS = ("materials", "colour", "normal", "depth", "zero", "dense")
_KIND_PLANES = dict(materials=("albedo", "roughness", "metallic"), colour=("color", "opacity"), normal=("normal",),
                    depth=("depth",), zero=(), dense=tuple(k for k, _ in PLANES))
# the tiles with the long lists hold every kind side by side; the others draw theirs
_FIXED_QUADRANTS = {(3, 1): ("materials", "colour", "normal", "depth"), (2, 1): ("zero", "dense", "materials", "colour"),
                    (1, 1): ("normal", "zero", "dense", "depth"), (0, 1): ("dense", "zero", "colour", "materials")}


def _quadrant_planes(rng):
    """Planes that are non-zero only in chosen 8x8 quadrants (the blend backward switches its four reduction groups per
    quadrant), plus a normal gradient on the image border, which the reference zeroes."""
    pg = _dense_planes(rng)
    kinds = {}
    for ty in range(GY):
        for tx in range(GX):
            fixed = _FIXED_QUADRANTS.get((tx, ty))
            for q in range(4):
                kind = fixed[q] if fixed else QUADRANT_KINDS[int(rng.integers(len(QUADRANT_KINDS)))]
                x0, y0 = 16 * tx + 8 * (q & 1), 16 * ty + 8 * (q >> 1)
                if x0 >= W or y0 >= H:
                    continue
                kinds[(tx, ty, q)] = kind
                for k, _ in PLANES:
                    if k not in _KIND_PLANES[kind]:
                        pg[k][:, y0:y0 + 8, x0:x0 + 8] = 0
    edge = np.zeros((H, W), bool)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    pg["normal"][:, edge] = rng.normal(size=(3, int(edge.sum()))).astype(np.float32) + 3.0
    return pg, kinds


class Case:
    def __init__(self, name, scene, tags, planes, needs, scale_modifier=1.0, colors_precomp=None, cov3D_precomp=None,
                 quadrant_kinds=None):
        self.name, self.scene, self.tags, self.planes, self.needs = name, scene, np.asarray(tags), planes, needs
        self.cam, self.bg, self.scale_modifier = camera(), BG, scale_modifier
        self.colors_precomp, self.cov3D_precomp, self.quadrant_kinds = colors_precomp, cov3D_precomp, quadrant_kinds

    def forward_kwargs(self):
        """Arguments of helpers.oracle_forward beyond (scene, cam, bg)."""
        kw = dict(scale_modifier=self.scale_modifier)
        if self.colors_precomp is not None:
            kw.update(shs=None, colors_precomp=self.colors_precomp)
        if self.cov3D_precomp is not None:
            kw.update(scales=None, rotations=None, cov3D_precomp=self.cov3D_precomp)
        return kw


# seeds found on the CPU (search_seed): the float64 reference alone keeps every decision MIN_MARGIN away from its threshold
SEEDS = dict(lists=0, rich=3)

_LIST_NEEDS = dict(list_lengths_exact=1, sh_clamped_1=4, sh_clamped_2=4, sh_clamped_3=4, border=3, ragged=20)
_RICH_NEEDS = dict(cap_pairs=10, capped=8, terminated_pixels=8, behind_terminated=2, fov_x_only=2, fov_y_only=2, fov_both=2,
                   culled_near=10, culled_norect=10, undercap=8, needle=6, tiny=8, nonunit_quaternion=60, sh_clamped_1=3, sh_clamped_2=3,
                   sh_clamped_3=3)


def _cov3d_of(sc, scale_modifier):
    q = sc["rotations"].astype(np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    Mm = R * (scale_modifier * sc["scales"].astype(np.float64))[:, None, :]
    S = Mm @ Mm.transpose(0, 2, 1)
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1), np.float32)


def build(name):
    if name in ("lists", "quadrants", "matonly"):
        sc, tags = _list_geometry(SEEDS["lists"])
        rng = np.random.default_rng(100 + SEEDS["lists"])
        if name == "lists":
            return Case(name, sc, tags, _dense_planes(rng), dict(_LIST_NEEDS))
        if name == "quadrants":
            pg, kinds = _quadrant_planes(rng)
            needs = dict(list_lengths_exact=1, border=3, **{"quadrant_" + k: 2 for k in QUADRANT_KINDS})
            return Case(name, sc, tags, pg, needs, quadrant_kinds=kinds)
        pg = _dense_planes(rng)
        for k in ("color", "opacity", "depth", "normal"):
            pg[k][:] = 0
        return Case(name, sc, tags, pg, dict(list_lengths_exact=1, chunk_single=1, chunk_odd=4, chunk_even=4))
    if name in ("rich", "rich_lowdeg", "rich_colors", "rich_cov3d"):
        sc, tags = _rich_geometry(SEEDS["rich"])
        rng = np.random.default_rng(200 + SEEDS["rich"])
        pg = _dense_planes(rng)
        needs = dict(_RICH_NEEDS)
        kw = {}
        if name == "rich_lowdeg":
            sc["sh_degree"] = 1  # 16 coefficients allocated, degree 1 active: the rows above it get zeros
            needs.update(sh_rows_above_active=1, sh_clamped_1=0, sh_clamped_2=0, sh_clamped_3=0)
        if name == "rich_colors":
            kw["colors_precomp"] = rng.uniform(0.0, 1.0, size=(len(tags), 3)).astype(np.float32)
            needs.update(sh_clamped_1=0, sh_clamped_2=0, sh_clamped_3=0)
        if name == "rich_cov3d":
            kw["cov3D_precomp"] = _cov3d_of(sc, 0.8)  # what the quaternions and scales of `rich` give, handed in ready-made
            needs.update(nonunit_quaternion=0)
        return Case(name, sc, tags, pg, needs, scale_modifier=0.8, **kw)
    raise KeyError(name)


CASES = ("lists", "quadrants", "matonly", "rich", "rich_lowdeg", "rich_colors", "rich_cov3d")
GEOMETRY_RICH = "rich"


# ------------------------------------------------------------------------------------------
def reference(orc, case):
    """One oracle forward (binning, fp32 state) + the float64 restatement on its lists.  Returns (rasterizer, forward
    outputs, reference dict); the reference's CPU time is ref['seconds']."""
    from helpers import oracle_forward
    from oracle import torch_ref
    r, out = oracle_forward(orc, case.scene, case.cam, bg=case.bg, **case.forward_kwargs())
    t0 = time.perf_counter()
    ref = torch_ref.render_with_grads(case.scene, case.cam, np.asarray(case.bg), r.state("point_list"), r.state("ranges"),
                                      out["radii"] > 0, case.planes, scale_modifier=case.scale_modifier,
                                      colors_precomp=case.colors_precomp, cov3D_precomp=case.cov3D_precomp)
    ref["seconds"] = time.perf_counter() - t0
    ref["radii"] = out["radii"]
    ref["num_rendered"] = out["num_rendered"]
    return r, out, ref


def oracle_backward(r, case):
    pg = case.planes
    return r.backward(grad_color=pg["color"], grad_opacity=pg["opacity"], grad_depth=pg["depth"], grad_normal=pg["normal"],
                      grad_albedo=pg["albedo"], grad_roughness=pg["roughness"], grad_metallic=pg["metallic"])


def populations(case, ref):
    """What the case actually exercises, from the reference's bookkeeping."""
    bk, tags = ref["book"], case.tags
    vis = ref["radii"] > 0
    P = len(tags)
    lengths = np.asarray(bk["list_lengths"]).reshape(GY, GX)
    pop = dict(R=int(ref["num_rendered"]), longest_list=int(lengths.max()), margin=float(bk["margin"]),
               cap_pairs=int(bk["cap_pairs"]), capped=int(bk["capped"].sum()), terminated_pixels=int(bk["terminated_pixels"]),
               behind_terminated=int((bk["behind_terminated"] & (tags == "behind")).sum()))
    pop["list_lengths_exact"] = int(all(lengths[ty, tx] == n for (tx, ty), n in LIST_LENGTHS.items())
                                    and all(lengths[ty, tx] == n for (tx, ty), n in RAGGED_TILES.items()))
    got_colour = np.abs(ref["d_colors"]).max(axis=1) > 0
    nclamp = bk["sh_clamped"].sum(axis=1)
    for k in (1, 2, 3):
        pop[f"sh_clamped_{k}"] = int(((nclamp == k) & got_colour).sum())
    cx, cy = bk["fov_clamped_x"] & bk["contributes"], bk["fov_clamped_y"] & bk["contributes"]
    pop.update(fov_x_only=int((cx & ~cy).sum()), fov_y_only=int((cy & ~cx).sum()), fov_both=int((cx & cy).sum()))
    pop.update(culled_near=int((~vis & (tags == "near")).sum()), culled_norect=int((~vis & (tags == "norect")).sum()))
    pop["undercap"] = int((bk["contributes"] & (tags == "undercap")).sum())
    pop.update(needle=int((bk["contributes"] & (tags == "needle")).sum()), tiny=int((bk["contributes"] & (tags == "tiny")).sum()))
    qn = np.linalg.norm(case.scene["rotations"].astype(np.float64), axis=1)
    pop["nonunit_quaternion"] = int((bk["contributes"] & (np.abs(qn - 1.0) > 0.05)).sum()) if case.cov3D_precomp is None else 0
    pop["border"] = int(bk["on_border"].sum())
    pop["ragged"] = int((bk["contributes"] & (tags == "ragged")).sum())
    M = case.scene["shs"].shape[1]
    pop["sh_rows_above_active"] = int(M > (case.scene["sh_degree"] + 1) ** 2)
    # survivors of a (tile, quadrant, chunk of 64): the materials-only walk pairs them and has a remainder
    counts = np.asarray([s[3] for s in bk["survivors"]])
    pop.update(chunk_single=int((counts == 1).sum()), chunk_odd=int(((counts >= 3) & (counts % 2 == 1)).sum()),
               chunk_even=int(((counts >= 2) & (counts % 2 == 0)).sum()))
    if case.quadrant_kinds is not None:
        alive = {}
        for tile, q, _, n in bk["survivors"]:
            alive[(tile % GX, tile // GX, q)] = alive.get((tile % GX, tile // GX, q), 0) + n
        for kind in QUADRANT_KINDS:
            pop["quadrant_" + kind] = sum(1 for key, k in case.quadrant_kinds.items() if k == kind and alive.get(key, 0) > 0)
    return pop


def check_populations(case, ref):
    pop = populations(case, ref)
    short = {k: (pop[k], n) for k, n in case.needs.items() if pop[k] < n}
    assert not short, f"case {case.name} no longer exercises its branches (have, need): {short}"
    assert pop["margin"] >= MIN_MARGIN, f"case {case.name}: a decision is {pop['margin']:.2e} (relative) from its threshold"
    assert pop["R"] <= 3000, pop["R"]
    return pop


def branch_masks(case, ref):
    """Per-Gaussian masks by branch, for reports: the worst row of a tensor is named with the branch it sits in."""
    bk = ref["book"]
    vis = ref["radii"] > 0
    nclamp = bk["sh_clamped"].sum(axis=1)
    masks = dict(culled=~vis, behind_terminated=bk["behind_terminated"], capped=bk["capped"], sh_clamped=(nclamp > 0) & vis,
                 fov_clamped=(bk["fov_clamped_x"] | bk["fov_clamped_y"]), border=bk["on_border"])
    for tag in ("needle", "tiny", "stack", "ragged", "undercap"):
        masks[tag] = case.tags == tag
    rest = np.ones(len(case.tags), bool)
    for m in masks.values():
        rest &= ~m
    masks["plain"] = rest
    return masks


def _rows(a, P):
    return np.asarray(a, np.float64).reshape(P, -1)


def row_errors(got, ref_t):
    """e_i of the module docstring for one tensor; shape [P]."""
    P = ref_t.shape[0]
    g, r = _rows(got, P), _rows(ref_t, P)
    if r.shape[1] == 0:
        return np.zeros(P)
    rn = np.abs(r).max(axis=1)
    nz = rn[rn > 0]
    m = float(np.median(nz)) if nz.size else 1.0
    return np.abs(g - r).max(axis=1) / (rn + m)


def result_tensor(got, name):
    a = np.asarray(got[name])
    return a[:, :2] if name == "means2D" else a


def all_row_errors(got, ref):
    return {name: row_errors(result_tensor(got, name), ref[key]) for name, key in TENSORS.items() if name in got}


def exact_zero_violations(got, ref):
    """Elements whose reference is an exact zero (culled rows, rows only behind terminated pixels, rows above the active SH
    degree, clamped channels, planes without a gradient) and whose result is not."""
    bad = {}
    for name, key in TENSORS.items():
        if name not in got:
            continue
        P = ref[key].shape[0]
        g, r = _rows(result_tensor(got, name), P), _rows(ref[key], P)
        n = int(((r == 0) & (g != 0)).sum())
        if n:
            bad[name] = n
    return bad


def report(case, ref, errs, bounds):
    """Worst row per tensor and per branch, failing entries first."""
    masks = branch_masks(case, ref)
    lines = []
    for name, e in errs.items():
        for br, m in masks.items():
            if m.any() and e[m].max() > 0:
                i = int(np.flatnonzero(m)[np.argmax(e[m])])
                flag = "FAIL" if e[i] > bounds[name] else "ok  "
                lines.append((flag, f"{flag} {case.name}.{name} [{br}] row {i} ({case.tags[i]}): e = {e[i]:.3e} (bound {bounds[name]:.3e})"))
    lines.sort(key=lambda x: x[0] != "FAIL")
    return "\n".join(x[1] for x in lines)


def load_bounds():
    with open(BOUNDS_JSON) as f:
        return json.load(f)


def hip_bounds(recorded, case_name):
    """Per tensor: BOUND_FACTOR x the oracle's recorded worst e_i, unless the file records a raised factor (with its reason)."""
    rec = recorded["cases"][case_name]["oracle_worst"]
    out = {}
    for name, v in rec.items():
        raised = recorded.get("raised", {}).get(case_name, {}).get(name)
        out[name] = (raised["factor"] if raised else BOUND_FACTOR) * v
        if raised:
            assert out[name] <= BOUND_CAP, (case_name, name, out[name])
    return out


def search_seed(orc, which, tries=200):
    """Offline helper: the first seed whose cases all keep MIN_MARGIN (run on the CPU, result goes into SEEDS)."""
    names = [n for n in CASES if (n in ("lists", "quadrants", "matonly")) == (which == "lists")]
    for seed in range(tries):
        SEEDS[which] = seed
        try:
            for n in names[:1] if which == "lists" else names:
                case = build(n)
                check_populations(case, reference(orc, case)[2])
            return seed
        except AssertionError as ex:
            print(seed, str(ex)[:200])
    raise RuntimeError("no seed found")
