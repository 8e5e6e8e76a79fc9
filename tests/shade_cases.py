"""Shared cases for the per-pixel / per-texel float64 checks of the deferred shade (tests/test_shade_f64_cpu.py,
tests/test_gpu_shade_f64.py, tests/golden/make_shade_f64_bounds.py): csrc/shade.hip shade_pixel_n, shade_fwd_kernel,
shade_bwd_kernel, cube_taps, wave_dedup_add, run_add3.

A case is a small G-buffer, a light, upstream gradients and the entry points' options, built deterministically so that it
ENTERS the branches it is there for: it declares their minimum populations (`Case.needs`), `populations()` measures them from
the decisions the float64 restatement reports (oracle/torch_pbr_ref.shade, `details`) and `check_populations()` fails when
a case has silently stopped entering one.  Every decision of every pixel (cube face, bilinear tap cell on the levels it
uses, LUT cell, mip knots and level pair, the [0, 1] clamp, the sRGB knee) is at least MIN_MARGIN from its threshold, so that
float32, float64 and the kernel take the same side: pixels are re-drawn while building until the float64 margin is twice
that.  (The index of a tap that wraps to a neighbouring face needs no margin: it is found from a texel CENTRE pushed one
texel over the edge, whose coordinate on the neighbour lies odd * res / (2 res + 2) texels from the face centre -- never
within 1 / (2 res + 2) of a texel border.)

Directions are placed in the light's frame (the frame of cube_taps): to reflect into d, pick a normal n near d and set
v = 2 (n.d) n - d; `from_light` turns both into the G-buffer's frame.

The metric is backward_cases.row_errors: e_i = |got_i - ref_i|_inf / (|ref_i|_inf + median live row norm), rows = pixels
for per-pixel tensors and texels for the light gradients; no row is left out.  Where float64 is an exact zero the result
has to be one.  The bound of a (case, tensor) is BOUND_FACTOR x the worst e_i of an fp32 CPU evaluation of the same formulae
(tests/golden/shade_f64_bounds.json).  A recorded figure of 0 belongs to a tensor that is an exact zero in float64 (the
all-masked image, the levels one pixel does not reach): there the bound is 0 and the result has to be exactly 0.
"""
import json
import os

import numpy as np
import torch

import backward_cases as bc
from oracle import torch_pbr_ref as tp

MIN_MARGIN = 2e-4
BOUND_FACTOR = bc.BOUND_FACTOR
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_f64_bounds.json")
SPEC_RES5 = (256, 128, 64, 32, 16)
SPEC_RES3 = (64, 32, 16)
DIFFUSE_RES = 16
ROUGH_SCALE, ROUGH_BIAS = float(np.float32(0.96)), float(np.float32(0.04))  # as the kernel receives them
G_SCALE = 0.75
D_DARK = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])        # texels of order 1e-3 around it (light frame)
D_BRIGHT = np.array([1.0, 0.25, 0.35]) / np.linalg.norm([1.0, 0.25, 0.35])  # texels in [1.25, 1.4] around it
COS_PATCH = 0.94
FORWARD = ("render_rgb", "diffuse_rgb", "specular_rgb", "diffuse_light")
FORWARD_EXT = ("F0", "linear", "roughness_out")
PIXEL_GRADS = ("albedo", "roughness", "metallic")


def lut_np():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gi-gs_amd", "pbr", "brdf_256_256.bin")
    return np.fromfile(path, dtype=np.float32).reshape(256, 256, 2)


def unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


def from_light(d):
    """a direction of the light's frame in the G-buffer's: the inverse of the shade's (x, y, z) -> (-y, z, -x)"""
    d = np.asarray(d, np.float64)
    return np.stack([-d[..., 2], -d[..., 0], d[..., 1]], -1)


def face_dir(a, b, face):
    """the direction of face coordinates (a, b) in [-1, 1]^2 (u = (a + 1) / 2), light frame, normalised"""
    return unit([(1, -b, -a), (-1, -b, a), (a, 1, b), (a, -1, -b), (a, -b, 1), (-a, -b, -1)][face])


def make_light(spec_res, seed):
    rng = np.random.default_rng(seed)

    def level(r):
        tex = rng.uniform(0.0, 1.4, (6, r, r, 3))
        d = tp.texel_dirs(r).numpy().reshape(6, r, r, 3)
        dark, bright = d @ D_DARK > COS_PATCH, d @ D_BRIGHT > COS_PATCH
        tex[dark] = rng.uniform(0.2e-3, 1.2e-3, (int(dark.sum()), 3))
        tex[bright] = rng.uniform(1.25, 1.4, (int(bright.sum()), 3))
        return tex.astype(np.float32)

    return level(DIFFUSE_RES), [level(r) for r in spec_res]


def rough_for_level(lvl, L):
    """the roughness get_mip maps to `lvl` (0 <= lvl <= L - 1)"""
    return 0.08 + 0.42 * lvl / (L - 2) if lvl < L - 2 else 0.5 + 0.5 * (lvl - (L - 2))


def mip_knots(L):
    return [rough_for_level(float(k), L) for k in range(L)]


class Case:
    """g: numpy fp32 G-buffer ([H,W,*], mask bool [H,W,1]; occlusion / metallic may be None); grads: the four upstream planes
    (None = NULL); ext: None or a dict (the roughness remap and the backward extras, see _ext); skip: gradient outputs passed
    as NULL; planar: the [3,H,W] layout; forward_only: the case holds pixels ON a threshold, where only values are compared."""

    def __init__(self, name, g, tags, light, needs, tone=False, gamma=False, grads=None, ext=None, background=None,
                 planar=False, skip=(), forward_only=False, spec_res=SPEC_RES5):
        self.name, self.g, self.tags, self.needs = name, g, np.asarray(tags), needs
        self.diffuse, self.spec = light
        self.tone, self.gamma, self.grads, self.ext, self.background = tone, gamma, grads or {}, ext, background
        self.planar, self.skip, self.forward_only, self.spec_res = planar, tuple(skip), forward_only, spec_res
        self.H, self.W = g["mask"].shape[:2]

    @property
    def gradient_names(self):
        names = ["albedo", "roughness"] + (["metallic"] if self.g.get("metallic") is not None else [])
        names += ["diffuse"] + ["spec%d" % r for r in self.spec_res]
        return [n for n in names if n not in self.skip]

    @property
    def forward_names(self):
        return list(FORWARD) + (list(FORWARD_EXT) if self.ext else [])


# ---- pixels --------------------------------------------------------------------------------------
def _pixel(rng, nl, dl, rough, tag, albedo=None, occ=None, metal=None, mask=True):
    """one pixel whose normal is nl and whose reflected direction is dl (light frame)"""
    nl, dl = unit(nl), unit(dl)
    v = 2.0 * float(nl @ dl) * nl - dl
    return dict(normals=from_light(nl), view_dirs=from_light(v), roughness=[rough], tag=tag, mask=[mask],
                albedo=rng.uniform(0.05, 0.95, 3) if albedo is None else np.broadcast_to(albedo, (3,)),
                occlusion=[rng.uniform(0.3, 1.0) if occ is None else occ], metallic=[rng.uniform(0.05, 0.95) if metal is None else metal])


def _normal_near(rng, d, spread=0.25):
    while True:
        n = unit(d + spread * rng.normal(size=3))
        if n @ d > 0.5:
            return n


def _generic_dir(rng):
    return unit(rng.normal(size=3))


def _seam_uv(rng, res, kind):
    """face (u, v) within half a texel of an edge (kind 0..3: x low / x high / y low / y high) or of a corner (kind 4..7:
    2 * y_high + x_high) of a res^2 face; the free coordinate sits inside a texel cell"""
    near = lambda high: (1.0 - rng.uniform(0.3, 0.7) * 0.5 / res) if high else rng.uniform(0.3, 0.7) * 0.5 / res  # noqa: E731
    free = lambda: (rng.integers(1, res - 2) + rng.uniform(0.25, 0.75) + 0.5) / res  # noqa: E731
    if kind < 2:
        return near(kind == 1), free()
    if kind < 4:
        return free(), near(kind == 3)
    return near((kind - 4) & 1), near((kind - 4) >> 1)


def _seam_dir(rng, res, face, kind):
    u, v = _seam_uv(rng, res, kind)
    return face_dir(2.0 * u - 1.0, 2.0 * v - 1.0, face)


def _rough_for_role(rng, level, role, L):
    """a roughness that makes `level` the lower (role 0) or the upper (role 1) level of the blend"""
    if role == 0:
        return 1.02 if level == L - 1 else rough_for_level(level + rng.uniform(0.3, 0.6), L)
    if level == 0:
        return rng.uniform(0.02, 0.07)  # below the first knot: level 0 with its neighbour at weight 0
    return rough_for_level(level - rng.uniform(0.4, 0.7), L)


def _specular_seam(res_list, level, face, kind, role):
    def gen(rng):
        d = _seam_dir(rng, res_list[level], face, kind)
        return _pixel(rng, _normal_near(rng, d), d, _rough_for_role(rng, level, role, len(res_list)), "seam")
    return gen


def _diffuse_seam(face, kind):
    def gen(rng):
        n = _seam_dir(rng, DIFFUSE_RES, face, kind)
        return _pixel(rng, n, _normal_near(rng, n, 0.4), rng.uniform(0.1, 0.95), "dseam")
    return gen


def _interior(face):
    def gen(rng):
        d = face_dir(rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7), face)
        return _pixel(rng, _normal_near(rng, d), d, rng.uniform(0.02, 1.0), "interior")
    return gen


def _filler(rng):
    d = _generic_dir(rng)
    return _pixel(rng, _normal_near(rng, d, 0.5), d, rng.uniform(0.0, 1.05), "filler", mask=rng.uniform() > 0.1)


def _at_roughness(r, tag):
    def gen(rng):
        d = _generic_dir(rng)
        return _pixel(rng, _normal_near(rng, d), d, r(rng) if callable(r) else r, tag)
    return gen


def _patch(n_centre, d_centre, albedo, tag, rough=(0.1, 0.9)):
    """normal inside one patch of the light, reflected direction inside another (or a generic one: None)"""
    def gen(rng):
        n = unit(n_centre + 0.03 * rng.normal(size=3)) if n_centre is not None else None
        d = unit(d_centre + 0.03 * rng.normal(size=3)) if d_centre is not None else _generic_dir(rng)
        if n is None:
            n = _normal_near(rng, d)
        while n @ d < 0.2:  # the generic reflected direction has to be in front of the normal
            d = _generic_dir(rng)
        a = albedo(rng) if callable(albedo) else albedo
        return _pixel(rng, n, d, rng.uniform(*rough), tag, albedo=a, occ=rng.uniform(0.8, 1.0))
    return gen


def _back_facing(rng):
    d = _generic_dir(rng)  # n.v < 0: the reflected direction is -v, so v = -d
    while True:
        n = unit(d + 0.8 * rng.normal(size=3))
        if n @ d > 0.2:
            break
    p = _pixel(rng, n, d, rng.uniform(0.1, 0.9), "back")
    p["view_dirs"] = from_light(-d)
    return p


def _perpendicular(rng):
    v = _generic_dir(rng)
    n = unit(np.cross(v, rng.normal(size=3)))
    p = _pixel(rng, n, v, rng.uniform(0.1, 0.9), "perp")
    p["view_dirs"] = from_light(v)
    return p


def _head_on(rng):
    n = _generic_dir(rng)
    return _pixel(rng, n, n, rng.uniform(0.1, 0.9), "head_on")


def _zero_normal(rng):
    p = _filler(rng)
    p.update(normals=np.zeros(3), tag="zero_normal", mask=[True])
    return p


def _masked_out(rng):
    p = _filler(rng)
    p.update(tag="masked_out", mask=[False])
    return p


_KEYS = ("normals", "view_dirs", "albedo", "roughness", "occlusion", "metallic")


def _image(rows, H, W):
    assert len(rows) == H * W, (len(rows), H, W)
    g = {k: np.ascontiguousarray(np.stack([np.asarray(r[k], np.float64) for r in rows]).reshape(H, W, -1), np.float32)
         for k in _KEYS}
    g["mask"] = np.stack([np.asarray(r["mask"], bool) for r in rows]).reshape(H, W, 1)
    return g, [r["tag"] for r in rows]


def _build_image(gens, H, W, seed, margin_of, order=None):
    """Draw one pixel per generator (padding with fillers up to H * W), then re-draw every pixel whose float64 decision
    margin (margin_of(g) -> [H,W]) is below 2 * MIN_MARGIN.  order: pixel position of every generator (default: row-major)."""
    rng = np.random.default_rng(seed)
    gens = list(gens) + [_filler] * (H * W - len(gens))
    if order is not None:
        placed = [None] * (H * W)
        for gen, pos in zip(gens, order):
            placed[pos] = gen
        gens = placed
    rows = [gen(rng) for gen in gens]
    for _ in range(40):
        g, tags = _image(rows, H, W)
        bad = np.flatnonzero(~(margin_of(g).reshape(-1) >= 2.0 * MIN_MARGIN))
        if bad.size == 0:
            return g, tags
        for i in bad:
            rows[i] = gens[i](rng)
    raise RuntimeError("no margin-clean image after 40 rounds")


def _planes(rng, H, W, names=("g_render", "g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light")):
    full = {k: (rng.normal(size=(H, W, 3)) * (1.0 if k == "g_render" else 0.5)).astype(np.float32)
            for k in ("g_render", "g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light")}
    return {k: (v if k in names else None) for k, v in full.items()}


def _ext(rng, g, extras=True):
    H, W = g["mask"].shape[:2]
    e = dict(rough_scale=ROUGH_SCALE, rough_bias=ROUGH_BIAS)
    if extras:
        lamb = g["mask"][..., 0].astype(np.float32)
        e.update(mul_a=rng.normal(size=(H, W, 3)).astype(np.float32), mul_b=rng.uniform(0, 1, (H, W, 3)).astype(np.float32),
                 add_r=rng.normal(size=(H, W)).astype(np.float32), add_m=rng.normal(size=(H, W)).astype(np.float32),
                 g_scale=G_SCALE, lamb_mask=lamb, lamb_cnt=max(float(lamb.sum()), 1.0))
    return e


def _margin(g, light, configs):
    """the float64 decision margin per pixel, the smallest over `configs` = [(tone, gamma, remap)]"""
    lut = lut_np()
    out = None
    for tone, gamma, remap in configs:
        ext = dict(rough_scale=ROUGH_SCALE, rough_bias=ROUGH_BIAS) if remap else None
        m = tp.shade_with_grads(g, light[0], light[1], lut, {}, tone=tone, gamma=gamma, ext=ext)["details"]["margin"].numpy()
        out = m if out is None else np.minimum(out, m)
    return out


# ---- the cases -----------------------------------------------------------------------------------
SEAM_KINDS = 8
TCK = {"tck_t%dg%d" % (t, gm): (bool(t), bool(gm)) for t in (0, 1) for gm in (0, 1)}
OPTIONALS = ("opt_plain", "opt_no_metallic", "opt_no_occlusion_bg", "opt_only_render", "opt_no_render",
             "opt_no_d_metallic_d_diffuse", "opt_no_d_spec", "opt_ext_bare")
CASES = (("seams", "seams3", "levels", "levels_ext", "levels3") + tuple(TCK) + ("degenerate", "all_masked", "one_pixel")
         + OPTIONALS)
FORWARD_ONLY_CASES = ("knots", "knots3")
SEAM_CASES = ("seams", "seams3")
_memo = {}


def _seam_needs(res_list):
    needs = dict(wrap_diffuse=24, drop_diffuse=24, faces_interior=6)
    for l, r in enumerate(res_list):
        needs.update({f"wrap_{r}": 24, f"drop_{r}": 24, f"as_l0_{r}": 24})
        if l > 0:
            needs[f"as_l1_{r}"] = 24
    return needs


def _build_seams(name):
    res_list = SPEC_RES5 if name == "seams" else SPEC_RES3
    light = make_light(res_list, 5 if name == "seams" else 6)
    gens = [_specular_seam(res_list, l, f, k, role) for l in range(len(res_list)) for f in range(6) for k in range(SEAM_KINDS)
            for role in (0, 1)]
    gens += [_diffuse_seam(f, k) for f in range(6) for k in range(SEAM_KINDS)] + [_interior(f) for f in range(6) for _ in range(3)]
    H, W = (8, 96) if name == "seams" else (8, 56)
    g, tags = _build_image(gens, H, W, 11, lambda g: _margin(g, light, [(False, True, False)]))
    rng = np.random.default_rng(12)
    return Case(name, g, tags, light, _seam_needs(res_list), gamma=True, grads=_planes(rng, H, W), spec_res=res_list)


def _level_gens(L, remap):
    """roughness (as the shade uses it) on either side of every knot, below the first (slope 0), below the LUT's first row
    centre (row clamp), in the LUT's last row, and above 1; raw = (r - bias) / scale under the remap"""
    raw = (lambda r: (r - ROUGH_BIAS) / ROUGH_SCALE) if remap else (lambda r: r)
    gens = []
    for k in mip_knots(L):
        for off in (-0.012, -0.004, 0.004, 0.012):
            gens += [_at_roughness(raw(k + off), "knot_side")] * 4
    for r, tag in ((0.0012, "lut_first_row"), (0.0017, "lut_first_row"), (0.03, "flat_mip"), (0.06, "flat_mip"),
                   (0.9985, "lut_last_row"), (0.9993, "lut_last_row"), (1.02, "above_one"), (1.08, "above_one")):
        gens += [_at_roughness(raw(r), tag)] * 6
    gens += [_at_roughness(lambda rng: raw(rng.uniform(0.0, 1.0)), "any")] * 40
    return gens


def _build_levels(name):
    L, remap = (3 if name == "levels3" else 5), name == "levels_ext"
    res_list = SPEC_RES3 if L == 3 else SPEC_RES5
    light = make_light(res_list, 7)
    gens = _level_gens(L, remap)
    H, W = 8, (len(gens) + 7) // 8
    g, tags = _build_image(gens, H, W, 21, lambda g: _margin(g, light, [(False, False, remap)]))
    rng = np.random.default_rng(22)
    needs = dict(flat_mip=12, lut_first_row=12, lut_last_row=12, above_one=12, top_level_only=12,
                 **{f"l0_is_{l}": 8 for l in range(L)})
    return Case(name, g, tags, light, needs, grads=_planes(rng, H, W), ext=_ext(rng, g) if remap else None, spec_res=res_list)


def _build_knots(name):
    """pixels exactly on a knot of get_mip (as fp32 holds it): the level pair may differ between precisions, the value not"""
    L = 3 if name == "knots3" else 5
    res_list = SPEC_RES3 if L == 3 else SPEC_RES5
    light = make_light(res_list, 7)
    rng = np.random.default_rng(31)
    rows = [_at_roughness(k, "on_knot")(rng) for k in mip_knots(L) for _ in range(8)]
    H, W = 8, len(rows) // 8
    g, tags = _image(rows, H, W)
    return Case(name, g, tags, light, dict(on_knot=8 * L), forward_only=True, spec_res=res_list)


def _build_tck():
    """the same image for the four tone / gamma combinations: normal and reflected direction in the dark patch, the bright
    patch or anywhere, albedo small, ordinary or (for ACES, which reaches 1 at 7.24) large"""
    light = make_light(SPEC_RES5, 8)
    ordinary = lambda rng: rng.uniform(0.2, 0.95, 3)  # noqa: E731
    large = lambda rng: rng.uniform(7.0, 12.0, 3)  # noqa: E731
    mixed = lambda rng: np.where(rng.uniform(size=3) < 0.5, rng.uniform(0.2, 0.6, 3), rng.uniform(7.0, 12.0, 3))  # noqa: E731
    gens = []
    for nc, dc, alb, tag, n in ((D_DARK, D_DARK, ordinary, "dark_dark", 24), (D_DARK, D_BRIGHT, ordinary, "dark_bright", 16),
                                (D_BRIGHT, D_DARK, ordinary, "bright_dark", 16), (D_BRIGHT, D_BRIGHT, ordinary, "bright_bright", 24),
                                (D_BRIGHT, D_BRIGHT, large, "bright_large", 16), (D_BRIGHT, None, mixed, "bright_mixed", 32),
                                (None, None, ordinary, "anywhere", 32), (D_DARK, None, ordinary, "dark_any", 16)):
        gens += [_patch(nc, dc, alb, tag)] * n
    H, W = 8, (len(gens) + 15) // 8
    combos = [(t, gm, False) for t, gm in TCK.values()]
    g, tags = _build_image(gens, H, W, 41, lambda g: _margin(g, light, combos))
    return g, tags, light


_TCK_NEEDS = dict({f"{what}_{side}_{c}": 4 for what in ("knee_render", "knee_diffuse", "knee_specular")
                   for side in ("below", "above") for c in "rgb"},
                  **{f"clamp_{side}_{c}": 4 for side in ("below", "above") for c in "rgb"})


def _build_degenerate():
    """37 x 45: neither a multiple of 8 nor of 32.  The last tile row (y >= 32) and the last tile column (x >= 32) are
    partial tiles, x >= 40 and y >= 32 partial 8 x 8 waves: seam pixels go there, the degenerate pixels anywhere."""
    H, W = 37, 45
    light = make_light(SPEC_RES5, 9)
    special = ([_back_facing] * 24 + [_perpendicular] * 16 + [_head_on] * 16 + [_zero_normal] * 16 + [_masked_out] * 40)
    seams = [_specular_seam(SPEC_RES5, l, f, k, role) for l in range(5) for f in range(6) for k in (0, 3, 5, 6) for role in (0, 1)]
    seams += [_diffuse_seam(f, k) for f in range(6) for k in (1, 2, 4, 7)]
    partial = [y * W + x for y in range(H) for x in range(W) if x >= 32 or y >= 32]
    rest = [y * W + x for y in range(H) for x in range(W) if x < 32 and y < 32]
    rs = np.random.default_rng(50)
    partial = [partial[i] for i in rs.permutation(len(partial))]
    assert len(seams) <= len(partial)
    order = partial[:len(seams)] + [rest[i] for i in rs.permutation(len(rest))] + partial[len(seams):]
    gens = seams + special
    g, tags = _build_image(gens, H, W, 51, lambda g: _margin(g, light, [(True, True, False)]), order=order)
    rng = np.random.default_rng(52)
    needs = dict(back_facing=20, perpendicular=12, head_on=12, zero_normal_inside=12, masked_out=40, masked_out_with_gradient=40,
                 seams_in_partial_tiles=200, wrapped_in_partial_tiles=100, dropped_in_partial_tiles=50, ragged=1)
    return Case("degenerate", g, tags, light, needs, tone=True, gamma=True, grads=_planes(rng, H, W))


def _build_small(name):
    light = make_light(SPEC_RES5, 10)
    H, W = (1, 1) if name == "one_pixel" else (9, 13)
    g, tags = _build_image([], H, W, 61, lambda g: _margin(g, light, [(False, True, False)]))
    rng = np.random.default_rng(62)
    if name == "one_pixel":
        g["mask"][:] = True
        return Case(name, g, tags, light, dict(pixels=1), gamma=True, grads=_planes(rng, H, W))
    g["mask"][:] = False
    return Case(name, g, tags, light, dict(masked_out=H * W, everything_zero=1), gamma=True, grads=_planes(rng, H, W, ("g_render",)))


def _build_optionals():
    light = make_light(SPEC_RES5, 13)
    H, W = 12, 20
    gens = [_specular_seam(SPEC_RES5, l, f, k, 0) for l in range(5) for f in (0, 3, 4) for k in (1, 6)] + [_zero_normal] * 4
    g, tags = _build_image(gens, H, W, 71, lambda g: _margin(g, light, [(True, True, False), (True, True, True),
                                                                         (False, False, False), (False, False, True)]))
    return g, tags, light


def _optional_case(name, g, tags, light):
    H, W = g["mask"].shape[:2]
    rng = np.random.default_rng(72)
    planes, ext, bare = _planes(rng, H, W), _ext(rng, g), _ext(rng, g, extras=False)
    bgd = rng.uniform(0, 1, (H, W, 3)).astype(np.float32)
    none = lambda key: {k: (None if k == key else v) for k, v in g.items()}  # noqa: E731
    only = lambda *names: {k: (v if k in names else None) for k, v in planes.items()}  # noqa: E731
    kw = dict(
        opt_plain=dict(g=g, grads=planes, tone=True, gamma=True),
        opt_no_metallic=dict(g=none("metallic"), grads=planes, gamma=True),
        opt_no_occlusion_bg=dict(g=none("occlusion"), grads=planes, ext=ext, background=bgd, tone=True, gamma=True),
        opt_only_render=dict(g=g, grads=only("g_render"), ext=ext, planar=True, tone=True, gamma=True),
        opt_no_render=dict(g=g, grads=only("g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light"), ext=ext, planar=True),
        opt_no_d_metallic_d_diffuse=dict(g=g, grads=planes, skip=("metallic", "diffuse"), tone=True, gamma=True),
        opt_no_d_spec=dict(g=g, grads=planes, ext=ext, skip=("spec128", "spec16")),
        opt_ext_bare=dict(g=g, grads=only("g_render", "g_diffuse_rgb", "g_diffuse_light"), ext=bare, planar=True, gamma=True),
    )[name]
    return Case(name, kw.pop("g"), tags, light, dict(pixels=H * W, zero_normal_inside=4, wrapped=20), **kw)


def build(name):
    if name in SEAM_CASES:
        return _build_seams(name)
    if name in ("levels", "levels_ext", "levels3"):
        return _build_levels(name)
    if name in FORWARD_ONLY_CASES:
        return _build_knots(name)
    if name in TCK:
        if "tck" not in _memo:
            _memo["tck"] = _build_tck()
        g, tags, light = _memo["tck"]
        H, W = g["mask"].shape[:2]
        tone, gamma = TCK[name]
        # the image is shared by the four combinations; the sRGB knee is only exercised (and only required) with gamma on
        needs = {k: v for k, v in _TCK_NEEDS.items() if gamma or not k.startswith("knee_")}
        return Case(name, g, tags, light, needs, tone=tone, gamma=gamma, grads=_planes(np.random.default_rng(42), H, W))
    if name == "degenerate":
        return _build_degenerate()
    if name in ("all_masked", "one_pixel"):
        return _build_small(name)
    if name in OPTIONALS:
        if "opt" not in _memo:
            _memo["opt"] = _build_optionals()
        return _optional_case(name, *_memo["opt"])
    raise KeyError(name)


# ---- evaluation ----------------------------------------------------------------------------------
def reference(case, dtype=torch.float64, mut=()):
    """the restatement's forward and backward of the case in `dtype` -> the dict of torch_pbr_ref.shade_with_grads"""
    return tp.shade_with_grads(case.g, case.diffuse, case.spec, lut_np(), case.grads, tone=case.tone, gamma=case.gamma,
                               ext=case.ext, dtype=dtype, mut=mut, background=case.background)


def roughness_used(case):
    """the roughness plane the shade works from, formed in fp32 as a caller without the fused remap would"""
    r = case.g["roughness"]
    return (r * np.float32(ROUGH_SCALE) + np.float32(ROUGH_BIAS)).astype(np.float32) if case.ext else r


def srgb_to_linear32(x):
    x = np.asarray(x, np.float32)
    hi = ((np.maximum(x, np.float32(0.04045)) + np.float32(0.055)) / np.float32(1.055)) ** np.float32(2.4)
    return np.where(x <= np.float32(0.04045), np.float32(25.0 / 323.0) * x, hi).astype(np.float32)


def oracle_forward(orc, case):
    """the fp32 comparator of the forward: oracle/pbr_oracle.cpp, plus the ext outputs in numpy fp32"""
    g = case.g
    out = orc.shade_fwd(g["normals"], g["view_dirs"], g["albedo"], roughness_used(case), g["mask"], g.get("occlusion"),
                        g.get("metallic"), case.background, case.diffuse, case.spec, lut_np(), tone=case.tone, gamma=case.gamma)
    if case.ext:
        m = g.get("metallic")
        one, f04 = np.float32(1.0), np.float32(0.04)
        out["F0"] = (np.full_like(g["albedo"], f04) if m is None else ((one - m) * f04 + g["albedo"] * m)).astype(np.float32)
        out["linear"] = srgb_to_linear32(out["render_rgb"])
        out["roughness_out"] = roughness_used(case)
    return out


def forward_reference(case, ref):
    out = {k: ref[k] for k in FORWARD}
    if case.ext:
        out["F0"] = ref["details"]["F0"].to(torch.float64).numpy()
        out["linear"] = tp.srgb_to_linear(torch.from_numpy(ref["render_rgb"])).numpy()
        out["roughness_out"] = ref["roughness_used"]
    return out


def gradient_tensors(case, res):
    """a result of `reference` (or any dict with d_albedo ... d_spec) by the names of Case.gradient_names"""
    out = dict(albedo=res["d_albedo"], roughness=res["d_roughness"], metallic=res["d_metallic"], diffuse=res["d_diffuse"])
    out.update({"spec%d" % r: d for r, d in zip(case.spec_res, res["d_spec"])})
    return {k: out[k] for k in case.gradient_names}


def _as_rows(name, a):
    a = np.asarray(a, np.float64)
    return a.reshape(-1, 3) if a.ndim >= 3 and a.shape[-1] == 3 else a.reshape(-1, 1)


def row_errors(name, got, ref):
    """e_i of the module docstring: rows are pixels, or texels for the light gradients"""
    return bc.row_errors(_as_rows(name, got), _as_rows(name, ref))


def exact_zero_violations(got, ref):
    """elements whose float64 reference is an exact zero and whose result is not, per tensor"""
    bad = {}
    for k, r in ref.items():
        n = int(((np.asarray(r) == 0) & (np.asarray(got[k]).reshape(np.shape(r)) != 0)).sum())
        if n:
            bad[k] = n
    return bad


def all_row_errors(got, ref):
    return {k: row_errors(k, np.asarray(got[k]).reshape(np.shape(r)), r) for k, r in ref.items()}


def decisions(details):
    """the discrete decisions of every pixel as one integer array: faces, tap indices of the diffuse lookup and of the two
    levels used, the level pair and the LUT cell"""
    l0, l1 = details["l0"], details["l1"]
    idx = torch.stack([i["idx"] for i in details["spec"]], 0)
    pick = lambda l: torch.gather(idx, 0, l[None, ..., None].expand(1, *l.shape, 4))[0]  # noqa: E731
    lut = details["lut"]
    cols = [details["diffuse"]["face"][..., None], details["spec"][0]["face"][..., None], details["diffuse"]["idx"], pick(l0),
            pick(l1), l0[..., None], l1[..., None], lut["x0"][..., None], lut["y0"][..., None], lut["x1"][..., None],
            lut["y1"][..., None]]
    return torch.cat(cols, -1).numpy()


# ---- populations ---------------------------------------------------------------------------------
def _pairs(face, code, sel):
    """distinct (face, code) among the selected (pixel, tap) entries with code >= 0"""
    f = np.broadcast_to(face[..., None] if code.ndim > face.ndim else face, code.shape)
    ok = sel & (code >= 0)
    return len(set(zip(f[ok].tolist(), code[ok].tolist())))


def populations(case, ref):
    det = ref["details"]
    n = lambda t: t.numpy()  # noqa: E731
    l0, l1 = n(det["l0"]), n(det["l1"])
    tags, H, W = case.tags.reshape(case.H, case.W), case.H, case.W
    mask = case.g["mask"][..., 0]
    pop = dict(pixels=H * W, margin=float(np.min(n(det["margin"]))) if not case.forward_only else 0.0)
    dif = det["diffuse"]
    everyone = np.ones((H, W), bool)
    pop["wrap_diffuse"] = _pairs(n(dif["face"]), n(dif["edge"]), everyone[..., None])
    pop["drop_diffuse"] = _pairs(n(dif["face"]), n(dif["corner"]), everyone)
    wrapped_any, dropped_any = n(dif["wrapped"]).any(-1), n(dif["dropped"]).copy()
    for l, r in enumerate(case.spec_res):
        s = det["spec"][l]
        as0, as1 = l0 == l, (l1 == l) & (l1 != l0)
        used = as0 | as1
        pop[f"wrap_{r}"] = _pairs(n(s["face"]), n(s["edge"]), used[..., None])
        pop[f"drop_{r}"] = _pairs(n(s["face"]), n(s["corner"]), used)
        seam = n(s["wrapped"]).any(-1) | n(s["dropped"])
        pop[f"as_l0_{r}"], pop[f"as_l1_{r}"] = int((as0 & seam).sum()), int((as1 & seam).sum())
        pop[f"l0_is_{l}"] = int(as0.sum())
        wrapped_any |= used & n(s["wrapped"]).any(-1)
        dropped_any |= used & n(s["dropped"])
    pop["wrapped"] = int(wrapped_any.sum())
    pop["faces_interior"] = len(set(n(det["spec"][0]["face"])[tags == "interior"].tolist()))
    r = n(det["roughness"])
    lut = det["lut"]
    pop.update(flat_mip=int((r < tp.MIP_MINR).sum()), above_one=int((r > 1.0).sum()), top_level_only=int((l0 == l1).sum()),
               lut_first_row=int((n(lut["row_clamped"]) & (r < 0.01)).sum()), lut_last_row=int((n(lut["row_clamped"]) & (r > 0.99)).sum()),
               on_knot=int((tags == "on_knot").sum()))
    pre, (a_render, a_dif, a_spec) = n(det["pre_clamp"]), [n(x) for x in det["srgb_args"]]
    for c, ch in enumerate("rgb"):
        pop[f"clamp_below_{ch}"], pop[f"clamp_above_{ch}"] = int((mask & (pre[..., c] < 1)).sum()), int((mask & (pre[..., c] > 1)).sum())
        for what, a, where in (("render", a_render, mask), ("diffuse", a_dif, everyone), ("specular", a_spec, everyone)):
            pop[f"knee_{what}_below_{ch}"] = int((where & (a[..., c] <= tp.SRGB_KNEE)).sum())
            pop[f"knee_{what}_above_{ch}"] = int((where & (a[..., c] > tp.SRGB_KNEE)).sum())
    ndv = (case.g["normals"].astype(np.float64) * case.g["view_dirs"]).sum(-1)
    zero_n = ~(case.g["normals"] != 0).any(-1)
    pop.update(back_facing=int(((ndv < -0.05) & ~zero_n).sum()), perpendicular=int(((np.abs(ndv) < 1e-6) & ~zero_n).sum()),
               head_on=int((ndv > 1 - 1e-6).sum()), zero_normal_inside=int((zero_n & mask).sum()), masked_out=int((~mask).sum()))
    flows = np.zeros((H, W), bool)
    for k in ("g_diffuse_rgb", "g_specular_rgb", "g_diffuse_light"):
        if case.grads.get(k) is not None:
            flows |= (case.grads[k] != 0).any(-1)
    pop["masked_out_with_gradient"] = int((~mask & flows).sum())
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    partial = ((xx >= 32 * (W // 32)) & (W % 32 != 0)) | ((yy >= 32 * (H // 32)) & (H % 32 != 0))
    is_seam = (tags == "seam") | (tags == "dseam")
    pop.update(seams_in_partial_tiles=int((partial & is_seam).sum()), wrapped_in_partial_tiles=int((partial & wrapped_any).sum()),
               dropped_in_partial_tiles=int((partial & dropped_any).sum()), ragged=int(H % 8 != 0 and W % 8 != 0 and H % 32 != 0 and W % 32 != 0))
    grads = gradient_tensors(case, ref) if not case.forward_only else {}
    pop["everything_zero"] = int(all(not np.any(v) for v in grads.values()) and not np.any(ref["render_rgb"]))
    return pop


def check_populations(case, ref):
    pop = populations(case, ref)
    short = {k: (pop[k], n) for k, n in case.needs.items() if pop[k] < n}
    assert not short, f"case {case.name} no longer exercises its branches (have, need): {short}"
    if not case.forward_only:
        assert pop["margin"] >= MIN_MARGIN, f"case {case.name}: a decision is {pop['margin']:.2e} from its threshold"
    return pop


# ---- gigs_cube_taps ------------------------------------------------------------------------------
def seam_taps():
    """res -> (dirs fp32 [n,3], dict): the reflected directions of the `seams` case (as an fp32 caller forms them) whose
    float64 tap coordinates at that resolution keep MIN_MARGIN, with float64's taps (idx, w: -1 / 0 where a tap is dropped),
    the float32 evaluation's worst weight difference, and how many directions wrap / drop a tap."""
    if "taps" in _memo:
        return _memo["taps"]
    g = build("seams").g
    n, v = g["normals"].reshape(-1, 3), g["view_dirs"].reshape(-1, 3)
    ref = (np.float32(2.0) * np.maximum((n * v).sum(-1, keepdims=True), np.float32(0.0)) * n - v).astype(np.float32)
    rt = np.ascontiguousarray(np.stack([-ref[:, 1], ref[:, 2], -ref[:, 0]], -1), np.float32)
    out = {}
    for res in SPEC_RES5:
        info = {}
        tp.cube_taps(res, tp.to64(rt), info)
        face = info["face"].numpy()
        a = np.sort(np.abs(rt.astype(np.float64)), -1)
        keep = (info["margin"].numpy() >= MIN_MARGIN) & ((a[:, 2] - a[:, 1]) / a[:, 2] >= MIN_MARGIN)
        d = np.ascontiguousarray(rt[keep])
        info = {}
        idx, w = tp.cube_taps(res, tp.to64(d), info)
        idx32, w32 = tp.cube_taps(res, tp.as_dtype(d, torch.float32))
        assert torch.equal(idx32, idx), res
        wrapped, dropped = info["wrapped"].numpy(), info["dropped"].numpy()
        edges = _pairs(face[keep], info["edge"].numpy(), np.ones_like(wrapped))
        corners = _pairs(face[keep], info["corner"].numpy(), np.ones_like(dropped))
        assert edges == 24 and corners == 24, (res, edges, corners)
        out[res] = (d, dict(idx=idx.numpy(), w=w.numpy(), weight_worst=float((w32.double() - w).abs().max()),
                            directions=int(keep.sum()), wrapped=int(wrapped.any(-1).sum()), dropped=int(dropped.sum())))
    _memo["taps"] = out
    return out


# ---- bounds --------------------------------------------------------------------------------------
def load_bounds():
    with open(BOUNDS_JSON) as f:
        return json.load(f)


def hip_bounds(recorded, case_name):
    """per tensor: BOUND_FACTOR x the fp32 comparator's recorded worst e_i"""
    return {k: BOUND_FACTOR * v for k, v in recorded["cases"][case_name]["comparator_worst"].items()}


def comparator_worst(orc, case, ref=None):
    """the worst e_i of the fp32 comparators against float64, per tensor: the C oracle for the forward planes, the float32
    evaluation of the restatement for the gradients.  Also asserts what the bounds rest on: exact zeros where float64 has
    them and, on every pixel, float64's decisions."""
    ref = ref or reference(case)
    fwd_ref = forward_reference(case, ref)
    fwd = oracle_forward(orc, case)
    assert not exact_zero_violations(fwd, fwd_ref), case.name
    worst = {k: float(e.max()) for k, e in all_row_errors(fwd, fwd_ref).items()}
    if not case.forward_only:
        f32 = reference(case, dtype=torch.float32)
        assert np.array_equal(decisions(f32["details"]), decisions(ref["details"])), case.name
        g_ref, g32 = gradient_tensors(case, ref), gradient_tensors(case, f32)
        # (no exact-zero demand on this comparator: where a LUT row is clamped autograd sums +a and -a of the two equal
        # rows in an order that leaves a rounding residue in fp32; the kernel differences the two texels first)
        worst.update({k: float(e.max()) for k, e in all_row_errors(g32, g_ref).items()})
    return worst
