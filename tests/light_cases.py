"""Shared cases for the per-texel float64 checks of the cubemap light filters (tests/test_light_f64_cpu.py,
tests/test_gpu_light_f64.py, tests/golden/make_light_f64_bounds.py): csrc/light_filter.hip -- the GGX bounds, the table-free
GGX pre-filter, the table-driven one (raw, normalised, pre-divided, sparse), the diffuse filter -- and pbr.light.cubemap_mip.

A level is (res, roughness) at energy cutoff 0.99.  Its per-face AABBs are DISCRETE STRUCTURE and come from the C oracle
(oracle/pbr_oracle.cpp orc_specular_bounds, the reference's corner-only tile cull restated), as in
oracle/torch_pbr_ref.bounds_mask; everything else is float64: texel directions, solid angles, pair weights
    w(o, i) = max(L.V, 0) D_ggx(V.H) area(i) / 4,   accepted iff  i in AABB_o  and  L.V >= cutoff
(the cutoff and the roughness are the float32 values both fp32 evaluations receive).  The reference is WINDOWED: it
enumerates each output's AABB candidates (table order: output-major, faces in order, row-major) and evaluates them in chunks;
the dense [out, in] form of torch_pbr_ref needs 100 s at res 64.

    forward      rgbw[o]  = sum_{i accepted by o} w(o, i) (tex[i], 1);   normalised: rgb / wsum, NaN where nothing is accepted
    backward     g_in[i]  = sum_{o accepting i} g[o] w(o, i)             -- the TRANSPOSE, over the outputs whose window
                                                                            accepts i, never over i's own window
    normalised   g_in[i]  = sum_{o accepting i} g[o] / wsum[o] w(o, i)   (the weights do not depend on the cubemap)
`backward(..., form="gather")` is the sum over i's OWN window (the defect the suite exists to catch: the accepted set is not
symmetric where the tile cull drops in-cone texels); the other `mut` names are further seeded defects for the teeth tests.

Each level declares in `needs` what it is there for; `check_populations()` measures it from the structure and fails when a
level has stopped providing it.

The metric is backward_cases.row_errors per texel: |got - ref|_inf / (|ref|_inf + median row magnitude).  The bound of a
tensor is BOUND_FACTOR x the worst row error of the fp32 comparator (the C oracle) against float64 on the same input
(tests/golden/light_f64_bounds.json): both are fp32 evaluations of one formula.  Where float64 is an exact zero the result
has to be one; result buffers start as NaN, so every texel has to be written.  A recorded figure below ROUND_OFF = 2^-24 is
taken as 2^-24: a result stored in fp32 is no closer to float64 than half an ulp of the row's largest element, and a comparator
that lands below that (single-candidate windows: w / w = 1) does so by luck.

Undecided pairs.  A pair with |L.V - cutoff| <= UNDECIDED (1e-6: a dozen fp32 roundings of a unit dot product) may fall either
way in fp32.  A texel whose sum holds such pairs gets its bound widened by the summed magnitude of their contributions
(`slack`, same row normalisation); every other texel keeps the plain bound.  At most CAP_UNDECIDED of a level's texels may be
widened, in every tensor: `judge` asserts it.  Through rgb / wsum an undecided pair of output o would move EVERY term of o
in the normalised backward, i.e. widen o's whole window (41 % of the texels at (32, 0.22), 90 % at (64, 0.22)); so the
gradients of the normalised backward are exact zeros on the outputs that hold an undecided pair (`zero_undecided_outputs`,
1 - 3 % of a level's outputs) and nothing spreads.  Those outputs' pairs are checked by the raw backward, which has no wsum.
"""
import json
import os

import numpy as np

from backward_cases import row_errors  # noqa: F401  (the metric: imported, not copied)
from oracle import torch_pbr_ref as tp

F32 = np.float32
CUTOFF = 0.99
BOUND_FACTOR = 4.0
UNDECIDED = 1e-6
CAP_UNDECIDED = 0.05
ROUND_OFF = 2.0 ** -24  # half an ulp of a result stored in fp32
K_U = 4  # candidates per lane and iteration of specular_apply_body
TILE, LDS_TILE = 16, 32
BOUNDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "light_f64_bounds.json")

# name -> (res, roughness, needs).  needs: asym (True: asymmetric entries > 0, False: = 0), empty (windows without candidates),
# single (single-candidate windows), empty_faces, tiles (more than one bounds tile per face), ragged (6 res^2 no multiple
# of 8), straddle (lane widths whose batch kLanes kU the candidate counts lie on both sides of).
LEVELS = {
    "16_1.0": (16, 1.0, dict(asym=False, empty_faces=True)),       # 16-lane groups by default, five or six faces
    "32_0.5": (32, 0.5, dict(asym=False, tiles=True)),             # 64-lane groups, 2 x 2 bounds tiles per face
    "32_0.22": (32, 0.22, dict(asym=False, tiles=True, empty_faces=True, straddle=(8, 16))),  # 8-lane groups
    "64_0.22": (64, 0.22, dict(asym=False, tiles=True, straddle=(64,))),
    "64_0.08": (64, 0.08, dict(asym=False, tiles=True)),           # ~3 candidates per texel: ill-conditioned weights
    "16_0.22": (16, 0.22, dict(asym=True, empty=True)),
    "9_0.3": (9, 0.3, dict(asym=True, empty=True, ragged=True)),
    "7_0.4": (7, 0.4, dict(asym=True, ragged=True, straddle=(8,))),
    "9_0.5": (9, 0.5, dict(asym=True, ragged=True, empty_faces=True)),   # few asymmetric entries, wide windows
    "5_0.2": (5, 0.2, dict(asym=False, empty=True, single=True, ragged=True)),
    "16_0.08": (16, 0.08, dict(asym=False, empty=True, single=True)),
}
SYMMETRIC = [k for k, v in LEVELS.items() if not v[2]["asym"]]
ASYMMETRIC = [k for k, v in LEVELS.items() if v[2]["asym"]]
SPARSE_ONLY = {"64_0.36": (64, 0.36)}  # the sparse backward's level with several tiles per face: sparse gradients only


def ndf_cutoff(roughness, cutoff=CUTOFF):
    """The cosine both fp32 evaluations receive: the oracle's restatement of the reference's ndf cutoff (independent of the
    library; the GPU tests assert that the library's value rounds to the same float32), rounded to float32."""
    from oracle.stage2_ref import ndf_cutoff as restated
    return float(F32(restated(roughness, cutoff)))


def texel(res, face, y, x):
    return (face * res + y) * res + x


class Level:
    """The float64 structure of one level.  Pairs are kept for the outputs in `outputs` (default: all): po, pi (output and
    input texel of each AABB candidate, table order), dot, core = max(dot, 0) D / 4 (symmetric in the pair), acc, und, last
    (the last candidate of its face rectangle)."""

    def __init__(self, orc, res, rough, outputs=None, name=None):
        self.name, self.res, self.rough, self.T = name or f"{res}_{rough}", res, float(F32(rough)), 6 * res * res
        self.rough_arg = rough
        self.cc = ndf_cutoff(rough)
        self.bounds32 = orc.specular_bounds(res, self.cc)
        b = self.bounds32.reshape(self.T, 6, 4).astype(np.int64)
        self.b = b
        w = np.where((b[..., 0] <= b[..., 1]) & (b[..., 2] <= b[..., 3]), b[..., 1] - b[..., 0] + 1, 0)
        h = np.where(w > 0, b[..., 3] - b[..., 2] + 1, 0)
        self.face_counts = w * h
        self.counts = self.face_counts.sum(1)
        self.d = tp.texel_dirs(res).numpy()
        self.area = tp.pixel_areas(res).numpy().copy()
        sel = np.arange(self.T) if outputs is None else np.unique(np.asarray(outputs, np.int64))
        self.outputs = sel
        cnt = self.face_counts[sel].reshape(-1)
        starts = np.cumsum(cnt) - cnt
        rep = np.repeat(np.arange(cnt.size), cnt)
        local = np.arange(int(cnt.sum())) - starts[rep]
        wd = np.maximum(w[sel].reshape(-1), 1)[rep]
        o, s = sel[rep // 6], rep % 6
        yy = local // wd
        self.po = o.astype(np.int32)
        self.pi = ((s * res + b[sel][:, :, 2].reshape(-1)[rep] + yy) * res + b[sel][:, :, 0].reshape(-1)[rep] + local - yy * wd).astype(np.int32)
        self.last = local == cnt[rep] - 1
        n = self.po.size
        self.dot, self.core = np.empty(n), np.empty(n)
        a2 = self.rough ** 4
        for c0 in range(0, n, 1 << 21):
            sl = slice(c0, c0 + (1 << 21))
            V, L = self.d[self.po[sl]], self.d[self.pi[sl]]
            dot = (V * L).sum(1)
            Hh = V + L
            Hh /= np.maximum(np.linalg.norm(Hh, axis=1, keepdims=True), 1e-30)
            c = np.clip((V * Hh).sum(1), 0.0, 1.0)
            dd = (c * a2 - c) * c + 1.0
            self.dot[sl], self.core[sl] = dot, np.maximum(dot, 0.0) * (a2 / (dd * dd * np.pi)) / 4.0
        self.acc = self.dot >= self.cc
        self.und = np.abs(self.dot - self.cc) <= UNDECIDED

    # ---- sums ------------------------------------------------------------------------------------------------------
    def _sum(self, rows, terms, keep):
        out = np.zeros((self.T, terms.shape[1]))
        for ch in range(terms.shape[1]):
            out[:, ch] = np.bincount(rows[keep], terms[keep, ch], minlength=self.T)
        return out

    def _keep(self, mut):
        return self.acc & ~self.last if "drop_last_candidate_of_face" in mut else self.acc

    def weights(self, mut=()):
        """w(o, i) per pair (area of the input texel)."""
        return self.core * self.area[self.po if "area_of_wrong_texel" in mut else self.pi]

    def forward(self, tex, mut=()):
        """tex [T, 3] -> (rgbw [T, 4], slack [T])."""
        tex = np.asarray(tex, np.float64).reshape(self.T, 3)
        w = self.weights(mut)
        terms = np.concatenate([tex[self.pi] * w[:, None], w[:, None]], 1)
        out = self._sum(self.po, terms, self._keep(mut))
        slack = np.bincount(self.po[self.und], np.abs(terms[self.und]).max(1), minlength=self.T)
        return out, slack

    def forward_norm(self, tex):
        """-> (rgb / wsum [T, 3], NaN where nothing is accepted; slack [T]): an undecided pair moves rgb by w |tex| and
        wsum by w, hence the quotient by at most w (|tex| + |rgb / wsum|) / (wsum - w)."""
        tex = np.asarray(tex, np.float64).reshape(self.T, 3)
        rgbw, _ = self.forward(tex)
        with np.errstate(all="ignore"):
            out = rgbw[:, :3] / rgbw[:, 3:]
        w = self.weights()
        wu = np.bincount(self.po[self.und], w[self.und], minlength=self.T)
        tu = np.bincount(self.po[self.und], (w * np.abs(tex[self.pi]).max(1))[self.und], minlength=self.T)
        with np.errstate(all="ignore"):
            slack = np.where(wu > 0, (tu + wu * np.abs(np.nan_to_num(out)).max(1)) / np.maximum(rgbw[:, 3] - wu, 1e-300), 0.0)
        return out, slack

    def wsum(self):
        return np.bincount(self.po[self.acc], self.weights()[self.acc], minlength=self.T)

    def backward(self, g, form="transpose", mut=()):
        """g [T, 3 or 4] (a fourth channel, the gradient of wsum, does not reach the cubemap) -> (g_in [T, 3], slack [T]).
        form = "gather": the sum over the texel's own window with the roles exchanged (the defect)."""
        g = np.asarray(g, np.float64).reshape(self.T, -1)[:, :3]
        keep = self._keep(mut)
        if form == "gather":
            terms = g[self.pi] * (self.core * self.area[self.po])[:, None]
            rows = self.po
        else:
            terms = g[self.po] * self.weights(mut)[:, None]
            rows = self.pi
        out = self._sum(rows, terms, keep)
        return out, np.bincount(rows[self.und], np.abs(terms[self.und]).max(1), minlength=self.T)

    def backward_norm(self, g, mut=()):
        """The backward through rgb / wsum.  Slack: an undecided pair of output o moves its own term by |g[o]| w / wsum[o] and,
        through wsum[o], every term of o by the share wu / (wsum - wu)."""
        g = np.asarray(g, np.float64).reshape(self.T, 3)
        ws = self.wsum()
        with np.errstate(all="ignore"):
            q = g if "wsum_left_out" in mut else np.where(ws[:, None] > 0, g / ws[:, None], 0.0)
        out, _ = self.backward(q)
        w = self.weights()
        wu = np.bincount(self.po[self.und], w[self.und], minlength=self.T)
        rest = np.maximum(ws - wu, 1e-300)
        mag = np.abs(g).max(1)
        share = np.where(wu > 0, wu / rest, 0.0)
        t = mag[self.po] * w / rest[self.po]
        slack = np.bincount(self.pi[self.und], t[self.und], minlength=self.T)
        touched = self.acc & (share[self.po] > 0)
        slack += np.bincount(self.pi[touched], (t * share[self.po])[touched], minlength=self.T)
        return out, slack

    # ---- structure -------------------------------------------------------------------------------------------------
    def accepted_matrix(self):
        A = np.zeros((self.T, self.T), bool)
        A[self.po[self.acc], self.pi[self.acc]] = True
        return A

    def populations(self):
        p = dict(texels=self.T, accepted=int(self.acc.sum()), undecided=int(self.und.sum()),
                 empty=int((self.counts == 0).sum()), single=int((self.counts == 1).sum()),
                 empty_faces=int(((self.face_counts == 0).any(1) & (self.counts > 0)).sum()),
                 min_count=int(self.counts.min()), max_count=int(self.counts.max()), mean_count=float(self.counts.mean()),
                 tiles=((self.res + TILE - 1) // TILE) ** 2)
        texels_u = np.union1d(self.po[self.und], self.pi[self.und])
        p["undecided_share"] = texels_u.size / self.T
        if self.T <= 6 * 16 * 16:
            A = self.accepted_matrix()
            incone = (self.d @ self.d.T) >= self.cc
            p["asymmetric"] = int((A != A.T).sum())
            p["in_cone_outside_aabb"] = int((incone & ~A).sum())
            p["self_rejected"] = int((~np.diag(A)).sum())
        else:
            # large levels: symmetric iff every accepted pair is accepted in the other direction
            fwd = self.po[self.acc].astype(np.int64) * self.T + self.pi[self.acc]
            rev = self.pi[self.acc].astype(np.int64) * self.T + self.po[self.acc]
            p["asymmetric"] = int(2 * (~np.isin(fwd, rev)).sum())
        return p


def check_populations(lv, needs):
    """Fails when the level no longer provides what it declares; returns the populations."""
    p = lv.populations()
    n = needs
    if "asym" in n:
        assert (p["asymmetric"] > 0) == n["asym"], (lv.name, "asymmetric entries", p["asymmetric"])
    if n.get("empty"):
        assert p["empty"] > 0, (lv.name, "no empty window")
    if n.get("single"):
        assert p["single"] > 0, (lv.name, "no single-candidate window")
    if n.get("empty_faces"):
        assert p["empty_faces"] > 0, (lv.name, "no window with empty faces")
    if n.get("tiles"):
        assert p["tiles"] > 1, (lv.name, "one bounds tile per face")
    if n.get("ragged"):
        assert lv.T % 8 != 0, (lv.name, "texel count is a multiple of 8")
    for lanes in n.get("straddle", ()):
        c = lv.counts[lv.counts > 0]
        assert (c <= lanes * K_U).any() and (c > lanes * K_U).any(), (lv.name, f"counts on one side of {lanes} x {K_U}", p)
    assert p["undecided_share"] <= CAP_UNDECIDED, (lv.name, "undecided share", p["undecided_share"])
    return p


# ---- inputs ------------------------------------------------------------------------------------------------------------
def probes(res):
    """The eight cube corners, the mid-point of every face edge (each cube edge from both sides), texels on both sides of
    every 16-texel bounds-tile border and of the 32-texel LDS tile border, one face centre."""
    m, e = res // 2, res - 1
    p = [texel(res, f, y, x) for f in (4, 5) for y in (0, e) for x in (0, e)]
    p += [texel(res, f, y, x) for f in range(6) for y, x in ((0, m), (e, m), (m, 0), (m, e))]
    for border in sorted(set(range(TILE, res, TILE)) | set(range(LDS_TILE, res, LDS_TILE))):
        p += [texel(res, 0, m, border - 1), texel(res, 0, m, border), texel(res, 3, border - 1, m), texel(res, 3, border, m),
              texel(res, 1, border - 1, border - 1), texel(res, 1, border, border)]
    p.append(texel(res, 2, m, m))
    return np.unique(np.asarray(p, np.int64))


def _rng(name, salt):
    return np.random.default_rng([salt] + [ord(c) for c in name])


def hdr_map(lv):
    """Uniform [0, 1) with one HDR texel (1e3) at a cube corner."""
    tex = _rng(lv.name, 1).uniform(0.0, 1.0, size=(lv.T, 3)).astype(F32)
    tex[texel(lv.res, 4, 0, 0)] = 1e3
    return tex


def onehot_maps(lv, limit=12):
    """One-hot cubemaps, one probe per channel: the forward then returns single pair weights."""
    pr = probes(lv.res)
    pr = pr[np.linspace(0, pr.size - 1, min(limit, pr.size)).astype(int)]
    maps = []
    for k in range(0, pr.size, 3):
        tex = np.zeros((lv.T, 3), F32)
        for ch, i in enumerate(pr[k:k + 3]):
            tex[i, ch] = 1.0
        maps.append(tex)
    return maps


def dense_grad(lv, channels=4):
    return _rng(lv.name, 2).normal(size=(lv.T, channels)).astype(F32)


def zero_undecided_outputs(lv, g):
    """g with exact zeros on the outputs that hold an undecided pair (module docstring: the normalised backward)."""
    g = g.copy()
    g[np.unique(lv.po[lv.und])] = 0.0
    return g


def sparse_grad(lv_or_name, res=None, channels=3):
    """A normal gradient on the probe set, exact zeros elsewhere."""
    name, res = (lv_or_name.name, lv_or_name.res) if res is None else (lv_or_name, res)
    g = np.zeros((6 * res * res, channels), F32)
    pr = probes(res)
    g[pr] = _rng(name, 3).normal(size=(pr.size, channels)).astype(F32)
    return g


_levels = {}


def level(orc, name):
    """The Level of LEVELS / SPARSE_ONLY[name], built once per process.  A SPARSE_ONLY level holds the probe outputs only."""
    if name not in _levels:
        if name in SPARSE_ONLY:
            res, rough = SPARSE_ONLY[name]
            _levels[name] = Level(orc, res, rough, outputs=probes(res), name=name)
        else:
            res, rough, _ = LEVELS[name]
            _levels[name] = Level(orc, res, rough, name=name)
    return _levels[name]


# ---- comparator (the C oracle, fp32) and the bounds ----------------------------------------------------------------------
def comparator(orc, lv, tensor, x):
    """The C oracle's fp32 evaluation of `tensor` on input x."""
    r, shp = lv.res, (6, lv.res, lv.res, -1)
    if tensor == "fwd":
        return orc.specular_cubemap_fwd(x.reshape(shp), lv.bounds32, lv.rough_arg, lv.cc).reshape(lv.T, 4)
    if tensor == "fwd_norm":
        o = orc.specular_cubemap_fwd(x.reshape(shp), lv.bounds32, lv.rough_arg, lv.cc).reshape(lv.T, 4)
        with np.errstate(all="ignore"):
            return o[:, :3] / o[:, 3:]
    if tensor == "bwd":
        g4 = np.concatenate([x[:, :3], np.zeros((lv.T, 1), F32)], 1)
        return orc.specular_cubemap_bwd(lv.bounds32, g4.reshape(shp), lv.rough_arg, lv.cc).reshape(lv.T, 3)
    if tensor == "bwd_norm":
        ws = orc.specular_cubemap_fwd(np.zeros((6, r, r, 3), F32), lv.bounds32, lv.rough_arg, lv.cc).reshape(lv.T, 4)[:, 3:]
        with np.errstate(all="ignore"):
            q = np.where(ws > 0, x[:, :3] / ws, 0).astype(F32)
        g4 = np.concatenate([q, np.zeros((lv.T, 1), F32)], 1)
        return orc.specular_cubemap_bwd(lv.bounds32, g4.reshape(shp), lv.rough_arg, lv.cc).reshape(lv.T, 3)
    raise KeyError(tensor)


def reference(lv, tensor, x):
    """(float64 value, slack) of `tensor` on input x."""
    return dict(fwd=lv.forward, fwd_norm=lv.forward_norm, bwd=lv.backward, bwd_norm=lv.backward_norm)[tensor](x)


def inputs(lv):
    """(tensor, input name) -> array, for a full level."""
    out = {}
    for t in ("fwd", "fwd_norm"):
        out[(t, "hdr")] = hdr_map(lv)
        for k, m in enumerate(onehot_maps(lv)):
            out[(t, f"onehot{k}")] = m
    out[("bwd", "dense")], out[("bwd", "sparse")] = dense_grad(lv)[:, :3].copy(), sparse_grad(lv)
    out[("bwd_norm", "dense")] = zero_undecided_outputs(lv, out[("bwd", "dense")])
    out[("bwd_norm", "sparse")] = zero_undecided_outputs(lv, out[("bwd", "sparse")])
    return out


def judge(got, ref, slack, bound):
    """-> (worst plain row error over the rows without slack, number of rows over their bound, worst excess).  Rows whose
    reference is NaN (the normalised forward of an empty window) must be NaN and are left out of the metric; exact zeros of
    the reference must be exact zeros."""
    got, ref = np.asarray(got, np.float64).reshape(ref.shape), np.asarray(ref, np.float64)
    assert (slack > 0).mean() <= CAP_UNDECIDED, f"{(slack > 0).mean():.4f} of the texels would be widened"
    nan = np.isnan(ref).any(1)
    assert np.array_equal(np.isnan(got).any(1), nan), "NaN exactly where nothing is accepted"
    zero = (ref == 0) & ~nan[:, None]
    assert not got[zero].any(), f"{int((got[zero] != 0).sum())} exact zeros of float64 are not zero"
    g, r = np.where(nan[:, None], 0.0, got), np.where(nan[:, None], 0.0, ref)
    e = row_errors(g, r)
    wide = np.zeros_like(r)
    wide[:, 0] = slack
    allowed = bound + row_errors(r + wide, r)
    plain = float(e[slack == 0].max()) if (slack == 0).any() else 0.0
    over = e > allowed
    return plain, int(over.sum()), float((e - allowed).max())


def load_bounds():
    with open(BOUNDS_JSON) as f:
        return json.load(f)


def bound(doc, level_name, tensor, input_name, section="levels"):
    """BOUND_FACTOR x the comparator's recorded figure, the figure taken as at least ROUND_OFF (module docstring)."""
    return BOUND_FACTOR * max(doc[section][level_name]["comparator_worst"][f"{tensor}/{input_name}"], ROUND_OFF)


# ---- diffuse filter and mip ----------------------------------------------------------------------------------------------
DIFFUSE_RES = (8, 16)
MIP_RES = (32, 2)  # source resolutions: 32 -> 16 and 2 -> 1


def diffuse_reference(res):
    """(input, fwd64, gradient, bwd64): torch_pbr_ref.diffuse_cubemap and its transpose."""
    rng = _rng(f"diffuse{res}", 4)
    tex = rng.uniform(0.0, 1.0, size=(6, res, res, 3)).astype(F32)
    tex[4, 0, 0] = 1e3
    g = rng.normal(size=(6, res, res, 3)).astype(F32)
    x = tp.to64(tex).requires_grad_(True)
    y = tp.diffuse_cubemap(x)
    (y * tp.to64(g)).sum().backward()
    return tex, y.detach().numpy().reshape(-1, 3), g, x.grad.numpy().reshape(-1, 3)


def mip_reference(res):
    """(input [6,res,res,3], fwd64, gradient [6,res/2,res/2,3], bwd64): 2 x 2 mean and torch_pbr_ref.cubemap_mip_bwd."""
    rng = _rng(f"mip{res}", 5)
    tex = rng.uniform(0.0, 1.0, size=(6, res, res, 3)).astype(F32)
    tex[4, 0, 0] = 1e3
    h = res // 2
    g = rng.normal(size=(6, h, h, 3)).astype(F32)
    fwd = tex.astype(np.float64).reshape(6, h, 2, h, 2, 3).mean((2, 4))
    return tex, fwd.reshape(-1, 3), g, tp.cubemap_mip_bwd(tp.to64(g)).numpy().reshape(-1, 3)
