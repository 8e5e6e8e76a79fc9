"""GPU tests: the SSAO / SSR march kernels (csrc/gi.hip) reproduce, bit for bit, arrays recorded from the build BEFORE the
finish of ssr_kernel rebuilt its inputs (normal, position, tangent frame) behind the march and before a workgroup with nothing
to march returned ahead of the certification table's staging: tests/golden/gi_scoping.npz, written by
tests/golden/make_gi_scoping_golden.py with this module's inputs and runners from the build of commit 75cb5dc (the file's
"provenance" entry says so; the generator refuses to record without being told the commit its library was built from).

The shapes are the smallest at which either change can go wrong:
  * ragged   37 x 21: ragged in both axes, partial tiles, certification blocks (16 px) only partly covered in both axes' last
                      block, one whole block row;
  * band     40 x 24: a band of zero normals (NaN tangent frame: such pixels never march and finish with zero sums and a NaN
                      normal) over two whole 8 x 8 tiles and half of a third -- an empty workgroup next to a marching one;
  * nanrad   the same with NaN and Inf radiance on rows the rays hit.
Each with metallic 0 and 1, delta 0.0625 and 0.125, (start, step) = (8, 16) and (16, 16) (no march: the finish alone), and
certification on and off (both must give the recorded bits).  Two lights through gigs_ssr_multi, the hit list (count, then
fill: counts, entries and both calls' planes) and the exact march once each.  Compared: the NaN pattern, and every other bit.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gi_scoping.npz")
GI = dict(radius=0.8, bias=0.01, thick=0.05)
GEOMS = {"ragged": (37, 21), "band": (40, 24), "nanrad": (40, 24)}
DELTAS = (0.0625, 0.125)
MARCHES = ((8, 16), (16, 16))  # (start, step)

# planes of a small room, camera space (z forward): (normal towards the camera, a point); the slab stands in front of the wall
PLANES = [((0.12, 0.2, -1.0), (0.0, 0.0, 3.0)), ((0.3, -0.85, -0.3), (0.0, 0.55, 3.0)), ((0.9, 0.25, -0.35), (-0.9, 0.0, 3.0)),
          ((-0.9, 0.2, -0.3), (1.0, 0.0, 3.0))]
SLAB = ((0.05, 0.15, -1.0), (0.0, 0.0, 2.55), (0.5, 0.8, 0.15, 0.7))  # normal, point, image rectangle (x0, x1, y0, y1) as shares


def inputs(geom):
    """Seeded numpy planes of one geometry: normal, pos [3,H,W]; rgb [2,3,H,W] (two lights); albedo, F0 [3,H,W]; roughness
    [1,H,W]; the focal length.  Pixel (i, j) looks along ((i - W/2) / f, (j - H/2) / f, 1), the march's own projection."""
    W, H = GEOMS[geom]
    rng = np.random.default_rng({"ragged": 2901, "band": 2902, "nanrad": 2902}[geom])
    f = 1.35 * W
    dx = ((np.arange(W) - W / 2) / f)[None, :].repeat(H, 0)
    dy = ((np.arange(H) - H / 2) / f)[:, None].repeat(W, 1)
    d = np.stack([dx, dy, np.ones_like(dx)])
    best = np.full((H, W), np.inf)
    nrm = np.zeros((3, H, W))
    planes = [(n, p, (0.0, 1.0, 0.0, 1.0)) for n, p in PLANES] + [SLAB]
    for n, p, (x0, x1, y0, y1) in planes:
        n = np.asarray(n, np.float64) / np.linalg.norm(n)
        den = (n[:, None, None] * d).sum(0)
        t = float(np.dot(n, p)) / np.where(den < 0, den, np.nan)
        inside = (np.arange(W)[None, :] >= x0 * W) & (np.arange(W)[None, :] < x1 * W) & (np.arange(H)[:, None] >= y0 * H) & (np.arange(H)[:, None] < y1 * H)
        take = (t > 0) & (t < best) & inside
        best = np.where(take, t, best)
        nrm = np.where(take[None], n[:, None, None], nrm)
    assert np.isfinite(best).all()
    pos = (d * best[None]).astype(np.float32)
    normal = (nrm + 0.04 * rng.normal(size=nrm.shape)).astype(np.float32)
    rgb = rng.uniform(0, 1, size=(2, 3, H, W)).astype(np.float32)
    albedo = rng.uniform(0.05, 1, size=(3, H, W)).astype(np.float32)
    F0 = rng.uniform(0.02, 0.9, size=(3, H, W)).astype(np.float32)
    roughness = rng.uniform(0, 1, size=(1, H, W)).astype(np.float32)
    if geom in ("band", "nanrad"):
        normal[:, 0:8, 0:20] = 0.0  # tiles (0,0), (1,0) whole, the left half of (2,0)
    if geom == "nanrad":
        rgb[:, :, 12:14, :] = np.nan
        rgb[:, :, 14:15, :] = np.inf
        rgb[1, :, 13, :] = 0.5  # the second light's NaN rows differ from the first's
    return dict(W=W, H=H, f=f, normal=normal, pos=pos, rgb=rgb, albedo=albedo, F0=F0, roughness=roughness)


def _tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _p(t):
    return None if t is None else t.data_ptr()


class Runner:
    """the device copies of one geometry's planes and the launches over them"""

    def __init__(self, geom):
        import gigs_lib
        self.gl, self.lib = gigs_lib, gigs_lib.lib()
        g = inputs(geom)
        self.W, self.H = g["W"], g["H"]
        self.f = float(g["f"])
        self.t = {k: _tt(v) for k, v in g.items() if isinstance(v, np.ndarray)}
        self.metal = {m: torch.full((1, self.H, self.W), float(m), device=DEV) for m in (0, 1)}
        self.scratch = torch.empty(max(16, int(self.lib.gigs_gi_scratch_bytes(self.W, self.H))), dtype=torch.uint8, device=DEV)
        self.s = torch.cuda.current_stream().cuda_stream

    def args(self, delta, start, step):
        return (self.W, self.H, self.f, self.f, GI["radius"], GI["bias"], GI["thick"], float(delta), int(step), int(start))

    def planes(self, metallic, rgb):
        t = self.t
        return (_p(t["normal"]), _p(t["pos"]), _p(rgb), _p(t["albedo"]), _p(t["roughness"]), _p(self.metal[metallic]), _p(t["F0"]))

    def fresh(self, *shape):
        return torch.full(shape, 7.0, device=DEV)

    def ssao(self, delta, start, step, **opts):
        occ = self.fresh(1, self.H, self.W)
        with self.gl.options(**opts) as cx:
            self.gl.check(self.lib.gigs_ssao_ex(cx.ptr, *self.args(delta, start, step), _p(self.t["normal"]), _p(self.t["pos"]), _p(occ),
                                                _p(self.scratch), self.s), "ssao")
        return {"occlusion": occ.cpu().numpy()}

    def ssr(self, metallic, delta, start, step, **opts):
        color, abd = self.fresh(3, self.H, self.W), self.fresh(3, self.H, self.W)
        with self.gl.options(**opts) as cx:
            self.gl.check(self.lib.gigs_ssr_ex(cx.ptr, *self.args(delta, start, step), *self.planes(metallic, self.t["rgb"][0]), _p(color),
                                               _p(abd), _p(self.scratch), self.s), "ssr")
        return {"color": color.cpu().numpy(), "abd": abd.cpu().numpy()}

    def ssr_multi(self, metallic, delta, start, step, **opts):
        color, abd = self.fresh(2, 3, self.H, self.W), self.fresh(2, 3, self.H, self.W)
        with self.gl.options(**opts) as cx:
            self.gl.check(self.lib.gigs_ssr_multi(cx.ptr, 2, *self.args(delta, start, step), *self.planes(metallic, self.t["rgb"]), _p(color),
                                                  _p(abd), _p(self.scratch), self.s), "ssr_multi")
        return {"color": color.cpu().numpy(), "abd": abd.cpu().numpy()}

    def ssr_hits(self, metallic, delta, start, step, **opts):
        """count (kHits 1), exclusive prefix, fill (kHits 2): both calls' planes, the counts and the entries"""
        N = self.W * self.H
        a, pl = self.args(delta, start, step), self.planes(metallic, self.t["rgb"][0])
        counts = torch.zeros(4 * N, dtype=torch.int32, device=DEV)
        offsets = torch.zeros(4 * N + 1, dtype=torch.int32, device=DEV)
        c1, a1, c2, a2 = (self.fresh(3, self.H, self.W) for _ in range(4))
        with self.gl.options(**opts) as cx:
            self.gl.check(self.lib.gigs_ssr_hits(cx.ptr, *a, *pl, _p(c1), _p(a1), 1, _p(counts), None, None, 0, _p(self.scratch), self.s), "count")
            torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
            total = int(offsets[-1])
            entries = torch.full((max(total, 1), 2), -1, dtype=torch.int32, device=DEV)
            self.gl.check(self.lib.gigs_ssr_hits(cx.ptr, *a, *pl, _p(c2), _p(a2), 2, None, _p(offsets), _p(entries), total, _p(self.scratch),
                                                 self.s), "fill")
        e = entries[:total].cpu().numpy()
        assert total > 0 and e.min() >= 0 and e.max() < 65536 and int(counts.max()) < 65536
        return {"count_color": c1.cpu().numpy(), "count_abd": a1.cpu().numpy(), "color": c2.cpu().numpy(), "abd": a2.cpu().numpy(),
                "counts": counts.cpu().numpy().astype(np.uint16), "entries": e.astype(np.uint16)}


def ssr_settings():
    return [(m, d, st, sp) for m in (0, 1) for d in DELTAS for st, sp in MARCHES]


def key(kind, geom, metallic, delta, start, name):
    return "%s/%s/m%d/d%g/s%d/%s" % (kind, geom, metallic, delta, start, name)


def stored_delta(delta, start, step):
    """Without a march (start >= step) nothing of the ray set reaches the outputs: both deltas are held to ONE recorded array."""
    return delta if start < step else DELTAS[0]


def same_bits(got, want, what):
    """the NaN pattern, and every bit of everything else"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind != "f":
        assert np.array_equal(got, want), what
        return
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN pattern", int((gn != wn).sum()))
    a, b = got.view(np.uint32)[~gn], want.view(np.uint32)[~gn]
    assert np.array_equal(a, b), (what, "%d of %d values differ" % (int((a != b).sum()), a.size))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    assert "75cb5dc" in str(g["provenance"]), "the fixture must be the recording of the parent build"
    return g


_RUNNERS = {}


def runner(geom):
    if geom not in _RUNNERS:
        _RUNNERS[geom] = Runner(geom)
    return _RUNNERS[geom]


@pytest.mark.parametrize("geom", list(GEOMS))
def test_ssr_matches_the_recorded_march(geom, golden):
    r = runner(geom)
    for m, d, st, sp in ssr_settings():
        for cert in (1, 0):
            for name, got in r.ssr(m, d, st, sp, gi_cert=cert).items():
                same_bits(got, golden[key("ssr", geom, m, stored_delta(d, st, sp), st, name)], (geom, m, d, st, sp, cert, name))


@pytest.mark.parametrize("geom", ["ragged", "band"])
def test_ssao_matches_the_recorded_march(geom, golden):
    r = runner(geom)
    for d in DELTAS:
        for st, sp in MARCHES:
            for cert in (1, 0):
                got = r.ssao(d, st, sp, gi_cert=cert)["occlusion"]
                same_bits(got, golden[key("ssao", geom, 0, stored_delta(d, st, sp), st, "occlusion")], (geom, d, st, sp, cert))


def test_two_lights_match_the_recorded_march(golden):
    for cert in (1, 0):
        for name, got in runner("nanrad").ssr_multi(0, 0.125, 8, 16, gi_cert=cert).items():
            same_bits(got, golden[key("multi", "nanrad", 0, 0.125, 8, name)], (cert, name))


def test_hit_list_matches_the_recorded_march(golden):
    for cert in (1, 0):
        for name, got in runner("ragged").ssr_hits(0, 0.125, 8, 16, gi_cert=cert).items():
            same_bits(got, golden[key("hits", "ragged", 0, 0.125, 8, name)], (cert, name))


def test_exact_march_matches_the_recorded_march(golden):
    r = runner("band")
    for st, sp in ((8, 16), (5, 12)):  # a power-of-two step and the general form
        for name, got in r.ssr(0, 0.125, st, sp, gi_march="exact").items():
            same_bits(got, golden[key("exact%d" % sp, "band", 0, 0.125, st, name)], (st, sp, name))
        same_bits(r.ssao(0.125, st, sp, gi_march="exact")["occlusion"], golden[key("exact%d" % sp, "band", 0, 0.125, st, "occlusion")], (st, sp))
