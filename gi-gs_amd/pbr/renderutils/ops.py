"""diffuse_cubemap / specular_cubemap with the reference's signatures (pbr/renderutils/ops.py:404-458),
backed by the HIP kernels of libgigs_hip.so instead of the JIT-compiled CUDA plugin."""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import numpy as np
import torch

import gigs_lib

_lib = gigs_lib.lib()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _gpu(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA/HIP tensor: pbr.renderutils (gigs-hip) has no CPU path")
    return t.contiguous().float()


class _diffuse_cubemap_func(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cubemap):
        c = _gpu(cubemap, "cubemap")
        out = torch.empty_like(c)
        with torch.cuda.device(c.device):
            gigs_lib.check(_lib.gigs_diffuse_cubemap_fwd(c.shape[1], c.data_ptr(), out.data_ptr(), _stream()),
                           "diffuse_cubemap_fwd")
        ctx.res = c.shape[1]
        return out

    @staticmethod
    def backward(ctx, dout):
        d = _gpu(dout, "dout")
        g = torch.empty_like(d)
        with torch.cuda.device(d.device):
            gigs_lib.check(_lib.gigs_diffuse_cubemap_bwd(ctx.res, d.data_ptr(), g.data_ptr(), _stream()),
                           "diffuse_cubemap_bwd")
        return g


def diffuse_cubemap(cubemap, use_python=False):
    if use_python:
        assert False
    assert cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2] and cubemap.shape[3] == 3
    out = _diffuse_cubemap_func.apply(cubemap)
    if torch.is_anomaly_enabled():
        assert not torch.isnan(out).any(), "Output of diffuse_cubemap contains inf or NaN"
    return out


class _specular_cubemap(torch.autograd.Function):
    """`tables` = None (recompute the pair weights every call, like the reference) or the cached
    `WeightTables` of `_weight_tables`."""

    @staticmethod
    def forward(ctx, cubemap, roughness, costheta_cutoff, bounds, tables=None):
        c = _gpu(cubemap, "cubemap")
        res = c.shape[1]
        out = torch.empty((6, res, res, 4), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            if tables is None:
                gigs_lib.check(_lib.gigs_specular_cubemap_fwd(res, c.data_ptr(), bounds.data_ptr(), float(roughness),
                                                              float(costheta_cutoff), out.data_ptr(), _stream()),
                               "specular_cubemap_fwd")
            else:
                gigs_lib.check(_lib.gigs_specular_cubemap_fwd_w(gigs_lib.ctx_ptr(), res, c.data_ptr(), bounds.data_ptr(), tables.offsets.data_ptr(),
                                                                tables.fwd.data_ptr(), _avg_window(tables, res),
                                                                out.data_ptr(), None, _stream()),
                               "specular_cubemap_fwd_w")
        ctx.save_for_backward(bounds)
        ctx.tables = tables
        ctx.lib_ctx = gigs_lib.current()  # for the backward, which autograd runs on its own thread
        ctx.res, ctx.roughness, ctx.theta_cutoff = res, roughness, costheta_cutoff
        return out

    @staticmethod
    @gigs_lib.with_forward_context
    def backward(ctx, dout):
        (bounds,) = ctx.saved_tensors
        d = _gpu(dout, "dout")
        g = torch.empty((6, ctx.res, ctx.res, 3), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            if ctx.tables is None:
                gigs_lib.check(_lib.gigs_specular_cubemap_bwd(ctx.res, bounds.data_ptr(), d.data_ptr(), float(ctx.roughness),
                                                              float(ctx.theta_cutoff), g.data_ptr(), _stream()),
                               "specular_cubemap_bwd")
            elif not ctx.tables.symmetric:
                _scatter_backward(ctx.res, bounds, ctx.tables, None, d, 0, g)
            else:
                gigs_lib.check(_lib.gigs_specular_cubemap_bwd_w(gigs_lib.ctx_ptr(), ctx.res, bounds.data_ptr(), ctx.tables.offsets.data_ptr(),
                                                                ctx.tables.bwd.data_ptr(), _avg_window(ctx.tables, ctx.res),
                                                                d.data_ptr(), 0, g.data_ptr(), _stream()),
                               "specular_cubemap_bwd_w")
        return g, None, None, None, None


def _scatter_backward(res, bounds, tables, wsum, d, grad_is_rgb, g):
    """The backward of a level whose accepted set is not symmetric (WeightTables.symmetric): the gather through the
    role-swapped tables is not the transpose of the forward there, the scatter from the forward table is."""
    gigs_lib.check(_lib.gigs_specular_cubemap_bwd_scatter_w(res, bounds.data_ptr(), tables.offsets.data_ptr(), tables.fwd.data_ptr(),
                                                            None if wsum is None else wsum.data_ptr(), d.data_ptr(),
                                                            int(grad_is_rgb), g.data_ptr(), _stream()),
                   "specular_cubemap_bwd_scatter_w")


def _avg_window(tables, res: int) -> int:
    """Mean number of window candidates per texel (scheduling hint of the *_w entry points)."""
    return max(1, tables.fwd.numel() // (6 * res * res))


def _ndf_cutoff(roughness: float, cutoff: float) -> float:
    """Cosine of the GGX cone that keeps `cutoff` of the energy (ops.py:428-440, host numpy)."""
    def ndfGGX(alphaSqr, costheta):
        costheta = np.clip(costheta, 0.0, 1.0)
        d = (costheta * alphaSqr - costheta) * costheta + 1.0
        return alphaSqr / (d * d * np.pi)

    nSamples = 1000000
    costheta = np.cos(np.linspace(0, np.pi / 2.0, nSamples))
    D = np.cumsum(ndfGGX(roughness ** 4, costheta))
    idx = np.argmax(D >= D[..., -1] * cutoff)
    return float(costheta[idx])


_ndfBoundsDict = {}


def _ndf_bounds(res, roughness, cutoff, device):
    key = (res, roughness, cutoff, str(device))
    if key not in _ndfBoundsDict:
        cos_cut = _ndf_cutoff(roughness, cutoff)
        bounds = torch.zeros((6, res, res, 24), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            gigs_lib.check(_lib.gigs_specular_bounds(res, cos_cut, bounds.data_ptr(), _stream()), "specular_bounds")
        _ndfBoundsDict[key] = (cos_cut, bounds)
    return _ndfBoundsDict[key]


class _specular_cubemap_normalized(torch.autograd.Function):
    """rgb / wsum in ONE launch (table path): forward = streaming filter + division, backward =
    (g / wsum) then the gather; replaces kernel + slice + div and their ~10 autograd launches."""

    @staticmethod
    def forward(ctx, cubemap, bounds, tables):
        c = _gpu(cubemap, "cubemap")
        res = c.shape[1]
        out = torch.empty((6, res, res, 3), dtype=torch.float32, device=c.device)
        wsum = torch.empty((6, res, res, 1), dtype=torch.float32, device=c.device)
        with torch.cuda.device(c.device):
            gigs_lib.check(_lib.gigs_specular_cubemap_fwd_w(gigs_lib.ctx_ptr(), res, c.data_ptr(), bounds.data_ptr(), tables.offsets.data_ptr(),
                                                            tables.fwd.data_ptr(), _avg_window(tables, res), out.data_ptr(),
                                                            wsum.data_ptr(), _stream()),
                           "specular_cubemap_fwd_w")
        ctx.save_for_backward(bounds, wsum)
        ctx.tables, ctx.res = tables, res
        ctx.lib_ctx = gigs_lib.current()
        return out

    @staticmethod
    @gigs_lib.with_forward_context
    def backward(ctx, dout):
        bounds, wsum = ctx.saved_tensors
        if not ctx.tables.symmetric:
            d = _gpu(dout, "dout")
            g = torch.empty((6, ctx.res, ctx.res, 3), dtype=torch.float32, device=d.device)
            with torch.cuda.device(d.device):
                _scatter_backward(ctx.res, bounds, ctx.tables, wsum, d, 1, g)
            return g, None, None
        if ctx.tables.bwd_scaled is not None:
            # the 1 / wsum of d(rgb / w) / d(rgb) is folded into the cached table (gigs_specular_weights_divide)
            d, table = _gpu(dout, "dout"), ctx.tables.bwd_scaled
        else:
            d, table = (_gpu(dout, "dout") / wsum).contiguous(), ctx.tables.bwd  # w does not depend on the cubemap
        g = torch.empty((6, ctx.res, ctx.res, 3), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            gigs_lib.check(_lib.gigs_specular_cubemap_bwd_w(gigs_lib.ctx_ptr(), ctx.res, bounds.data_ptr(), ctx.tables.offsets.data_ptr(),
                                                            table.data_ptr(), _avg_window(ctx.tables, ctx.res),
                                                            d.data_ptr(), 1, g.data_ptr(), _stream()),
                           "specular_cubemap_bwd_w")
        return g, None, None


bwd_head_start_ns = 0


class _specular_levels(torch.autograd.Function):
    """specular_cubemap of every level of a light in ONE launch each way (gigs_specular_cubemap_multi_w).  Inputs:
    the per-level (bounds, tables) as a Python list, then the level mips; needs the cached tables incl. the pre-divided
    backward table of every level (otherwise CubemapLight.build_mips falls back to one call per level)."""

    @staticmethod
    def forward(ctx, meta, sparse, *mips):
        import ctypes as C
        cs = [_gpu(m, "cubemap") for m in mips]
        dev = cs[0].device
        shapes = [c.shape[1] for c in cs]
        # `sparse` (a SparseFineLevels): the fine levels live in its persistent buffers; once those hold a dense build, this
        # launch filters the coarse levels only and the fine ones follow in sparse.fill(), for the view's texels alone
        fine = sparse.begin(shapes, dev) if sparse is not None else 0
        outs, wsums, arr = [], [], (gigs_lib.SpecLevel * len(cs))()
        for i, (c, (bounds, tables)) in enumerate(zip(cs, meta)):
            res = c.shape[1]
            if sparse is not None and i < len(sparse.out):
                out, wsum = sparse.out[i], sparse.wsum[i]
            else:
                out = torch.empty((6, res, res, 3), dtype=torch.float32, device=dev)
                wsum = torch.empty((6, res, res, 1), dtype=torch.float32, device=dev)
            outs.append(out)
            wsums.append(wsum)
            arr[i] = gigs_lib.SpecLevel(res, _avg_window(tables, res), c.data_ptr(), bounds.data_ptr(), tables.offsets.data_ptr(),
                                        tables.fwd.data_ptr(), out.data_ptr(), wsum.data_ptr())
        with torch.cuda.device(dev):
            dense = (gigs_lib.SpecLevel * (len(cs) - fine))(*arr[fine:])
            gigs_lib.check(_lib.gigs_specular_cubemap_multi_w(gigs_lib.ctx_ptr(), len(cs) - fine, C.cast(dense, C.c_void_p), 0,
                                                              _stream()), "specular_cubemap_multi_w")
        if fine:
            sparse.pending = ((gigs_lib.SpecLevel * fine)(*arr[:fine]), cs[:fine])  # the mips stay alive with the record
        ctx.meta = meta
        ctx.lib_ctx = gigs_lib.current()
        ctx.shapes = [c.shape[1] for c in cs]
        return tuple(outs)

    @staticmethod
    @gigs_lib.with_forward_context
    def backward(ctx, *douts):
        import ctypes as C
        dev = next(d for d in douts if d is not None).device
        # the levels whose accepted set is symmetric share one launch (the standard chains are symmetric at every level);
        # any other level is scattered from its forward table, on its own, behind that launch
        n = sum(1 for _, tables in ctx.meta if tables.symmetric)
        gs, keep, scattered, shapes = [], [], [], []
        arr, w_fwd, w_sum = (gigs_lib.SpecLevel * max(n, 1))(), (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
        i = 0
        for d, res, (bounds, tables) in zip(douts, ctx.shapes, ctx.meta):
            d = torch.zeros((6, res, res, 3), dtype=torch.float32, device=dev) if d is None else _gpu(d, "dout")
            keep.append(d)
            g = torch.empty((6, res, res, 3), dtype=torch.float32, device=dev)
            gs.append(g)
            if not tables.symmetric:
                scattered.append((res, bounds, tables, d, g))
                continue
            arr[i] = gigs_lib.SpecLevel(res, _avg_window(tables, res), d.data_ptr(), bounds.data_ptr(), tables.offsets.data_ptr(),
                                        tables.bwd_scaled.data_ptr(), g.data_ptr(), None)
            w_fwd[i], w_sum[i] = tables.fwd.data_ptr(), tables.wsum.data_ptr()
            shapes.append(res)
            i += 1
        with torch.cuda.device(dev):
            if bwd_head_start_ns > 0:  # see gigs_stream_delay: set by pipeline.WholeStepGraph while it captures the backward
                gigs_lib.check(_lib.gigs_stream_delay(int(bwd_head_start_ns), _stream()), "stream_delay")
            if n > 0:
                # nonzero-texel census, then one launch: tile gather or scatter of the sparse levels, gather of the others
                # (gigs_options.spec_sparse = 0: the gather alone)
                state, lists = _sparse_buffers(tuple(shapes), dev)
                gigs_lib.check(_lib.gigs_specular_cubemap_multi_bwd_sparse(gigs_lib.ctx_ptr(), n, C.cast(arr, C.c_void_p), w_fwd, w_sum,
                                                                           None if state is None else state.data_ptr(),
                                                                           None if lists is None else lists.data_ptr(), _stream()),
                               "specular_cubemap_multi_bwd_sparse")
            for res, bounds, tables, d, g in scattered:
                _scatter_backward(res, bounds, tables, tables.wsum, d, 1, g)
        return (None, None, *gs)


class SparseFineLevels:
    """The sparse forward of a light's fine GGX levels, for a caller that shades ONE view with the light it has just built
    (a training step; pipeline.Stage2Step).  The view's shade reads a few percent of the two finest levels, which are two
    thirds of the cached weight table, so these levels are filtered for the texels it reads only:
      * specular_cubemap_levels(..., sparse=self) filters the coarse levels as ever and leaves the fine ones pending;
      * fill(), called once the view's G-buffer exists and before the shade, marks the texels the shade will read -- for
        every pixel, as the shade kernels sample for every pixel (gigs_spec_tap_census) --, lists them and filters them
        (gigs_specular_cubemap_multi_fwd_sparse: the dense bits).
    The fine levels' outputs are persistent tensors of this object.  A texel that is not listed keeps an older value,
    which this view's shade never reads; for any other reader the levels are incomplete (CubemapLight.fine_levels_partial).
    The first build through the object is dense, so that the tensors never expose uninitialised memory, and so is any level
    whose count of texels exceeds its capacity.  One object per light and stepper; its calls are ordered by the caller's
    streams."""

    N_FINE = 2           # the two finest levels; the levels below them always stay dense
    # Per fine level, the fraction of its texels up to which it is listed; beyond it the dense level is launched.  Measured
    # alone on the device (tools/spec_fwd_sweep.py, profiles/r28/spec_fwd_sweep.txt): with the 17 us tap census charged to
    # each level in full, the listed 256^2 level stays below its dense launch minus that launch's spread (53 us) up to
    # 10 % (46 us; 25 %: 51 - 56 us, the break-even) and the 128^2 level (133 us) far beyond 25 % (60 us; 50 %: 87 us).
    # The bench views need 4 - 6 % and 10 - 11 %.  A scalar serves both levels.
    CAPACITY = (0.10, 0.25)

    def __init__(self):
        self.shapes = None
        self.out, self.wsum, self.needed = [], [], []
        self.caps, self.state, self.lists = (), None, None
        self.primed, self.pending = False, None

    def begin(self, shapes, device) -> int:
        """Called by the levels' forward: (re)allocates for the chain `shapes` and returns how many fine levels THIS build
        leaves to fill() -- 0 for the first build, which is dense."""
        self.pending = None
        n_fine = self.N_FINE if len(shapes) > self.N_FINE else 0
        key = (tuple(shapes), str(device))
        if key != self.shapes:
            self.shapes = key
            fine = shapes[:n_fine]
            self.out = [torch.empty((6, r, r, 3), dtype=torch.float32, device=device) for r in fine]
            self.wsum = [torch.empty((6, r, r, 1), dtype=torch.float32, device=device) for r in fine]
            self.needed = [torch.zeros((6, r, r, 3), dtype=torch.float32, device=device) for r in fine]
            frac = self.CAPACITY if isinstance(self.CAPACITY, tuple) else (self.CAPACITY,) * n_fine
            self.caps = tuple(int(6 * r * r * f) for r, f in zip(fine, frac))
            self.state = torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=device)
            self.lists = torch.empty(max(1, sum(self.caps)), dtype=torch.int32, device=device)
            self.primed = False
        if not self.primed:
            self.primed = True
            return 0
        return n_fine

    def fill(self, H, W, view_dirs, roughness, normals=None, planar=False, mask=None, normal_map=None, viewmatrix=None,
             rough_scale=1.0, rough_bias=0.0) -> bool:
        """Filters the pending fine levels for the view whose shade has these inputs (see gigs_spec_tap_census for the two
        ways to give the normal), on the current stream.  False if nothing is pending (the last build was dense).  The record
        of the last build is kept: a build that is replayed from a graph, without its Python code, is filled like the captured one."""
        import ctypes as C
        if self.pending is None:
            return False
        arr, _keep = self.pending
        n, L = len(arr), len(self.shapes[0])
        res = (C.c_int * L)(*self.shapes[0])
        need_all = (C.c_void_p * L)(*([t.data_ptr() for t in self.needed] + [None] * (L - n)))
        need = (C.c_void_p * n)(*[t.data_ptr() for t in self.needed])
        caps = (C.c_int * n)(*self.caps)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(view_dirs.device):
            gigs_lib.check(_lib.gigs_spec_tap_census(gigs_lib.ctx_ptr(), H, W, p(normals), int(bool(planar)), p(normal_map),
                                                     p(viewmatrix), p(view_dirs), p(roughness), p(mask), float(rough_scale),
                                                     float(rough_bias), L, res, need_all, _stream()), "spec_tap_census")
            gigs_lib.check(_lib.gigs_specular_cubemap_multi_fwd_sparse(gigs_lib.ctx_ptr(), n, C.cast(arr, C.c_void_p), need, caps,
                                                                       self.state.data_ptr(), self.lists.data_ptr(), _stream()),
                           "specular_cubemap_multi_fwd_sparse")
        return True

    def report(self):
        """[(listed, texels marked)] per fine level from the last fill(): a device read after a synchronisation."""
        torch.cuda.synchronize(self.state.device)
        v = self.state.cpu().tolist()
        return [(bool(v[8 + i]), v[16 + i]) for i in range(len(self.out))]


# Persistent device buffers of gigs_specular_cubemap_multi_bwd_sparse: the state ints (zero before the first call; the
# library clears its counters itself afterwards) and the levels' index lists.  A pair belongs to ONE owner: eager calls
# share one pair per (level chain, capacities, device, stream) -- a stream orders its own calls -- and every graph capture
# takes a pair of its own, because a replay is ordered with nothing an eager stream does.  The pair of a capture comes from
# the spares that eager calls of the same chain leave zero-filled (a stepper warms up eagerly before it captures), so the
# graph holds no fill node for the state; without a spare it is allocated inside the capture.  The dictionaries grow with
# the distinct chains, capacities and streams of a process, a few hundred bytes to 200 KB per entry.
_sparseBuffers = {}
_sparseSpares = {}
_sparseCaptured = []


def _new_sparse_pair(caps, device):
    return (torch.zeros(gigs_lib.SPEC_SPARSE_STATE_INTS, dtype=torch.int32, device=device),
            torch.empty(max(1, sum(caps)), dtype=torch.int32, device=device))


def _sparse_buffers(shapes, device):
    if not gigs_lib.current().option("spec_sparse"):
        return None, None  # the library launches the gather alone and reads neither
    caps = tuple(gigs_lib.check(_lib.gigs_spec_sparse_capacity(gigs_lib.ctx_ptr(), r), "spec_sparse_capacity") for r in shapes)
    chain = (shapes, caps, str(device))
    if torch.cuda.is_current_stream_capturing():
        spares = _sparseSpares.get(chain)
        pair = spares.pop() if spares else _new_sparse_pair(caps, device)
        _sparseCaptured.append(pair)  # a graph may be replayed as long as the process lives: so does its pair (< 200 KB)
    else:
        key = chain + (_stream(),)
        if key not in _sparseBuffers:
            _sparseBuffers[key] = _new_sparse_pair(caps, device)
        if not _sparseSpares.get(chain):
            _sparseSpares[chain] = [_new_sparse_pair(caps, device)]
        pair = _sparseBuffers[key]
    _sparseLast[(shapes, str(device))] = pair[0]
    return pair


_sparseLast = {}


def spec_sparse_report(shapes, device=None):
    """[(scattered, nonzero texels)] per level from the last backward queued for the chain `shapes` (the resolutions of the
    levels with a symmetric accepted set: the others never enter that launch), or None if none ran: a device read after a
    synchronisation, for tests and diagnostics."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    state = _sparseLast.get((tuple(shapes), str(device)))
    if state is None:
        return None
    torch.cuda.synchronize(device)
    v = state.cpu().tolist()
    return [(bool(v[8 + i]), v[16 + i]) for i in range(len(shapes))]


def specular_cubemap_levels(mips, roughnesses, cutoff=0.99, sparse=None):
    """[specular_cubemap(m, r, cutoff) for m, r in zip(mips, roughnesses)] as one launch each way, or None if a level
    lacks its cached tables (then the caller filters level by level).  sparse = a SparseFineLevels: the fine levels are
    returned pending, the caller completes them with sparse.fill() before anything reads them."""
    if not gigs_lib.current().switch("spec_multi") or torch.is_anomaly_enabled() or not mips[0].is_cuda:
        return None
    meta = []
    for m, r in zip(mips, roughnesses):
        _, bounds = _ndf_bounds(m.shape[1], r, cutoff, m.device)
        tables = _weight_tables(m.shape[1], r, cutoff, m.device)
        if tables is None or tables.bwd_scaled is None:
            return None
        meta.append((bounds, tables))
    return list(_specular_levels.apply(meta, sparse, *mips))


# Cached pair-weight tables (see csrc/light_filter.hip): 0.74 GB for the 256..16 chain, x2 for the backward.
# HBM is 288 GB on MI355X; set GIGS_SPEC_TABLE_MAX_GB=0 to recompute the weights every call instead.
_TABLE_MAX_BYTES = float(os.environ.get("GIGS_SPEC_TABLE_MAX_GB", "8")) * 1e9
_weightTables = {}


class WeightTables(NamedTuple):
    """The cached tables of one (resolution, roughness, cutoff): `fwd` / `bwd` hold the pair weights in the forward's
    and the gather-form backward's roles, `bwd_scaled` is `bwd` pre-divided by the forward's weight sums `wsum` (both
    None without the switch spec_prescaled or past the byte budget).  `symmetric`: whether every accepted pair (o, i) is
    also accepted as (i, o), decided once when the tables are built (gigs_specular_window_symmetric); only then is the gather
    through `bwd` / `bwd_scaled` the transpose of the forward, else the backward scatters from `fwd`."""
    offsets: torch.Tensor
    fwd: torch.Tensor
    bwd: torch.Tensor
    bwd_scaled: Optional[torch.Tensor]
    wsum: Optional[torch.Tensor]
    symmetric: bool = True


def _weight_tables(res, roughness, cutoff, device):
    key = (res, roughness, cutoff, str(device))
    if key not in _weightTables:
        cos_cut, bounds = _ndf_bounds(res, roughness, cutoff, device)
        b = bounds.view(-1, 6, 4)
        w = torch.where(b[..., 0] <= b[..., 1], b[..., 1] - b[..., 0] + 1, torch.zeros_like(b[..., 0]))
        h = torch.where(b[..., 2] <= b[..., 3], b[..., 3] - b[..., 2] + 1, torch.zeros_like(b[..., 0]))
        cnt = (w * h).to(torch.int64).reshape(-1)
        total = int(cnt.sum().item())
        used = sum(t.fwd.numel() * (12 if t.bwd_scaled is not None else 8) for t in _weightTables.values() if t is not None)
        if total == 0 or total >= 2 ** 31 or used + total * 8 > _TABLE_MAX_BYTES:
            _weightTables[key] = None
        else:
            offsets = (torch.cumsum(cnt, 0) - cnt).to(torch.int32).contiguous()
            tabs = []
            with torch.cuda.device(device):
                for swap in (0, 1):
                    wt = torch.empty(total, dtype=torch.float32, device=device)
                    gigs_lib.check(_lib.gigs_specular_weights(res, bounds.data_ptr(), offsets.data_ptr(), float(roughness),
                                                              float(cos_cut), swap, wt.data_ptr(), _stream()),
                                   "specular_weights")
                    tabs.append(wt)
            scaled = wsum = None
            if gigs_lib.current().switch("spec_prescaled") and used + total * 12 <= _TABLE_MAX_BYTES:
                # weight sums of the forward (independent of the cubemap's values), then the backward table divided by them
                with torch.cuda.device(device):
                    ones = torch.ones((6, res, res, 3), dtype=torch.float32, device=device)
                    tmp = torch.empty_like(ones)
                    wsum = torch.empty((6, res, res), dtype=torch.float32, device=device)
                    gigs_lib.check(_lib.gigs_specular_cubemap_fwd_w(gigs_lib.ctx_ptr(), res, ones.data_ptr(), bounds.data_ptr(),
                                                                    offsets.data_ptr(), tabs[0].data_ptr(), 0,
                                                                    tmp.data_ptr(), wsum.data_ptr(), _stream()),
                                   "specular_cubemap_fwd_w")
                    scaled = torch.empty(total, dtype=torch.float32, device=device)
                    gigs_lib.check(_lib.gigs_specular_weights_divide(res, bounds.data_ptr(), offsets.data_ptr(),
                                                                     tabs[1].data_ptr(), wsum.data_ptr(), scaled.data_ptr(),
                                                                     _stream()), "specular_weights_divide")
            with torch.cuda.device(device):
                symmetric = bool(gigs_lib.check(_lib.gigs_specular_window_symmetric(res, float(cos_cut), _stream()),
                                                "specular_window_symmetric"))
            _weightTables[key] = WeightTables(offsets, tabs[0], tabs[1], scaled, wsum if scaled is not None else None, symmetric)
    return _weightTables[key]


def specular_cubemap(cubemap, roughness, cutoff=0.99, use_python=False):
    assert cubemap.shape[0] == 6 and cubemap.shape[1] == cubemap.shape[2], \
        "Bad shape for cubemap tensor: %s" % str(cubemap.shape)
    if use_python:
        assert False
    if not cubemap.is_cuda:
        raise RuntimeError("cubemap must be a CUDA/HIP tensor: pbr.renderutils (gigs-hip) has no CPU path")
    cos_cut, bounds = _ndf_bounds(cubemap.shape[1], roughness, cutoff, cubemap.device)
    tables = _weight_tables(cubemap.shape[1], roughness, cutoff, cubemap.device)
    if tables is not None and not torch.is_anomaly_enabled():
        return _specular_cubemap_normalized.apply(cubemap, bounds, tables)
    out = _specular_cubemap.apply(cubemap, roughness, cos_cut, bounds, tables)
    if torch.is_anomaly_enabled():
        assert not torch.isnan(out).any(), "Output of specular_cubemap contains inf or NaN"
    return out[..., 0:3] / out[..., 3:]
