#!/usr/bin/env python
"""How many global float adds the shade backward's fine light levels take on the bench view, per scatter scheme.

Works on the CPU from the oracle G-buffer of bench.py's C2 view (oracle/stage2_ref.py: rasterizer, filters, SSAO,
gbuffer_post -- the path `bench.py --full` checks parity against) and restates the kernel's cube taps in float32
numpy (csrc/cube.h cube_taps).  Every masked pixel contributes 4 taps of its level l0 and, between two levels, 4 of
l1; an entry of weight 0 adds nothing.  The fine levels are those the kernel keeps in global memory (256^2, 128^2,
64^2 at base 256: they do not fit the 30 720-float LDS plan).  One "add" is one (texel, RGB) triple.

    (a) rows   row-major 1024-pixel chunks, one add per run of equal keys among consecutive lanes of a 16-lane row
               and tap slot (run_add3: the kernel before 8x8 waves)
    (b) wave   8 x 8 pixel waves, one add per distinct (level, texel) of the wave over all 8 tap slots
    (c) tile   (b) plus a per-workgroup LDS table over 32 x 32 pixel tiles with S slots: a tile whose distinct keys
               fit adds each of them once, a tile that overflows pays (b) -- counted for several S

    python tools/shade_scatter_count.py [--view 0] [--res 800] [--out profiles/r05/shade_scatter_count.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gi-gs_amd"))

f32 = np.float32
SLOTS = (512, 1024, 2048, 3072)


def cube_face_uv(x, y, z):
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    face = np.where(az > np.maximum(ax, ay), 4, np.where(ay > ax, 2, 0))
    c = np.where(face == 4, z, np.where(face == 2, y, x))
    xx = np.where(face == 0, z, x)
    yy = np.where(face == 2, z, y)
    face = face + (c < 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (f32(1.0) / np.abs(c)).astype(f32) * f32(0.5)
        m0 = np.where((face == 0) | (face == 5), -m, m)
        m1 = np.where(face != 2, -m, m)
        u = (xx * m0 + f32(0.5)).astype(f32)
        v = (yy * m1 + f32(0.5)).astype(f32)
    ok = np.isfinite(u) & np.isfinite(v)
    return np.where(ok, face, -1), np.clip(np.nan_to_num(u), 0, 1).astype(f32), np.clip(np.nan_to_num(v), 0, 1).astype(f32)


def cube_dir_raw(a, b, face):
    one = np.ones_like(a)
    sel = [face == 0, face == 1, face == 2, face == 3, face == 4]
    return np.stack([np.select(sel, [one, -one, a, a, a], -a), np.select(sel, [-b, -b, one, -one, -b], -b),
                     np.select(sel, [-a, a, b, -b, one], -one)]).astype(f32)


def cube_taps(res, d):
    """[4, N] texel indices (-1 = dropped) and weights of the bilinear cube lookup of directions d [3, N]."""
    face, u, v = cube_face_uv(d[0], d[1], d[2])
    fu, fv = (u * f32(res) - f32(0.5)).astype(f32), (v * f32(res) - f32(0.5)).astype(f32)
    flu, flv = np.floor(fu), np.floor(fv)
    iu0, iv0 = flu.astype(np.int64), flv.astype(np.int64)
    tu, tv = fu - flu, fv - flv
    idx = np.empty((4,) + face.shape, np.int64)
    w = np.empty((4,) + face.shape, f32)
    for k in range(4):
        ox, oy = k & 1, k >> 1
        ix, iy = iu0 + ox, iv0 + oy
        w[k] = (tu if ox else 1 - tu) * (tv if oy else 1 - tv)
        out_x, out_y = (ix < 0) | (ix >= res), (iy < 0) | (iy >= res)
        inside = (face * res + iy) * res + ix
        a = f32(2.0) * ((ix.astype(f32) + f32(0.5)) / f32(res)) - f32(1.0)
        b = f32(2.0) * ((iy.astype(f32) + f32(0.5)) / f32(res)) - f32(1.0)
        f2, u2, v2 = cube_face_uv(*cube_dir_raw(a, b, face))
        x2 = np.clip(np.floor(u2 * f32(res)).astype(np.int64), 0, res - 1)
        y2 = np.clip(np.floor(v2 * f32(res)).astype(np.int64), 0, res - 1)
        edge = (f2 * res + y2) * res + x2
        idx[k] = np.where(~out_x & ~out_y, inside, np.where(out_x & out_y, -1, edge))
    idx[:, face < 0] = -1
    return idx, w


def get_mip(r, L):
    MINR, MAXR = f32(0.08), f32(0.5)
    lo = (np.clip(r, MINR, MAXR) - MINR) / (MAXR - MINR) * f32(L - 2)
    hi = (np.clip(r, MAXR, f32(1.0)) - MAXR) / (f32(1.0) - MAXR) + f32(L) - f32(2.0)
    return np.where(r < MAXR, lo, hi).astype(f32)


def entries(normals, view_dirs, rough, mask, spec_res, fine):
    """[8, H*W]: per pixel and tap slot (4 of l0, then 4 of l1) the key (level << 24 | texel) of every entry that adds
    to one of the `fine` levels, else -1.  normals [3, H, W] (view space, as shade_bwd reads them), view_dirs [H, W, 3]."""
    n = normals.reshape(3, -1).astype(f32)
    v = np.transpose(view_dirs, (2, 0, 1)).reshape(3, -1).astype(f32)
    ndv = (n * v).sum(0, dtype=f32)
    ref = f32(2.0) * np.maximum(ndv, f32(0)) * n - v
    rt = np.stack([-ref[1], ref[2], -ref[0]])
    L = len(spec_res)
    lvl = np.clip(get_mip(rough.reshape(-1).astype(f32), L), 0, L - 1)
    l0 = np.minimum(np.floor(lvl).astype(np.int64), L - 1)
    l1 = np.minimum(l0 + 1, L - 1)
    lf = lvl - l0
    keys = np.full((8, n.shape[1]), -1, np.int64)
    live = mask.reshape(-1)
    for slot, (lev, wl) in enumerate(((l0, np.where(l1 != l0, 1 - lf, 1)), (l1, np.where(l1 != l0, lf, 0)))):
        for li in fine:
            sel = np.nonzero((lev == li) & live & (wl != 0))[0]
            if sel.size == 0:
                continue
            idx, w = cube_taps(spec_res[li], rt[:, sel])
            for k in range(4):
                good = (idx[k] >= 0) & (w[k] * wl[sel] != 0)
                keys[4 * slot + k, sel[good]] = (li << 24) | idx[k][good]
    return keys


def count(keys, H, W):
    npx = H * W
    res = {"entries": int((keys >= 0).sum())}
    row_start = (np.arange(npx) % 16) == 0
    a = 0
    for s in range(8):
        k = keys[s]
        head = row_start.copy()
        head[1:] |= k[1:] != k[:-1]
        a += int((head & (k >= 0)).sum())
    res["rows"] = a
    yy, xx = np.divmod(np.arange(npx), W)
    blk = (yy // 8) * ((W + 7) // 8) + xx // 8
    tile = (yy // 32) * ((W + 31) // 32) + xx // 32
    ok = keys >= 0
    kk = keys[ok]
    wave_pairs = np.unique((np.broadcast_to(blk, keys.shape)[ok] << 27) | kk)
    tile_pairs = np.unique((np.broadcast_to(tile, keys.shape)[ok] << 27) | kk)
    res["wave"] = int(wave_pairs.size)
    n_tiles = int(tile.max()) + 1
    per_tile = np.bincount(tile_pairs >> 27, minlength=n_tiles)
    blk_tile = np.zeros(int(blk.max()) + 1, np.int64)
    blk_tile[blk] = tile
    b_per_tile = np.bincount(blk_tile[wave_pairs >> 27], minlength=n_tiles)
    hit = per_tile[per_tile > 0]
    res["tiles_hit"] = int(hit.size)
    res["tile_keys"] = (int(np.percentile(hit, 50)), int(np.percentile(hit, 90)), int(hit.max())) if hit.size else (0, 0, 0)
    for S in SLOTS:
        fits = per_tile <= S
        res["lds%d" % S] = int(np.where(fits, per_tile, b_per_tile).sum())
        res["lds%d_overflow" % S] = int((~fits).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--view", type=int, default=0, help="orbit view of bench.py's 64 (C2)")
    ap.add_argument("--res", type=int, default=800)
    ap.add_argument("--gaussians", type=int, default=300_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import scenes
    from oracle import oracle as orc
    from oracle import stage2_ref
    orc.build()
    orc.set_threads(orc.max_threads())
    t0 = time.time()
    sc = scenes.surface_scene(P=a.gaussians, sh_degree=2, seed=0)
    cam = scenes.orbit_camera(a.view, 64, a.res, a.res, radius=3.5)
    raw = stage2_ref.operator_forward(orc, sc, cam, dict(scenes.GI_DEFAULTS, start=8), 2)
    post = stage2_ref.gbuffer_post(orc, raw, cam["viewmatrix"])
    rough = (post["roughness_map"] * f32(1.0 - 0.04) + f32(0.04)).astype(f32)  # stage 2's remap (train.py:297-298)
    mask = post["normal_mask"].reshape(a.res, a.res)
    vd = stage2_ref.canonical_view_dirs(cam)
    spec_res = [256, 128, 64, 32, 16]  # CubemapLight(base_res=256).build_mips
    lines = ["shade backward, global adds into the fine light levels (one add = one texel's RGB triple)",
             "C2 view %d: %d Gaussians, %dx%d, %d masked pixels (oracle G-buffer, %.0f s)"
             % (a.view, a.gaussians, a.res, a.res, int(mask.sum()), time.time() - t0)]
    for name, fine in (("256^2+128^2+64^2", (0, 1, 2)), ("256^2", (0,)), ("128^2", (1,)), ("64^2", (2,))):
        r = count(entries(post["normal_map"], vd, rough, mask, spec_res, fine), a.res, a.res)
        lines += ["", "levels %s: %d tap entries" % (name, r["entries"]),
                  "  (a) rows, 16-lane runs       %9d adds" % r["rows"],
                  "  (b) 8x8 waves, distinct      %9d adds  (%.2fx fewer than (a))" % (r["wave"], r["rows"] / max(r["wave"], 1)),
                  "  32x32 tiles hit: %d, distinct keys per tile p50 / p90 / max %s"
                  % (r["tiles_hit"], " / ".join(map(str, r["tile_keys"])))]
        for S in SLOTS:
            lines.append("  (c) (b) + LDS table %4d slots %9d adds  (%.2fx fewer than (a)), %d tiles overflow"
                         % (S, r["lds%d" % S], r["rows"] / max(r["lds%d" % S], 1), r["lds%d_overflow" % S]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
