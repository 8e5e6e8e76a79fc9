"""The sparse paths of the GGX backward (csrc/light_filter.hip) under clustered gradients.

specular_tile_gather_body: a workgroup owns a 16 x 16 tile of destination texels of one face and a slice of 256 slots of
the level's list, and sums the listed texels whose own rectangle on that face meets the tile.  A level whose mean window
holds at most 256 candidates is scattered instead, one wave per slot (specular_scatter_body); tile_plan below restates
the host's choice.

The levels and the float64 reference are those of test_gpu_spec_sparse.py (imported), the capacity is its 100 permille:
  (16, 0.08)  narrow windows: scattered              (16, 1.0)   the window spans the whole cube, one tile per face
  (32, 0.22)  four tiles per face                    (64, 0.08)  window narrower than a tile: scattered
  (64, 0.28)  window about a tile                    (64, 0.36)  window wider than a tile, 16 tiles per face, 10 slices
The gradients are clustered, as the step's are: a filled block in a cube corner (windows over three faces), two blocks
on opposite faces, one tile's worth of texels all nonzero up to the capacity (the hot tile: at res 64 its 256 sources
fill one slice and land in every tile around it), a one-texel line along a face edge, and the NaN / Inf / -0 cases.

Every case asserts the path taken and the count from the state buffer, the project's bound -- the largest deviation from
the float64 reference is at most 4x max(the gather's own deviation, one ulp of the peak) -- and that an all-zero gradient
gives an all-zero output.
"""
import numpy as np
import pytest

from test_gpu_spec_sparse import PERMILLE, deviation, level, reference, run, texel

pytestmark = pytest.mark.gpu
LEVELS = [(16, 0.08), (16, 1.0), (32, 0.22), (64, 0.08), (64, 0.28), (64, 0.36)]


def tile_plan(res, avg_window, cap):
    """(scattered, tiles per face, slices) as gigs_specular_cubemap_multi_bwd_sparse of csrc/light_filter.hip chooses them."""
    return avg_window <= 256, ((res + 15) // 16) ** 2, (cap + 255) // 256


def test_levels_cover_both_sparse_paths():
    plans = {(r, a): tile_plan(r, level(r, a)["avg"], 6 * r * r * PERMILLE // 1000) for r, a in LEVELS}
    print("plans (scattered, tiles per face, slices):", plans)
    tiled = [p for p in plans.values() if not p[0]]
    assert any(p[0] for p in plans.values())
    assert any(p[1] == 1 for p in tiled) and any(p[1] > 1 for p in tiled), plans  # one tile per face, and several
    assert any(p[2] == 1 for p in tiled) and any(p[2] > 1 for p in tiled), plans  # stored, and added slice by slice


def block(res, face, y0, x0, h, w):
    return [texel(res, face, y, x) for y in range(y0, min(res, y0 + h)) for x in range(x0, min(res, x0 + w))]


def gradients(res, rng, cap):
    """name -> [total, 3] gradient; every pattern holds at most `cap` nonzero texels."""
    total = 6 * res * res

    def at(idx):
        idx = list(idx)[:cap]
        g = np.zeros((total, 3), np.float32)
        g[idx] = rng.normal(size=(len(idx), 3)).astype(np.float32)
        g[idx, 0] += 4.0  # no listed texel rounds to all-zero
        return g

    out = {"zero": np.zeros((total, 3), np.float32)}
    out["corner_block"] = at(block(res, 4, 0, 0, 10, 10))
    out["opposite_blocks"] = at(block(res, 0, res // 2 - 3, res // 2 - 3, 6, 6) + block(res, 1, res // 2 - 3, 1, 6, 6))
    # the hot tile: the 16 x 16 tile at (16, 16) of face 2 (the whole face at res 16), filled up to the capacity
    t0 = 16 if res >= 32 else 0
    out["hot_tile"] = at(block(res, 2, t0, t0, 16, 16))
    out["edge_line"] = at([texel(res, 3, y, res - 1) for y in range(res)])
    g = at(block(res, 5, 2, 2, 3, 3))
    g[texel(res, 0, 3, 4)] = (0.0, -0.0, 1.5)  # one channel only
    g[texel(res, 5, 7, 7)] = (-0.0, -0.0, -0.0)  # -0 is not nonzero
    g[texel(res, 1, 2, 3)] = (np.nan, 0.0, 0.0)
    g[texel(res, 4, res - 1, res - 1)] = (0.0, np.inf, -1.0)
    out["nan_inf_minus_zero"] = g
    return out


@pytest.mark.parametrize("res,rough", LEVELS)
def test_tile_gather_matches_float64_reference(res, rough):
    lv = level(res, rough)
    total = 6 * res * res
    cap = total * PERMILLE // 1000
    rng = np.random.default_rng(1000 * res + int(100 * rough))
    for name, g in gradients(res, rng, cap).items():
        count = int((g != 0).any(1).sum())
        assert count <= cap, (name, count, cap)
        (sp,), ((sparse, n),) = run([lv], [g], sparse=True)
        assert sparse and n == count, (name, sparse, n, count)
        if name == "zero":
            assert not sp.any()
            continue
        (de,), _ = run([lv], [g], sparse=False)
        ref = reference(lv, g)
        dev_s, dev_d = deviation(sp, ref), deviation(de, ref, gather=True)
        peak = float(np.abs(ref[np.isfinite(ref)]).max()) if np.isfinite(ref).any() else 0.0
        floor = float(np.spacing(np.float32(peak)))
        print(f"res {res} roughness {rough} {name}: count {n} peak {peak:.3e} sparse dev {dev_s:.3e} dense dev {dev_d:.3e} "
              f"floor {floor:.3e}")
        assert dev_s <= 4.0 * max(dev_d, floor), (name, dev_s, dev_d, floor)
