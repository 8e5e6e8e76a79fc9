"""numpy restatement of the image writer's device stages, written from the PNG specification (section 9, "Filtering") and
from torchvision's save_image rounding -- the reference the GPU kernels are compared with, byte for byte."""
import numpy as np


def quantize(x, bias=0.5):
    """[C,H,W] float32 (C = 1 or 3) -> [H,W,3] uint8: trunc(clamp(x * 255 + bias, 0, 255)) with the product and the sum
    rounded to float32 one after the other; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    t = (x * np.float32(255.0)).astype(np.float32) + np.float32(bias)
    t = np.where(np.isnan(t), np.float32(0.0), np.clip(t, 0.0, 255.0))
    q = t.astype(np.uint8)
    if q.shape[0] == 1:
        q = np.repeat(q, 3, axis=0)
    return np.ascontiguousarray(q.transpose(1, 2, 0))


def filter_row(cur, up, ftype, bpp=3):
    """One row (uint8 [N]) filtered with `ftype`; `up` is the unfiltered row above (zeros for the first row)."""
    x = cur.astype(np.int32)
    b = up.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), x[:-bpp]]) if len(x) > bpp else np.zeros_like(x)
    c = np.concatenate([np.zeros(bpp, np.int32), b[:-bpp]]) if len(x) > bpp else np.zeros_like(x)
    if ftype == 0:
        pred = np.zeros_like(x)
    elif ftype == 1:
        pred = a
    elif ftype == 2:
        pred = b
    elif ftype == 3:
        pred = (a + b) // 2
    else:
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return ((x - pred) & 0xFF).astype(np.uint8)


def scanlines(img):
    """[H,W,3] uint8 -> (the scanline stream as bytes: per row the filter type and the filtered row; the filter types
    [H]).  Each row takes the filter with the smallest sum of |residual as int8|, ties to the lowest type."""
    H, W, _ = img.shape
    rows = img.reshape(H, 3 * W)
    out = np.empty((H, 1 + 3 * W), np.uint8)
    types = np.empty(H, np.int64)
    zero = np.zeros(3 * W, np.uint8)
    for y in range(H):
        cand = [filter_row(rows[y], rows[y - 1] if y else zero, f) for f in range(5)]
        sums = [int(np.abs(r.astype(np.int8).astype(np.int32)).sum()) for r in cand]
        f = int(np.argmin(sums))  # the first minimum
        types[y] = f
        out[y, 0] = f
        out[y, 1:] = cand[f]
    return out.tobytes(), types


def test_image(H, W, seed=0):
    """[3,H,W] float32 with regions that favour different filters: constant rows, a horizontal ramp, a vertical ramp,
    uniform noise, and sinusoids with mild noise elsewhere."""
    rng = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    img = np.stack([0.5 + 0.4 * np.sin(x / 7.0 + y / 11.0), 0.5 + 0.4 * np.sin(x / 5.0 - y / 3.0),
                    0.5 + 0.4 * np.cos(x / 13.0) * np.sin(y / 4.0)]).astype(np.float32)
    img += rng.normal(0.0, 0.01, img.shape).astype(np.float32)
    img[:, :H // 8] = 0.0
    img[:, H // 8:H // 4] = (x / W)[H // 8:H // 4]
    img[:, H // 4:H // 2] = (y / H)[H // 4:H // 2]
    img[:, H // 2:5 * H // 8] = rng.uniform(0.0, 1.0, (3, 5 * H // 8 - H // 2, W)).astype(np.float32)
    return img


test_image.__test__ = False  # a helper, not a test
