"""The a-trous denoiser of include/gigs_hip.h, "Denoising ray-traced planes", restated in numpy float32: every product and
sum is one float32 operation in the header's order, every max(a, b) is where(a > b, a, b), taps run row-major and a tap that is
not live or lies outside the image adds nothing.  csrc/denoise.hip must reproduce every bit (tests/test_gpu_denoise.py).
Vectorised over the pixels, one pass per tap; nothing here reads the product."""
import numpy as np

F = np.float32
H5 = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], F)  # exact in binary
EPS = F(1e-10)


def parameters(plane_distance, normal_power=32, sigma_l=4.0, roughness_sigma=None):
    """The host's numbers: e, inv_plane2, sigma_l2, eps, inv_rough2 (None without a roughness guide)."""
    e = int(normal_power).bit_length() - 1
    assert 1 << e == int(normal_power) and 0 <= e <= 7
    s = float(sigma_l)
    return dict(e=e, inv_plane2=F(1.0 / (float(plane_distance) * float(plane_distance))), sigma_l2=F(s * s),
                eps=EPS if s > 0.0 else F(np.inf),
                inv_rough2=None if roughness_sigma is None else F(1.0 / (float(roughness_sigma) * float(roughness_sigma))))


def live_pixels(signal, points, normals, mask, roughness=None):
    """[H,W] bool: mask set, and every guide component and signal value finite."""
    C, H, W = signal.shape
    live = (np.asarray(mask).reshape(H, W) != 0) & np.isfinite(signal).all(0)
    live &= np.isfinite(points).all(1).reshape(H, W) & np.isfinite(normals).all(1).reshape(H, W)
    if roughness is not None:
        live &= np.isfinite(roughness).reshape(H, W)
    return live


def _shift(a, oy, ox):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that pixel exists (inside), 0 elsewhere.  a: [H, W, ...]."""
    H, W = a.shape[:2]
    b = np.zeros_like(a)
    inside = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def _max0(a):
    return np.where(a > 0, a, F(0))


def _values(x, groups):
    """[G,H,W]: the value of each group, x_0 or (x_0 + x_1) + x_2."""
    out, c = [], 0
    for n in groups:
        out.append(x[c] if n == 1 else (x[c] + x[c + 1]) + x[c + 2])
        c += n
    return np.stack(out)


class _Guide:
    def __init__(self, points, normals, roughness, live, prm):
        H, W = live.shape
        self.P, self.N = points.reshape(H, W, 3).astype(F), normals.reshape(H, W, 3).astype(F)
        self.R = None if roughness is None else roughness.reshape(H, W).astype(F)
        self.live, self.prm = live, prm

    def tap(self, oy, ox):
        """(g [H,W] float32, alive [H,W] bool) of the tap at offset (oy, ox) from every centre."""
        Pq, inside = _shift(self.P, oy, ox)
        Nq, _ = _shift(self.N, oy, ox)
        lq, _ = _shift(self.live, oy, ox)
        alive = inside & lq
        P, N, prm = self.P, self.N, self.prm
        with np.errstate(all="ignore"):
            c = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
            c = _max0(c)
            for _ in range(prm["e"]):
                c = c * c
            d = ((Pq[..., 0] - P[..., 0]) * N[..., 0] + (Pq[..., 1] - P[..., 1]) * N[..., 1]) + (Pq[..., 2] - P[..., 2]) * N[..., 2]
            z = _max0(F(1) - (d * d) * prm["inv_plane2"])
            g = c * (z * z)
            if self.R is not None:
                Rq, _ = _shift(self.R, oy, ox)
                t = Rq - self.R
                u = _max0(F(1) - (t * t) * prm["inv_rough2"])
                g = g * (u * u)
        assert g.dtype == F
        return g, alive


def variance(x, groups, guide):
    """Launch A: [G,H,W] float32."""
    y = _values(x, groups)
    Gn, H, W = y.shape
    taps = [(dy, dx) + guide.tap(dy, dx) for dy in (-2, -1, 0, 1, 2) for dx in (-2, -1, 0, 1, 2)]
    var = np.zeros((Gn, H, W), F)
    with np.errstate(all="ignore"):
        for j in range(Gn):
            yq = [_shift(y[j], dy, dx)[0] for dy, dx, _, _ in taps]
            Gs, T = np.zeros((H, W), F), np.zeros((H, W), F)
            for (_, _, g, alive), q in zip(taps, yq):
                Gs = np.where(alive, Gs + g, Gs)
                T = np.where(alive, T + g * (q - y[j]), T)
            m = y[j] + T / Gs
            U = np.zeros((H, W), F)
            for (_, _, g, alive), q in zip(taps, yq):
                t = q - m
                U = np.where(alive, U + g * (t * t), U)
            var[j] = np.where(guide.live & (Gs > 0), U / Gs, F(0))
    return var


def step(x, var, groups, guide, s):
    """Launch B at step s: (x' [C,H,W], var' [G,H,W])."""
    prm = guide.prm
    y = _values(x, groups)
    Gn, H, W = y.shape
    taps = [(i, k) + guide.tap((i - 2) * s, (k - 2) * s) for i in range(5) for k in range(5)]
    x2, var2 = x.copy(), var.copy()
    with np.errstate(all="ignore"):
        c0 = 0
        for j, n in enumerate(groups):
            r = F(1) / (prm["sigma_l2"] * var[j] + prm["eps"])
            Wsum, V = np.zeros((H, W), F), np.zeros((H, W), F)
            D = [np.zeros((H, W), F) for _ in range(n)]
            for i, k, g, alive in taps:
                oy, ox = (i - 2) * s, (k - 2) * s
                delta = _shift(y[j], oy, ox)[0] - y[j]
                l = _max0(F(1) - (delta * delta) * r)
                w = ((H5[i] * H5[k]) * g) * (l * l)
                assert w.dtype == F
                Wsum = np.where(alive, Wsum + w, Wsum)
                for c in range(n):
                    D[c] = np.where(alive, D[c] + w * (_shift(x[c0 + c], oy, ox)[0] - x[c0 + c]), D[c])
                V = np.where(alive, V + (w * w) * _shift(var[j], oy, ox)[0], V)
            ok = guide.live & (Wsum > 0)
            for c in range(n):
                x2[c0 + c] = np.where(ok, x[c0 + c] + D[c] / Wsum, x[c0 + c])
            var2[j] = np.where(ok, V / (Wsum * Wsum), var[j])
            c0 += n
    return x2, var2


def atrous(signal, points, normals, mask, groups=None, iterations=4, plane_distance=1.0, normal_power=32, sigma_l=4.0,
           roughness=None, roughness_sigma=0.25):
    """(filtered [C,H,W], variance [G,H,W]) float32, as denoise.atrous with an explicit plane_distance."""
    signal = np.ascontiguousarray(signal, F)
    C, H, W = signal.shape
    groups = [1] * C if groups is None else [int(g) for g in groups]
    assert all(g in (1, 3) for g in groups) and sum(groups) == C and 1 <= C <= 16 and 1 <= iterations <= 5
    points, normals = np.asarray(points, F).reshape(H * W, 3), np.asarray(normals, F).reshape(H * W, 3)
    roughness = None if roughness is None else np.asarray(roughness, F).reshape(H * W)
    prm = parameters(plane_distance, normal_power, sigma_l, None if roughness is None else roughness_sigma)
    live = live_pixels(signal, points, normals, mask, roughness)
    guide = _Guide(points, normals, roughness, live, prm)
    # a pixel that is not live is never read as a tap (alive is False there), and np.where keeps its bits as a centre
    x = signal.copy()
    var = variance(x, groups, guide)
    for i in range(iterations):
        x, var = step(x, var, groups, guide, 1 << i)
    keep = ~live
    x[:, keep] = signal[:, keep]
    var[:, keep] = 0
    return x, var


# ---- guides for the tests ---------------------------------------------------------------------------------------------------
def flat_guide(H, W, pitch=1.0):
    """A plane z = 0 seen head on: points (x pitch, y pitch, 0), normals +z, mask all set."""
    ys, xs = np.mgrid[0:H, 0:W]
    points = np.stack([xs * pitch, ys * pitch, np.zeros((H, W))], -1).reshape(-1, 3).astype(F)
    normals = np.tile(np.array([0.0, 0.0, 1.0], F), (H * W, 1))
    return points, normals, np.ones(H * W, np.uint8)


def crease_guide(H, W, pitch=1.0, step_height=3.0):
    """A floor z = 0 left of the column W // 2 that meets a wall at 90 degrees there (normal -x, rising with x), and a depth step
    of `step_height` below the row H // 3 of the floor.  -> (points, normals, mask, region [H,W] int: 0 floor, 1 lowered
    floor, 2 wall)."""
    ys, xs = np.mgrid[0:H, 0:W]
    fold = W // 2
    wall = xs >= fold
    low = (~wall) & (ys < H // 3)
    px = np.where(wall, fold * pitch, xs * pitch)
    pz = np.where(wall, (xs - fold) * pitch, np.where(low, -step_height, 0.0))
    points = np.stack([px, ys * pitch, pz], -1).reshape(-1, 3).astype(F)
    normals = np.where(wall[..., None], np.array([-1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])).reshape(-1, 3).astype(F)
    region = np.where(wall, 2, np.where(low, 1, 0))
    return points, normals, np.ones(H * W, np.uint8), region
