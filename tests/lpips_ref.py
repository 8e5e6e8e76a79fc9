"""Float64 restatement of LPIPS 0.1 with the VGG16 backbone (net="vgg", lpips=True, spatial=False, eval mode) on the
CPU, written with plain conv2d / max_pool2d from the same 13 + 13 + 5 tensors the drop-in lpips package loads.  Test
helper only; also the seeded random weights the tests use."""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# conv layers per tap (the pools sit before the first conv of taps 1..4)
LAYERS_PER_TAP = (2, 2, 3, 3, 3)
VGG_CHANNELS = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512),
                (512, 512), (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)


def random_weights(seed: int = 0):
    """He-initialised conv weights (activations stay O(1) through 13 layers), small biases, non-negative lin weights."""
    g = torch.Generator().manual_seed(seed)
    ws, bs = [], []
    for co, ci in VGG_CHANNELS:
        ws.append(torch.randn((co, ci, 3, 3), generator=g, dtype=torch.float64).mul_((2.0 / (9 * ci)) ** 0.5).float())
        bs.append(torch.randn((co,), generator=g, dtype=torch.float64).mul_(0.05).float())
    lin = [torch.rand((c,), generator=g, dtype=torch.float64).mul_(2.0 / c).float() for c in TAP_CHANNELS]
    return ws, bs, lin


def _conv3x3_matmul(h: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """3x3 conv, padding 1, as nine shifted float64 matrix products (for large images on the GPU, where it needs nothing
    but a float64 GEMM)."""
    n, c, H, W = h.shape
    hp = F.pad(h, (1, 1, 1, 1))
    out = b[:, None].expand(-1, n * H * W).clone()
    for ky in range(3):
        for kx in range(3):
            xs = hp[:, :, ky:ky + H, kx:kx + W].transpose(0, 1).reshape(c, -1)
            out += w[:, :, ky, kx] @ xs
    return out.reshape(-1, n, H, W).transpose(0, 1)


def taps(x: torch.Tensor, ws, bs, normalize: bool = False, device=None):
    """The five raw taps (after the ReLU of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3) of x [N,3,H,W], float64.
    device=None: on the CPU with conv2d; otherwise on that device with _conv3x3_matmul (still float64 throughout)."""
    dev = torch.device("cpu") if device is None else torch.device(device)
    conv = (lambda h, w, b: F.conv2d(h, w, b, padding=1)) if device is None else _conv3x3_matmul
    x = x.to(dev).double()
    if normalize:
        x = 2 * x - 1
    shift = torch.tensor(SHIFT, dtype=torch.float64, device=dev)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=torch.float64, device=dev)[None, :, None, None]
    h = (x - shift) / scale
    out, layer = [], 0
    for t, nl in enumerate(LAYERS_PER_TAP):
        if t > 0:
            h = F.max_pool2d(h, 2, 2)
        for _ in range(nl):
            h = F.relu(conv(h, ws[layer].to(dev).double(), bs[layer].to(dev).double()))
            layer += 1
        out.append(h)
    return out


def lpips(in0: torch.Tensor, in1: torch.Tensor, ws, bs, lin, normalize: bool = False, device=None):
    """(value [N], per-tap terms [5][N]) in float64 (on `device` as taps() says; the results on the CPU)."""
    t0, t1 = taps(in0, ws, bs, normalize, device), taps(in1, ws, bs, normalize, device)
    terms = []
    for k, (a, b) in enumerate(zip(t0, t1)):
        na = a / (torch.sqrt((a * a).sum(dim=1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b * b).sum(dim=1, keepdim=True)) + 1e-10)
        d = ((na - nb) ** 2 * lin[k].to(a.device).double()[None, :, None, None]).sum(dim=1)
        terms.append(d.mean(dim=(1, 2)).cpu())
    val = terms[0]
    for t in terms[1:]:
        val = val + t
    return val, terms


def state_dicts(ws, bs, lin):
    """The same weights in the three key layouts the loader accepts: (torchvision, lpips lin file, whole LPIPS)."""
    idx = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
    slices = ((1, 0, 4), (2, 4, 9), (3, 9, 16), (4, 16, 23), (5, 23, 30))
    tv, whole = {}, {}
    for i, w, b in zip(idx, ws, bs):
        tv[f"features.{i}.weight"], tv[f"features.{i}.bias"] = w.clone(), b.clone()
        s = next(s for s, a, e in slices if a <= i < e)
        whole[f"net.slice{s}.{i}.weight"], whole[f"net.slice{s}.{i}.bias"] = w.clone(), b.clone()
    tv["classifier.0.weight"] = torch.zeros(4, 4)
    linf = {f"lin{k}.model.1.weight": w.reshape(1, -1, 1, 1).clone() for k, w in enumerate(lin)}
    whole.update(linf)
    whole["scaling_layer.shift"] = torch.tensor(SHIFT)[None, :, None, None]
    whole["scaling_layer.scale"] = torch.tensor(SCALE)[None, :, None, None]
    return tv, linf, whole
