"""Drop-in `lpips` (LPIPS 0.1, VGG16 backbone) on the HIP library: the import the reference's evaluation scripts make.

    from lpips import LPIPS
    lpips_fn = LPIPS(net="vgg").cuda()          # render.py:200, relight_eval.py
    d = lpips_fn(gt_image, render_rgb)          # [3,H,W] or [N,3,H,W] -> float32 [N,1,1,1]

The whole network runs in libgigs_hip (gigs_lpips_vgg: f32 convolutions on MFMA, the value reduced in double in a fixed
order), so a pair gives the same bits on every call, alone or inside a batch, and the call can be captured in a graph.
Only the forward of lpips=True, spatial=False, version "0.1" with net="vgg" exists; there is no backward.

Weights (nothing is ever downloaded; a missing file raises FileNotFoundError naming the path):
  vgg_path     torchvision's VGG16 checkpoint (features.{idx}.weight / .bias), by default
               <torch.hub.get_dir()>/checkpoints/vgg16-397923af.pth, where torchvision caches it
  model_path   the lpips lin file (lin{k}.model.1.weight), by default weights/v0.1/vgg.pth next to this file, where the
               lpips package ships it
  state_dict   a whole lpips.LPIPS().state_dict() (net.slice{s}.{idx}.*, lin{k}.model.1.weight), as a dict or a file;
               it replaces both files
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

import gigs_lib

__all__ = ["LPIPS", "VGG_CONV_INDICES", "VGG_CHANNELS", "TAP_CHANNELS", "vgg_weights", "lin_weights", "load_weights",
           "default_vgg_path", "default_model_path"]

# torchvision vgg16().features: the conv indices, their (Cout, Cin); the pools sit at 4, 9, 16, 23
VGG_CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
VGG_CHANNELS = ((64, 3), (64, 64), (128, 64), (128, 128), (256, 128), (256, 256), (256, 256), (512, 256), (512, 512),
                (512, 512), (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
# lpips/pretrained_networks.py vgg16: slice s holds features[a:b] under their global index
_SLICE_BOUNDS = ((1, 0, 4), (2, 4, 9), (3, 9, 16), (4, 16, 23), (5, 23, 30))
MIN_SIDE = 16

Weights = Tuple[List[torch.Tensor], List[torch.Tensor], List[torch.Tensor]]


def _slice_of(idx: int) -> int:
    for s, a, b in _SLICE_BOUNDS:
        if a <= idx < b:
            return s
    raise ValueError(idx)


def default_vgg_path() -> str:
    return os.path.join(torch.hub.get_dir(), "checkpoints", "vgg16-397923af.pth")


def default_model_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "weights", "v0.1", "vgg.pth")


def _checked(t, shape, what: str) -> torch.Tensor:
    t = torch.as_tensor(t)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"lpips: {what} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.detach().to(torch.float32).contiguous()


def vgg_weights(sd: Dict[str, torch.Tensor]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """The 13 conv weights [Cout,Cin,3,3] and biases [Cout] from a torchvision VGG16 state dict (features.{idx}.*) or a
    whole LPIPS state dict (net.slice{s}.{idx}.*), in network order."""
    ws, bs = [], []
    for idx, (co, ci) in zip(VGG_CONV_INDICES, VGG_CHANNELS):
        for prefix in (f"features.{idx}.", f"net.slice{_slice_of(idx)}.{idx}."):
            if prefix + "weight" in sd:
                break
        else:
            raise KeyError(f"lpips: no weight for VGG16 feature {idx} (features.{idx}.weight or "
                           f"net.slice{_slice_of(idx)}.{idx}.weight)")
        ws.append(_checked(sd[prefix + "weight"], (co, ci, 3, 3), prefix + "weight"))
        bs.append(_checked(sd[prefix + "bias"], (co,), prefix + "bias"))
    return ws, bs


def lin_weights(sd: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
    """The 5 lin weights [1,C,1,1] -> [C] from the lpips lin file or a whole LPIPS state dict (lin{k}.model.1.weight)."""
    out = []
    for k, c in enumerate(TAP_CHANNELS):
        key = f"lin{k}.model.1.weight"
        if key not in sd:
            raise KeyError(f"lpips: no {key}")
        out.append(_checked(sd[key], (1, c, 1, 1), key).reshape(c))
    return out


def _load_file(path: str, what: str) -> Dict[str, torch.Tensor]:
    if not os.path.isfile(path):
        raise FileNotFoundError(f"lpips: {what} not found at {path} (it is never downloaded: put the file there or pass "
                                "its path)")
    return torch.load(path, map_location="cpu", weights_only=True)


def load_weights(pretrained: bool = True, model_path: Optional[str] = None, vgg_path: Optional[str] = None,
                 state_dict: Union[None, str, Dict[str, torch.Tensor]] = None) -> Weights:
    """(13 conv weights, 13 biases, 5 lin vectors) on the CPU.  state_dict (a whole LPIPS state dict or its file) gives
    everything; otherwise the convolutions come from vgg_path and, with pretrained=True, the lin weights from model_path.
    pretrained=False initialises the lin layers as torch.nn.Conv2d(C, 1, 1, bias=False) does."""
    if isinstance(state_dict, (str, os.PathLike)):
        state_dict = _load_file(os.fspath(state_dict), "LPIPS state dict")
    if state_dict is not None:
        ws, bs = vgg_weights(state_dict)
        return ws, bs, lin_weights(state_dict)
    ws, bs = vgg_weights(_load_file(vgg_path or default_vgg_path(), "torchvision VGG16 checkpoint"))
    if pretrained:
        lin = lin_weights(_load_file(model_path or default_model_path(), "lpips lin weights (v0.1/vgg.pth)"))
    else:
        lin = [torch.nn.Conv2d(c, 1, 1, bias=False).weight.detach().reshape(c).contiguous() for c in TAP_CHANNELS]
    return ws, bs, lin


def _ptrs(ts: Sequence[torch.Tensor]):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class LPIPS(torch.nn.Module):
    """lpips.LPIPS(net="vgg") in eval mode, forward only.  The weights are packed once per device (at construction on
    the current HIP device, and on the first call on any other); scratch is kept per (n, H, W, device).

    That scratch is shared by every call of one shape on this instance, graphs captured with it included (they hold its
    address).  Calls on one stream are ordered and safe.  Work that may overlap on different streams -- two evaluators
    replaying graphs on their own streams, or an evaluator and user code -- needs one LPIPS instance per stream."""

    def __init__(self, pretrained: bool = True, net: str = "vgg", version: str = "0.1", lpips: bool = True,
                 spatial: bool = False, pnet_rand: bool = False, pnet_tune: bool = False, use_dropout: bool = True,
                 model_path: Optional[str] = None, eval_mode: bool = True, verbose: bool = False,
                 vgg_path: Optional[str] = None, state_dict: Union[None, str, Dict[str, torch.Tensor]] = None):
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f"lpips: only net='vgg' is implemented, not {net!r}")
        if version != "0.1":
            raise NotImplementedError(f"lpips: only version '0.1' is implemented, not {version!r}")
        if spatial:
            raise NotImplementedError("lpips: spatial=True (per-pixel maps) is not implemented")
        if not lpips:
            raise NotImplementedError("lpips: lpips=False (the baseline without lin layers) is not implemented")
        if pnet_rand:
            raise NotImplementedError("lpips: pnet_rand=True needs random VGG weights: pass them as state_dict")
        self.net, self.version, self.spatial, self.pnet_tune = net, version, False, pnet_tune
        self._conv_w, self._conv_b, self._lin = load_weights(pretrained, model_path, vgg_path, state_dict)
        self._packed: Dict[torch.device, torch.Tensor] = {}
        self._scratch: Dict[tuple, torch.Tensor] = {}
        if verbose:
            print("Loading model from: %s" % ("state_dict" if state_dict is not None else (model_path or default_model_path())))
        if torch.cuda.is_available():
            self.packed(torch.device("cuda", torch.cuda.current_device()))
        self.eval()

    # -- nn.Module plumbing: there are no parameters; moving the module packs the weights on that device ---------------
    def _apply(self, fn, *args, **kwargs):
        probe = fn(torch.zeros(1))
        if probe.is_cuda:
            self.packed(probe.device)
        return self

    def weights(self) -> Weights:
        """(13 conv weights, 13 biases, 5 lin vectors) as loaded, on the CPU."""
        return self._conv_w, self._conv_b, self._lin

    def packed(self, device) -> torch.Tensor:
        """The gigs_lpips_vgg_pack buffer on `device`, packed on first use."""
        device = torch.device(device)
        t = self._packed.get(device)
        if t is None:
            lib = gigs_lib.lib()
            t = torch.empty(int(lib.gigs_lpips_vgg_weight_floats()), dtype=torch.float32, device=device)
            ws = [w.to(device) for w in self._conv_w]
            bs = [b.to(device) for b in self._conv_b]
            ls = [w.to(device) for w in self._lin]
            with torch.cuda.device(device):
                gigs_lib.check(lib.gigs_lpips_vgg_pack(_ptrs(ws), _ptrs(bs), _ptrs(ls), t.data_ptr(),
                                                       torch.cuda.current_stream().cuda_stream), "lpips_vgg_pack")
                torch.cuda.current_stream().synchronize()  # the unpacked copies die here
            self._packed[device] = t
        return t

    def scratch(self, n: int, H: int, W: int, device) -> torch.Tensor:
        device = torch.device(device)
        key = (int(n), int(H), int(W), device)
        t = self._scratch.get(key)
        if t is None:
            nbytes = int(gigs_lib.lib().gigs_lpips_vgg_scratch_bytes(n, H, W))
            if nbytes == 0:
                raise ValueError(f"lpips: images must be at least {MIN_SIDE}x{MIN_SIDE}, got {H}x{W}")
            t = self._scratch[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return t

    @staticmethod
    def _batched(x: torch.Tensor) -> torch.Tensor:
        if x.dim() == 3:
            x = x[None]
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"lpips: inputs must be [N,3,H,W] or [3,H,W], got {tuple(x.shape)}")
        return x.contiguous().float()

    @torch.no_grad()
    def record(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, slot: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, taps: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
        """gigs_lpips_vgg: the float64 records {lpips, tap 0 .. 4} (stride 6) of the n pairs.  With `slot` (an int32 device
        scalar) they go to rows *slot .. *slot + n - 1 of `out` and *slot advances on the device.  taps: None, or 10
        tensors [n,C,H_l,W_l] float32 that receive the raw taps of in0 then in1."""
        a, b = self._batched(in0), self._batched(in1)
        if a.shape != b.shape:
            raise ValueError(f"lpips: the inputs differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
        if not a.is_cuda or not b.is_cuda or a.device != b.device:
            raise RuntimeError("lpips needs both inputs on one HIP device: gigs-hip has no CPU path")
        n, _, H, W = a.shape
        if H < MIN_SIDE or W < MIN_SIDE:
            raise ValueError(f"lpips: images must be at least {MIN_SIDE}x{MIN_SIDE}, got {H}x{W}")
        dev = a.device
        if out is None:
            out = torch.empty((n, 6), dtype=torch.float64, device=dev)
        tp = None
        if taps is not None:
            if len(taps) != 10:
                raise ValueError("lpips: taps needs 10 tensors")
            tp = _ptrs(taps)
        packed, scratch = self.packed(dev), self.scratch(n, H, W, dev)
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            gigs_lib.check(gigs_lib.lib().gigs_lpips_vgg(n, H, W, a.data_ptr(), b.data_ptr(), int(bool(normalize)),
                                                         packed.data_ptr(), scratch.data_ptr(), p(slot), out.data_ptr(), tp,
                                                         torch.cuda.current_stream().cuda_stream), "lpips_vgg")
        return out

    def forward(self, in0: torch.Tensor, in1: torch.Tensor, retPerLayer: bool = False, normalize: bool = False):
        """lpips.LPIPS.forward: float32 [N,1,1,1] ([1,1,1,1] for [3,H,W] inputs); retPerLayer: (value, [5 x [N,1,1,1]])."""
        rec = self.record(in0, in1, normalize=normalize)
        n = rec.shape[0]
        val = rec[:, 0].float().reshape(n, 1, 1, 1)
        if retPerLayer:
            return val, [rec[:, 1 + k].float().reshape(n, 1, 1, 1) for k in range(5)]
        return val
