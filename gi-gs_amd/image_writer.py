"""Writing images: PNG files from device planes, Radiance .hdr files on the host.

    png_bytes(stream, W, H)          a complete 8-bit RGB PNG around a scanline stream that is already filtered (H rows of
                                     1 + 3 W bytes: filter type, filtered row): signature, IHDR, one IDAT, IEND.  Pure Python
                                     + zlib, no GPU.
    encode / quantize                the two device stages on their own (gigs_pack_images, gigs_png_filter), synchronous
                                     conveniences for tests and for callers that want the 8-bit sheet back
    ImageWriter(workers, slots)      the asynchronous writer: submit() enqueues quantisation + PNG filtering of every image
                                     of a view on the current stream (one launch each), copies the scanline streams -- 3
                                     bytes per pixel instead of 12 -- into pinned memory and returns; threads deflate
                                     and write
    read_hdr / write_hdr             Radiance RGBE (.hdr) <-> float32 [H,W,3]

Why the split: of a PNG encoder only the entropy coder is serial.  Quantisation and the per-row filter choice are
byte-parallel with a per-row reduction and run where the planes already are; the host deflates filtered bytes with
zlib's run-length strategy at level 1 (the filters have done the modelling; zlib releases the GIL, so the threads
scale) and writes path + ".tmp", then renames.

The 8-bit values are torchvision.utils.save_image's (bias 0.5: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)) or, with
bias 0, ToPILImage's x.mul(255).byte(), bit for bit (gigs_pack_images, include/gigs_hip.h).
"""
from __future__ import annotations

import ctypes as C
import os
import queue
import struct
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Union

import numpy as np

MAX_WORKERS = 16
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- PNG container (host, no GPU) -----------------------------------------------------------------------------------------
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF)


def png_bytes(stream, W: int, H: int) -> bytes:
    """The PNG file (8 bits per sample, colour type 2) whose filtered scanlines are `stream`: any object with the buffer
    protocol holding H * (1 + 3 W) bytes.  The stream is deflated with level 1 and Z_RLE: after the PNG filters the
    redundancy left is runs, and run-length matching costs a fraction of the hash-chain search."""
    W, H = int(W), int(H)
    if W <= 0 or H <= 0:
        raise ValueError("png_bytes: W and H must be positive")
    view = memoryview(stream).cast("B")
    if view.nbytes != H * (1 + 3 * W):
        raise ValueError("png_bytes: the stream has %d bytes, %d x %d needs %d" % (view.nbytes, W, H, H * (1 + 3 * W)))
    z = zlib.compressobj(1, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    data = z.compress(view) + z.flush()
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return _PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", data) + _chunk(b"IEND", b"")


# ---- Radiance RGBE --------------------------------------------------------------------------------------------------------
def _rgbe_to_float(rgbe: np.ndarray) -> np.ndarray:
    e = rgbe[..., 3].astype(np.int32)
    scale = np.where(e > 0, np.ldexp(np.float32(1.0), e - 136), np.float32(0.0)).astype(np.float32)
    return rgbe[..., :3].astype(np.float32) * scale[..., None]


def float_to_rgbe(rgb: np.ndarray) -> np.ndarray:
    """Radiance's float2rgbe (color.c setcolr): v = max(r, g, b); v < 1e-32 -> (0, 0, 0, 0); otherwise v = m 2^e with m in
    [0.5, 1), the mantissas trunc(c * m * 256 / v) and the exponent byte e + 128.  uint8 [..., 4]."""
    rgb = np.asarray(rgb, dtype=np.float32)
    v = rgb.max(axis=-1)
    ok = v >= 1e-32
    m, e = np.frexp(np.where(ok, v, 1.0).astype(np.float32))
    scale = (m.astype(np.float32) * np.float32(256.0) / np.where(ok, v, 1.0).astype(np.float32)).astype(np.float32)
    mant = np.clip(np.maximum(rgb, 0.0) * scale[..., None], 0, 255).astype(np.uint8)
    out = np.concatenate([mant, np.clip(e + 128, 0, 255).astype(np.uint8)[..., None]], axis=-1)
    out[~ok] = 0
    return out


def _rle_channel(row: np.ndarray) -> bytes:
    """One channel of a scanline in Radiance's new run-length form: a count byte > 128 is a run of count - 128 copies of
    the next byte (runs of at least 4 are taken), a count byte <= 128 that many literal bytes."""
    out = bytearray()
    n = len(row)
    change = np.flatnonzero(row[1:] != row[:-1]) + 1
    starts = np.concatenate(([0], change))
    lengths = np.diff(np.concatenate((starts, [n])))
    lit_from = None

    def flush_literals(upto):
        nonlocal lit_from
        p = lit_from
        while p is not None and p < upto:
            k = min(128, upto - p)
            out.append(k)
            out.extend(row[p:p + k].tobytes())
            p += k
        lit_from = None

    for s, ln in zip(starts.tolist(), lengths.tolist()):
        if ln >= 4:
            flush_literals(s)
            left, val = ln, int(row[s])
            while left > 0:
                k = min(127, left)
                if k < 4 and left != ln:  # a short remainder of a long run goes out as literals
                    out.append(k)
                    out.extend(bytes([val]) * k)
                else:
                    out.append(128 + k)
                    out.append(val)
                left -= k
        elif lit_from is None:
            lit_from = s
    flush_literals(n)
    return bytes(out)


def write_hdr(path: str, rgb, rle: bool = False) -> None:
    """float [H,W,3] RGB -> a Radiance picture ("#?RADIANCE", FORMAT=32-bit_rle_rgbe, "-Y H +X W"), quantised by
    float_to_rgbe.  rle=False writes flat scanlines (4 bytes per pixel; every reader accepts them), rle=True the new
    run-length form (needs 8 <= W <= 32767, otherwise flat as the format demands)."""
    rgb = np.asarray(rgb, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("write_hdr: expected [H,W,3]")
    H, W = rgb.shape[:2]
    px = float_to_rgbe(rgb)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n" + ("-Y %d +X %d\n" % (H, W)).encode()
    if rle and 8 <= W <= 32767:
        body = bytearray()
        for y in range(H):
            body += bytes([2, 2, W >> 8, W & 255])
            for c in range(4):
                body += _rle_channel(np.ascontiguousarray(px[y, :, c]))
        body = bytes(body)
    else:
        body = px.tobytes()
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(head + body)
    os.replace(tmp, path)


def read_hdr(path: str) -> np.ndarray:
    """A Radiance picture -> float32 [H,W,3] RGB.  Header "#?RADIANCE" / "#?RGBE", resolution "-Y H +X W", flat or new-style
    run-length scanlines (the old repeat-pixel encoding is not supported).  A pixel decodes to mantissa * 2^(e - 136) and
    e = 0 to 0, without the half step ((m + 0.5) * ...) some decoders add: that is what cv2.imdecode gives the reference's
    reader (relight.py:32-45) as far as OpenCV's rgbe decoder is remembered here -- OpenCV was not at hand, so this
    convention is stated, not checked against it.  Malformed input raises ValueError."""
    with open(path, "rb") as f:
        data = f.read()
    if not (data.startswith(b"#?RADIANCE") or data.startswith(b"#?RGBE")):
        raise ValueError(f"{path}: not a Radiance picture (magic)")
    end = data.find(b"\n\n")
    if end < 0:
        raise ValueError(f"{path}: truncated header")
    if b"FORMAT=32-bit_rle_xyze" in data[:end]:
        raise ValueError(f"{path}: XYZE pictures are not supported")
    nl = data.find(b"\n", end + 2)
    if nl < 0:
        raise ValueError(f"{path}: truncated header (no resolution line)")
    res = data[end + 2:nl].split()
    if len(res) != 4 or res[0] != b"-Y" or res[2] != b"+X":
        raise ValueError(f"{path}: unsupported resolution line {data[end + 2:nl]!r} (expected -Y H +X W)")
    try:
        H, W = int(res[1]), int(res[3])
    except ValueError:
        raise ValueError(f"{path}: bad resolution line") from None
    if H <= 0 or W <= 0:
        raise ValueError(f"{path}: bad resolution")
    buf = np.frombuffer(data, dtype=np.uint8, offset=nl + 1)
    px = np.empty((H, W, 4), dtype=np.uint8)
    if buf.size == H * W * 4 and not (8 <= W <= 32767 and buf[0] == 2 and buf[1] == 2 and ((int(buf[2]) << 8) | int(buf[3])) == W):
        px[:] = buf.reshape(H, W, 4)
        return _rgbe_to_float(px)
    p, n = 0, buf.size
    for y in range(H):
        if p + 4 > n:
            raise ValueError(f"{path}: truncated at scanline {y}")
        if 8 <= W <= 32767 and buf[p] == 2 and buf[p + 1] == 2 and ((int(buf[p + 2]) << 8) | int(buf[p + 3])) == W:
            p += 4
            for c in range(4):
                x = 0
                while x < W:
                    if p >= n:
                        raise ValueError(f"{path}: truncated at scanline {y}")
                    k = int(buf[p])
                    p += 1
                    if k > 128:
                        k -= 128
                        if p >= n or x + k > W:
                            raise ValueError(f"{path}: bad run at scanline {y}")
                        px[y, x:x + k, c] = buf[p]
                        p += 1
                    else:
                        if k == 0 or p + k > n or x + k > W:
                            raise ValueError(f"{path}: bad literal packet at scanline {y}")
                        px[y, x:x + k, c] = buf[p:p + k]
                        p += k
                    x += k
        else:
            if p + 4 * W > n:
                raise ValueError(f"{path}: truncated at scanline {y}")
            px[y] = buf[p:p + 4 * W].reshape(W, 4)
            p += 4 * W
    return _rgbe_to_float(px)


def load_latlong(path: str) -> np.ndarray:
    """An environment map for --hdri: `.npy` ([H,W,3] float32, as before) or a Radiance `.hdr`."""
    if path.endswith(".npy"):
        return np.load(path).astype(np.float32)
    if path.endswith(".hdr"):
        return read_hdr(path)
    raise ValueError("--hdri: pass the latitude-longitude map as a .npy [H,W,3] float32 array or a Radiance .hdr file")


# ---- the device stages ----------------------------------------------------------------------------------------------------
class Image:
    """One file to write: `planes` is a tensor [C,H,W] (C = 1 or 3; [H,W] counts as C = 1) or a sequence of such tensors of
    one height, laid side by side (render.py's brdf image).  bias: 0.5 = save_image's rounding, 0 = ToPILImage's
    truncation.  normalize=True maps each plane to (x - min) / (max - min) first (render.py:376's depth image)."""

    def __init__(self, path: Optional[str], planes, bias: float = 0.5, normalize: bool = False):
        import torch
        if isinstance(planes, torch.Tensor):
            planes = [planes]
        ps = []
        for t in planes:
            if t.dim() == 2:
                t = t[None]
            if t.dim() != 3 or t.shape[0] not in (1, 3) or t.shape[1] < 1 or t.shape[2] < 1:
                raise ValueError("Image: planes must be [C,H,W] with C = 1 or 3, got %s" % (tuple(t.shape),))
            if not t.is_cuda:
                raise RuntimeError("Image: planes must be CUDA/HIP tensors: gigs-hip has no CPU path")
            ps.append(t.detach().float().contiguous())
        if not ps or any(t.shape[1] != ps[0].shape[1] for t in ps):
            raise ValueError("Image: the planes of one file must have the same height")
        self.path, self.planes, self.bias, self.normalize = path, ps, float(bias), bool(normalize)
        self.H = int(ps[0].shape[1])
        self.W = sum(int(t.shape[2]) for t in ps)


def _as_image(item) -> Image:
    if isinstance(item, Image):
        return item
    path, planes = item[0], item[1]
    return Image(path, planes, *item[2:])


def _up(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class _Layout:
    """Where the sheets and scanline streams of a batch of images lie in two byte buffers (16-byte aligned starts, sheet
    rows padded to 16 bytes so that the filter kernel takes its dwordx4 path), and the two descriptor tables."""

    def __init__(self, images: Sequence[Image]):
        import gigs_lib
        self.images = images
        self.sheet_off, self.stream_off, self.strides = [], [], []
        so = to = 0
        self.n_pack = self.n_norm = 0
        for im in images:
            stride = _up(3 * im.W)
            self.sheet_off.append(so)
            self.stream_off.append(to)
            self.strides.append(stride)
            so += _up(stride * im.H)
            to += _up(im.H * (1 + 3 * im.W))
            self.n_pack += len(im.planes)
            if im.normalize:
                self.n_norm += len(im.planes)
        self.sheet_bytes, self.stream_bytes = so, to
        if len(images) > gigs_lib.MAX_IMAGES or self.n_pack > gigs_lib.MAX_IMAGES:
            raise ValueError("too many images in one batch (limit %d)" % gigs_lib.MAX_IMAGES)
        self.table_bytes = _up(self.n_pack * C.sizeof(gigs_lib.PackDesc)) + _up(len(images) * C.sizeof(gigs_lib.FilterDesc))

    def tables(self, sheet_ptr: int, stream_ptr: int, lohi_ptr: int):
        """(pack descriptors, filter descriptors, [(plane, lohi pointer)] for the planes to normalise)."""
        import gigs_lib
        pack = (gigs_lib.PackDesc * max(1, self.n_pack))()
        filt = (gigs_lib.FilterDesc * max(1, len(self.images)))()
        norms = []
        k = 0
        for i, im in enumerate(self.images):
            x = 0
            for t in im.planes:
                lohi = 0
                if im.normalize:
                    lohi = lohi_ptr + 8 * len(norms)
                    norms.append((t, lohi))
                d = pack[k]
                d.src, d.dst, d.lohi = t.data_ptr(), sheet_ptr + self.sheet_off[i], lohi or None
                d.channels, d.height, d.width = int(t.shape[0]), im.H, int(t.shape[2])
                d.dst_x, d.dst_stride, d.bias = x, self.strides[i], im.bias
                x += int(t.shape[2])
                k += 1
            f = filt[i]
            f.sheet, f.out = sheet_ptr + self.sheet_off[i], stream_ptr + self.stream_off[i]
            f.height, f.width, f.stride, f.reserved = im.H, im.W, self.strides[i], 0
        return pack, filt, norms


def _launch(layout: _Layout, sheets, streams, lohi, scratch, table_host, table_dev, stream_handle) -> None:
    """minmax (per normalised plane), the descriptor upload, pack, filter -- all on the current stream."""
    import gigs_lib
    lib = gigs_lib.lib()
    pack, filt, norms = layout.tables(sheets.data_ptr(), streams.data_ptr(), 0 if lohi is None else lohi.data_ptr())
    for t, ptr in norms:
        gigs_lib.check(lib.gigs_plane_minmax(t.numel(), t.data_ptr(), scratch.data_ptr(), ptr, stream_handle), "plane_minmax")
    npk, nf = layout.n_pack * C.sizeof(gigs_lib.PackDesc), len(layout.images) * C.sizeof(gigs_lib.FilterDesc)
    host = table_host.numpy()
    C.memmove(host.ctypes.data, pack, npk)
    C.memmove(host.ctypes.data + _up(npk), filt, nf)
    table_dev[:layout.table_bytes].copy_(table_host[:layout.table_bytes], non_blocking=True)
    gigs_lib.check(lib.gigs_pack_images(layout.n_pack, table_dev.data_ptr(), stream_handle), "pack_images")
    gigs_lib.check(lib.gigs_png_filter(len(layout.images), table_dev.data_ptr() + _up(npk), stream_handle), "png_filter")


def encode(images: Sequence, want_sheets: bool = False):
    """Synchronous form: the scanline streams of `images` as uint8 numpy arrays (and, with want_sheets, the 8-bit sheets
    [H,W,3] as device tensors).  For tests and one-off files; a render loop uses ImageWriter."""
    import gigs_lib
    import torch
    images = [_as_image(i) for i in images]
    if not images:
        return ([], []) if want_sheets else []
    dev = images[0].planes[0].device
    lay = _Layout(images)
    with torch.cuda.device(dev):
        sheets = torch.empty(lay.sheet_bytes, dtype=torch.uint8, device=dev)
        streams = torch.empty(lay.stream_bytes, dtype=torch.uint8, device=dev)
        lohi = torch.empty(max(2, 2 * lay.n_norm), dtype=torch.float32, device=dev)
        scratch = torch.empty(gigs_lib.MINMAX_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
        th = torch.empty(lay.table_bytes, dtype=torch.uint8).pin_memory()
        td = torch.empty(lay.table_bytes, dtype=torch.uint8, device=dev)
        _launch(lay, sheets, streams, lohi, scratch, th, td, torch.cuda.current_stream().cuda_stream)
        host = streams.cpu().numpy()
    out = [host[o:o + im.H * (1 + 3 * im.W)] for o, im in zip(lay.stream_off, images)]
    if not want_sheets:
        return out
    sh = [sheets[o:o + s * im.H].view(im.H, s)[:, :3 * im.W].reshape(im.H, im.W, 3)
          for o, s, im in zip(lay.sheet_off, lay.strides, images)]
    return out, sh


def quantize(planes, bias: float = 0.5, normalize: bool = False):
    """The 8-bit sheet [H,W,3] (device uint8) of one image, as the PNG will hold it."""
    return encode([Image(None, planes, bias, normalize)], want_sheets=True)[1][0]


class _Slot:
    def __init__(self):
        self.sheets = self.streams = self.host = self.lohi = self.table_host = self.table_dev = None
        self.host_np = None
        self.event = None
        self.pending = 0


class ImageWriter:
    """Asynchronous PNG writer.  submit(images) -- `images`: Image objects or (path, planes[, bias[, normalize]]) tuples --
    enqueues on the CURRENT stream: min / max of the planes to normalise, one gigs_pack_images launch, one gigs_png_filter
    launch, an asynchronous copy of the scanline streams into one of `slots` pinned staging buffers, an event.  It
    returns at once: the source planes may be overwritten by later work on the same stream (the next replay of an
    evaluator's graph).  `workers` threads wait for the event, deflate and write path + ".tmp", then rename.  submit blocks
    only while every slot is in flight (`blocked_s` sums that time).  close() (or leaving the `with` block) drains; a
    worker's exception is re-raised in the caller at the next submit or at close.  Threads only: no other process opens
    the GPU.  One writer belongs to one stream: its buffers are reused in that stream's order."""

    def __init__(self, workers: int = 12, slots: int = 3):
        if workers < 1 or slots < 1:
            raise ValueError("ImageWriter: workers and slots must be at least 1")
        self.workers = min(int(workers), MAX_WORKERS)
        self._pool = ThreadPoolExecutor(max_workers=self.workers, thread_name_prefix="image_writer")
        self._slots = [_Slot() for _ in range(int(slots))]
        self._free: "queue.Queue[int]" = queue.Queue()
        for i in range(len(self._slots)):
            self._free.put(i)
        self._lock = threading.Lock()
        self._errors: List[BaseException] = []
        self._scratch = None
        self._closed = False
        self.blocked_s = 0.0
        self.files = 0
        self.bytes_written = 0

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        try:
            self.close()
        except Exception:
            if exc_type is None:
                raise
        return False

    def _raise_pending(self) -> None:
        with self._lock:
            if self._errors:
                e = self._errors[0]
                self._errors = []
                raise e

    @staticmethod
    def _fit(t, n, **kw):
        import torch
        if t is None or t.numel() < n:
            t = None  # release before allocating
            t = torch.empty(n, **kw)
        return t

    def submit(self, images: Sequence[Union[Image, tuple]]) -> None:
        import gigs_lib
        import torch
        if self._closed:
            raise RuntimeError("ImageWriter: submit after close")
        self._raise_pending()
        images = [_as_image(i) for i in images]
        if not images:
            return
        if any(im.path is None for im in images):
            raise ValueError("ImageWriter.submit: every image needs a path")
        dev = images[0].planes[0].device
        lay = _Layout(images)
        t0 = time.perf_counter()
        idx = self._free.get()
        self.blocked_s += time.perf_counter() - t0
        slot = self._slots[idx]
        try:
            with torch.cuda.device(dev):
                u8 = dict(dtype=torch.uint8, device=dev)
                slot.sheets = self._fit(slot.sheets, lay.sheet_bytes, **u8)
                slot.streams = self._fit(slot.streams, lay.stream_bytes, **u8)
                slot.table_dev = self._fit(slot.table_dev, lay.table_bytes, **u8)
                slot.lohi = self._fit(slot.lohi, max(2, 2 * lay.n_norm), dtype=torch.float32, device=dev)
                self._scratch = self._fit(self._scratch, gigs_lib.MINMAX_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
                if slot.host is None or slot.host.numel() < lay.stream_bytes:
                    slot.host = slot.host_np = None
                    slot.host = torch.empty(lay.stream_bytes, dtype=torch.uint8).pin_memory()
                    slot.host_np = slot.host.numpy()
                if slot.table_host is None or slot.table_host.numel() < lay.table_bytes:
                    slot.table_host = torch.empty(lay.table_bytes, dtype=torch.uint8).pin_memory()
                if slot.event is None:
                    slot.event = torch.cuda.Event()
                _launch(lay, slot.sheets, slot.streams, slot.lohi, self._scratch, slot.table_host, slot.table_dev,
                        torch.cuda.current_stream().cuda_stream)
                slot.host[:lay.stream_bytes].copy_(slot.streams[:lay.stream_bytes], non_blocking=True)
                slot.event.record()
        except BaseException:
            self._free.put(idx)
            raise
        slot.pending = len(images)
        for off, im in zip(lay.stream_off, images):
            self._pool.submit(self._work, idx, off, im.W, im.H, im.path)

    def _work(self, idx: int, off: int, W: int, H: int, path: str) -> None:
        slot = self._slots[idx]
        tmp = path + ".tmp"
        try:
            slot.event.synchronize()
            data = png_bytes(slot.host_np[off:off + H * (1 + 3 * W)], W, H)
            with open(tmp, "wb") as f:
                f.write(data)
            os.replace(tmp, path)
            with self._lock:
                self.files += 1
                self.bytes_written += len(data)
        except BaseException as e:  # noqa: BLE001 - handed to the caller
            try:
                if os.path.exists(tmp):
                    os.remove(tmp)
            except OSError:
                pass
            with self._lock:
                self._errors.append(e)
        finally:
            with self._lock:
                slot.pending -= 1
                done = slot.pending == 0
            if done:
                self._free.put(idx)

    def close(self) -> None:
        """Waits for every file, releases the staging buffers, re-raises the first worker exception."""
        if not self._closed:
            self._closed = True
            self._pool.shutdown(wait=True)
            for s in self._slots:
                s.__init__()
            self._scratch = None
        self._raise_pending()
