"""CPU: the host half of the image writer (gi-gs_amd/image_writer.py) -- the PNG container around scanlines that are
already filtered, the Radiance .hdr reader / writer -- the numpy reference of the device half (tests/png_ref.py), and the
file-name tables of render_scene / relight_scene."""
import io

import numpy as np
import pytest

import png_ref


def _noisy_and_constant(H, W, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    img[: max(1, H // 2), : max(1, W // 2)] = 37  # a constant region beside the noise
    return img


@pytest.mark.parametrize("H,W", [(1, 1), (7, 5), (128, 128), (800, 3)])
def test_png_bytes_round_trip(H, W):
    from PIL import Image

    import image_writer
    for img in (_noisy_and_constant(H, W, H * 1000 + W), png_ref.quantize(png_ref.test_image(H, W))):
        stream, _ = png_ref.scanlines(img)
        data = image_writer.png_bytes(stream, W, H)
        Image.open(io.BytesIO(data)).verify()  # chunk CRCs
        im = Image.open(io.BytesIO(data))
        assert im.mode == "RGB" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), img)
    with pytest.raises(ValueError):
        image_writer.png_bytes(stream[:-1], W, H)


@pytest.mark.parametrize("H,W", [(128, 128), (127, 130)])
def test_reference_row_choice_uses_every_filter(H, W):
    _, types = png_ref.scanlines(png_ref.quantize(png_ref.test_image(H, W)))
    counts = np.bincount(types, minlength=5)
    print("rows per filter None/Sub/Up/Average/Paeth:", counts.tolist())
    assert (counts >= 2).all(), counts


def _rgbe(rgb):
    """Radiance's float2rgbe, restated with Python floats: (r, g, b, e) bytes."""
    import math
    out = np.zeros(rgb.shape[:-1] + (4,), np.uint8)
    for idx in np.ndindex(*rgb.shape[:-1]):
        r, g, b = (float(v) for v in rgb[idx])
        v = max(r, g, b)
        if v < 1e-32:
            continue
        m, e = math.frexp(v)
        s = np.float32(np.float32(m) * np.float32(256.0) / np.float32(v))
        out[idx] = [int(np.float32(max(c, 0.0)) * s) for c in (r, g, b)] + [e + 128]
    return out


def _decode(px):
    e = px[..., 3].astype(np.int64)
    scale = np.where(e > 0, 2.0 ** (e - 136.0), 0.0)
    return (px[..., :3].astype(np.float64) * scale[..., None]).astype(np.float32)


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_round_trip(tmp_path, rle):
    import image_writer
    rng = np.random.RandomState(3)
    x = (10.0 ** rng.uniform(-4, 4, (12, 40, 3))).astype(np.float32)
    x[0, :5] = 0.0          # exact zeros
    x[3, 8:30] = 0.75       # a run for the run-length coder
    x[5] = x[5, :1]         # a constant scanline
    path = str(tmp_path / "a.hdr")
    image_writer.write_hdr(path, x, rle=rle)
    got = image_writer.read_hdr(path)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got, _decode(_rgbe(x)))
    assert np.all(got[0, :5] == 0.0)
    # the quantisation error of a pixel is below one mantissa step of its largest channel
    assert np.all(np.abs(got - x) <= x.max(-1, keepdims=True) / 128.0)


def _hand_written(tmp_path):
    """8 x 2 pixels: as flat scanlines and as run-length scanlines, written by hand."""
    row0 = [(128, 64, 32, 129)] * 5 + [(1, 2, 3, 120), (255, 0, 7, 136), (9, 9, 9, 0)]
    row1 = [(10 * i, 255 - i, i, 128 + i) for i in range(8)]
    head = b"#?RADIANCE\n# hand written\nFORMAT=32-bit_rle_rgbe\n\n-Y 2 +X 8\n"
    flat = head + bytes(v for px in row0 + row1 for v in px)
    body = bytearray()
    for row in (row0, row1):
        body += bytes([2, 2, 0, 8])
        for c in range(4):
            vals = [px[c] for px in row]
            if row is row0:  # a run of five, then three literals
                body += bytes([128 + 5, vals[0], 3] + vals[5:])
            else:            # two literal packets
                body += bytes([4] + vals[:4] + [4] + vals[4:])
    a, b = str(tmp_path / "flat.hdr"), str(tmp_path / "rle.hdr")
    open(a, "wb").write(flat)
    open(b, "wb").write(head + bytes(body))
    px = np.array([row0, row1], dtype=np.uint8)
    return a, b, px, flat


def test_hdr_flat_and_run_length_decode_alike(tmp_path):
    import image_writer
    a, b, px, flat = _hand_written(tmp_path)
    fa, fb = image_writer.read_hdr(a), image_writer.read_hdr(b)
    assert fa.shape == (2, 8, 3) and np.array_equal(fa, fb)
    want = px[..., :3].astype(np.float64) * np.where(px[..., 3:] > 0, 2.0 ** (px[..., 3:].astype(np.float64) - 136.0), 0.0)
    assert np.array_equal(fa, want.astype(np.float32))
    assert fa[0, 0, 0] == 128 * 2.0 ** (129 - 136) and np.all(fa[0, 7] == 0.0)  # no half step; e = 0 is black
    for name, data in (("magic", b"P6\n8 2\n255\n" + flat[40:]), ("short", flat[:-5]), ("header", flat[:30]),
                       ("rle", open(b, "rb").read()[:-3])):
        p = str(tmp_path / ("bad_%s.hdr" % name))
        open(p, "wb").write(data)
        with pytest.raises(ValueError):
            image_writer.read_hdr(p)


def test_load_latlong_accepts_npy_and_hdr(tmp_path):
    import image_writer
    x = np.random.RandomState(0).uniform(0.0, 4.0, (8, 16, 3)).astype(np.float32)
    np.save(str(tmp_path / "m.npy"), x)
    image_writer.write_hdr(str(tmp_path / "m.hdr"), x)
    assert np.array_equal(image_writer.load_latlong(str(tmp_path / "m.npy")), x)
    # truncation to 8-bit mantissas under the pixel's largest channel v in [2^(E-1), 2^E): one step is 2^(E-8) <= v / 128
    assert np.all(np.abs(image_writer.load_latlong(str(tmp_path / "m.hdr")) - x) <= x.max(-1, keepdims=True) / 128.0)
    with pytest.raises(ValueError):
        image_writer.load_latlong(str(tmp_path / "m.exr"))


def test_render_scene_file_table():
    import render_scene
    got = render_scene.planned_paths("out", "test", 1200, ["r_0", "r_7"])
    base = "out/test/ours_1200"
    want = ["out/test/envmap.hdr", "out/test/envmap.png", "out/test/unscaled_envmap.png"]
    for idx, name in enumerate(["r_0", "r_7"]):
        want.append("%s/normal/%05d_from_depth.png" % (base, idx))
        want += ["%s/pbr/%s%s.png" % (base, name, s) for s in
                 ("", "_DIR", "_indirect", "_albedo", "_roughness", "_metallic", "_brdf", "_diffuse", "_specular", "_occlusion")]
        want.append("%s/normal/%05d_normal.png" % (base, idx))
        want.append("%s/depth/%s_depth.png" % (base, name))
    want.append(base + "/pbr/r_7_NVS.json")
    assert got == want
    assert len(render_scene.view_paths("out", "test", 1200, 0, "r_0")) == 13
    # without --pbr only the normals from depth are written (render.py:258-263)
    assert render_scene.planned_paths("out", "train", 5, ["a"], pbr=False) == [
        "out/train/envmap.hdr", "out/train/envmap.png", "out/train/unscaled_envmap.png",
        "out/train/ours_5/normal/00000_from_depth.png"]


def test_relight_scene_file_table():
    import relight_scene
    assert relight_scene.light_name("/maps/bridge.4k.hdr") == "bridge" and relight_scene.light_name("city.npy") == "city"
    got = relight_scene.planned_paths("out", "test", 30000, ["r_0", "r_1"], ["bridge", "city"], with_metrics=True)
    base = "out/test/ours_30000/relight"
    want = ["out/test/envmap_relight_bridge.png", "out/test/envmap_relight_city.png"]
    for name in ("r_0", "r_1"):
        for light in ("bridge", "city"):
            want += ["%s/%s_%s.png" % (base, name, light), "%s/%s_%s_occlusion.png" % (base, name, light)]
    want += [base + "/bridge.json", base + "/city.json"]
    assert got == want


def test_cli_arguments_and_cfg_args(tmp_path):
    from argparse import Namespace

    import relight_scene
    import render_scene
    a = render_scene.parse_args(["--checkpoint", str(tmp_path / "chkpnt7.pth"), "--pbr"])
    assert (a.radius, a.bias, a.thick, a.delta, a.step, a.start) == (0.8, 0.01, 0.05, 0.0625, 16, 8)  # render.py:651-656
    assert a.pbr and not (a.metallic or a.indirect or a.tone or a.gamma or a.skip_train or a.skip_test or a.brdf_eval)
    assert a.source_path is None and a.eval is None  # sentinels: cfg_args shows through
    (tmp_path / "cfg_args").write_text(str(Namespace(sh_degree=2, source_path="/data/lego", model_path=str(tmp_path),
                                                      images="images", resolution=2, white_background=False,
                                                      data_device="cuda", eval=True)))
    c = render_scene.combine_args(a)
    assert c.source_path == "/data/lego" and c.eval is True and c.resolution == 2 and c.sh_degree == 2
    assert c.model_path == str(tmp_path)
    c = render_scene.combine_args(render_scene.parse_args(["--checkpoint", str(tmp_path / "chkpnt7.pth"), "-s", "/other", "-r", "4"]))
    assert c.source_path == "/other" and c.resolution == 4 and c.eval is True
    (tmp_path / "cfg_args").write_text("__import__('os').getcwd()")
    with pytest.raises(ValueError):
        render_scene.combine_args(a)
    r = relight_scene.parse_args(["--checkpoint", "x/chkpnt1.pth", "--hdri", "a.hdr", "b.hdr", "--metallic"])
    assert r.hdri == ["a.hdr", "b.hdr"] and r.metallic and r.start == 8 and r.gt_dir is None
    with pytest.raises(ValueError):
        render_scene.combine_args(render_scene.parse_args([]))
