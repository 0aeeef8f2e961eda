"""cmdiad_amd/utils/png.py on the host (no GPU): the parser, the raw reader and the fallback rule against Pillow and against the numpy
restatement of tests/png_ref.py, on files whose filter types are forced by the tests' own writer.  Every comparison is for equal bytes."""
import os
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_ref as pg  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402
from cmdiad_amd.utils import png  # noqa: E402
from cmdiad_amd.utils import tiff  # noqa: E402

COLOR_TYPES = (0, 2, 4, 6)
SHAPES = ((1, 1), (2, 3), (65, 67), (130, 5))
TARGETS = ("rgb", "l", "raw")


def _restated(raw):
    lay = raw.layout
    return pg.to_target(pg.unfilter(raw.data, lay.height, lay.row_bytes, lay.bpp), lay.width, lay.channels, raw.target)


def _check_file(path, array):
    """read_raw + the restatement == Pillow, for the three targets; 'raw' is the array the file was written from."""
    for target in TARGETS:
        raw = png.read_raw(path, target)
        want = pg.pillow(path, target)
        lay = raw.layout
        assert raw.data.dtype == np.uint8 and raw.data.shape == (lay.height * (1 + lay.row_bytes),)
        assert raw.shape == want.shape and raw.ndim == want.ndim and raw.dtype == want.dtype and raw.target == target
        assert np.array_equal(_restated(raw), want), (path, target)
    assert np.array_equal(pg.pillow(path, "raw"), array)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("color_type", COLOR_TYPES)
def test_read_raw_and_the_restatement_equal_pillow(tmp_path, color_type, shape):
    """Colour types 0 / 2 / 4 / 6 x four shapes: every row forced to each of the types 0..4, then a random type per row, then a file
    Pillow wrote."""
    from PIL import Image
    H, W = shape
    C = pg.CHANNELS_OF_COLOR_TYPE[color_type]
    rs = np.random.RandomState(100 * color_type + H)
    for k, filters in enumerate([0, 1, 2, 3, 4, rs.randint(0, 5, H)]):
        a = pg.image(H, W, C, seed=7 * k + color_type, smooth=k % 2 == 0)
        path = str(tmp_path / f"f{k}.png")
        pg.write(path, a, filters=filters)
        lay = png.read_layout(path)
        assert (lay.width, lay.height, lay.bit_depth, lay.color_type, lay.channels, lay.bpp, lay.row_bytes, lay.interlace, lay.has_plte,
                lay.has_trns) == (W, H, 8, color_type, C, C, W * C, 0, False, False)
        assert png.supported(lay)
        assert np.array_equal(png.read_raw(path).data[::1 + W * C], np.full(H, filters) if np.isscalar(filters) else filters)
        _check_file(path, a)
    a = pg.image(H, W, C, seed=99, smooth=True)
    path = str(tmp_path / "pillow.png")
    Image.fromarray(a).save(path)
    assert png.supported(png.read_layout(path))
    _check_file(path, a)


def test_idat_split_into_several_chunks_one_of_them_empty(tmp_path):
    a = pg.image(65, 67, 3, seed=5, smooth=True)
    filters = np.random.RandomState(2).randint(0, 5, 65)
    whole = pg.write(str(tmp_path / "whole.png"), a, filters=filters)
    parts = pg.write(str(tmp_path / "parts.png"), a, filters=filters, split=(1, 0, 100, 7, 0, 1000))
    assert parts.count(b"IDAT") >= 7 > whole.count(b"IDAT") == 1
    one, many = png.read_raw(str(tmp_path / "whole.png")), png.read_raw(str(tmp_path / "parts.png"))
    assert np.array_equal(one.data, many.data) and one.layout == many.layout
    assert np.array_equal(_restated(many), a)
    assert np.array_equal(png.read_raw(parts).data, one.data)            # (bytes in place of a path)


# ------------------------------------------------------------------------------------------------ the subset and the fallback
def _unsupported_files(tmp):
    """{name: path} of one file per reason `supported` has to say no; every one is a file Pillow decodes."""
    from PIL import Image
    rs = np.random.RandomState(11)
    out = {}
    idx = rs.randint(0, 4, (9, 7)).astype(np.uint8)
    pal = Image.fromarray(idx, "P")
    pal.putpalette([0, 0, 0, 255, 255, 255, 200, 10, 10, 10, 200, 10] + [0] * (252 * 3))
    out["palette"] = str(tmp / "palette.png")
    pal.save(out["palette"])
    out["16-bit"] = str(tmp / "deep.png")
    Image.fromarray(rs.randint(0, 65536, (6, 5)).astype(np.uint16)).save(out["16-bit"])
    out["1-bit"] = str(tmp / "one.png")
    Image.fromarray(rs.randint(0, 2, (6, 11)).astype(bool)).save(out["1-bit"])
    for bits in (2, 4):          # grey, W = 8: 8 * bits / 8 bytes a row, filter type 0
        rows = rs.randint(0, 256, (5, bits)).astype(np.uint8)
        lines = np.concatenate([np.zeros((5, 1), np.uint8), rows], axis=1)
        out[f"{bits}-bit"] = str(tmp / f"bits{bits}.png")
        pg.write(out[f"{bits}-bit"], np.zeros((5, 8), np.uint8), bit_depth=bits, scanlines=lines)
    a = pg.image(9, 10, 3, seed=3)
    out["interlaced"] = str(tmp / "adam7.png")
    pg.write(out["interlaced"], a, interlace=1, scanlines=pg.adam7_scanlines(a))
    assert np.array_equal(np.array(Image.open(out["interlaced"])), a)          # (the generator's Adam7 is the one Pillow reads)
    out["tRNS"] = str(tmp / "trns.png")
    pg.write(out["tRNS"], pg.image(4, 5, 3, seed=4), filters=4, extra=((b"tRNS", struct.pack(">HHH", 1, 2, 3)),))
    out["wide"] = str(tmp / "wide.png")
    pg.write(out["wide"], pg.image(1, 21846, 3, seed=6), filters=1)             # 65 538 bytes a row
    return out


def _one_sample_tree(root, rgb_file, gt_file):
    """<root>/bagel/test/crack/{rgb,xyz,gt}/000.*: the given PNG bytes as rgb and as gt, a tiny real TIFF as the cloud."""
    base = os.path.join(str(root), "bagel", "test", "crack")
    for d in ("rgb", "xyz", "gt"):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    for d, src in (("rgb", rgb_file), ("gt", gt_file)):
        with open(src, "rb") as fh, open(os.path.join(base, d, "000.png"), "wb") as out:
            out.write(fh.read())
    tiff.imwrite(os.path.join(base, "xyz", "000.tiff"), np.ones((4, 4, 3), np.float32))
    return ds.TestDataset(class_name="bagel", rgb_size=224, xyz_size=224, gt_size=224, dataset_path=str(root), img_process_method="hip")


def test_unsupported_files_take_the_pillow_path_and_supported_ones_do_not(tmp_path, monkeypatch):
    """`supported` is False for palette, 16-bit, 1 / 2 / 4-bit, interlaced, tRNS and over-wide files, and `decoded()` with the switch on
    returns for each the ndarray Pillow gives; for a supported file it returns a RawImage (under 'hip' only, and only with the switch)."""
    monkeypatch.setitem(sys.modules, "tifffile", None)
    files = _unsupported_files(tmp_path)
    assert sorted(files) == sorted(["palette", "16-bit", "1-bit", "2-bit", "4-bit", "interlaced", "tRNS", "wide"])
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "1")
    for name, path in files.items():
        lay = png.read_layout(path)
        assert not png.supported(lay), name
        assert png.read_for_device(path, "rgb") is None, name
        data = _one_sample_tree(tmp_path / ("tree_" + name), path, path)
        rgb, _, gt = data.decoded(0)
        assert isinstance(rgb, np.ndarray) and isinstance(gt, np.ndarray), name
        assert np.array_equal(rgb, pg.pillow(path, "rgb")) and rgb.dtype == np.uint8 and rgb.ndim == 3, name
        assert np.array_equal(gt, pg.pillow(path, "l")) and gt.dtype == np.uint8 and gt.ndim == 2, name
    assert png.read_layout(files["palette"]).has_plte and png.read_layout(files["tRNS"]).has_trns
    assert png.read_layout(files["interlaced"]).interlace == 1 and png.read_layout(files["16-bit"]).bit_depth == 16
    assert [png.read_layout(files[f"{b}-bit"]).bit_depth for b in (1, 2, 4)] == [1, 2, 4]
    assert png.read_layout(files["wide"]).row_bytes == 65538

    rgb_file, gt_file = str(tmp_path / "rgb.png"), str(tmp_path / "gt.png")
    a, g = pg.image(12, 9, 3, seed=1), pg.image(12, 9, 1, seed=2)
    pg.write(rgb_file, a, filters=3)
    pg.write(gt_file, g, filters=4)
    data = _one_sample_tree(tmp_path / "tree_ok", rgb_file, gt_file)
    rgb, cloud, gt = data.decoded(0)
    assert isinstance(rgb, png.RawImage) and rgb.target == "rgb" and rgb.shape == (12, 9, 3) and isinstance(cloud, np.ndarray)
    assert isinstance(gt, png.RawImage) and gt.target == "l" and gt.shape == (12, 9)
    assert np.array_equal(_restated(rgb), a) and np.array_equal(_restated(gt), g)
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "0")
    rgb, _, gt = data.decoded(0)
    assert isinstance(rgb, np.ndarray) and isinstance(gt, np.ndarray) and np.array_equal(rgb, a) and np.array_equal(gt, g)
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "1")
    data.img_process_method = "cpu_v1"                                        # the host methods never see a RawImage
    rgb, _, gt = data.decoded(0)
    assert isinstance(rgb, np.ndarray) and isinstance(gt, np.ndarray)


# ------------------------------------------------------------------------------------------------ malformed files
def _good(filters=4, **kw):
    return pg.encode(pg.image(6, 5, 3, seed=8), filters=filters, **kw)


def test_malformed_files_are_value_errors_that_name_the_path(tmp_path):
    good = _good()
    idat = good.index(b"IDAT")
    length, = struct.unpack(">I", good[idat - 4:idat])
    flipped = bytearray(good)
    flipped[idat + 4 + length] ^= 0x01                                       # first byte of the IDAT's CRC
    cases = {"cut inside IHDR": good[:20], "cut inside IDAT": good[:idat + 10], "cut before IEND": good[:-12],
             "flipped IDAT CRC": bytes(flipped)}
    for name, data in cases.items():
        path = str(tmp_path / (name.replace(" ", "_") + ".png"))
        with open(path, "wb") as fh:
            fh.write(data)
        for call in (png.read_layout, png.read_raw):
            with pytest.raises(ValueError, match=os.path.basename(path)):
                call(path)
    lines = pg.filter_rows(pg.image(6, 5, 3, seed=8).reshape(6, 15), 3, np.full(6, 1))
    for name, rows in (("one row short", lines[:5]), ("one row long", np.concatenate([lines, lines[:1]]))):
        path = str(tmp_path / (name.replace(" ", "_") + ".png"))
        pg.write(path, pg.image(6, 5, 3, seed=8), scanlines=rows)
        assert png.read_layout(path).height == 6                             # (the chunks are fine: the stream is not)
        with pytest.raises(ValueError, match=os.path.basename(path) + ".*inflates"):
            png.read_raw(path)
    path = str(tmp_path / "type5.png")
    pg.write(path, pg.image(6, 5, 3, seed=8), filters=[0, 1, 2, 5, 3, 4])
    with pytest.raises(ValueError, match="type5.png.*filter type 5 in row 3"):
        png.read_raw(path)
    with pytest.raises(ValueError, match="signature"):
        png.read_layout(b"GIF89a" + good[6:])
    with pytest.raises(ValueError, match="IHDR"):
        png.read_layout(pg.SIGNATURE + pg.chunk(b"IDAT", zlib.compress(b"\0")) + pg.chunk(b"IEND"))
    with pytest.raises(ValueError, match="13 bytes"):
        png.read_layout(pg.SIGNATURE + pg.chunk(b"IHDR", struct.pack(">IIBBBBBB", 1, 1, 8, 0, 0, 0, 0, 0)) + good[33:])
    with pytest.raises(ValueError, match="no IDAT"):
        png.read_layout(good[:33] + pg.chunk(b"IEND"))


def test_the_switch_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv("CMDIAD_PNG_DEVICE", raising=False)
    assert not png.device_decode_enabled()
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "1")
    assert png.device_decode_enabled()
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "0")
    assert not png.device_decode_enabled()
