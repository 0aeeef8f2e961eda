"""CPU (no GPU): cmdiad_amd/utils/tiff.py, the project's own reader and writer of the xyz TIFFs, against tests/tiff_ref.py (an
independent generator), against Pillow's libtiff where Pillow can read or write the file (single-channel float32), and the fallback
of the three call sites that used to need the `tifffile` package."""
import os
import struct
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiff_ref as tr  # noqa: E402

SIZES = [(13, 17), (37, 29)]      # (H, W): odd against 16 x 16 tiles and 5-row strips -- a short last strip, padded tile edges


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(tr.bits_of(a), tr.bits_of(b))


@pytest.mark.parametrize("kw", tr.variants(1), ids=tr.variant_id)
def test_generator_agrees_with_pillow(tmp_path, kw):
    """The generator is right where an independent reader exists: Pillow returns the source bits of every single-channel float32
    variant (MM, tiles, strips, deflate, predictor 3, odd chunk offsets).  Two properties of Pillow 12 itself, found by running this:
    * MM + deflate: libtiff decodes into the HOST's byte order, and Pillow then unpacks that buffer with its big-endian rawmode
      ('F;32BF'): the array it returns is the source with every sample byte-swapped.  libtiff read the file correctly, so the
      assertion is equality after swapping back -- no weaker than equality.
    * uncompressed + predictor 3: Pillow decodes uncompressed files itself, without libtiff, and never looks at the Predictor tag.
      No independent reader undoes the predictor of those files; they are tied to their deflate twins instead, which libtiff does
      decode: chunk for chunk the stored bytes must be the twin's inflated bytes."""
    import zlib
    from PIL import Image
    src = tr.random_bits((37, 29), np.float32, seed=1)
    path = str(tmp_path / "g.tiff")
    offsets = tr.write(path, src, **kw)
    if kw["predictor"] == 3 and not kw["deflate"]:
        twin = str(tmp_path / "twin.tiff")
        twin_offsets = tr.write(twin, src, **{**kw, "deflate": True})
        with open(path, "rb") as fh, open(twin, "rb") as ft:
            raw, packed = fh.read(), ft.read()
        assert len(offsets) == len(twin_offsets)
        for k, (off, toff) in enumerate(zip(offsets, twin_offsets)):
            stored = zlib.decompressobj().decompress(packed[toff:])
            assert len(stored) >= 29 * 4 and raw[off:off + len(stored)] == stored, k
        with Image.open(twin) as im:
            got = np.array(im)
    else:
        with Image.open(path) as im:
            got = np.array(im)
    if kw["big_endian"] and (kw["deflate"] or kw["predictor"] == 3):
        got = got.view(np.uint32).byteswap().view(np.float32)
    assert _same_bits(got, src)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_imread_equals_source_bits_on_the_cross_product(tmp_path, size, channels, dtype):
    from cmdiad_amd.utils import tiff
    shape = size if channels == 1 else size + (channels,)
    src = tr.random_bits(shape, dtype, seed=size[0] + channels)
    path = str(tmp_path / "v.tiff")
    for kw in tr.variants(channels):
        offsets = tr.write(path, src, **kw)
        lay = tiff.read_layout(path)
        assert (lay.width, lay.height, lay.channels, lay.dtype) == (size[1], size[0], channels, np.dtype(dtype)), kw
        assert lay.big_endian == kw["big_endian"] and lay.planar == (kw["planar"] and channels > 1) and lay.predictor == kw["predictor"], kw
        assert lay.offsets.dtype == np.int64 and lay.counts.dtype == np.int64 and lay.offsets.tolist() == offsets, kw
        assert offsets[0] % 4 == kw["misalign"]
        assert lay.all_chunk_bytes().tolist() == [lay.chunk_bytes(k) for k in range(lay.n_chunks)], kw
        assert _same_bits(tiff.imread(path), src), kw
        with open(path, "rb") as fh:
            assert _same_bits(tiff._decoded_array(tiff.read_raw(fh.read())).reshape(src.shape), src), kw      # bytes in place of a path


def test_read_raw_inflates_and_keeps_the_predictor(tmp_path):
    from cmdiad_amd.utils import tiff
    src = tr.random_bits((37, 29, 3), np.float32, seed=5)
    plain, packed = str(tmp_path / "a.tiff"), str(tmp_path / "b.tiff")
    tr.write(plain, src, rows_per_strip=5, predictor=3)
    tr.write(packed, src, rows_per_strip=5, predictor=3, deflate=True, compression_tag=32946)
    a, b = tiff.read_raw(plain), tiff.read_raw(packed)
    assert a.data.dtype == np.uint8 and b.layout.compression == 1 and b.layout.predictor == 3 and tiff.read_layout(packed).compression == 32946
    assert a.shape == b.shape == (37, 29, 3) and a.dtype == np.float32
    for k in range(a.layout.n_chunks):           # the same stored (still predicted) bytes, at the rewritten offsets
        n = a.layout.chunk_bytes(k)
        assert n == int(b.layout.counts[k])
        assert bytes(a.data[int(a.layout.offsets[k]):][:n]) == bytes(b.data[int(b.layout.offsets[k]):][:n])
    with pytest.raises(ValueError, match="out holds 100 bytes"):       # refused before anything is read
        tiff.read_raw(plain, out=np.zeros(100, np.uint8))
    buf = np.full(max(os.path.getsize(plain), os.path.getsize(packed)) + 64, 0xAB, np.uint8)        # caller-supplied buffer: read in place
    c = tiff.read_raw(plain, out=buf)
    assert np.shares_memory(c.data, buf) and bytes(c.data) == open(plain, "rb").read() and buf[len(c.data)] == 0xAB
    d = tiff.read_raw(packed, out=buf)
    assert np.shares_memory(d.data, buf) and bytes(d.data) == bytes(b.data)


@pytest.mark.parametrize("size", SIZES + [(64, 300)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_files_written_by_libtiff_with_predictor_3_decode(tmp_path, size):
    from PIL import Image
    from cmdiad_amd.utils import tiff
    src = tr.random_bits(size, np.float32, seed=9)
    path = str(tmp_path / "p.tiff")
    Image.fromarray(src, "F").save(path, compression="tiff_adobe_deflate", tiffinfo={317: 3})
    lay = tiff.read_layout(path)
    assert lay.predictor == 3 and lay.compression == 8
    assert _same_bits(tiff.imread(path), src)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(37, 29), (37, 29, 3), (37, 29, 4), (300, 310, 3)], ids=str)
def test_imwrite_imread_round_trip(tmp_path, shape, dtype):
    from cmdiad_amd.utils import tiff
    src = tr.random_bits(shape, dtype, seed=3)
    path = str(tmp_path / "w.tiff")
    tiff.imwrite(path, src)
    assert _same_bits(tiff.imread(path), src)
    lay = tiff.read_layout(path)
    assert not lay.big_endian and not lay.planar and lay.compression == 1 and lay.predictor == 1 and lay.chunk_w == lay.width
    assert int(lay.offsets[0]) % 16 == 0 and np.all(np.diff(lay.offsets) == lay.chunk_h * lay.row_bytes)      # whole rows, back to back
    with open(path, "rb") as fh:
        raw = fh.read()
    assert raw[:4] == b"II*\0"
    n, = struct.unpack_from("<H", raw, 8)
    tags = {struct.unpack_from("<H", raw, 10 + 12 * k)[0]: struct.unpack_from("<HHI4s", raw, 10 + 12 * k) for k in range(n)}
    channels = shape[2] if len(shape) == 3 else 1
    assert struct.unpack("<H", tags[262][3][:2])[0] == (2 if channels == 3 else 1)
    assert (338 in tags) == (channels not in (1, 3)) and 339 in tags
    if len(shape) == 2 and dtype == np.float32:
        from PIL import Image
        with Image.open(path) as im:
            assert _same_bits(np.array(im), src)


def _entry(raw, tag):
    n, = struct.unpack_from("<H", raw, 8)
    for k in range(n):
        if struct.unpack_from("<H", raw, 10 + 12 * k)[0] == tag:
            return 10 + 12 * k
    raise KeyError(tag)


def _good(tmp_path, **kw):
    path = str(tmp_path / "good.tiff")
    tr.write(path, tr.random_bits((13, 17, 3), np.float32, seed=2), **kw)
    with open(path, "rb") as fh:
        return bytearray(fh.read())


def test_refusals_name_the_cause(tmp_path):
    from cmdiad_amd.utils import tiff
    raw = _good(tmp_path, rows_per_strip=5)
    tiff.read_layout(bytes(raw))

    def patched(tag, value, code="<H"):
        b = bytearray(raw)
        struct.pack_into(code, b, _entry(raw, tag) + 8, value)
        return bytes(b)

    big = bytearray(raw)
    struct.pack_into("<H", big, 2, 43)
    with pytest.raises(ValueError, match="BigTIFF.*tifffile"):
        tiff.read_layout(bytes(big))
    with pytest.raises(ValueError, match=r"Compression \(259\) = 5.*tifffile"):
        tiff.read_layout(patched(259, 5))
    with pytest.raises(ValueError, match=r"Predictor \(317\) = 2.*tifffile"):
        tiff.read_layout(bytes(_patch_predictor(tmp_path, 2)))
    # sample format: unsigned integers (1) in place of IEEE float (3); the three values lie out of line
    fmt = bytearray(raw)
    at, = struct.unpack_from("<I", raw, _entry(raw, 339) + 8)
    struct.pack_into("<3H", fmt, at, 1, 1, 1)
    with pytest.raises(ValueError, match=r"SampleFormat \(339\) = \[1, 1, 1\].*tifffile"):
        tiff.read_layout(bytes(fmt))
    bits = bytearray(raw)
    at, = struct.unpack_from("<I", raw, _entry(raw, 258) + 8)
    struct.pack_into("<3H", bits, at, 16, 16, 16)
    with pytest.raises(ValueError, match=r"BitsPerSample \(258\) = \[16, 16, 16\].*tifffile"):
        tiff.read_layout(bytes(bits))
    struct.pack_into("<3H", bits, at, 32, 32, 64)
    with pytest.raises(ValueError, match=r"BitsPerSample \(258\) = \[32, 32, 64\].*mixed"):
        tiff.read_layout(bytes(bits))


def _patch_predictor(tmp_path, value):
    raw = _good(tmp_path, predictor=3)
    struct.pack_into("<H", raw, _entry(raw, 317) + 8, value)
    return raw


def test_truncated_and_inconsistent_files_are_refused_at_parse_time(tmp_path):
    from cmdiad_amd.utils import tiff
    raw = _good(tmp_path, rows_per_strip=5)
    with pytest.raises(ValueError, match="chunk 2 .*past the end of the file"):
        tiff.read_layout(bytes(raw[:-1]))                                  # one byte short of its last strip
    path = str(tmp_path / "cut.tiff")
    with open(path, "wb") as fh:
        fh.write(raw[:-1])
    for reader in (tiff.imread, tiff.read_raw):
        with pytest.raises(ValueError, match="past the end of the file"):
            reader(path)
    counts_at, = struct.unpack_from("<I", raw, _entry(raw, 279) + 8)
    short = bytearray(raw)
    struct.pack_into("<I", short, counts_at, 5 * 17 * 12 - 4)               # an uncompressed count below the chunk's geometry
    with pytest.raises(ValueError, match="chunk 0 holds 1016 bytes.*needs 1020"):
        tiff.read_layout(bytes(short))
    fewer = bytearray(raw)
    struct.pack_into("<I", fewer, _entry(raw, 278) + 8, 4)                  # 4-row strips need 4 chunks, the file lists 3
    with pytest.raises(ValueError, match="needs 4 chunks"):
        tiff.read_layout(bytes(fewer))
    ifd = bytearray(raw)
    struct.pack_into("<I", ifd, 4, len(raw) + 100)
    with pytest.raises(ValueError, match="IFD offset .* outside the file"):
        tiff.read_layout(bytes(ifd))
    entries = bytearray(raw[:8]) + struct.pack("<H", 500) + bytes(40)       # an IFD whose entries run past the end
    with pytest.raises(ValueError, match="IFD .*outside the file"):
        tiff.read_layout(bytes(entries))
    deflated = _good(tmp_path, deflate=True)
    lay = tiff.read_layout(bytes(deflated))
    off, cnt = int(lay.offsets[0]), int(lay.counts[0])
    half = bytearray(deflated)
    half[off + cnt // 2:off + cnt] = bytes(cnt - cnt // 2)                  # a deflate stream cut in the middle
    with pytest.raises(ValueError, match="chunk 0"):
        tiff.read_raw(bytes(half))


def test_fallback_when_the_package_is_absent(tmp_path, monkeypatch):
    from cmdiad_amd.utils import mvtec3d_util, preprocessing, preprocessing_eyecandies, tiff
    monkeypatch.setitem(sys.modules, "tifffile", None)          # `import tifffile` raises ImportError
    with pytest.raises(ImportError):
        import tifffile  # noqa: F401
    src = tr.random_bits((37, 29, 3), np.float32, seed=4)
    path = str(tmp_path / "000.tiff")
    tr.write(path, src, big_endian=True, tile=(16, 16), misalign=2)
    assert _same_bits(mvtec3d_util.read_tiff_organized_pc(path), src)
    # the writer of utils/preprocessing.py: <dir>/xyz/000.tiff + rgb + gt, real files
    for d in ("xyz", "rgb", "gt"):
        os.makedirs(tmp_path / "w" / d)
    out = str(tmp_path / "w" / "xyz" / "000.tiff")
    rgb = np.random.RandomState(0).randint(0, 256, (37, 29, 3)).astype(np.uint8)
    preprocessing._write(out, src, rgb, None)
    assert open(out, "rb").read(4) == b"II*\0"
    assert _same_bits(mvtec3d_util.read_tiff_organized_pc(out), src) and _same_bits(preprocessing._read(out)[0], src)
    assert preprocessing_eyecandies._tifffile() is tiff
    f64 = tr.random_bits((20, 24, 3), np.float64, seed=6)
    preprocessing_eyecandies._tifffile().imwrite(path, f64)
    assert _same_bits(mvtec3d_util.read_tiff_organized_pc(path), f64)


def test_an_installed_package_is_still_the_one_called(tmp_path, monkeypatch):
    from cmdiad_amd.utils import mvtec3d_util, preprocessing, preprocessing_eyecandies
    calls = []
    fake = types.ModuleType("tifffile")
    fake.imread = lambda path: calls.append(("imread", str(path))) or "sentinel"
    fake.imwrite = lambda path, a: calls.append(("imwrite", str(path)))
    monkeypatch.setitem(sys.modules, "tifffile", fake)
    assert mvtec3d_util.read_tiff_organized_pc("nowhere.tiff") == "sentinel"
    for d in ("xyz", "rgb", "gt"):
        os.makedirs(tmp_path / d)
    out = str(tmp_path / "xyz" / "000.tiff")
    preprocessing._write(out, np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 3), np.uint8), None)
    assert preprocessing_eyecandies._tifffile() is fake
    assert calls == [("imread", "nowhere.tiff"), ("imwrite", out)] and not os.path.exists(out)


def test_raw_cloud_groups_like_the_array_it_stands_for(tmp_path):
    from cmdiad_amd.utils import tiff
    from cmdiad_amd.utils.batching import group_by_shape
    a = tr.random_bits((13, 17, 3), np.float32, seed=7)
    path = str(tmp_path / "a.tiff")
    tr.write(path, a, tile=(16, 16))
    raw = tiff.read_raw(path)
    assert group_by_shape([a, raw, np.zeros((13, 17, 3))], range(3), with_dtype=True) == {((13, 17), "float32"): [0, 1], ((13, 17), "float64"): [2]}
    assert tiff.device_decode_enabled() is (os.environ.get("CMDIAD_TIFF_DEVICE") == "1")


def test_the_c_entry_rejects_bad_arguments_without_a_launch():
    """cmdiad_tiff_unpack validates like its neighbours: -1 and a message, on a machine without a GPU (no launch happens)."""
    import ctypes
    from cmdiad_amd import _native as nat
    L = nat.lib()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(raw=p, raw_bytes=64, chunk_off=p, B=1, n_chunks=1, W=2, H=2, C=3, chunk_w=2, chunk_h=2, planar=0, bps=4, big_endian=0,
                predictor=1, out=p)

    def call(**kw):
        a = {**good, **kw}
        return L.cmdiad_tiff_unpack(a["raw"], a["raw_bytes"], a["chunk_off"], a["B"], a["n_chunks"], a["W"], a["H"], a["C"], a["chunk_w"],
                                    a["chunk_h"], a["planar"], a["bps"], a["big_endian"], a["predictor"], a["out"], None)

    for kw, text in ((dict(raw=None), b"null pointer"), (dict(chunk_off=None), b"null pointer"), (dict(out=None), b"null pointer"),
                     (dict(B=0), b"bad sizes"), (dict(W=0), b"bad sizes"), (dict(H=-1), b"bad sizes"), (dict(C=5), b"bad sizes"),
                     (dict(C=0), b"bad sizes"), (dict(W=(1 << 14) + 1, chunk_w=(1 << 14) + 1), b"bad sizes"), (dict(chunk_h=1 << 15), b"bad sizes"),
                     (dict(bps=2), b"bytes_per_sample=2"), (dict(bps=16), b"bytes_per_sample=16"), (dict(predictor=2), b"predictor=2"),
                     (dict(planar=2), b"planar=2"), (dict(raw_bytes=0), b"raw_bytes=0"), (dict(raw_bytes=62), b"raw_bytes=62"),
                     (dict(n_chunks=2), b"n_chunks=2, the geometry needs 1"), (dict(planar=1, n_chunks=1), b"the geometry needs 3"),
                     (dict(predictor=3, W=6000, chunk_w=6000), b"72000 bytes exceeds 65536")):
        assert call(**kw) == -1 and text in L.cmdiad_last_error(), (kw, L.cmdiad_last_error())
