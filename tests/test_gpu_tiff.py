"""GPU: cmdiad_tiff_unpack (csrc/tiff.hip) through cmdiad_amd.utils.tiff.unpack_on_device and ops.tiff_unpack, against the host decode
`tiff.imread` (itself held to the generator's source bits and to Pillow's libtiff in tests/test_tiff_cpu.py); then the two MVTec 3D-AD
class sources over trees of real TIFFs with CMDIAD_TIFF_DEVICE=1 and =0.  Every comparison is for equal bits (torch.equal on integer
views: the arrays hold NaN payloads, -0.0 and denormals).  Files come from tests/tiff_ref.py; nothing is read from outside the tree."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as pr  # noqa: E402
import sample_prep_ref as spr  # noqa: E402
import tiff_ref as tr  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd.utils import tiff  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _assert_unpacks(paths, sources=None):
    """unpack_on_device(read_raw of every path) == imread of every path (== the source arrays when given), bit for bit."""
    raws = [tiff.read_raw(p) for p in paths]
    got = tiff.unpack_on_device(raws, DEV)
    want = np.stack([tiff.imread(p).reshape(raws[0].shape) for p in paths])
    assert got.is_cuda and tuple(got.shape) == want.shape and got.dtype == getattr(torch, want.dtype.name)
    assert torch.equal(_bits(got).cpu(), _bits(torch.from_numpy(want)))
    if sources is not None:
        assert np.array_equal(tr.bits_of(want), tr.bits_of(np.stack([np.asarray(s).reshape(raws[0].shape) for s in sources])))
    return got


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("channels", [1, 3])
def test_unpack_equals_imread_on_the_cross_product(tmp_path, channels, dtype):
    """37 x 29 (odd against 16 x 16 tiles and 5-row strips), B = 2: byte order x strips / tiles x chunky / planar x none / deflate x
    predictor 1 / 3, chunk offsets at every residue mod 4 and different in the two files of a batch."""
    shape = (37, 29) if channels == 1 else (37, 29, channels)
    a, b = tr.random_bits(shape, dtype, seed=11), tr.random_bits(shape, dtype, seed=12)
    pa, pb = str(tmp_path / "a.tiff"), str(tmp_path / "b.tiff")
    for kw in tr.variants(channels):
        oa = tr.write(pa, a, **kw)
        ob = tr.write(pb, b, **{**kw, "misalign": (kw["misalign"] + 1) % 4})
        assert oa != ob
        _assert_unpacks([pa, pb], [a, b])


def test_predictor_3_row_lengths(tmp_path):
    """A chunk row that is no multiple of the dword or the wave size (29 x 3 float32 = 348 bytes), and one of 9 608 bytes (1 201
    float64, planar): more than one byte per thread segment, a last segment that is cut short."""
    p = str(tmp_path / "r.tiff")
    a = tr.random_bits((7, 29, 3), np.float32, seed=21)
    for kw in (dict(), dict(big_endian=True, rows_per_strip=2, misalign=3), dict(deflate=True, misalign=1)):
        tr.write(p, a, predictor=3, **kw)
        assert tiff.read_layout(p).row_bytes == 348
        _assert_unpacks([p], [a])
    b = tr.random_bits((5, 1201, 3), np.float64, seed=22)
    tr.write(p, b, predictor=3, planar=True, rows_per_strip=2, misalign=2)
    assert tiff.read_layout(p).row_bytes == 9608
    _assert_unpacks([p], [b])
    c = tr.random_bits((3, 1201, 4), np.float32, seed=23)          # stride 4, 19 216 bytes
    tr.write(p, c, predictor=3, misalign=1)
    _assert_unpacks([p], [c])
    d = tr.random_bits((40, 70, 2), np.float64, seed=24)           # stride 2, tiles of 32 x 16 with padded edges
    tr.write(p, d, predictor=3, tile=(32, 16), big_endian=True, misalign=3)
    _assert_unpacks([p], [d])


def test_production_size(tmp_path):
    """800 x 800 x 3 float32 (7.7 MB), little-endian, uncompressed: one strip, 64-row strips (the last one short), and the file
    tiff.imwrite writes; then the same width with predictor 3 (rows of 9 600 bytes)."""
    a = tr.random_bits((800, 800, 3), np.float32, seed=31)
    p = str(tmp_path / "full.tiff")
    for kw in (dict(), dict(rows_per_strip=64, misalign=2)):
        tr.write(p, a, **kw)
        _assert_unpacks([p], [a])
    tiff.imwrite(p, a)
    _assert_unpacks([p], [a])
    tr.write(p, a[:96], predictor=3, rows_per_strip=64, misalign=2)
    _assert_unpacks([p], [a[:96]])


def test_a_predictor_3_row_longer_than_64_kib_is_undone_on_the_host(tmp_path):
    a = tr.random_bits((3, 5500, 3), np.float32, seed=41)           # 66 000 bytes per row
    p, q = str(tmp_path / "long.tiff"), str(tmp_path / "edge.tiff")
    tr.write(p, a, predictor=3, misalign=1)
    raw = tiff.read_raw(p)
    assert raw.layout.row_bytes == 66000 > tiff.MAX_DEVICE_ROW_BYTES and tiff.host_unpacked(raw).layout.predictor == 1
    _assert_unpacks([p], [a])
    with pytest.raises(ValueError, match="66000 bytes exceeds"):     # the binding refuses what the kernel cannot hold: nothing is launched
        ops.tiff_unpack(torch.zeros(raw.data.size + (-raw.data.size) % 16, dtype=torch.uint8, device=DEV), [raw.layout], raw.layout.offsets[None])
    b = tr.random_bits((2, 4096, 4), np.float32, seed=42)           # exactly 64 KiB: the longest row the device handles
    tr.write(q, b, predictor=3)
    assert tiff.read_layout(q).row_bytes == 65536
    _assert_unpacks([q], [b])


def _upload_padded(data, fill):
    n = data.size
    buf = np.full((n + 31) & ~15, fill, np.uint8)          # at least 16 bytes of padding
    buf[:n] = data
    return torch.from_numpy(buf).to(DEV)


def test_the_binding_refuses_a_table_that_leaves_the_buffer(tmp_path):
    """ops.tiff_unpack checks every chunk against raw_u8's length BEFORE the launch: ValueError, and the output it was given is
    untouched.  (The kernel's own guard -- a source dword outside the buffer reads as 0 -- is covered below by a CORRECT file.)"""
    a = tr.random_bits((13, 17, 3), np.float32, seed=51)
    p = str(tmp_path / "g.tiff")
    tr.write(p, a, rows_per_strip=5)
    raw = tiff.read_raw(p)
    buf = _upload_padded(raw.data, 0)
    table = raw.layout.offsets[None].copy()
    out = torch.full((1, 13, 17, 3), 7.0, device=DEV)
    assert torch.equal(_bits(ops.tiff_unpack(buf, [raw.layout], table, out=out)).cpu(), torch.from_numpy(tr.bits_of(a)[None].view(np.int32)))
    out.fill_(7.0)
    last = raw.layout.chunk_bytes(raw.layout.n_chunks - 1)
    for k, off, what in ((2, buf.numel() - last + 1, "chunk 2 of image 0"), (0, -4, "chunk 0 of image 0")):
        bad = table.copy()
        bad[0, k] = off
        with pytest.raises(ValueError, match=what + ".*does not lie inside"):
            ops.tiff_unpack(buf, [raw.layout], bad, out=out)
    with pytest.raises(ValueError, match=r"chunk_table must be \[1,3\]"):
        ops.tiff_unpack(buf, [raw.layout], table[:, :2], out=out)
    with pytest.raises(ValueError, match="padded to a multiple of 4"):
        ops.tiff_unpack(buf[:-3], [raw.layout], table, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_garbage_behind_the_last_chunk_is_never_a_sample(tmp_path, dtype):
    """A correct file whose last chunk ends at the last byte, at an odd address, in a buffer whose padding is 0xA5 garbage: the aligned
    dword loads around the last samples take garbage in and shift it out; with a non-zero tail in the file the same."""
    a = tr.random_bits((13, 17, 3), dtype, seed=61)
    p = str(tmp_path / "t.tiff")
    for kw in (dict(misalign=1), dict(misalign=3, rows_per_strip=5, big_endian=True), dict(misalign=2, predictor=3), dict(misalign=1, tile=(16, 16))):
        tr.write(p, a, **kw)
        raw = tiff.read_raw(p)
        got = ops.tiff_unpack(_upload_padded(raw.data, 0xA5), [raw.layout], raw.layout.offsets[None])
        assert torch.equal(_bits(got).cpu(), _bits(torch.from_numpy(a[None])))
        tr.write(p, a, tail=bytes([0xC3]) * 37, **kw)
        _assert_unpacks([p], [a])


def test_mixed_layouts_and_host_arrays_share_a_batch(tmp_path):
    """SamplePrep.prepare_batch takes RawCloud objects beside decoded arrays: three layouts and one array of one shape in a batch give
    the tensors the decoded arrays give."""
    size = 64
    clouds = [spr.cloud(size, size, seed=70 + k) for k in range(4)]
    rgbs = [spr.image("random", size, size, seed=k) for k in range(4)]
    kws = [dict(), dict(big_endian=True, tile=(16, 16), misalign=2), None, dict(deflate=True, predictor=3, rows_per_strip=7, misalign=1)]
    mixed = []
    for k, (pc, kw) in enumerate(zip(clouds, kws)):
        if kw is None:
            mixed.append(pc)
            continue
        p = str(tmp_path / f"{k}.tiff")
        tr.write(p, pc, **kw)
        mixed.append(tiff.read_raw(p))
    prep = ds.SamplePrep(device=DEV)
    want, got = prep.prepare_batch(rgbs, clouds), prep.prepare_batch(rgbs, mixed)
    for (ws, _), (gs, _) in zip(want, got):
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(ws, gs)) and ws.n_valid == gs.n_valid > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_last_sample_at_the_end_of_the_buffer_reads_zeros_beyond_it(tmp_path, dtype):
    """The kernel's own guard on a CORRECT file: the last chunk ends exactly at raw_bytes, at a dword-aligned address, in a buffer with
    no padding at all -- the upper aligned dword of the last sample's load lies outside the buffer, reads as 0 and is shifted out."""
    a = tr.random_bits((13, 17, 3), dtype, seed=71)
    p = str(tmp_path / "e.tiff")
    for kw in (dict(), dict(predictor=3), dict(big_endian=True, rows_per_strip=5)):
        offsets = tr.write(p, a, misalign=0, **kw)
        raw = tiff.read_raw(p)
        if len(offsets) > 1:           # (the generator's 3-byte gaps: keep the last strip alone, at an aligned offset, ending the buffer)
            continue_at = int(raw.layout.offsets[-1])
            pad = (-continue_at) % 4
            data = np.concatenate([raw.data[:continue_at], np.zeros(pad, np.uint8), raw.data[continue_at:]])
            table = raw.layout.offsets.copy()
            table[-1] += pad
        else:
            data, table = raw.data, raw.layout.offsets
        end = int(table[-1]) + raw.layout.chunk_bytes(raw.layout.n_chunks - 1)
        assert end == data.size and end % 4 == 0 and int(table[-1]) % 4 == 0
        got = ops.tiff_unpack(torch.from_numpy(np.ascontiguousarray(data)).to(DEV), [raw.layout], table[None])
        assert torch.equal(_bits(got).cpu(), _bits(torch.from_numpy(a[None])))


# ------------------------------------------------------------------------------------------------ the loaders
LAYOUTS = [dict(), dict(big_endian=True, tile=(16, 16), misalign=2), dict(deflate=True, predictor=3, rows_per_strip=9, misalign=1),
           dict(rows_per_strip=64, misalign=2), dict(planar=True, misalign=3), dict(predictor=3, big_endian=True), dict(deflate=True, tile=(64, 32))]


def _items(source, monkeypatch, device_decode):
    monkeypatch.setenv("CMDIAD_TIFF_DEVICE", "1" if device_decode else "0")
    return list(source.train()), list(source.test())


def _assert_same_items(got, want):
    assert len(got) == len(want) > 0
    for k, (x, y) in enumerate(zip(got, want)):
        assert len(x) == len(y), k
        assert len(x[0]) == len(y[0]) == 3 and all(a.is_cuda and torch.equal(_bits(a), _bits(b)) for a, b in zip(x[0], y[0])), k
        assert x[0].n_valid == y[0].n_valid and x[0].n_valid > 0, k
        if len(x) == 4:
            assert torch.equal(x[1], y[1]) and int(x[2]) == int(y[2]) and x[3] == y[3], k
        else:
            assert int(x[1]) == int(y[1]), k


def _count_device_unpacks(monkeypatch):
    """Every path whose RawCloud reaches tiff.unpack_on_device from here on."""
    calls = []
    real = tiff.unpack_on_device
    monkeypatch.setattr(tiff, "unpack_on_device", lambda raws, device: calls.extend(r.path for r in raws) or real(raws, device))
    return calls


def test_sample_class_yields_the_same_items_with_device_decode(tmp_path, monkeypatch):
    """MVTec3DClass('hip') over the tree of sample_prep_ref.write_tree with its clouds rewritten as REAL TIFFs of seven layouts (one
    big-endian and tiled, one deflate with predictor 3), `tifffile` absent: CMDIAD_TIFF_DEVICE=1 and =0 yield equal tensors, order,
    labels and rgb_path; with =1 every cloud was unpacked on the device, with =0 none; the host methods never see a RawCloud."""
    root = str(tmp_path)
    items = spr.write_tree(root, size=160)
    monkeypatch.setitem(sys.modules, "tifffile", None)
    for k, (stem, (pc, _, _)) in enumerate(sorted(items.items())):
        sub, name = os.path.split(stem)
        tr.write(os.path.join(root, "bagel", sub, "xyz", name + ".tiff"), pc, **LAYOUTS[k % len(LAYOUTS)])
    args = types.SimpleNamespace(dataset_path=root, img_process_method="hip", num_workers=2)
    cls = ds.MVTec3DClass(root, "bagel", args)
    assert (cls.n_train, cls.n_test) == (3, 4)
    calls = _count_device_unpacks(monkeypatch)
    host = _items(cls, monkeypatch, False)
    assert not calls
    dev = _items(cls, monkeypatch, True)
    assert len(calls) == 7
    for got, want in zip(dev, host):
        _assert_same_items(got, want)
    assert [int(t[2]) for t in dev[1]] == [1, 1, 0, 0] and [t[3] for t in dev[1]] == [t[3] for t in host[1]]
    one = cls._loader("test").dataset[0]                      # the item path (one prepare call per item) takes a RawCloud too
    assert all(torch.equal(_bits(a[0]), _bits(b)) for a, b in zip(dev[1][0][0], one[0]))
    del calls[:]
    cpu = ds.MVTec3DClass(root, "bagel", types.SimpleNamespace(dataset_path=root, img_process_method="cpu_v1", num_workers=0))
    sample, label = next(iter(cpu.train()))
    assert not calls and not sample[1].is_cuda and torch.equal(_bits(sample[1]), _bits(dev[0][0][0][1].cpu()))


def test_raw_scan_class_yields_the_same_items_with_device_decode(tmp_path, monkeypatch):
    """MVTec3DRawClass over preprocess_ref.write_raw_tree (two shapes) written as real TIFFs by the generator."""
    from cmdiad_amd import evaluate as ev
    root = str(tmp_path)
    count = [0]

    def imwrite(path, a):
        tr.write(path, a, **LAYOUTS[(count[0] + 1) % len(LAYOUTS)])
        count[0] += 1

    stems = pr.write_raw_tree(root, types.SimpleNamespace(imwrite=imwrite))
    monkeypatch.setitem(sys.modules, "tifffile", None)
    args = ev.mtfi_args(dataset_path=root, img_process_method="hip", num_workers=2)
    cls = ds.MVTec3DRawClass(root, "bagel", args)
    assert (cls.n_train, cls.n_test) == (3, 4) and count[0] == 7
    calls = _count_device_unpacks(monkeypatch)
    host = _items(cls, monkeypatch, False)
    assert not calls
    dev = _items(cls, monkeypatch, True)
    assert len(calls) == 7
    for got, want in zip(dev, host):
        _assert_same_items(got, want)
    assert [int(t[2]) for t in dev[1]] == [0, 0, 1, 1]
    assert [t[3] for t in dev[1]] == [[os.path.join(root, "bagel", os.path.dirname(s), "rgb", os.path.basename(s) + ".png")] for s, _, _ in stems[3:]]
    # the dtype check of the reader reads the layout: a float64 file is refused by name before anything is uploaded
    bad = os.path.join(root, "bagel", "train", "good", "xyz", "000.tiff")
    tr.write(bad, np.zeros((120, 120, 3), np.float64))
    with pytest.raises(TypeError, match="000.tiff.*float32.*float64"):
        list(cls.train())
