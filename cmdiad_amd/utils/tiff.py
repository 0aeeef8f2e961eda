"""A self-contained codec for the floating-point TIFFs this project meets: the xyz files of MVTec 3D-AD (3-channel float32) and of
the Eyecandies preprocessing script (3-channel float64).  Pure Python + numpy; `tifffile` is not needed (docs/tiff.md).

  read_layout(path | bytes) -> TiffLayout     the first IFD of a classic TIFF, checked against the file's length
  imread(path)              -> ndarray        host decode, [H,W] or [H,W,C] in native byte order, every bit preserved
  imwrite(path, array)                        little-endian, uncompressed, chunky, strips of whole rows
  read_raw(path, out=None)  -> RawCloud       the file's bytes + layout, deflate chunks inflated, the predictor NOT undone
  unpack_on_device(list[RawCloud], device) -> tensor [B,H,W,C]     one pinned upload, one launch per group of equal layout
                                                                   (csrc/tiff.hip: cmdiad_tiff_unpack)

Supported: classic TIFF (magic 42), `II` and `MM`, strips or tiles, chunky or planar, IEEE float 32 / 64, no compression or deflate
(8 and 32946), predictor 1 or 3.  Everything else is refused with a ValueError that names the tag and its value.

Predictor 3 (floating-point horizontal differencing) follows libtiff's fpAcc: per chunk row of chunk_w * Cc * bps bytes -- Cc = C
for chunky files, 1 for planar ones -- a running byte sum mod 256 with stride Cc, then byte k of sample i is taken from plane k of
the row (plane 0 holds the most significant bytes, whatever the file's byte order).  The single-channel case was checked bit for bit
against files written by Pillow's libtiff; the stride of multi-channel files rests on libtiff's source alone.
"""
import os
import struct
import sys
import zlib
from dataclasses import dataclass, replace

import numpy as np

TIFF_DEVICE_ENV = "CMDIAD_TIFF_DEVICE"
MAX_DEVICE_ROW_BYTES = 64 * 1024      # a predictor-3 chunk row must fit the kernel's LDS row buffer; longer rows are undone on the host
_HINT = "; this reader covers uncompressed / deflate IEEE-float TIFFs only: install `tifffile` to read this file"
_TYPE_SIZES = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 16: 8}
_TYPE_CODES = {1: "u1", 3: "u2", 4: "u4", 6: "i1", 8: "i2", 9: "i4", 16: "u8"}
_NATIVE_BIG = sys.byteorder == "big"


def device_decode_enabled():
    """CMDIAD_TIFF_DEVICE=1, read at call time: the reader threads of the 'hip' sample sources hand out RawCloud objects and the clouds
    are unpacked on the device.  Off by default."""
    return os.environ.get(TIFF_DEVICE_ENV, "0") == "1"


@dataclass(frozen=True)
class TiffLayout:
    """Where the samples of one image lie.  A strip is a tile of full width: chunk_w == width, chunk_h == rows per strip.  Chunks are
    numbered row-major over the image, plane after plane for planar files; offsets / counts are int64 arrays of one entry per chunk."""
    width: int
    height: int
    channels: int
    dtype: np.dtype            # float32 | float64, native byte order
    big_endian: bool
    planar: bool
    predictor: int             # 1 | 3
    compression: int           # 1 | 8 | 32946
    chunk_w: int
    chunk_h: int
    offsets: np.ndarray
    counts: np.ndarray

    @property
    def bytes_per_sample(self):
        return self.dtype.itemsize

    @property
    def chunk_channels(self):
        return 1 if self.planar else self.channels

    @property
    def chunks_across(self):
        return -(-self.width // self.chunk_w)

    @property
    def chunks_down(self):
        return -(-self.height // self.chunk_h)

    @property
    def n_chunks(self):
        return self.chunks_across * self.chunks_down * (self.channels if self.planar else 1)

    @property
    def row_bytes(self):
        """Bytes of one chunk row, padding columns of a tile included: the unit of predictor 3."""
        return self.chunk_w * self.chunk_channels * self.bytes_per_sample

    @property
    def is_tiled(self):
        return self.chunk_w != self.width

    def chunk_rows(self, k):
        """Rows that chunk k holds in the file: chunk_h for a tile (tiles are stored whole), the remaining rows for the last strip."""
        if self.is_tiled:
            return self.chunk_h
        down = (k % (self.chunks_across * self.chunks_down)) // self.chunks_across
        return min(self.chunk_h, self.height - down * self.chunk_h)

    def chunk_bytes(self, k):
        return self.chunk_rows(k) * self.row_bytes

    def all_chunk_bytes(self):
        """chunk_bytes of every chunk as one int64 array (a file of 64 KiB strips has hundreds: no Python loop on the reader threads)."""
        if self.is_tiled:
            return np.full(self.n_chunks, self.chunk_h * self.row_bytes, dtype=np.int64)
        down = np.arange(self.n_chunks, dtype=np.int64) % self.chunks_down       # (strips: one chunk across)
        return np.minimum(self.chunk_h, self.height - down * self.chunk_h) * self.row_bytes

    def geometry(self):
        """What two images must share to go through one launch: everything but the offsets."""
        return (self.width, self.height, self.channels, self.dtype.str, self.big_endian, self.planar, self.predictor, self.chunk_w,
                self.chunk_h)


class RawCloud:
    """The bytes of one xyz TIFF as `read_raw` returns them (`data`, uint8, uncompressed chunks at `layout.offsets`) in place of the
    decoded array: `shape`, `dtype` and `ndim` are those of the array `imread` would return for a multi-channel file."""

    def __init__(self, data, layout, path=None):
        self.data, self.layout, self.path = data, layout, path

    @property
    def shape(self):
        return (self.layout.height, self.layout.width, self.layout.channels)

    @property
    def dtype(self):
        return self.layout.dtype

    ndim = 3


# ------------------------------------------------------------------------------------------------ parsing
def _buffer(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return memoryview(src).cast("B") if not isinstance(src, bytes) else src
    if isinstance(src, np.ndarray):
        return memoryview(np.ascontiguousarray(src, dtype=np.uint8)).cast("B")
    with open(src, "rb") as fh:
        return fh.read()


def read_layout(src):
    """path or bytes -> TiffLayout of the first IFD.  ValueError for anything outside the supported subset (the message names the tag and
    its value) and for a truncated or inconsistent file: every chunk is checked against the file's length here, at parse time."""
    buf = _buffer(src)
    size = len(buf)
    if size < 8:
        raise ValueError(f"not a TIFF file: {size} bytes")
    order = bytes(buf[0:2])
    if order not in (b"II", b"MM"):
        raise ValueError(f"not a TIFF file: byte-order mark {order!r}")
    e = "<" if order == b"II" else ">"
    magic, = struct.unpack_from(e + "H", buf, 2)
    if magic == 43:
        raise ValueError("BigTIFF (magic 43) is not supported" + _HINT)
    if magic != 42:
        raise ValueError(f"not a TIFF file: magic {magic}")
    ifd, = struct.unpack_from(e + "I", buf, 4)
    if ifd < 8 or ifd + 2 > size:
        raise ValueError(f"truncated TIFF: the IFD offset {ifd} points outside the file ({size} bytes)")
    n_entries, = struct.unpack_from(e + "H", buf, ifd)
    if ifd + 2 + 12 * n_entries > size:
        raise ValueError(f"truncated TIFF: the IFD at {ifd} with {n_entries} entries ends outside the file ({size} bytes)")
    tags = {}
    for k in range(n_entries):
        pos = ifd + 2 + 12 * k
        tag, typ, count = struct.unpack_from(e + "HHI", buf, pos)
        if tag not in (256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317, 322, 323, 324, 325, 338, 339):
            continue
        if typ not in _TYPE_CODES:
            raise ValueError(f"tag {tag}: field type {typ} is not an integer type" + _HINT)
        nbytes = _TYPE_SIZES[typ] * count
        at = pos + 8
        if nbytes > 4:
            at, = struct.unpack_from(e + "I", buf, pos + 8)
            if at + nbytes > size:
                raise ValueError(f"truncated TIFF: the {count} values of tag {tag} at offset {at} end outside the file ({size} bytes)")
        tags[tag] = np.frombuffer(buf, dtype=np.dtype(e + _TYPE_CODES[typ]), count=count, offset=at).astype(np.int64)

    def one(tag, default=None):
        v = tags.get(tag)
        if v is None or len(v) == 0:
            if default is None:
                raise ValueError(f"tag {tag} is missing")
            return default
        return int(v[0])

    width, height = one(256), one(257)
    channels = one(277, 1)
    if width < 1 or height < 1 or channels < 1:
        raise ValueError(f"bad image size: ImageWidth (256) = {width}, ImageLength (257) = {height}, SamplesPerPixel (277) = {channels}")
    bits = tags.get(258, np.array([1]))
    if len(set(bits.tolist())) != 1:
        raise ValueError(f"BitsPerSample (258) = {bits.tolist()}: mixed sample sizes are not supported" + _HINT)
    fmt = tags.get(339, np.array([1]))
    if set(fmt.tolist()) != {3} or int(bits[0]) not in (32, 64):
        raise ValueError(f"SampleFormat (339) = {fmt.tolist()} with BitsPerSample (258) = {bits.tolist()}: only IEEE float 32 / 64 "
                         f"samples (SampleFormat 3) are supported" + _HINT)
    compression = one(259, 1)
    if compression not in (1, 8, 32946):
        raise ValueError(f"Compression (259) = {compression}: only none (1) and deflate (8, 32946) are supported" + _HINT)
    predictor = one(317, 1)
    if predictor not in (1, 3):
        raise ValueError(f"Predictor (317) = {predictor}: only none (1) and floating-point (3) are supported" + _HINT)
    planar_cfg = one(284, 1)
    if planar_cfg not in (1, 2):
        raise ValueError(f"PlanarConfiguration (284) = {planar_cfg}")
    planar = planar_cfg == 2 and channels > 1
    if 322 in tags or 324 in tags:
        chunk_w, chunk_h = one(322), one(323)
        offsets, counts = tags.get(324), tags.get(325)
        names = "TileOffsets (324) / TileByteCounts (325)"
        if chunk_w < 1 or chunk_h < 1:
            raise ValueError(f"TileWidth (322) = {chunk_w}, TileLength (323) = {chunk_h}")
    else:
        chunk_w, chunk_h = width, min(max(one(278, height), 1), height)
        offsets, counts = tags.get(273), tags.get(279)
        names = "StripOffsets (273) / StripByteCounts (279)"
    if offsets is None or counts is None:
        raise ValueError(f"{names} missing")
    lay = TiffLayout(width, height, channels, np.dtype(np.float32 if int(bits[0]) == 32 else np.float64), e == ">", planar, predictor,
                     compression, chunk_w, chunk_h, offsets, counts)
    if len(offsets) != lay.n_chunks or len(counts) != lay.n_chunks:
        raise ValueError(f"{names} hold {len(offsets)} / {len(counts)} entries, the image geometry needs {lay.n_chunks} chunks")
    _check_chunks(lay, size)
    return lay


def _check_chunks(lay, size):
    off, cnt, need = lay.offsets, lay.counts, lay.all_chunk_bytes()
    bad = np.flatnonzero((off < 0) | (cnt < 0) | (off + cnt > size))
    if len(bad):
        k = int(bad[0])
        raise ValueError(f"truncated TIFF: chunk {k} at offset {int(off[k])} with {int(cnt[k])} bytes ends past the end of the file ({size} bytes)")
    bad = np.flatnonzero(cnt < need) if lay.compression == 1 else ()
    if len(bad):
        k = int(bad[0])
        raise ValueError(f"inconsistent TIFF: chunk {k} holds {int(cnt[k])} bytes, its geometry ({lay.chunk_rows(k)} rows of {lay.row_bytes} "
                         f"bytes) needs {int(need[k])}")


def _inflate(buf, lay, k):
    off, cnt = int(lay.offsets[k]), int(lay.counts[k])
    try:
        raw = zlib.decompress(buf[off:off + cnt])      # (zlib releases the GIL)
    except zlib.error as exc:
        raise ValueError(f"corrupt TIFF: chunk {k} does not inflate ({exc})") from exc
    if len(raw) < lay.chunk_bytes(k):
        raise ValueError(f"inconsistent TIFF: chunk {k} inflates to {len(raw)} bytes, its geometry needs {lay.chunk_bytes(k)}")
    return raw


# ------------------------------------------------------------------------------------------------ host decode
def undo_predictor3(rows, stride, bps):
    """rows uint8 [n, row_bytes] as stored -> uint8 [n, row_bytes / bps, bps] holding every sample's bytes most significant first."""
    n, row_bytes = rows.shape
    acc = np.cumsum(rows.reshape(n, row_bytes // stride, stride), axis=1, dtype=np.uint8).reshape(n, bps, row_bytes // bps)
    return np.ascontiguousarray(acc.transpose(0, 2, 1))


def _decode(buf, lay):
    """uint8 buffer with UNCOMPRESSED chunks at lay.offsets -> [H,W,C] array of native unsigned integers (the samples' bits)."""
    bps, cc = lay.bytes_per_sample, lay.chunk_channels
    uint = np.dtype(f"u{bps}")
    per_plane = lay.chunks_across * lay.chunks_down
    data = np.frombuffer(buf, dtype=np.uint8)
    if lay.predictor == 1 and lay.big_endian == _NATIVE_BIG and not lay.planar and not lay.is_tiled:
        # strips of native samples lying back to back (what imwrite and most writers produce) ARE the image: no copy
        ends = lay.offsets + lay.all_chunk_bytes()
        first = int(lay.offsets[0])
        if np.array_equal(ends[:-1], lay.offsets[1:]) and (data.ctypes.data + first) % bps == 0:
            return data[first:int(ends[-1])].view(uint).reshape(lay.height, lay.width, lay.channels)
    out = np.empty((lay.height, lay.width, lay.channels), dtype=uint)
    for k in range(lay.n_chunks):
        plane, rest = divmod(k, per_plane) if lay.planar else (0, k)
        down, across = divmod(rest, lay.chunks_across)
        y0, x0 = down * lay.chunk_h, across * lay.chunk_w
        rows, cols = min(lay.chunk_h, lay.height - y0), min(lay.chunk_w, lay.width - x0)
        off = int(lay.offsets[k])
        chunk = data[off:off + rows * lay.row_bytes].reshape(rows, lay.row_bytes)
        if lay.predictor == 3:
            vals = undo_predictor3(chunk, cc, bps).view(uint.newbyteorder(">")).reshape(rows, lay.chunk_w, cc)
        else:
            vals = chunk.view(uint.newbyteorder(">" if lay.big_endian else "<")).reshape(rows, lay.chunk_w, cc)
        if lay.planar:
            out[y0:y0 + rows, x0:x0 + cols, plane] = vals[:, :cols, 0]
        else:
            out[y0:y0 + rows, x0:x0 + cols, :] = vals[:, :cols, :]
    return out


def _decoded_array(raw):
    arr = _decode(raw.data, raw.layout).view(raw.layout.dtype)
    return arr


def imread(path):
    """Host decode: [H,W] for one channel, [H,W,C] otherwise, float32 or float64 in native byte order; every sample's bits are the
    file's (NaN payloads, -0.0, denormals).  Planar files (PlanarConfiguration 2) come back as [H,W,C] too -- `tifffile` would return
    [C,H,W] for those, a shape the dataset classes cannot use."""
    raw = read_raw(path)
    arr = _decoded_array(raw)
    return arr[:, :, 0] if raw.layout.channels == 1 else arr


def imwrite(path, array):
    """float32 or float64 [H,W] or [H,W,C] -> a little-endian, uncompressed, chunky TIFF with strips of whole rows (about 64 KiB each);
    photometric RGB for C = 3, else MinIsBlack with the further channels as ExtraSamples; SampleFormat 3; the strip data start
    16-byte aligned."""
    a = np.asarray(array)
    if a.dtype not in (np.float32, np.float64) or a.ndim not in (2, 3) or a.size == 0:
        raise ValueError(f"tiff.imwrite: a non-empty float32 or float64 [H,W] or [H,W,C] array is expected, got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    data = np.ascontiguousarray(a, dtype=a.dtype.newbyteorder("<"))
    bps = a.dtype.itemsize
    row = w * c * bps
    rps = max(1, min(h, (64 * 1024) // row))
    n_strips = -(-h // rps)
    entries = []          # (tag, type, values)
    entries += [(256, 4, [w]), (257, 4, [h]), (258, 3, [8 * bps] * c), (259, 3, [1]), (262, 3, [2 if c == 3 else 1]),
                (273, 4, None), (277, 3, [c]), (278, 4, [rps]), (279, 4, None), (284, 3, [1])]
    if c != 3 and c > 1:
        entries.append((338, 3, [0] * (c - 1)))
    entries.append((339, 3, [3] * c))
    entries.sort(key=lambda t: t[0])
    ifd_at = 8
    ifd_bytes = 2 + 12 * len(entries) + 4
    pos = ifd_at + ifd_bytes
    placed = {}
    for tag, typ, vals in entries:         # where the out-of-line values go
        n = n_strips if vals is None else len(vals)
        nbytes = n * (2 if typ == 3 else 4)
        if nbytes > 4:
            placed[tag] = pos
            pos += nbytes + (nbytes & 1)
    data_at = (pos + 15) & ~15
    counts = [min(rps, h - s * rps) * row for s in range(n_strips)]
    offsets = [data_at + s * rps * row for s in range(n_strips)]
    if offsets[-1] + counts[-1] >= 1 << 32:
        raise ValueError("tiff.imwrite: the image does not fit a classic TIFF (4 GiB)")
    head = bytearray(data_at)
    head[0:8] = struct.pack("<2sHI", b"II", 42, ifd_at)
    struct.pack_into("<H", head, ifd_at, len(entries))
    for k, (tag, typ, vals) in enumerate(entries):
        vals = offsets if tag == 273 else counts if tag == 279 else vals
        code = "H" if typ == 3 else "I"
        at = ifd_at + 2 + 12 * k
        struct.pack_into("<HHI", head, at, tag, typ, len(vals))
        if tag in placed:
            struct.pack_into("<I", head, at + 8, placed[tag])
            struct.pack_into(f"<{len(vals)}{code}", head, placed[tag], *vals)
        else:
            struct.pack_into(f"<{len(vals)}{code}", head, at + 8, *vals)
    with open(path, "wb") as fh:
        fh.write(head)
        fh.write(data.reshape(-1).view(np.uint8))


# ------------------------------------------------------------------------------------------------ raw bytes for the device
def _pad16(n):
    return (n + 15) & ~15


def read_raw(path, out=None):
    """The file's bytes and its layout.  `data` is a uint8 array; with `out` (a writable uint8 array, e.g. a slice of a pinned batch
    buffer, large enough for the file and for its inflated chunks: else ValueError, for the file before anything is read) the file
    is read straight into it with readinto.  Deflate chunks are inflated here, on the calling (reader) thread, and the returned
    layout then describes uncompressed chunks at rewritten offsets.  The predictor is NOT undone."""
    if isinstance(path, (bytes, bytearray, memoryview, np.ndarray)):
        data, where = np.frombuffer(_buffer(path), dtype=np.uint8), None
    else:
        size, where = os.path.getsize(path), path
        if out is not None and len(out) < size:
            raise ValueError(f"tiff.read_raw: out holds {len(out)} bytes, the file {path} has {size}")
        data = out[:size] if out is not None else np.zeros(_pad16(size), dtype=np.uint8)[:size]
        with open(path, "rb") as fh:
            got = fh.readinto(memoryview(data).cast("B"))
        if got != size:
            raise ValueError(f"{path}: short read, {got} of {size} bytes")
    try:
        lay = read_layout(data)
    except ValueError as exc:
        raise ValueError(f"{where or 'tiff'}: {exc}") from exc
    if lay.compression == 1:
        if out is not None and where is None:          # (bytes given in place of a path: they are copied into out)
            if len(out) < len(data):
                raise ValueError(f"tiff.read_raw: out holds {len(out)} bytes, the file has {len(data)}")
            out[:len(data)] = data
            data = out[:len(data)]
        return RawCloud(data, lay, where)
    chunks = [_inflate(data, lay, k)[:lay.chunk_bytes(k)] for k in range(lay.n_chunks)]
    counts = np.array([len(c) for c in chunks], dtype=np.int64)
    offsets = np.zeros(len(chunks), dtype=np.int64)
    np.cumsum(counts[:-1], out=offsets[1:])
    total = int(counts.sum())
    if out is not None:
        if len(out) < total:
            raise ValueError(f"tiff.read_raw: out holds {len(out)} bytes, the inflated chunks need {total}")
        flat = out[:total]
    else:
        flat = np.zeros(_pad16(total), dtype=np.uint8)[:total]
    for off, c in zip(offsets, chunks):
        flat[off:off + len(c)] = np.frombuffer(c, dtype=np.uint8)
    return RawCloud(flat, replace(lay, compression=1, offsets=offsets, counts=counts), where)


def host_unpacked(raw):
    """A RawCloud whose predictor and byte order have been undone on the host: one strip of native samples (the form the device kernel
    copies).  For predictor-3 rows longer than MAX_DEVICE_ROW_BYTES."""
    arr = np.ascontiguousarray(_decoded_array(raw))
    lay = raw.layout
    simple = replace(lay, big_endian=_NATIVE_BIG, planar=False, predictor=1, compression=1, chunk_w=lay.width, chunk_h=lay.height,
                     offsets=np.zeros(1, dtype=np.int64), counts=np.array([arr.nbytes], dtype=np.int64))
    return RawCloud(arr.reshape(-1).view(np.uint8), simple, raw.path)


def unpack_on_device(raws, device):
    """list of RawCloud of one shape and dtype -> device tensor [B,H,W,C] of the files' float type, in the list's order.  The bytes of
    all files and their chunk tables go up in ONE pinned buffer on the shared copy stream; every group of equal layout is one
    cmdiad_tiff_unpack launch on the current stream.  A predictor-3 file whose chunk row exceeds 64 KiB is undone on the host first."""
    import torch
    from .. import ops
    from ..dataset import _shared_stream
    if not raws:
        raise ValueError("tiff.unpack_on_device: no clouds")
    raws = [host_unpacked(r) if r.layout.predictor == 3 and r.layout.row_bytes > MAX_DEVICE_ROW_BYTES else r for r in raws]
    first = raws[0]
    for r in raws:
        if r.shape != first.shape or r.dtype != first.dtype:
            raise ValueError(f"tiff.unpack_on_device: clouds of one shape and dtype expected, got {r.dtype} {r.shape} beside "
                             f"{first.dtype} {first.shape}")
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    groups = {}
    for i, r in enumerate(raws):
        groups.setdefault(r.layout.geometry(), []).append(i)
    # pinned buffer: [tables of every group, int64] [file 0, padded to 16] [file 1] ...
    table_bytes = _pad16(8 * sum(r.layout.n_chunks for r in raws))
    starts, pos = [], table_bytes
    for r in raws:
        starts.append(pos)
        pos += _pad16(len(r.data))
    host = torch.empty(pos, dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    tables, at = {}, 0
    for key, idx in groups.items():
        n = raws[idx[0]].layout.n_chunks
        tab = view[at:at + 8 * n * len(idx)].view(np.int64).reshape(len(idx), n)
        for row, i in enumerate(idx):
            tab[row] = raws[i].layout.offsets + starts[i]
        tables[key] = (at, tab)
        at += 8 * n * len(idx)
    view[at:table_bytes] = 0
    for r, s in zip(raws, starts):
        n = len(r.data)
        view[s:s + n] = r.data
        view[s + n:s + _pad16(n)] = 0
    cur = torch.cuda.current_stream(dev)
    with torch.cuda.stream(_shared_stream(dev, "dataset.copy")):
        buf = host.to(dev, non_blocking=True)
    cur.wait_stream(_shared_stream(dev, "dataset.copy"))
    buf.record_stream(cur)
    out = torch.empty((len(raws), *first.shape), dtype=getattr(torch, first.dtype.name), device=dev)
    with torch.cuda.device(dev):
        for key, idx in groups.items():
            at, tab = tables[key]
            n = tab.shape[1]
            tab_dev = buf[at:at + tab.size * 8].view(torch.int64).view(len(idx), n)
            whole = len(groups) == 1
            got = ops.tiff_unpack(buf, [raws[i].layout for i in idx], tab, table_dev=tab_dev, out=out if whole else None)
            if not whole:
                out.index_copy_(0, torch.tensor(idx, dtype=torch.int64).pin_memory().to(dev, non_blocking=True), got)
    return out
