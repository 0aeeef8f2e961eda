"""The datasets' PNGs without Pillow: a chunk parser, a raw reader that inflates on the calling (reader) thread, and the upload to the
device, where csrc/png.hip undoes the row filters (docs/png.md).  Pure Python + numpy + zlib.

  read_layout(path | bytes) -> PngLayout      signature, chunk walk (lengths against the file's length), IHDR first, CRC of IHDR and IDATs
  supported(layout)         -> bool           the subset the device decodes; everything else stays with Pillow, it is no error
  read_raw(path, target)    -> RawImage       the inflated, still FILTERED scanlines: uint8, exactly H * (1 + row_bytes) bytes
  decode_on_device(list[RawImage], device) -> uint8 tensor [B, ...]    one pinned upload, one cmdiad_png_unfilter launch per layout
and the way back, for the overlays (docs/overlay.md):
  encode(scanlines, layout, level) -> bytes   signature, IHDR, one IDAT of zlib.compress, IEND
  encode_on_device(images) / write_many(paths, images)    one cmdiad_png_filter launch, one copy down, deflate on writer threads

`target` names what the caller would have done with Pillow: 'rgb' = .convert('RGB') -> [H,W,3] (alpha dropped, grey replicated),
'l' = .convert('L') -> [H,W] (the grey byte, or (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16), 'raw' = np.array(Image.open(p))
-> the file's own channels, [H,W] for one channel, else [H,W,C].  The switch: CMDIAD_PNG_DEVICE=1, read per file by the reader.
"""
import os
import struct
import zlib
from dataclasses import dataclass

import numpy as np

PNG_DEVICE_ENV = "CMDIAD_PNG_DEVICE"
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_DEVICE_ROW_BYTES = 64 * 1024       # the kernel's carry row; holds for any side <= 2^14 at 4 bytes per pixel
TARGETS = ("rgb", "l", "raw")          # the index is the kernel's target code
_CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def device_decode_enabled():
    """CMDIAD_PNG_DEVICE=1, read at call time: the reader threads of the 'hip' sample sources hand out RawImage objects for the PNGs
    `supported` accepts and the row filters are undone on the device.  Off by default."""
    return os.environ.get(PNG_DEVICE_ENV, "0") == "1"


@dataclass(frozen=True)
class PngLayout:
    width: int
    height: int
    bit_depth: int
    color_type: int            # 0 grey, 2 rgb, 3 palette, 4 grey + alpha, 6 rgb + alpha
    channels: int
    bpp: int                   # bytes per pixel as the filters see it: max(1, channels * bit_depth / 8)
    row_bytes: int             # bytes of a scanline without its filter byte
    interlace: int
    has_plte: bool
    has_trns: bool
    compression: int = 0
    filter_method: int = 0

    def geometry(self):
        """What two images must share to go through one launch."""
        return (self.width, self.height, self.bpp)


class RawImage:
    """The inflated, still filtered scanlines of one PNG (`data`, uint8 [H * (1 + row_bytes)]) in place of the decoded array: `shape`,
    `dtype` and `ndim` are those of the array the caller gets from Pillow for its `target`."""
    dtype = np.dtype(np.uint8)

    def __init__(self, data, layout, path=None, target="rgb"):
        if target not in TARGETS:
            raise ValueError(f"png: target must be one of {TARGETS}, got {target!r}")
        self.data, self.layout, self.path, self.target = data, layout, path, target

    @property
    def shape(self):
        lay = self.layout
        if self.target == "rgb":
            return (lay.height, lay.width, 3)
        if self.target == "l" or lay.channels == 1:
            return (lay.height, lay.width)
        return (lay.height, lay.width, lay.channels)

    @property
    def ndim(self):
        return len(self.shape)


# ------------------------------------------------------------------------------------------------ parsing
def _buffer(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return memoryview(src).cast("B")
    if isinstance(src, np.ndarray):
        return memoryview(np.ascontiguousarray(src, dtype=np.uint8)).cast("B")
    with open(src, "rb") as fh:
        return memoryview(fh.read())


def _name(src):
    return "png" if isinstance(src, (bytes, bytearray, memoryview, np.ndarray)) else str(src)


def _walk(buf, where):
    """(PngLayout, [memoryview of every IDAT payload]) of the file in buf; ValueError naming `where` for a malformed file."""
    size = len(buf)
    if size < 8 or bytes(buf[:8]) != SIGNATURE:
        raise ValueError(f"{where}: not a PNG file (bad signature)")
    pos, ihdr, idats, plte, trns, end = 8, None, [], False, False, False
    while pos < size:
        if pos + 8 > size:
            raise ValueError(f"{where}: truncated: a chunk header at byte {pos} leaves the file's {size} bytes")
        length, kind = struct.unpack_from(">I4s", buf, pos)
        if pos + 12 + length > size:
            raise ValueError(f"{where}: truncated: chunk {kind!r} at byte {pos} with {length} bytes leaves the file's {size} bytes")
        body = buf[pos + 8:pos + 8 + length]
        if ihdr is None and kind != b"IHDR":
            raise ValueError(f"{where}: the first chunk must be IHDR, got {kind!r}")
        if kind in (b"IHDR", b"IDAT"):
            crc, = struct.unpack_from(">I", buf, pos + 8 + length)
            if zlib.crc32(body, zlib.crc32(kind)) != crc:
                raise ValueError(f"{where}: bad CRC in chunk {kind!r} at byte {pos}")
        if kind == b"IHDR":
            if ihdr is not None or length != 13:
                raise ValueError(f"{where}: IHDR must come once, first, with 13 bytes (got {length} at byte {pos})")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idats.append(body)
        elif kind == b"PLTE":
            plte = True
        elif kind == b"tRNS":
            trns = True
        elif kind == b"IEND":
            end = True
            break
        pos += 12 + length
    if ihdr is None:
        raise ValueError(f"{where}: truncated: no IHDR")
    if not idats:
        raise ValueError(f"{where}: no IDAT chunk")
    if not end:
        raise ValueError(f"{where}: truncated: no IEND chunk")
    width, height, depth, ctype, comp, filt, lace = ihdr
    if width < 1 or height < 1 or ctype not in _CHANNELS or depth not in (1, 2, 4, 8, 16):
        raise ValueError(f"{where}: bad IHDR: {width} x {height}, bit depth {depth}, colour type {ctype}")
    channels = _CHANNELS[ctype]
    bits = channels * depth
    lay = PngLayout(width=width, height=height, bit_depth=depth, color_type=ctype, channels=channels, bpp=max(1, bits // 8),
                    row_bytes=(width * bits + 7) // 8, interlace=lace, has_plte=plte, has_trns=trns, compression=comp,
                    filter_method=filt)
    return lay, idats


def read_layout(src):
    """path or bytes -> PngLayout.  ValueError naming the path for a bad signature, a truncated file (a chunk that leaves the file, no
    IEND), a first chunk that is not a 13-byte IHDR, a bad CRC of IHDR or of an IDAT, or no IDAT."""
    return _walk(_buffer(src), _name(src))[0]


def supported(layout):
    """True for what the device decodes: non-interlaced, compression 0 and filter method 0, bit depth 8, colour types 0 / 2 / 4 / 6, no
    PLTE, no tRNS, row_bytes <= 64 KiB.  A file outside this subset is decoded with Pillow by the caller, as before."""
    return (layout.interlace == 0 and layout.compression == 0 and layout.filter_method == 0 and layout.bit_depth == 8
            and layout.color_type in (0, 2, 4, 6) and not layout.has_plte and not layout.has_trns
            and layout.row_bytes <= MAX_DEVICE_ROW_BYTES)


def _pad16(n):
    return (n + 15) & ~15


def _inflate(idats, lay, where):
    """The IDAT payloads through ONE decompressobj, as memoryviews, unjoined -> uint8 [H * (1 + row_bytes)] (in a buffer padded to 16)."""
    need = lay.height * (1 + lay.row_bytes)
    inflater = zlib.decompressobj()
    parts, got = [], 0
    try:
        for body in idats:
            if not len(body):
                continue
            piece = inflater.decompress(body, need + 1 - got)        # (never inflates past one byte too many)
            got += len(piece)
            parts.append(piece)
            if got > need:
                break
        if got <= need:
            piece = inflater.flush()
            got += len(piece)
            parts.append(piece)
    except zlib.error as exc:
        raise ValueError(f"{where}: the IDAT stream does not inflate: {exc}") from exc
    if got != need:
        raise ValueError(f"{where}: the IDAT stream inflates to {'more than ' + str(need) if got > need else got} bytes, "
                         f"{lay.height} scanlines of 1 + {lay.row_bytes} bytes are {need}")
    data = np.zeros(_pad16(need), dtype=np.uint8)[:need]
    at = 0
    for piece in parts:
        data[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
        at += len(piece)
    return data


def read_raw(path, target="rgb", layout_idats=None):
    """path or bytes -> RawImage(data, layout, path, target): the file parsed (`read_layout`'s checks), its IDAT stream inflated here, on
    the calling thread (zlib releases the GIL).  ValueError for any inflated length other than H * (1 + row_bytes) and for a filter
    byte above 4 (one strided comparison: the kernel never meets a bad type).  The filters are NOT undone."""
    where = _name(path)
    lay, idats = layout_idats if layout_idats is not None else _walk(_buffer(path), where)
    data = _inflate(idats, lay, where)
    types = data[::1 + lay.row_bytes]
    if (types > 4).any():
        row = int(np.argmax(types > 4))
        raise ValueError(f"{where}: filter type {int(types[row])} in row {row} (0..4 exist)")
    return RawImage(data, lay, None if where == "png" else path, target)


def read_for_device(path, target, color_types=(0, 2, 4, 6)):
    """What a reader thread calls under the switch: the file's RawImage when `supported` accepts it (and its colour type is one of
    color_types), else None -- the caller then decodes the file with Pillow exactly as before.  A malformed file raises ValueError."""
    where = str(path)
    lay, idats = _walk(_buffer(path), where)
    if not supported(lay) or lay.color_type not in color_types:
        return None
    return read_raw(path, target, layout_idats=(lay, idats))


# ------------------------------------------------------------------------------------------------ the device
def decode_on_device(raws, device):
    """list of RawImage of one shape and one target -> uint8 device tensor [B, *shape], in the list's order.  The scanlines of all
    images (each padded to 16 bytes) and their offset table go up in ONE pinned buffer on the shared copy stream; every group of
    equal layout is one cmdiad_png_unfilter launch on the current stream."""
    import torch
    from .. import ops
    from ..dataset import _shared_stream
    if not raws:
        raise ValueError("png.decode_on_device: no images")
    first = raws[0]
    for r in raws:
        if r.shape != first.shape or r.target != first.target:
            raise ValueError(f"png.decode_on_device: images of one shape and target expected, got {r.target!r} {r.shape} beside "
                             f"{first.target!r} {first.shape}")
        if not supported(r.layout):
            raise ValueError(f"png.decode_on_device: {r.path}: outside the subset the device decodes (decode it with Pillow)")
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    groups = {}
    for i, r in enumerate(raws):
        groups.setdefault(r.layout.geometry(), []).append(i)
    # pinned buffer: [offsets of every group, int64] [image 0, padded to 16] [image 1] ...
    table_bytes = _pad16(8 * len(raws))
    starts, pos = [], table_bytes
    for r in raws:
        starts.append(pos)
        pos += _pad16(len(r.data))
    host = torch.empty(pos, dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    tables, at = {}, 0
    for key, idx in groups.items():
        tab = view[at:at + 8 * len(idx)].view(np.int64)
        tab[:] = [starts[i] for i in idx]
        tables[key] = (at, tab)
        at += 8 * len(idx)
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
    out = torch.empty((len(raws), *first.shape), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        for key, idx in groups.items():
            at, tab = tables[key]
            tab_dev = buf[at:at + 8 * len(idx)].view(torch.int64)
            whole = len(groups) == 1
            got = ops.png_unfilter(buf, [raws[i].layout for i in idx], tab, first.target, out=out if whole else None, offsets_dev=tab_dev)
            if not whole:
                out.index_copy_(0, torch.tensor(idx, dtype=torch.int64).pin_memory().to(dev, non_blocking=True), got)
    return out


# ------------------------------------------------------------------------------------------------ the writer
_COLOR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}
FILTER_MODES = ("none", "sub", "up", "average", "paeth", "adaptive")       # the index is cmdiad_png_filter's mode


def _chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(body, zlib.crc32(kind)))


def write_layout(width, height, channels):
    """The PngLayout of the 8-bit file `encode` writes for an image of this size and channel count (1 grey, 2 grey + alpha, 3 rgb,
    4 rgb + alpha)."""
    if channels not in _COLOR_TYPE or width < 1 or height < 1:
        raise ValueError(f"png.write_layout: {width} x {height} with {channels} channels (sides >= 1, 1..4 channels)")
    return PngLayout(width=int(width), height=int(height), bit_depth=8, color_type=_COLOR_TYPE[channels], channels=channels, bpp=channels,
                     row_bytes=int(width) * channels, interlace=0, has_plte=False, has_trns=False)


def encode(scanlines, layout, level=6):
    """scanlines: the FILTERED rows of one image, uint8 [H * (1 + row_bytes)] (filter byte in front of every row: what `read_raw`
    returns and ops.png_filter produces) -> the bytes of a PNG: signature, IHDR, one IDAT holding zlib.compress(scanlines, level),
    IEND.  Runs on the calling thread; zlib releases the GIL."""
    if not supported(layout):
        raise ValueError("png.encode: 8-bit non-interlaced files of colour type 0 / 2 / 4 / 6 only")
    lines = np.ascontiguousarray(scanlines, dtype=np.uint8).reshape(-1)
    need = layout.height * (1 + layout.row_bytes)
    if lines.size != need:
        raise ValueError(f"png.encode: {lines.size} bytes of scanlines, {layout.height} rows of 1 + {layout.row_bytes} bytes are {need}")
    ihdr = struct.pack(">IIBBBBB", layout.width, layout.height, 8, layout.color_type, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(memoryview(lines), level)) + _chunk(b"IEND")


def _filtered_on_host(images_u8, mode):
    """(scanlines [n, H * (1 + W * C)] as a numpy view of one pinned buffer, layout): one ops.png_filter launch and one copy."""
    import torch
    from .. import ops
    if images_u8.dim() == 3:
        images_u8 = images_u8.unsqueeze(-1)
    n, H, W, C = images_u8.shape
    lay = write_layout(W, H, C)
    lines = ops.png_filter(images_u8.contiguous(), mode)
    host = torch.empty(lines.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(lines, non_blocking=True)
    torch.cuda.current_stream(lines.device).synchronize()
    return host.numpy(), lay


def encode_on_device(images_u8, level=6, mode="adaptive", writers=4):
    """images uint8 [n,H,W,C] (or [n,H,W]) ON THE DEVICE -> list of n PNG files as bytes.  The row filters run on the device
    (cmdiad_png_filter, one launch), the scanlines come down in one copy into a pinned buffer, and `writers` threads deflate."""
    import concurrent.futures as cf
    lines, lay = _filtered_on_host(images_u8, mode)
    if len(lines) <= 1 or writers <= 1:
        return [encode(row, lay, level) for row in lines]
    with cf.ThreadPoolExecutor(writers) as pool:
        return list(pool.map(lambda row: encode(row, lay, level), lines))


def write_many(paths, images_u8, level=6, mode="adaptive", writers=4):
    """One PNG per image of the device batch images_u8 [n,H,W,C] at paths[i] (the directories exist): filtered on the device,
    deflated and written by `writers` threads.  Returns the files' sizes in bytes."""
    import concurrent.futures as cf
    paths = list(paths)
    if len(paths) != images_u8.shape[0]:
        raise ValueError(f"png.write_many: {len(paths)} paths for {images_u8.shape[0]} images")
    if not paths:
        return []
    lines, lay = _filtered_on_host(images_u8, mode)

    def one(i):
        data = encode(lines[i], lay, level)
        with open(paths[i], "wb") as fh:
            fh.write(data)
        return len(data)
    if len(paths) == 1 or writers <= 1:
        return [one(i) for i in range(len(paths))]
    with cf.ThreadPoolExecutor(writers) as pool:
        return list(pool.map(one, range(len(paths))))
