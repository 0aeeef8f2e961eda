"""A small PNG WRITER for the tests of cmdiad_amd/utils/png.py and csrc/png.hip, and a plain numpy restatement of the five row filters
and of the three targets, both written from the PNG specification (5.3 chunk layout, 9.2 filter types, 9.4 Paeth) -- not from the code
under test: nothing here imports cmdiad_amd.

`write(path, array, filters=..., split=...)` exists because Pillow's encoder, for the inputs tried, never emits the Average filter: the
test files must force each type.  It filters the rows itself, calls zlib.compress and assembles the chunks with their CRCs.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOR_TYPE_OF_CHANNELS = {1: 0, 2: 4, 3: 2, 4: 6}
CHANNELS_OF_COLOR_TYPE = {0: 1, 4: 2, 2: 3, 6: 4}


def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def filter_rows(pixels, bpp, filters):
    """pixels [H, row_bytes] uint8, one filter type per row -> the scanlines [H, 1 + row_bytes] a PNG encoder would deflate."""
    H, rb = pixels.shape
    out = np.zeros((H, 1 + rb), dtype=np.uint8)
    px = pixels.astype(np.int64)
    for r in range(H):
        ft = int(filters[r])
        cur = px[r]
        up = px[r - 1] if r else np.zeros(rb, np.int64)
        left, upleft = np.zeros(rb, np.int64), np.zeros(rb, np.int64)
        left[bpp:], upleft[bpp:] = cur[:rb - bpp] if rb > bpp else [], up[:rb - bpp] if rb > bpp else []
        if ft == 0:
            pred = np.zeros(rb, np.int64)
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        elif ft == 4:
            pa, pb, pc = np.abs(up - upleft), np.abs(left - upleft), np.abs(left + up - 2 * upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        else:
            pred = np.zeros(rb, np.int64)           # (a bad type, written on purpose: the bytes go in as they are)
        out[r, 0] = ft
        out[r, 1:] = ((cur - pred) & 0xff).astype(np.uint8)
    return out


def encode(array, filters=0, split=None, color_type=None, bit_depth=8, interlace=0, extra=(), scanlines=None, level=6):
    """array uint8 [H,W] or [H,W,C] -> the bytes of a PNG.  filters: one type for every row, or one per row.  split: byte counts of
    the IDAT chunks the zlib stream is cut into (the rest goes into a last one; 0 gives an empty chunk).  extra: chunks (kind, body)
    between IHDR and the first IDAT.  scanlines: the bytes to deflate in place of the filtered rows (tests of malformed streams)."""
    a = np.asarray(array, dtype=np.uint8)
    a3 = a[:, :, None] if a.ndim == 2 else a
    H, W, C = a3.shape
    ctype = COLOR_TYPE_OF_CHANNELS[C] if color_type is None else color_type
    f = np.full(H, filters, dtype=np.int64) if np.isscalar(filters) else np.asarray(filters, dtype=np.int64)
    assert f.shape == (H,)
    lines = filter_rows(a3.reshape(H, W * C), C, f) if scanlines is None else np.asarray(scanlines, dtype=np.uint8)
    stream = zlib.compress(lines.tobytes(), level)
    parts, at = [], 0
    for n in (split or ()):
        parts.append(stream[at:at + n])
        at += n
    parts.append(stream[at:])
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, ctype, 0, 0, interlace))
    for kind, body in extra:
        out += chunk(kind, body)
    for p in parts:
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND")


ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))     # x0, y0, x step, y step


def adam7_scanlines(array):
    """The scanlines of an INTERLACED 8-bit file (interlace method 1): the seven reduced images one after the other, every row with
    filter type 0; an empty pass has no rows."""
    a = np.asarray(array, dtype=np.uint8)
    a3 = a[:, :, None] if a.ndim == 2 else a
    out = b""
    for x0, y0, dx, dy in ADAM7:
        sub = a3[y0::dy, x0::dx]
        if sub.size:
            out += b"".join(b"\0" + row.tobytes() for row in sub)
    return np.frombuffer(out, dtype=np.uint8)


def write(path, array, **kw):
    data = encode(array, **kw)
    with open(path, "wb") as fh:
        fh.write(data)
    return data


# ------------------------------------------------------------------------------------------------ the restatement
def unfilter(scanlines, H, row_bytes, bpp):
    """The inflated scanlines (filter byte + row_bytes per row) -> the image's bytes [H, row_bytes]: Recon(x) = Filt(x) + predictor of
    the already reconstructed a (left), b (above), c (above left), mod 256; bytes outside the image are 0."""
    lines = np.asarray(scanlines, dtype=np.uint8).reshape(H, 1 + row_bytes)
    out = np.zeros((H, row_bytes), dtype=np.uint8)
    for r in range(H):
        ft = int(lines[r, 0])
        xs = lines[r, 1:].tolist()
        ups = out[r - 1].tolist() if r else [0] * row_bytes
        cur = [0] * row_bytes
        for i in range(row_bytes):
            a = cur[i - bpp] if i >= bpp else 0
            b = ups[i]
            c = ups[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]
            cur[i] = (xs[i] + pred) & 0xff
        out[r] = cur
    return out


def to_target(pixels, W, channels, target):
    """The image's bytes [H, W * channels] -> what Pillow gives: 'rgb' = .convert('RGB'), 'l' = .convert('L') (ITU-R 601-2 luma in
    16.16 fixed point, rounded), 'raw' = np.array(Image.open(p))."""
    H = pixels.shape[0]
    px = pixels.reshape(H, W, channels)
    grey = channels <= 2
    if target == "raw":
        return px[:, :, 0].copy() if channels == 1 else px.copy()
    if target == "rgb":
        return np.repeat(px[:, :, :1], 3, axis=2) if grey else px[:, :, :3].copy()
    assert target == "l"
    if grey:
        return px[:, :, 0].copy()
    v = px.astype(np.uint32)
    return ((v[:, :, 0] * 19595 + v[:, :, 1] * 38470 + v[:, :, 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def pillow(path, target):
    """What the callers did before: the array of `target` through Pillow."""
    from PIL import Image
    img = Image.open(path)
    if target == "rgb":
        img = img.convert("RGB")
    elif target == "l":
        img = img.convert("L")
    return np.array(img)


def image(H, W, channels, seed, smooth=False):
    """A uint8 test image [H,W] (one channel) or [H,W,C]: random bytes, or (smooth) a gradient with noise, which gives the filters
    something to predict."""
    rs = np.random.RandomState(seed)
    if smooth:
        y, x = np.mgrid[0:H, 0:W]
        base = (3 * x + 2 * y)[:, :, None] + 40 * np.arange(channels)[None, None, :]
        a = (base + rs.randint(0, 9, (H, W, channels))).astype(np.int64) & 0xff
    else:
        a = rs.randint(0, 256, (H, W, channels))
    a = a.astype(np.uint8)
    return a[:, :, 0] if channels == 1 else a
