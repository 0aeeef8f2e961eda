"""A small TIFF GENERATOR for the tests of cmdiad_amd/utils/tiff.py and csrc/tiff.hip, written from the TIFF 6.0 layout (header, one
IFD of 12-byte entries, strips or tiles) and from libtiff's description of predictor 3 -- not from the code under test: nothing here
imports cmdiad_amd.  `write(path, array, ...)` covers byte order, strips / tiles, chunky / planar, float32 / float64, any channel count,
none / deflate, predictor 1 / 3 and the alignment of the chunk offsets (offset mod 4).

`random_bits(shape, dtype, seed)` gives arrays of random bits viewed as floats, with NaN payloads, +-0, denormals and +-inf planted."""
import struct
import zlib

import numpy as np


def random_bits(shape, dtype=np.float32, seed=0):
    dtype = np.dtype(dtype)
    uint = np.dtype(f"u{dtype.itemsize}")
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 256, size=tuple(shape) + (dtype.itemsize,), dtype=np.uint8).view(uint).reshape(shape).copy()
    flat = bits.reshape(-1)
    if dtype.itemsize == 4:
        special = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFA5A5A5, 0x7F800001]
    else:
        special = [0x0, 0x8000000000000000, 0x1, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000001,
                   0xFFF5A5A5A5A5A5A5, 0x7FF0000000000001]
    for k, v in enumerate(special):
        flat[(k * 7 + 3) % flat.size] = v
    return bits.view(dtype)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.dtype(f"u{a.dtype.itemsize}"))


def _predict3(rows, stride, bps):
    """rows: uint8 [n, wc, bps], every sample's bytes MOST SIGNIFICANT FIRST -> uint8 [n, wc * bps] as predictor 3 stores them: byte k of
    all samples in plane k, then every byte minus the byte `stride` positions before it (mod 256), from the end of the row."""
    n, wc, _ = rows.shape
    planes = rows.transpose(0, 2, 1).reshape(n, bps * wc).astype(np.int16)
    out = planes.copy()
    out[:, stride:] = planes[:, stride:] - planes[:, :-stride]
    return (out & 0xFF).astype(np.uint8)


def write(path, array, big_endian=False, rows_per_strip=None, tile=None, planar=False, deflate=False, predictor=1, misalign=0,
          compression_tag=8, tail=b""):
    """array [H,W] or [H,W,C] float32 / float64.  tile = (tw, th) or None (strips of rows_per_strip rows, default: one strip).  The
    first chunk's offset is congruent to `misalign` mod 4 and a 3-byte gap between chunks rotates the others through the residues.
    `tail` is appended after the last chunk.  Returns the list of chunk offsets."""
    a = np.asarray(array)
    h, w = a.shape[:2]
    c = a.shape[2] if a.ndim == 3 else 1
    a = a.reshape(h, w, c)
    bps = a.dtype.itemsize
    e = ">" if big_endian else "<"
    msb_first = np.ascontiguousarray(bits_of(a).astype(np.dtype(f">u{bps}"))).view(np.uint8).reshape(h, w, c, bps)
    file_order = msb_first if big_endian else msb_first[..., ::-1]
    tw, th = tile if tile else (w, rows_per_strip or h)
    planes = [[p] for p in range(c)] if (planar and c > 1) else [list(range(c))]
    chunks = []
    for chans in planes:
        for y0 in range(0, h, th):
            for x0 in range(0, w, tw):
                rows = th if tile else min(th, h - y0)          # tiles are stored whole, the last strip is short
                src = msb_first if predictor == 3 else file_order
                block = np.zeros((rows, tw, len(chans), bps), np.uint8)
                part = src[y0:y0 + rows, x0:x0 + tw][:, :, chans]
                block[:part.shape[0], :part.shape[1]] = part
                if predictor == 3:
                    data = _predict3(block.reshape(rows, tw * len(chans), bps), len(chans), bps).tobytes()
                else:
                    data = block.tobytes()
                chunks.append(zlib.compress(data, 6) if deflate else data)
    spp_multi = c > 1
    entries = [(256, "I", [w]), (257, "I", [h]), (258, "H", [8 * bps] * c), (259, "H", [compression_tag if deflate else 1]),
               (262, "H", [2 if c == 3 else 1]), (277, "H", [c]), (284, "H", [2 if (planar and spp_multi) else 1]), (339, "H", [3] * c)]
    if predictor != 1:
        entries.append((317, "H", [predictor]))
    if c not in (1, 3):
        entries.append((338, "H", [0] * (c - 1)))
    n = len(chunks)
    if tile:
        entries += [(322, "I", [tw]), (323, "I", [th]), (324, "I", [0] * n), (325, "I", [len(x) for x in chunks])]
    else:
        entries += [(278, "I", [th]), (273, "I", [0] * n), (279, "I", [len(x) for x in chunks])]
    entries.sort(key=lambda t: t[0])
    codes = {"H": (3, 2), "I": (4, 4)}
    pos = 8 + 2 + 12 * len(entries) + 4
    where = {}
    for tag, code, vals in entries:
        size = codes[code][1] * len(vals)
        if size > 4:
            where[tag] = pos
            pos += size + (size & 1)
    pos += (misalign - pos) % 4
    offsets = []
    for x in chunks:
        offsets.append(pos)
        pos += len(x) + 3
    out = bytearray(pos - 3)
    out[0:8] = struct.pack(e + "2sHI", b"MM" if big_endian else b"II", 42, 8)
    struct.pack_into(e + "H", out, 8, len(entries))
    for k, (tag, code, vals) in enumerate(entries):
        if tag in (273, 324):
            vals = offsets
        at = 10 + 12 * k
        struct.pack_into(e + "HHI", out, at, tag, codes[code][0], len(vals))
        struct.pack_into(e + f"{len(vals)}{code}", out, where.get(tag, at + 8), *vals)
        if tag in where:
            struct.pack_into(e + "I", out, at + 8, where[tag])
    for off, x in zip(offsets, chunks):
        out[off:off + len(x)] = x
    with open(path, "wb") as fh:
        fh.write(bytes(out) + tail)
    return offsets


def variants(channels):
    """The cross product of the generator's knobs as keyword dicts for `write`: byte order x (one strip, 5-row strips, 16 x 16 tiles) x
    (chunky, planar when C > 1) x (none, deflate) x predictor (1, 3); the offset residue mod 4 walks through 0..3 along the list."""
    out, k = [], 0
    for big in (False, True):
        for chunking in (dict(), dict(rows_per_strip=5), dict(tile=(16, 16))):
            for planar in ((False, True) if channels > 1 else (False,)):
                for deflate in (False, True):
                    for predictor in (1, 3):
                        out.append(dict(big_endian=big, planar=planar, deflate=deflate, predictor=predictor, misalign=k % 4, **chunking))
                        k += 1
    return out


def variant_id(kw):
    return "-".join(f"{k}={v}" for k, v in sorted(kw.items()))
