"""The numpy yardstick of the overlay render contract and of the PNG filter contract (docs/overlay.md), written from the contract's
text -- per-pixel Python loops, and the same steps on whole planes for the larger shapes -- not from the kernels: nothing here imports cmdiad_amd.

render(maps, Ho, Wo, lo, hi, lut, alpha, ...) -> (canvas uint8 [n,Ho,Wo,3], NaN count); every floating-point step is one numpy
float64 operation in the written order.  filter_image(image, mode) -> scanlines [H, 1 + W * C]; unfilter(...) is its inverse.
"""
import math

import numpy as np

F = np.float64


# ------------------------------------------------------------------------------------------------ render
def axis(c, size, out):
    """canvas coordinate c -> (i0, i1, f): u = (c + 0.5) * (size / out) - 0.5 clamped to [0, size - 1]."""
    u = (F(c) + F(0.5)) * (F(size) / F(out))
    u = u - F(0.5)
    u = min(max(u, F(0.0)), F(size - 1))
    i0 = int(math.floor(u))
    return i0, min(i0 + 1, size - 1), F(u) - F(i0)


def score(m, x, y, Ho, Wo):
    """The bilinear sample of map m [H,W] at canvas pixel (x, y); a tap of weight exactly 0 is not read and contributes nothing."""
    H, W = m.shape
    x0, x1, fx = axis(x, W, Wo)
    y0, y1, fy = axis(y, H, Ho)

    def row(r):
        v = F(m[r, x0]) * (F(1.0) - fx)
        if fx != 0:
            v = v + F(m[r, x1]) * fx
        return v
    with np.errstate(all="ignore"):
        s = row(y0) * (F(1.0) - fy)
        if fy != 0:
            s = s + row(y1) * fy
    return F(s)


def score_plane_loops(m, Ho, Wo):
    return np.array([[score(m, x, y, Ho, Wo) for x in range(Wo)] for y in range(Ho)], dtype=F).reshape(Ho, Wo)


def _axis_arrays(size, out):
    u = (np.arange(out, dtype=F) + F(0.5)) * (F(size) / F(out))
    u = u - F(0.5)
    u = np.minimum(np.maximum(u, F(0.0)), F(size - 1))
    fl = np.floor(u)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), u - fl


def score_plane(m, Ho, Wo):
    """The same sample for a whole canvas at once: the same float64 operations, element by element (numpy rounds each once); the
    zero-weight taps are computed and then dropped by np.where, which is what 'not read' amounts to."""
    m = np.asarray(m, dtype=F)
    H, W = m.shape
    x0, x1, fx = _axis_arrays(W, Wo)
    y0, y1, fy = _axis_arrays(H, Ho)
    fx, fy = fx[None, :], fy[:, None]
    with np.errstate(all="ignore"):
        def rows(r):
            a = m[r][:, x0] * (F(1.0) - fx)
            return np.where(fx != 0, a + m[r][:, x1] * fx, a)
        top = rows(y0) * (F(1.0) - fy)
        return np.where(fy != 0, top + rows(y1) * fy, top)


def index_of(s, lo, hi):
    """score -> (k, is NaN)"""
    s, lo, hi = F(s), F(lo), F(hi)
    if np.isnan(s):
        return 0, True
    with np.errstate(all="ignore"):
        d = hi - lo
        if d > 0:
            t = (s - lo) / d
        else:
            t = F(1.0) if s > lo else F(0.0)
    if not t > 0:
        t = F(0.0)
    if t > 1:
        t = F(1.0)
    return int(math.floor(t * F(255.0) + F(0.5))), False


def bg_byte(v, mean, std):
    """float32 normalised background value -> byte, in float64 from the widened float"""
    with np.errstate(all="ignore"):
        b = F(np.float32(v)) * F(std)
        b = b + F(mean)
        b = b * F(255.0)
        b = np.floor(b + F(0.5))
    if not b > 0:
        return 0
    return 255 if b > 255 else int(b)


def canvas_box(box, H, W, Ho, Wo):
    """map box (x0, y0, x1, y1) inclusive -> canvas box, clamped to the canvas"""
    x0, y0, x1, y1 = (int(v) for v in box)
    X0, X1 = x0 * Wo // W, ((x1 + 1) * Wo + W - 1) // W - 1
    Y0, Y1 = y0 * Ho // H, ((y1 + 1) * Ho + H - 1) // H - 1
    return max(X0, 0), max(Y0, 0), min(X1, Wo - 1), min(Y1, Ho - 1)


def render_loops(maps, Ho, Wo, lo, hi, lut, alpha, bg=None, bg_kind=0, mean=(0, 0, 0), std=(1, 1, 1), thr=None, contour_rgb=(255, 255, 255),
           count=None, ints=None, box_rgb=(0, 255, 0), line_px=1):
    """maps [n,H,W] float64; lo, hi, thr: scalars or one per image; lut [256,3], alpha [256] uint8; bg: kind 1 uint8 [n,Ho,Wo,3], kind 2
    float32 [n,3,Ho,Wo]; count [n], ints [n,K,8] the region tables -> (canvas uint8 [n,Ho,Wo,3], number of NaN scores)."""
    maps = np.asarray(maps, dtype=F)
    n, H, W = maps.shape
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=F).reshape(-1), (n,)), np.broadcast_to(np.asarray(hi, dtype=F).reshape(-1), (n,))
    thr_n = None if thr is None else np.broadcast_to(np.asarray(thr, dtype=F).reshape(-1), (n,))
    out = np.zeros((n, Ho, Wo, 3), dtype=np.uint8)
    nan = 0
    for i in range(n):
        S = score_plane_loops(maps[i], Ho, Wo)
        boxes = []
        if count is not None:
            K = ints.shape[1]
            boxes = [canvas_box(ints[i, j, 2:6], H, W, Ho, Wo) for j in range(min(int(count[i]), K))]
        with np.errstate(invalid="ignore"):
            above = S > thr_n[i] if thr_n is not None else None
        for y in range(Ho):
            for x in range(Wo):
                k, bad = index_of(S[y, x], lo[i], hi[i])
                nan += bad
                c = [int(v) for v in lut[k]]
                if bg_kind:
                    a = int(alpha[k])
                    if bg_kind == 1:
                        g = [int(v) for v in bg[i, y, x]]
                    else:
                        g = [bg_byte(bg[i, ch, y, x], mean[ch], std[ch]) for ch in range(3)]
                    c = [(c[ch] * a + g[ch] * (255 - a) + 127) // 255 for ch in range(3)]
                if above is not None and above[y, x]:
                    nb = [(x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)]
                    if any(0 <= xx < Wo and 0 <= yy < Ho and not above[yy, xx] for xx, yy in nb):
                        c = list(contour_rgb)
                for X0, Y0, X1, Y1 in boxes:
                    if X0 <= x <= X1 and Y0 <= y <= Y1 and min(x - X0, X1 - x, y - Y0, Y1 - y) < line_px:
                        c = list(box_rgb)
                out[i, y, x] = c
    return out, nan


def render(maps, Ho, Wo, lo, hi, lut, alpha, bg=None, bg_kind=0, mean=(0, 0, 0), std=(1, 1, 1), thr=None, contour_rgb=(255, 255, 255),
           count=None, ints=None, box_rgb=(0, 255, 0), line_px=1):
    """render_loops on whole planes: the same operations element by element (tests/test_overlay_cpu.py holds the two to each
    other); this is the one the production shapes are checked against."""
    maps = np.asarray(maps, dtype=F)
    n, H, W = maps.shape
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=F).reshape(-1), (n,)), np.broadcast_to(np.asarray(hi, dtype=F).reshape(-1), (n,))
    thr_n = None if thr is None else np.broadcast_to(np.asarray(thr, dtype=F).reshape(-1), (n,))
    lut, alpha = np.asarray(lut, dtype=np.int64), np.asarray(alpha, dtype=np.int64)
    out = np.zeros((n, Ho, Wo, 3), dtype=np.uint8)
    nan = 0
    yy, xx = np.mgrid[0:Ho, 0:Wo]
    for i in range(n):
        S = score_plane(maps[i], Ho, Wo)
        bad = np.isnan(S)
        nan += int(bad.sum())
        with np.errstate(all="ignore"):
            d = hi[i] - lo[i]
            t = (S - lo[i]) / d if d > 0 else np.where(S > lo[i], F(1.0), F(0.0))
            t = np.where(t > 0, t, F(0.0))          # (a NaN t, and every t of a NaN score, is 0)
            t = np.where(t > 1, F(1.0), t)
            t = np.where(bad, F(0.0), t)
            k = np.floor(t * F(255.0) + F(0.5)).astype(np.int64)
        c = lut[k]
        if bg_kind:
            a = alpha[k][:, :, None]
            if bg_kind == 1:
                g = np.asarray(bg[i], dtype=np.int64)
            else:
                with np.errstate(all="ignore"):
                    v = np.asarray(bg[i], dtype=np.float32).astype(F).transpose(1, 2, 0)
                    b = v * np.asarray(std, dtype=F)
                    b = b + np.asarray(mean, dtype=F)
                    b = b * F(255.0)
                    b = np.floor(b + F(0.5))
                    b = np.where(b > 0, b, F(0.0))
                    b = np.where(b > 255, F(255.0), b)
                g = b.astype(np.int64)
            c = (c * a + g * (255 - a) + 127) // 255
        c = c.copy()
        if thr_n is not None:
            with np.errstate(invalid="ignore"):
                above = S > thr_n[i]
            below = ~above
            edge = np.zeros_like(above)
            edge[:, 1:] |= below[:, :-1]
            edge[:, :-1] |= below[:, 1:]
            edge[1:] |= below[:-1]
            edge[:-1] |= below[1:]
            c[above & edge] = contour_rgb
        if count is not None:
            for j in range(min(int(count[i]), ints.shape[1])):
                X0, Y0, X1, Y1 = canvas_box(ints[i, j, 2:6], H, W, Ho, Wo)
                inside = (xx >= X0) & (xx <= X1) & (yy >= Y0) & (yy <= Y1)
                near = np.minimum(np.minimum(xx - X0, X1 - xx), np.minimum(yy - Y0, Y1 - yy)) < line_px
                c[inside & near] = box_rgb
        out[i] = c
    return out, nan


# ------------------------------------------------------------------------------------------------ filter
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def candidates(image):
    """image uint8 [H,W,C] -> the five filtered versions of every row, int64 [5, H, W*C].  The sources are the unfiltered image: a =
    the byte one pixel to the left, b = the byte above, c = above left, zero outside the image."""
    a3 = np.asarray(image, dtype=np.uint8)
    H, W, C = a3.shape
    rb = W * C
    x = a3.reshape(H, rb).astype(np.int64)
    a, b, c = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    a[:, C:] = x[:, :rb - C]
    b[1:] = x[:-1]
    c[1:, C:] = x[:-1, :rb - C]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, (x - a) & 0xff, (x - b) & 0xff, (x - ((a + b) >> 1)) & 0xff, (x - paeth) & 0xff])


def row_costs(cand):
    """[5, H, rb] -> [5, H]: the sum over a row of m(v) = v < 128 ? v : 256 - v"""
    return np.where(cand < 128, cand, 256 - cand).sum(axis=2)


def row_types(image, mode):
    """the filter type of every row: mode 0..4 everywhere, or (mode 5) the lowest type among the smallest costs"""
    H = np.asarray(image).shape[0]
    return np.full(H, mode, dtype=np.int64) if mode != 5 else np.argmin(row_costs(candidates(image)), axis=0)


def filter_image(image, mode):
    """image uint8 [H,W,C] -> scanlines uint8 [H, 1 + W*C].  mode 0..4: that type on every row; 5: per row the type with the smallest
    sum of m(b) = b < 128 ? b : 256 - b, ties to the lowest type (np.argmin returns the first minimum)."""
    cand = candidates(image)
    H, rb = cand.shape[1:]
    ft = row_types(image, mode)
    out = np.zeros((H, 1 + rb), dtype=np.uint8)
    out[:, 0] = ft
    out[:, 1:] = cand[ft, np.arange(H)]
    return out


def unfilter(scanlines, H, W, C):
    """the inverse: scanlines [H, 1 + W*C] -> image [H,W,C]"""
    rb = W * C
    lines = np.asarray(scanlines, dtype=np.uint8).reshape(H, 1 + rb)
    out = np.zeros((H, rb), dtype=np.uint8)
    for r in range(H):
        ft = int(lines[r, 0])
        xs = lines[r, 1:].tolist()
        ups = out[r - 1].tolist() if r else [0] * rb
        cur = [0] * rb
        for i in range(rb):
            a = cur[i - C] if i >= C else 0
            b = ups[i]
            c = ups[i - C] if i >= C else 0
            cur[i] = (xs[i] + (0, a, b, (a + b) >> 1, _paeth(a, b, c))[ft]) & 0xff
        out[r] = cur
    return out.reshape(H, W, C)
