"""CPU (no GPU): the yardstick of the overlay contract (tests/overlay_ref.py) checked against itself, the colour and alpha tables,
the PNG writer (utils/png.py: encode) read back through Pillow and through png.read_raw + the yardstick's inverse, and the argument
validation of cmdiad_overlay_render / cmdiad_png_filter, which happens before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlay_ref as R  # noqa: E402
import png_ref  # noqa: E402

from cmdiad_amd import overlay  # noqa: E402
from cmdiad_amd.utils import png  # noqa: E402

GREY = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)          # lut[k] = (k, k, k): the canvas shows k itself
OPAQUE = np.full(256, 255, np.uint8)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_identity_canvas_is_the_maps_own_index_plane():
    rs = np.random.RandomState(0)
    m = rs.rand(2, 5, 7) * 3 - 1
    m[0, 0, 0], m[0, 1, 1], m[1, 4, 6], m[1, 2, 2] = np.inf, -np.inf, -0.0, np.nan
    for i in range(2):
        assert R.score_plane(m[i], 5, 7).tobytes() == m[i].tobytes()             # bit for bit, infinities and the NaN included
        assert R.score_plane_loops(m[i], 5, 7).tobytes() == m[i].tobytes()
    got, nan = R.render(m, 5, 7, 0.25, 1.5, GREY, OPAQUE)
    want = np.array([[[R.index_of(v, 0.25, 1.5)[0] for v in row] for row in img] for img in m])
    assert np.array_equal(got[..., 0], want) and nan == 1
    assert got[0, 0, 0, 0] == 255 and got[0, 1, 1, 0] == 0 and got[1, 2, 2, 0] == 0
    for t, k in ((0.0, 0), (1.0, 255), (0.5, 128), (0.25, 64), (-3.0, 0), (7.0, 255)):      # 0.5 * 255 + 0.5 = 128 exactly: rounds up
        assert R.index_of(t, 0.0, 1.0) == (k, False)
    assert R.index_of(0.3, 1.0, 1.0) == (0, False) and R.index_of(1.5, 1.0, 1.0) == (255, False)      # hi == lo: a step at lo
    assert R.index_of(1.0, 1.0, 1.0) == (0, False) and R.index_of(2.0, 3.0, 1.0) == (0, False) and R.index_of(4.0, 3.0, 1.0) == (255, False)


def test_constant_map_gives_a_constant_canvas():
    for (H, W), (Ho, Wo) in (((1, 1), (1, 1)), ((1, 9), (4, 3)), ((7, 5), (16, 11)), ((9, 9), (4, 4))):
        got, nan = R.render(np.full((1, H, W), 0.7), Ho, Wo, 0.0, 1.0, GREY, OPAQUE)
        assert nan == 0 and (got == R.index_of(0.7, 0.0, 1.0)[0]).all(), (H, W, Ho, Wo)


def test_loops_and_planes_agree():
    rs = np.random.RandomState(1)
    lut, alpha = rs.randint(0, 256, (256, 3)).astype(np.uint8), rs.randint(0, 256, 256).astype(np.uint8)
    seen = 0
    for (H, W), (Ho, Wo) in (((1, 1), (1, 1)), ((1, 9), (4, 3)), ((5, 7), (5, 7)), ((7, 5), (16, 11)), ((9, 9), (4, 4))):
        m = rs.rand(2, H, W)
        m[0, 0, 0], m[1, H - 1, W - 1] = np.nan, np.inf
        count = np.array([2, 3], np.int32)
        ints = np.zeros((2, 2, 8), np.int32)
        ints[0, 0, 2:6], ints[0, 1, 2:6], ints[1, 0, 2:6], ints[1, 1, 2:6] = (0, 0, W - 1, H - 1), (W // 2, H // 2, W // 2, H // 2), (0, 0, 0, 0), (W - 1, 0, W - 1, H - 1)
        for kind, bg in ((0, None), (1, rs.randint(0, 256, (2, Ho, Wo, 3)).astype(np.uint8)), (2, (rs.randn(2, 3, Ho, Wo) * 2).astype(np.float32))):
            kw = dict(bg=bg, bg_kind=kind, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), thr=[0.4, 0.6], count=count, ints=ints,
                      line_px=2)
            a, b = R.render_loops(m, Ho, Wo, [0.1, 0.5], [0.9, 0.5], lut, alpha, **kw), R.render(m, Ho, Wo, [0.1, 0.5], [0.9, 0.5], lut, alpha, **kw)
            assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
            seen += a[1]
    assert seen >= 5          # (1 x 9 -> 4 x 3 never samples column 0: its NaN is not met)


def test_boxes_are_clamped_and_blend_endpoints():
    assert R.canvas_box((0, 0, 6, 4), 5, 7, 5, 7) == (0, 0, 6, 4)
    assert R.canvas_box((5, 3, 9, 9), 5, 7, 5, 7) == (5, 3, 6, 4)                  # a box that leaves the map is cut at the canvas
    assert R.canvas_box((2, 1, 2, 1), 5, 7, 10, 14) == (4, 2, 5, 3) and R.canvas_box((3, 3, 5, 5), 9, 9, 4, 4) == (1, 1, 2, 2)
    m = np.zeros((1, 5, 7))
    ints = np.zeros((1, 1, 8), np.int32)
    ints[0, 0, 2:6] = (5, 3, 9, 9)
    got, _ = R.render(m, 5, 7, 0.0, 1.0, GREY, OPAQUE, count=np.array([1]), ints=ints, box_rgb=(1, 2, 3))
    drawn = (got == (1, 2, 3)).all(axis=-1)[0]
    assert drawn[3:, 5:].all() and drawn.sum() == 4
    rs = np.random.RandomState(2)
    bg = rs.randint(0, 256, (1, 5, 7, 3)).astype(np.uint8)
    lut = rs.randint(0, 256, (256, 3)).astype(np.uint8)
    m = rs.rand(1, 5, 7)
    plain, _ = R.render(m, 5, 7, 0.0, 1.0, lut, OPAQUE)
    assert np.array_equal(R.render(m, 5, 7, 0.0, 1.0, lut, np.zeros(256, np.uint8), bg=bg, bg_kind=1)[0], bg)       # a = 0: the background
    assert np.array_equal(R.render(m, 5, 7, 0.0, 1.0, lut, OPAQUE, bg=bg, bg_kind=1)[0], plain)                      # a = 255: the table
    assert R.bg_byte(0.0, 0.5, 0.2) == 128 and R.bg_byte(-100.0, 0.5, 0.2) == 0 and R.bg_byte(100.0, 0.5, 0.2) == 255
    assert R.bg_byte(np.nan, 0.5, 0.2) == 0


def test_filter_yardstick_inverts_and_every_type_can_win():
    img = winners_image(64, 3)
    types = R.row_types(img, 5)
    assert set(types.tolist()) == {0, 1, 2, 3, 4}, types
    for mode in range(6):
        lines = R.filter_image(img, mode)
        assert np.array_equal(R.unfilter(lines, *img.shape), img)
        if mode < 5:
            assert np.array_equal(lines, png_ref.filter_rows(img.reshape(img.shape[0], -1), 3, [mode] * img.shape[0]))
    assert (R.row_types(np.zeros((4, 5, 3), np.uint8), 5) == 0).all()                               # every cost ties: type 0
    const = np.full((4, 5, 1), 200, np.uint8)
    costs = R.row_costs(R.candidates(const))
    assert costs[1, 1] < costs[0, 1] and costs[2, 1] == 0 and R.row_types(const, 5).tolist() == [1, 2, 2, 2]   # Sub keeps byte 0, Up none


def winners_image(W, C, seed=5):
    """[10, W, C]: rows built so that, under the adaptive rule, each of the five filter types wins at least one row
    (test_filter_yardstick_inverts_and_every_type_can_win checks exactly that on the yardstick)."""
    rs = np.random.RandomState(seed)
    x = np.arange(W)[:, None] + np.zeros((1, C), dtype=np.int64)
    rows = []
    rows.append(rs.randint(0, 3, (W, C)))                         # small bytes: None costs least
    rows.append((7 * x + 40) & 0xff)                              # a ramp unlike the row above: Sub
    rows.append(rows[-1].copy())                                  # the row above again: Up
    noise = rs.randint(0, 256, (W, C))
    rows.append(noise)                                            # noise
    avg = np.zeros((W, C), dtype=np.int64)                        # each byte the average of left and above, plus nothing: Average
    for i in range(W):
        left = avg[i - 1] if i else np.zeros(C, dtype=np.int64)
        avg[i] = (left + noise[i]) >> 1
    rows.append(avg)
    a = rs.randint(0, 256, (W, C))
    rows.append(a)
    pae = np.zeros((W, C), dtype=np.int64)                        # each byte the Paeth prediction itself: Paeth
    for i in range(W):
        for ch in range(C):
            left = pae[i - 1, ch] if i else 0
            ul = a[i - 1, ch] if i else 0
            pae[i, ch] = R._paeth(int(left), int(a[i, ch]), int(ul)) if i else a[i, ch]
    rows.append(pae)
    rows += [np.zeros((W, C), dtype=np.int64), rs.randint(0, 256, (W, C)), rs.randint(0, 256, (W, C))]
    return np.stack(rows).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ tables
def test_colour_tables():
    for name, stops in overlay.COLOR_STOPS.items():
        t = overlay.colormap(name)
        assert t.shape == (256, 3) and t.dtype == np.uint8 and t.tobytes() == overlay.colormap(name).tobytes()
        assert tuple(t[0]) == stops[0][1:] and tuple(t[255]) == stops[-1][1:]
        for p, *c in stops:
            assert tuple(t[p]) == tuple(c)
    assert np.array_equal(overlay.colormap("grey"), GREY)
    with pytest.raises(ValueError, match="unknown name"):
        overlay.colormap("viridis")
    a = overlay.alpha_ramp(10, 110, 200)
    assert a.shape == (256,) and a.dtype == np.uint8 and (a[:11] == 0).all() and (a[110:] == 200).all() and a[60] == 100
    assert (np.diff(a.astype(int)) >= 0).all()
    assert (overlay.alpha_ramp(0, 0, 77) == 77).all()
    with pytest.raises(ValueError):
        overlay.alpha_ramp(5, 4, 1)
    cal = type("Cal", (), dict(pixel_threshold=0.25))()
    s = overlay.OverlaySpec.from_calibration(cal, span=2.0)
    assert s.lo.tolist() == [0.0] and s.hi.tolist() == [0.5] and s.pixel_threshold.tolist() == [0.25] and s.line_px == 1
    for bad in (dict(lo=np.nan, hi=1), dict(lo=0, hi=np.inf), dict(lo=0, hi=1, line_px=9), dict(lo=0, hi=1, line_px=0),
                dict(lo=0, hi=1, box_rgb=(0, 0, 256)), dict(lo=0, hi=1, size=(0, 4))):
        with pytest.raises(ValueError):
            overlay.OverlaySpec(**bad)


# ------------------------------------------------------------------------------------------------ the writer
@pytest.mark.parametrize("C", [1, 3, 4])
def test_encode_reads_back_through_pillow_and_read_raw(C, tmp_path):
    from PIL import Image
    img = winners_image(9, C, seed=C)
    H, W = img.shape[:2]
    lay = png.write_layout(W, H, C)
    for mode in range(6):
        lines = R.filter_image(img, mode)
        data = png.encode(lines, lay)
        path = str(tmp_path / f"c{C}m{mode}.png")
        with open(path, "wb") as fh:
            fh.write(data)
        got = png.read_layout(path)
        assert png.supported(got) and got == lay
        pil = np.array(Image.open(path))
        assert np.array_equal(pil.reshape(H, W, C), img), (C, mode)
        raw = png.read_raw(path, "raw")
        assert np.array_equal(raw.data, lines.reshape(-1))                      # the scanlines come back as they went in
        assert np.array_equal(R.unfilter(raw.data, H, W, C), img)
        assert png.read_layout(png.encode(lines, lay, level=1)) == lay
    with pytest.raises(ValueError, match="bytes of scanlines"):
        png.encode(lines.reshape(-1)[:-1], lay)
    with pytest.raises(ValueError):
        png.write_layout(4, 4, 5)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_reject_bad_arguments_before_any_launch():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    assert L.cmdiad_abi_version() == 6
    for name in ("cmdiad_overlay_render", "cmdiad_png_filter"):
        assert name in nat.SIGNATURES and hasattr(L, name)
    one = ctypes.c_void_p(16)             # a non-null pointer that a rejected call never follows

    def render(n=1, H=4, W=4, Ho=4, Wo=4, lohi_per=0, thr_per=0, bg=None, kind=0, K=1, line=1, ptr=one, tables=(None, None)):
        return L.cmdiad_overlay_render(ptr, n, H, W, Ho, Wo, ptr, lohi_per, None, thr_per, bg, kind, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, ptr, ptr,
                                       tables[0], tables[1], K, line, 0, 0, ptr, None, None)
    cases = [dict(H=0), dict(W=0), dict(Ho=0), dict(Wo=0), dict(H=(1 << 14) + 1), dict(Wo=(1 << 14) + 1), dict(n=-1), dict(n=65536),
             dict(n=65535, Ho=1 << 14, Wo=1 << 14)]
    for kw in cases:
        assert render(**kw) == -1 and b"cmdiad_overlay_render: bad sizes" in L.cmdiad_last_error(), kw
    for kw, text in ((dict(kind=3), b"background kind"), (dict(kind=-1), b"background kind"), (dict(K=0), b"K=0"), (dict(K=65), b"K=65"),
                     (dict(line=0), b"line_px=0"), (dict(line=9), b"line_px=9"), (dict(lohi_per=2), b"lohi_per_image=2"),
                     (dict(ptr=None), b"null pointer"), (dict(kind=1, bg=None), b"null pointer"), (dict(kind=2, bg=None), b"null pointer"),
                     (dict(tables=(one, None)), b"null pointer"), (dict(tables=(None, one)), b"null pointer")):
        assert render(**kw) == -1 and text in L.cmdiad_last_error(), (kw, L.cmdiad_last_error())
    assert render(n=0, ptr=None) == 0                                            # nothing to do: no launch

    def filt(n=1, H=4, W=4, C=3, mode=5, ptr=one):
        return L.cmdiad_png_filter(ptr, n, H, W, C, mode, ptr, None)
    for kw in (dict(H=0), dict(W=0), dict(H=(1 << 14) + 1), dict(W=(1 << 14) + 1), dict(C=0), dict(C=5), dict(n=-1)):
        assert filt(**kw) == -1 and b"cmdiad_png_filter: bad sizes" in L.cmdiad_last_error(), kw
    for mode in (-1, 6):
        assert filt(mode=mode) == -1 and b"mode=" in L.cmdiad_last_error()
    assert filt(ptr=None) == -1 and b"null pointer" in L.cmdiad_last_error()
    assert filt(n=0, ptr=None) == 0
