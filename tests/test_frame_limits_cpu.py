"""The limits of a batch of frames are stated twice: cmdiad_amd/csrc/frames.h (kMaxImages, kMaxImagePixels, kMaxTotal, kMaxSide;
mesh.hip's kMeshMaxTotal) and cmdiad_amd/ops.py (FRAME_MAX_*, MESH_MAX_TOTAL; ops._frames is the one check).  This file holds the
two together without a GPU: an entry point that validates its sizes before its pointers answers a call with every pointer NULL by
"bad sizes" (the shape was refused) or by "null pointer" (the shape was accepted), and neither answer reaches the device.  Every
entry point used here has been read for that order: sizes, then pointers, then the first HIP call."""
import math

import pytest

from cmdiad_amd import _native as nat
from cmdiad_amd import ops

# (the limit, the last accepted (n, H, W), the first refused one)
FRAME_PAIRS = [("images", (65535, 1, 1), (65536, 1, 1)),
               ("pixels per image", (1, 4096, 4096), (1, 4096, 4097)),
               ("total", (64, 4096, 4096), (65, 4096, 4096))]
SIDE_PAIR = ((1, 16384, 1), (1, 16385, 1))
MESH_PAIR = ((1, 4096, 4096), (1, 4096, 4097))          # n*H*W <= 2^24; both sides are inside the side limit


def _threshold_mask(n, H, W):
    return nat.lib().cmdiad_threshold_mask(None, None, 0, n, H, W, None, None, None)


def _ccl_label(n, H, W):
    return nat.lib().cmdiad_ccl_label(None, 1, n, H, W, None, None, None, None, 0, None, None, 0, None)


def _region_measure(n, H, W):
    return nat.lib().cmdiad_region_measure(None, None, None, None, 1, H * W, n, H, W, 1, None, None, None, None)     # planar strides


def _organize_splat(n, H, W):
    return nat.lib().cmdiad_organize_splat(None, None, None, n, 0, 0, 0, H, W, None, None, None, None)


def _mesh_count(n, H, W):
    return nat.lib().cmdiad_mesh_count(None, 1, H * W, None, n, H, W, math.inf, None, None, None)


def _png_filter(n, H, W):
    return nat.lib().cmdiad_png_filter(None, n, H, W, 1, 5, None, None)


def _overlay_render(n, H, W):
    return nat.lib().cmdiad_overlay_render(None, n, H, W, H, W, None, 0, None, 0, None, 0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None, None, None, None,
                                           1, 1, 0, 0, None, None, None)


def c_accepts(call, shape):
    """True: the sizes passed and the NULL pointers were refused; False: the sizes were refused.  Anything else is a failure."""
    rc = call(*shape)
    msg = nat.lib().cmdiad_last_error().decode()
    assert rc < 0, (call.__name__, shape, rc)
    if "null pointer" in msg:
        return True
    assert "bad sizes" in msg or "bad grid" in msg, (call.__name__, shape, msg)
    return False


def py_accepts(shape, **limits):
    try:
        return ops._frames(shape, "test", **limits) == shape
    except ValueError:
        return False


def test_python_states_the_limits_once():
    assert (ops.FRAME_MAX_IMAGES, ops.FRAME_MAX_PIXELS, ops.FRAME_MAX_TOTAL, ops.FRAME_MAX_SIDE) == (65535, 1 << 24, 1 << 30, 1 << 14)
    assert ops.MESH_MAX_TOTAL == 1 << 24
    assert ops.METRICS_MAX_TOTAL == ops.ORGANIZE_MAX_TOTAL == ops.FRAME_MAX_TOTAL
    assert (ops.ORGANIZE_MAX_IMAGES, ops.ORGANIZE_MAX_PIXELS, ops.OVERLAY_MAX_SIDE) == (ops.FRAME_MAX_IMAGES, ops.FRAME_MAX_PIXELS,
                                                                                       ops.FRAME_MAX_SIDE)


@pytest.mark.parametrize("limit,accepted,refused", FRAME_PAIRS, ids=[p[0] for p in FRAME_PAIRS])
@pytest.mark.parametrize("call", [_threshold_mask, _ccl_label, _region_measure, _organize_splat], ids=lambda f: f.__name__.lstrip("_"))
def test_frame_limits_agree(call, limit, accepted, refused):
    assert c_accepts(call, accepted) and not c_accepts(call, refused), limit
    assert py_accepts(accepted) and not py_accepts(refused), limit


def test_mesh_total_agrees():
    accepted, refused = MESH_PAIR
    limits = dict(side=ops.FRAME_MAX_SIDE, total=ops.MESH_MAX_TOTAL)
    assert c_accepts(_mesh_count, accepted) and not c_accepts(_mesh_count, refused)
    assert py_accepts(accepted, **limits) and not py_accepts(refused, **limits)
    assert c_accepts(_mesh_count, (16, 1024, 1024)) and not c_accepts(_mesh_count, (17, 1024, 1024))       # a total, not a frame
    assert py_accepts((16, 1024, 1024), **limits) and not py_accepts((17, 1024, 1024), **limits)


@pytest.mark.parametrize("call", [_png_filter, _overlay_render], ids=lambda f: f.__name__.lstrip("_"))
def test_side_limit_agrees(call):
    accepted, refused = SIDE_PAIR
    for shape in (accepted, refused, accepted[:1] + accepted[:0:-1], refused[:1] + refused[:0:-1]):      # the long side as H and as W
        assert c_accepts(call, shape) == (max(shape) <= 16384), shape
        assert py_accepts(shape, side=ops.FRAME_MAX_SIDE) == (max(shape) <= 16384), shape
