"""csrc/png.hip (cmdiad_png_unfilter) and the CMDIAD_PNG_DEVICE=1 path of the sample sources against Pillow: every comparison is for
EQUAL BYTES.  The files come from the tests' own writer (tests/png_ref.py), which forces the filter type of every row."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eyecandies_ref as er  # noqa: E402
import png_ref as pg  # noqa: E402
import preprocess_ref as pr  # noqa: E402
import sample_prep_ref as spr  # noqa: E402
import tiff_ref as tr  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402
from cmdiad_amd import ops  # noqa: E402
from cmdiad_amd.utils import png  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _assert_decodes(paths, target):
    """decode_on_device(read_raw of every path) == Pillow's array of every path for `target`."""
    raws = [png.read_raw(p, target) for p in paths]
    got = png.decode_on_device(raws, DEV)
    want = np.stack([pg.pillow(p, target) for p in paths])
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want)), (paths, target)
    return got


@pytest.mark.parametrize("color_type", [2, 0])
def test_the_skew_at_its_edges(tmp_path, color_type):
    """H in {1, 63, 64, 65, 129} x W in {1, 2, 63, 64, 65, 130}: one band and its last lane, the first row of a second and of a third
    band, widths around one chunk of 64 steps; a random mix of the five filter types per row."""
    C = pg.CHANNELS_OF_COLOR_TYPE[color_type]
    rs = np.random.RandomState(color_type)
    for H in (1, 63, 64, 65, 129):
        for W in (1, 2, 63, 64, 65, 130):
            p = str(tmp_path / f"{H}x{W}.png")
            pg.write(p, pg.image(H, W, C, seed=H * 131 + W, smooth=(H + W) % 2 == 0), filters=rs.randint(0, 5, H))
            _assert_decodes([p], "rgb" if color_type == 2 else "l")


def test_colour_types_and_targets(tmp_path):
    """Colour types 0 / 2 / 4 / 6 x 'rgb' / 'l' / 'raw' at 65 x 67."""
    rs = np.random.RandomState(5)
    for color_type in (0, 2, 4, 6):
        p = str(tmp_path / f"c{color_type}.png")
        pg.write(p, pg.image(65, 67, pg.CHANNELS_OF_COLOR_TYPE[color_type], seed=color_type), filters=rs.randint(0, 5, 65))
        for target in ("rgb", "l", "raw"):
            _assert_decodes([p], target)


def test_all_paeth_and_all_average_of_random_bytes(tmp_path):
    """129 x 130 random bytes, every row Paeth / every row Average: each byte depends on all three neighbours across two band edges;
    then the same files through the one-wave baseline (waves=1)."""
    for name, ft in (("paeth", 4), ("average", 3)):
        p = str(tmp_path / f"{name}.png")
        pg.write(p, pg.image(129, 130, 3, seed=ft), filters=ft)
        got = _assert_decodes([p], "rgb")
        raw = png.read_raw(p)
        buf = torch.from_numpy(raw.data.copy()).to(DEV)
        one = ops.png_unfilter(buf, [raw.layout], np.zeros(1, np.int64), "rgb", waves=1)
        assert torch.equal(one, got)


def test_every_wave_count_the_width_selects(tmp_path):
    """W = 897 is the last width of 8 waves, 898 the first of 16, 1857 the last of 16, 1858 the first that falls back to one wave
    (70 rows: two bands, the second one short); the forced wave counts give the same bytes where the width admits them."""
    rs = np.random.RandomState(9)
    for W in (897, 898, 1857, 1858):
        p = str(tmp_path / f"w{W}.png")
        pg.write(p, pg.image(70, W, 3, seed=W, smooth=True), filters=rs.randint(0, 5, 70))
        got = _assert_decodes([p], "rgb")
        raw = png.read_raw(p)
        buf = torch.from_numpy(raw.data.copy()).to(DEV)
        for waves in (1, 8, 16):
            if waves == 1 or 2 * waves >= (W + 126) // 64 + 2:
                assert torch.equal(ops.png_unfilter(buf, [raw.layout], np.zeros(1, np.int64), "rgb", waves=waves), got), (W, waves)
            else:
                with pytest.raises(Exception, match="waves"):
                    ops.png_unfilter(buf, [raw.layout], np.zeros(1, np.int64), "rgb", waves=waves)


def test_three_images_in_one_launch(tmp_path, monkeypatch):
    calls = []
    real = ops.png_unfilter
    monkeypatch.setattr(ops, "png_unfilter", lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))
    paths = []
    for k in range(3):
        paths.append(str(tmp_path / f"{k}.png"))
        pg.write(paths[-1], pg.image(65, 67, 3, seed=20 + k, smooth=k == 1), filters=np.random.RandomState(k).randint(0, 5, 65))
    _assert_decodes(paths, "rgb")
    assert calls == [3]


def test_production_size(tmp_path):
    """2 x 800 x 800 x 3: thirteen bands (the last of 32 rows) on eight waves, a random mix of the five types, and a Pillow-written file."""
    from PIL import Image
    a = pg.image(800, 800, 3, seed=31, smooth=True)
    p, q = str(tmp_path / "mix.png"), str(tmp_path / "pillow.png")
    pg.write(p, a, filters=np.random.RandomState(31).randint(0, 5, 800), level=1)
    Image.fromarray(pg.image(800, 800, 3, seed=32, smooth=True)).save(q, compress_level=1)
    got = _assert_decodes([p, q], "rgb")
    assert torch.equal(got[0].cpu(), torch.from_numpy(a))


def test_raw_images_and_host_arrays_share_a_batch(tmp_path):
    """SamplePrep.prepare_images / prepare_masks take RawImage objects beside decoded arrays, two colour types in one group: the
    tensors are the ones the decoded arrays give."""
    size = 64
    rgbs = [pg.image(size, size, 3, seed=40 + k, smooth=True) for k in range(4)]
    gts = [(pg.image(size, size, 1, seed=50 + k) > 128).astype(np.uint8) * 255 for k in range(4)]
    mixed_rgb, mixed_gt = list(rgbs), [gts[0], None, gts[2], gts[3]]
    for k in (0, 3):
        p = str(tmp_path / f"rgb{k}.png")
        a = rgbs[k] if k == 0 else np.concatenate([rgbs[k], np.full((size, size, 1), 9, np.uint8)], axis=2)      # rgb, then rgb + alpha
        pg.write(p, a, filters=np.random.RandomState(k).randint(0, 5, size))
        mixed_rgb[k] = png.read_raw(p, "rgb")
    p = str(tmp_path / "gt2.png")
    pg.write(p, gts[2], filters=3)
    mixed_gt[2] = png.read_raw(p, "l")
    prep = ds.SamplePrep(device=DEV)
    for want, got in zip(prep.prepare_images(rgbs), prep.prepare_images(mixed_rgb)):
        assert torch.equal(want.view(torch.int32), got.view(torch.int32))
    want = prep.prepare_masks([gts[0], None, gts[2], gts[3]])
    got = prep.prepare_masks(mixed_gt)
    assert got[1] is None and all(torch.equal(w, g) for w, g in zip(want, got) if w is not None)
    clouds = [spr.cloud(size, size, seed=70 + k) for k in range(4)]
    for (ws, wm), (gs, gm) in zip(prep.prepare_batch(rgbs, clouds, [gts[0], None, gts[2], gts[3]]), prep.prepare_batch(mixed_rgb, clouds, mixed_gt)):
        assert all(torch.equal(x, y) for x, y in zip(ws, gs)) and (wm is None) == (gm is None) and (wm is None or torch.equal(wm, gm))


def test_the_binding_refuses_offsets_that_leave_the_buffer(tmp_path):
    """ops.png_unfilter checks every image's [offset, offset + H * (1 + row_bytes)) against raw_u8's length BEFORE the launch:
    ValueError, and the output it was given is untouched.  A correct image that ends at the buffer's last byte decodes."""
    a = pg.image(13, 17, 3, seed=61)
    p = str(tmp_path / "g.png")
    pg.write(p, a, filters=[0, 1, 2, 3, 4] * 2 + [4, 3, 1])
    raw = png.read_raw(p)
    n = raw.data.size
    buf = torch.from_numpy(np.concatenate([np.full(5, 0xA5, np.uint8), raw.data])).to(DEV)      # odd offset, no padding behind
    out = torch.full((2, 13, 17, 3), 7, dtype=torch.uint8, device=DEV)
    got = ops.png_unfilter(buf, [raw.layout], np.array([5]), "rgb")
    assert torch.equal(got.cpu(), torch.from_numpy(a[None]))
    for offsets, what in (([5, 6], "image 1 at offset 6"), ([-1, 5], "image 0 at offset -1"), ([5, buf.numel()], "image 1")):
        with pytest.raises(ValueError, match=what + ".*does not lie inside"):
            ops.png_unfilter(buf, [raw.layout] * 2, np.array(offsets), "rgb", out=out)
    with pytest.raises(ValueError, match=r"offsets must be \[2\]"):
        ops.png_unfilter(buf, [raw.layout] * 2, np.array([5]), "rgb", out=out)
    with pytest.raises(ValueError, match="target"):
        ops.png_unfilter(buf, [raw.layout] * 2, np.array([5, 5]), "bgr", out=out)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and n == 13 * 52


# ------------------------------------------------------------------------------------------------ the loaders
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _items(source, monkeypatch, png_device, tiff_device=False):
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "1" if png_device else "0")
    monkeypatch.setenv("CMDIAD_TIFF_DEVICE", "1" if tiff_device else "0")
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


def _count_device_decodes(monkeypatch):
    """Every path whose RawImage reaches png.decode_on_device from here on."""
    calls = []
    real = png.decode_on_device
    monkeypatch.setattr(png, "decode_on_device", lambda raws, device: calls.extend(str(r.path) for r in raws) or real(raws, device))
    return calls


def _as_palette(path):
    """Rewrite a 0 / 255 mask as a PALETTE PNG of the same picture (index 1 = white): outside the subset, so it takes the fallback."""
    from PIL import Image
    g = np.array(Image.open(path).convert("L"))
    img = Image.fromarray((g > 127).astype(np.uint8), "P")
    img.putpalette([0, 0, 0, 255, 255, 255] + [0] * (254 * 3))
    img.save(path)
    assert png.read_layout(path).color_type == 3


def _refilter(path, seed):
    """Rewrite a PNG with a random mix of the five filter types (Pillow's writer never chooses Average)."""
    a = pg.pillow(path, "raw")
    pg.write(path, a, filters=np.random.RandomState(seed).randint(0, 5, a.shape[0]))


def _check_source(cls, monkeypatch, n_png, fallback):
    calls = _count_device_decodes(monkeypatch)
    host = _items(cls, monkeypatch, False)
    assert not calls
    dev = _items(cls, monkeypatch, True)
    assert len(calls) == n_png and fallback not in calls
    both = _items(cls, monkeypatch, True, tiff_device=True)
    for got in (dev, both):
        for g, w in zip(got, host):
            _assert_same_items(g, w)
    return host, dev


def test_sample_class_yields_the_same_items_with_device_decode(tmp_path, monkeypatch):
    """get_data_loader('train' / 'test') under 'hip' over sample_prep_ref.write_tree (real TIFFs, three rgb files rewritten with
    forced filters, one mask rewritten as a palette file): CMDIAD_PNG_DEVICE=1 and =0 yield equal tensors, order, labels and
    rgb_path; with =1 every supported PNG went through the device and the palette mask did not; with both device switches on, the same."""
    root = str(tmp_path)
    items = spr.write_tree(root, size=160)
    monkeypatch.setitem(sys.modules, "tifffile", None)
    for stem, (pc, _, _) in items.items():
        sub, name = os.path.split(stem)
        tr.write(os.path.join(root, "bagel", sub, "xyz", name + ".tiff"), pc)
    for k, stem in enumerate(("train/good/001", "test/good/000", "test/crack/001")):
        _refilter(os.path.join(root, "bagel", os.path.dirname(stem), "rgb", os.path.basename(stem) + ".png"), k)
    palette = os.path.join(root, "bagel", "test", "crack", "gt", "000.png")
    _as_palette(palette)
    _refilter(os.path.join(root, "bagel", "test", "crack", "gt", "001.png"), 7)
    args = types.SimpleNamespace(dataset_path=root, img_process_method="hip", num_workers=2)
    cls = ds.MVTec3DClass(root, "bagel", args)
    assert (cls.n_train, cls.n_test) == (3, 4)
    host, dev = _check_source(cls, monkeypatch, n_png=7 + 1, fallback=palette)
    assert [int(t[2]) for t in dev[1]] == [1, 1, 0, 0] and float(dev[1][0][1].sum()) > 0 and float(dev[1][1][1].sum()) > 0
    monkeypatch.setenv("CMDIAD_PNG_DEVICE", "1")
    one = cls._loader("test").dataset[1]                      # the item path (one prepare call per item) takes RawImages too
    assert all(torch.equal(_bits(a[0]), _bits(b)) for a, b in zip(dev[1][1][0], one[0])) and torch.equal(dev[1][1][1][0], one[1].cpu())


def test_raw_scan_class_yields_the_same_items_with_device_decode(tmp_path, monkeypatch):
    """MVTec3DRawClass over preprocess_ref.write_raw_tree (two shapes, real TIFFs): 'raw' RawImages for the colour type 2 rgb and
    the colour type 0 gt; the palette mask goes through Pillow."""
    from cmdiad_amd import evaluate as ev
    root = str(tmp_path)
    pr.write_raw_tree(root, types.SimpleNamespace(imwrite=lambda path, a: tr.write(path, a)))
    monkeypatch.setitem(sys.modules, "tifffile", None)
    cls = ds.MVTec3DRawClass(root, "bagel", ev.mtfi_args(dataset_path=root, img_process_method="hip", num_workers=2))
    assert (cls.n_train, cls.n_test) == (3, 4)
    gts = [str(g) for g in cls._test.gt_paths if g != 0]
    assert len(gts) == 2
    _as_palette(gts[0])
    _refilter(gts[1], 3)
    _refilter(str(cls._train.img_paths[0][0]), 4)
    _check_source(cls, monkeypatch, n_png=7 + 1, fallback=gts[0])


def test_eyecandies_raw_class_yields_the_same_items_with_device_decode(tmp_path, monkeypatch):
    """EyecandiesRawClass: the *_image_4.png as 'rgb' and the RGB mask of a bad sample as 'l' (Pillow's luma); the 16-bit depth PNGs
    stay with Pillow."""
    from cmdiad_amd import evaluate as ev
    items = er.write_raw_tree(str(tmp_path), "CandyCane", n_train=2, n_test=3, bad=(1,))
    _refilter(items[("test", 1)]["rgb_path"].replace("_image_4", "_mask"), 5)
    _refilter(items[("train", 0)]["rgb_path"], 6)
    cls = ds.EyecandiesRawClass(str(tmp_path), "CandyCane", ev.mtfi_args(dataset_path=str(tmp_path), img_process_method="hip", num_workers=2,
                                                                        dataset_type="eyecandies"))
    host, dev = _check_source(cls, monkeypatch, n_png=5 + 1, fallback=None)
    assert [int(t[2]) for t in dev[1]] == [1, 0, 0] and float(dev[1][0][1].sum()) > 0
