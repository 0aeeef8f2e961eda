"""GPU: the one item loop of the device sources (cmdiad_amd.dataset._device_items) across a batch boundary.  Every other test writes
trees with at most four items per split and runs them with batch=16: one batch, no refill of the read-ahead window.  Here readers=1
and batch=3, so ahead = max(2 * 1, 3) = 3: the trees have more items than that and a last batch shorter than 3.  What the kernels
compute is the other tests' business; the yardstick here is the same source with batch=16, and every comparison is for equal bits."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eyecandies_ref as er  # noqa: E402
import preprocess_ref as pr  # noqa: E402
import sample_prep_ref as spr  # noqa: E402

from cmdiad_amd import dataset as ds  # noqa: E402

pytestmark = pytest.mark.gpu


def _assert_same_items(got, want):
    assert len(got) == len(want)
    for k, (x, y) in enumerate(zip(got, want)):
        assert len(x) == len(y), k
        assert all(a.is_cuda and torch.equal(a, b) for a, b in zip(x[0], y[0])) and len(x[0]) == len(y[0]) == 3, k
        assert x[0].n_valid == y[0].n_valid and x[0].n_valid > 0, k
        if len(x) == 4:
            assert not x[1].is_cuda and torch.equal(x[1], y[1]) and x[3] == y[3], k
        assert torch.equal(x[-1] if len(x) == 2 else x[2], y[-1] if len(y) == 2 else y[2]), k


def _small_batches(cls):
    cls.batch, cls.readers = 3, 1
    return cls


def test_mvtec3d_class_items_do_not_depend_on_the_batch(tmp_path, monkeypatch):
    """MVTec3DClass('hip') over 3 train / 4 test items of 160 x 160: the loader with batch=3, readers=1 (test: a refill and a last
    batch of one) yields what it yields with batch=16, and both yield dataset[i] with the leading 1 added."""
    spr.write_tree(str(tmp_path), size=160)
    spr.patch_tiff_reader(monkeypatch)
    args = types.SimpleNamespace(dataset_path=str(tmp_path), img_process_method="hip", num_workers=2)
    cls = ds.MVTec3DClass(str(tmp_path), "bagel", args)
    assert (cls.n_train, cls.n_test) == (3, 4)
    for split, n in (("train", 3), ("test", 4)):
        want = list(cls._loader(split))
        small = _small_batches(cls._loader(split))
        assert isinstance(small, ds.DeviceSampleLoader) and len(small) == n
        got = list(small)
        _assert_same_items(got, want)
        assert [int(x[-1] if split == "train" else x[2]) for x in got] == ([0, 0, 0] if split == "train" else [1, 1, 0, 0])
        for i, item in enumerate(got):
            one = small.dataset[i]
            assert all(torch.equal(a, b[None]) for a, b in zip(item[0], one[0])) and item[0].n_valid == one[0].n_valid
            if split == "test":
                assert torch.equal(item[1], one[1][None].cpu()) and int(item[2]) == one[2] and item[3] == [one[3]]
                assert bool(item[1].any()) == bool(one[2])
            else:
                assert int(item[1]) == one[1]


def _eyecandies(root):
    args = types.SimpleNamespace(dataset_path=str(root), img_process_method="hip", num_workers=2, dataset_type="eyecandies")
    return ds.EyecandiesRawClass(str(root), "CandyCane", args)


def test_eyecandies_raw_class_items_do_not_depend_on_the_batch(tmp_path):
    """EyecandiesRawClass over 5 train / 5 test scans of 40 x 48: batches of 3 + 2 equal one batch of 5; bad samples first."""
    items = er.write_raw_tree(str(tmp_path), "CandyCane", n_train=5, n_test=5, bad=(1, 3))
    want, small = _eyecandies(tmp_path), _small_batches(_eyecandies(tmp_path))
    assert want.batch == 16 and (small.n_train, small.n_test) == (5, 5)
    train, test = list(small.train()), list(small.test())
    _assert_same_items(train, list(want.train()))
    _assert_same_items(test, list(want.test()))
    assert [int(t[1]) for t in train] == [0] * 5 and [int(t[2]) for t in test] == [1, 1, 0, 0, 0]
    assert [t[3] for t in test] == [[items[("test", i)]["rgb_path"]] for i in (1, 3, 0, 2, 4)]
    assert [bool(t[1].any()) for t in test] == [True, True, False, False, False]


def test_mvtec3d_raw_class_items_do_not_depend_on_the_batch(tmp_path, monkeypatch):
    """MVTec3DRawClass over the raw tree of test_gpu_raw_mvtec.py (3 train, 4 test, two shapes): batches of 3 + 1 equal one of 4."""
    from cmdiad_amd import evaluate as ev
    root = str(tmp_path)
    stems = pr.write_raw_tree(root, pr.fake_tifffile(monkeypatch))
    args = ev.mtfi_args(dataset_path=root, img_process_method="hip", num_workers=2)
    want, small = ds.MVTec3DRawClass(root, "bagel", args), _small_batches(ds.MVTec3DRawClass(root, "bagel", args))
    assert want.batch == 16 and (small.n_train, small.n_test) == (3, 4)
    train, test = list(small.train()), list(small.test())
    _assert_same_items(train, list(want.train()))
    _assert_same_items(test, list(want.test()))
    assert [int(t[2]) for t in test] == [0, 0, 1, 1] and [bool(t[1].any()) for t in test] == [False, False, True, True]
    assert [t[3] for t in test] == [[os.path.join(root, "bagel", os.path.dirname(s), "rgb", os.path.basename(s) + ".png")] for s, _, _ in stems[3:]]


def test_a_decode_failure_surfaces_at_its_item_and_leaves_the_device_usable(tmp_path):
    """A train sample's pose file disappears after the class was constructed (a host error: nothing on the device is provoked).  With
    batches of 3 the failing item 3 opens the second batch: items 0..2 arrive as an intact class yields them, then the reader's
    error; the reader threads are gone, and a second, intact class on the same device still iterates."""
    import threading
    er.write_raw_tree(str(tmp_path / "a"), "CandyCane", n_train=5, n_test=1, bad=())
    er.write_raw_tree(str(tmp_path / "b"), "CandyCane", n_train=5, n_test=1, bad=())
    broken, intact = _small_batches(_eyecandies(tmp_path / "a")), _small_batches(_eyecandies(tmp_path / "b"))
    os.remove(broken._train_files[3]["pose"])
    pools = lambda: {t for t in threading.enumerate() if t.name.startswith("ThreadPoolExecutor")}  # noqa: E731
    before, got = pools(), []
    with pytest.raises(FileNotFoundError, match="003_pose.txt"):
        for item in broken.train():
            got.append(item)
    assert pools() <= before
    want = list(intact.train())
    assert len(want) == 5 and len(got) == 3
    _assert_same_items(got, want[:3])
