"""No GPU: the opt-in and the construction of dataset.MVTec3DRawClass (the raw MVTec 3D-AD download as a class source; the device
side is tests/test_gpu_raw_mvtec.py)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sample_prep_ref as sr  # noqa: E402


def _args(root, **kw):
    from cmdiad_amd import evaluate as ev
    return ev.mtfi_args(dataset_path=str(root), num_workers=2, **kw)


def test_mtfi_args_default_is_the_cleaned_tree():
    from cmdiad_amd import evaluate as ev
    assert ev.mtfi_args().raw_scans is False
    assert ev.mtfi_args(raw_scans=True).raw_scans is True


def test_dataset_classes_selects_the_raw_class_only_on_request(tmp_path):
    import types
    from cmdiad_amd import dataset as ds
    sr.write_tree(str(tmp_path), size=160)
    a = _args(tmp_path, img_process_method="cpu_v1", raw_scans=False)
    found = ds.dataset_classes(a)
    assert list(found) == ["bagel"] and type(found["bagel"]) is ds.MVTec3DClass
    bare = types.SimpleNamespace(**{k: v for k, v in vars(a).items() if k != "raw_scans"})      # an args object without the attribute
    assert type(ds.dataset_classes(bare)["bagel"]) is ds.MVTec3DClass
    found = ds.dataset_classes(_args(tmp_path, img_process_method="hip", raw_scans=True))
    assert list(found) == ["bagel"] and type(found["bagel"]) is ds.MVTec3DRawClass
    # the switch is MVTec 3D-AD's: an Eyecandies run does not look at it
    os.makedirs(tmp_path / "CandyCane" / "train" / "good" / "rgb")
    os.makedirs(tmp_path / "CandyCane" / "test" / "good" / "rgb")
    found = ds.dataset_classes(_args(tmp_path, img_process_method="cpu_v1", raw_scans=True, dataset_type="eyecandies"))
    assert type(found["CandyCane"]) is ds.MVTec3DClass


def test_raw_class_constructs_without_a_device(tmp_path):
    """Construction is file discovery: the same files, order and labels as the reference's dataset classes, no GPU touched."""
    from cmdiad_amd import dataset as ds
    sr.write_tree(str(tmp_path), size=160)
    cls = ds.MVTec3DRawClass(str(tmp_path), "bagel", _args(tmp_path, img_process_method="hip"))
    assert (cls.name, cls.n_train, cls.n_test) == ("bagel", 3, 4)
    ref = ds.MVTec3DClass(str(tmp_path), "bagel", _args(tmp_path, img_process_method="cpu_v1"))
    assert (ref.n_train, ref.n_test) == (cls.n_train, cls.n_test)
    test = ds.TestDataset("bagel", 224, 224, 224, str(tmp_path), "hip")
    assert cls._test.img_paths == test.img_paths and cls._test.labels == test.labels == [1, 1, 0, 0] and cls._test.gt_paths == test.gt_paths
    assert cls._prep is None
    os.makedirs(tmp_path / "bagel" / "validation" / "good" / "rgb")
    both = ds.MVTec3DRawClass(str(tmp_path), "bagel", _args(tmp_path, img_process_method="hip", train_with_validation=True))
    assert both.n_train == 3 and type(both._train) is ds.TrainValidationDataset


@pytest.mark.parametrize("method", ["cpu_v1", "cpu_v2"])
def test_raw_class_has_no_host_path(tmp_path, method):
    from cmdiad_amd import dataset as ds
    sr.write_tree(str(tmp_path), size=160)
    with pytest.raises(ValueError, match="img_process_method must be 'hip'.*preprocessing.py.*MVTec3DClass"):
        ds.MVTec3DRawClass(str(tmp_path), "bagel", _args(tmp_path, img_process_method=method))
    with pytest.raises(ValueError, match="img_process_method must be one of"):
        ds.MVTec3DRawClass(str(tmp_path), "bagel", _args(tmp_path, img_process_method="gpu"))
    with pytest.raises(ValueError, match="'hip'"):
        ds.dataset_classes(_args(tmp_path, img_process_method=method, raw_scans=True))
