"""Host side of the stored fits (cmdiad_amd/fitted.py, docs/fitted.md): the file format and its refusals, the numpy restatement
of the digest, the restore of a one-class SVM from its stored arrays, and the C ABI of cmdiad_digest64.  No GPU."""
import ctypes
import json
import os
import struct
import tracemalloc

import numpy as np
import pytest

from cmdiad_amd import fitted

M64 = (1 << 64) - 1


def _arrays():
    rs = np.random.RandomState(5)
    return {"lib": rs.randn(300, 24).astype(np.float32), "wide": rs.randn(7, 3), "count": np.arange(-4, 9, dtype=np.int64).reshape(13),
            "scalar": np.float32(rs.randn()).reshape(()), "empty": np.zeros((0, 24), dtype=np.float32)}


def test_round_trip_is_bit_exact_and_aligned(tmp_path):
    path = str(tmp_path / "a.cmdfit")
    arrays = _arrays()
    fitted.write_file(path, {"class_name": "bagel", "note": "ä"}, arrays)
    assert not [f for f in os.listdir(tmp_path) if f != "a.cmdfit"]          # the temporary name is gone
    raw = open(path, "rb").read()
    assert raw[:8] == b"CMDFIT\x00\x01" and struct.unpack("<II", raw[8:16])[0] == 1
    head = fitted.read_header(path)
    assert head["format"] == "cmdfit" and head["class_name"] == "bagel" and head["note"] == "ä"
    assert [e["name"] for e in head["arrays"]] == list(arrays)
    for e in head["arrays"]:
        a = arrays[e["name"]]
        assert e["offset"] % 4096 == 0 and e["offset"] >= 4096 and e["nbytes"] == a.nbytes and e["shape"] == list(a.shape)
        got = fitted.read_array(path, e["name"])
        assert got.dtype == a.dtype and got.shape == a.shape and got.tobytes() == a.tobytes()
        assert int(e["digest64"], 16) == fitted.digest64_host(a)
    assert {e["dtype"] for e in head["arrays"]} == {"float32", "float64", "int64"}
    for lo, hi in ((0, 300), (128, 200), (299, 300), (17, 17)):
        assert np.array_equal(fitted.read_array(path, "lib", rows=(lo, hi)), arrays["lib"][lo:hi])
    assert np.array_equal(fitted.read_array(path, "wide", rows=(2, 5)), arrays["wide"][2:5])
    assert np.array_equal(fitted.read_array(path, "count", rows=(3, 4)), arrays["count"][3:4])
    with pytest.raises(fitted.FitFileError, match="rows"):
        fitted.read_array(path, "lib", rows=(10, 301))
    with pytest.raises(fitted.FitFileError, match="nope"):
        fitted.read_array(path, "nope")
    # the 128-row block digests stored beside a 2-D array: a run of blocks is the digest of those rows at their offset
    e = fitted.array_entry(head, "lib")
    bl = [int(b, 16) for b in e["block_digests"]]
    assert len(bl) == 3 and sum(bl) & M64 == int(e["digest64"], 16)
    assert (bl[1] + bl[2]) & M64 == fitted.digest64_host(arrays["lib"][128:], 128 * 24)


def _raw_file(path, header, version=1, magic=b"CMDFIT\x00\x01", hlen=None, tail=b""):
    blob = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<II", version, len(blob) if hlen is None else hlen) + blob + tail)


def _entry(**kw):
    e = dict(name="lib", dtype="float32", shape=[4, 2], offset=4096, nbytes=32, digest64="0")
    e.update(kw)
    return e


def test_refusals_name_the_field_and_touch_no_payload(tmp_path):
    good = str(tmp_path / "good.cmdfit")
    fitted.write_file(good, {}, {"lib": np.ones((4, 2), dtype=np.float32)})
    raw = open(good, "rb").read()
    huge = 1 << 40          # a payload no host can allocate: whoever allocates before validating dies of MemoryError
    cases = {}
    cases["truncated"] = ("offset", raw[:4096 + 16])
    cases["lead"] = ("magic", raw[:11])
    cases["magic"] = ("magic", b"CMDFIX\x00\x01" + raw[8:])
    cases["version"] = ("version", raw[:8] + struct.pack("<I", 2) + raw[12:])
    cases["header"] = ("header_len", raw[:12] + struct.pack("<I", (1 << 20) + 1) + raw[16:] + b"\0" * (1 << 20))
    for tag, (field, blob) in cases.items():
        p = str(tmp_path / f"{tag}.cmdfit")
        open(p, "wb").write(blob)
        cases[tag] = (field, p)
    for tag, field, entry in (("far", "offset", _entry(offset=1 << 30)), ("odd", "offset", _entry(offset=4097)),
                              ("big", "offset", _entry(shape=[huge // 4], nbytes=huge)), ("lie", "nbytes", _entry(nbytes=huge)),
                              ("dtype", "dtype", _entry(dtype="object")), ("dtype2", "dtype", _entry(dtype="float16")),
                              ("shape", "shape", _entry(shape=[4, -2]))):
        p = str(tmp_path / f"{tag}.cmdfit")
        _raw_file(p, {"arrays": [entry]}, tail=b"\0" * 8192)
        cases[tag] = (field, p)
    tracemalloc.start()
    try:
        for tag, (field, p) in cases.items():
            for call in (lambda: fitted.read_header(p), lambda: fitted.read_array(p, "lib"), lambda: fitted.read_array(p, "lib", rows=(0, 1))):
                with pytest.raises(fitted.FitFileError) as err:
                    call()
                assert field in str(err.value) and p in str(err.value), (tag, str(err.value))
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert peak < (1 << 20), peak            # not even the refused 1 MiB header was read
    assert issubclass(fitted.FitFileError, ValueError) and issubclass(fitted.FitMismatch, ValueError)
    # version 2 is refused by name
    with pytest.raises(fitted.FitFileError, match="version 2"):
        fitted.read_header(cases["version"][1])
    # a writer refuses what no reader would take
    with pytest.raises(fitted.FitFileError, match="dtype"):
        fitted.write_file(str(tmp_path / "x.cmdfit"), {}, {"a": np.zeros(3, dtype=np.float16)})
    assert not os.path.exists(tmp_path / "x.cmdfit")


def _mix(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def test_digest64_host():
    assert fitted.digest64_host(np.zeros((0,), dtype=np.float32)) == 0 == fitted.digest64_host(np.zeros((0, 5)), 77)
    rs = np.random.RandomState(11)
    words = rs.randint(0, 1 << 32, size=1000, dtype=np.uint64).astype("<u4")
    # the definition, word by word in Python integers
    for seed in (0, 9, (1 << 63) + 5, M64):
        want = sum(_mix(_mix((seed + i) & M64) ^ int(w)) for i, w in enumerate(words)) & M64
        assert fitted.digest64_host(words, seed) == want
    assert fitted.digest64_host(words.view(np.float32)) == fitted.digest64_host(words) == fitted.digest64_host(words.reshape(10, 100))
    # not a plain sum of the words: swapping two unequal ones changes it
    sw = words.copy()
    assert sw[3] != sw[700]
    sw[3], sw[700] = words[700], words[3]
    assert fitted.digest64_host(sw) != fitted.digest64_host(words)
    # digest(a || b, s) = digest(a, s) + digest(b, s + len(a) / 4)
    big = rs.randint(0, 1 << 32, size=(1 << 20) + 77, dtype=np.uint64).astype("<u4")       # (crosses the host loop's chunk)
    for cut, seed in ((1, 0), (333, 12345), (1 << 20, (1 << 64) - 100)):
        whole = fitted.digest64_host(big, seed)
        assert whole == (fitted.digest64_host(big[:cut], seed) + fitted.digest64_host(big[cut:], seed + cut)) & M64
    # a byte count that is no multiple of 4 is zero-padded
    assert fitted.digest64_host(np.array([1, 2, 3, 4, 5], dtype=np.uint8)) == fitted.digest64_host(np.array([1, 2, 3, 4, 5, 0, 0, 0], dtype=np.uint8))


def test_fuser_restored_from_the_file(tmp_path, monkeypatch):
    from sklearn.linear_model import SGDOneClassSVM
    from cmdiad_amd.feature_extractors import multiple_features as mf
    rs = np.random.RandomState(2)
    x = (rs.randn(200, 2) * [0.3, 2.0] + [1.0, -4.0]).astype(np.float32)
    fit = SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000).fit(x)
    path = str(tmp_path / "f.cmdfit")
    fitted.write_file(path, {}, fitted.fuser_arrays(fit, "detect_fuser"))
    got = fitted.restore_fuser(SGDOneClassSVM(random_state=42, nu=0.5, max_iter=1000),
                               *(fitted.read_array(path, f"detect_fuser.{k}") for k in ("coef_", "offset_", "n_iter_")))
    assert got.coef_.tobytes() == fit.coef_.tobytes() and got.offset_.tobytes() == fit.offset_.tobytes() and got.n_iter_ == fit.n_iter_
    q = rs.randn(50, 2).astype(np.float32)
    for probe in (q, q.astype(np.float64)):
        assert np.array_equal(got.score_samples(probe), fit.score_samples(probe))
    # ... and it takes the method classes' fast path, which must not go through the object's own method
    want = fit.score_samples(q)
    monkeypatch.setattr(SGDOneClassSVM, "score_samples", lambda self, X: (_ for _ in ()).throw(AssertionError("slow path")))
    assert np.array_equal(mf._score_samples(got, q), want)


def test_digest64_abi():
    from cmdiad_amd import _native as nat
    L = nat.lib()
    assert "cmdiad_digest64" in nat.SIGNATURES and L.cmdiad_digest64.argtypes == nat.SIGNATURES["cmdiad_digest64"]
    assert L.cmdiad_abi_version() == 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cmdiad_hip.h")).read()
    assert "int cmdiad_digest64(const void* data, size_t bytes, uint64_t seed, uint64_t* acc, cmdiad_stream_t stream);" in hdr
    assert "adversar" in hdr[hdr.index("Content digest"):]
    # refused before anything is launched or read: the pointers below are never dereferenced
    data, acc = ctypes.c_void_p(0x7000_0000_1000), ctypes.c_void_p(0x7000_0000_2000)
    for args in ((None, 8, 0, acc, None), (data, 8, 0, None, None), (data, 6, 0, acc, None),
                 (ctypes.c_void_p(data.value + 2), 8, 0, acc, None)):
        assert L.cmdiad_digest64(*args) == -1          # CMDIAD_ERR_ARG
        assert b"cmdiad_digest64" in L.cmdiad_last_error()
    assert L.cmdiad_digest64(None, 0, 5, acc, None) == 0      # nothing to hash: a success that touches nothing


def test_info_cli(tmp_path, capsys):
    path = str(tmp_path / "a.cmdfit")
    fitted.write_file(path, {"class_name": "rope", "method_class": "PointFeatures"}, {"patch_xyz_lib": np.ones((130, 8), dtype=np.float32)})
    assert fitted.main(["info", path]) == 0
    out = capsys.readouterr().out
    assert '"class_name": "rope"' in out and "patch_xyz_lib" in out and "(130, 8)" in out and "4096" in out
    assert fitted.main([]) == 2
