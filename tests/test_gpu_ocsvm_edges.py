"""cmdiad_ocsvm_fit (cmdiad_amd/csrc/ocsvm.hip) through DeviceSGDOneClassSVM (cmdiad_amd/ocsvm.py) against scikit-learn's
SGDOneClassSVM on the same float32 rows, past the point the first suite (tests/test_gpu_ocsvm.py) stops at: fits long enough to
run the weight-rescale branch (`wscale < 1e-6`, step 681 755 at nu = 1.0, 1 829 034 at nu = 0.5) with the rescale on lane 0, on
lane 63, in the ragged last chunk and on either side of an epoch's end; stopping epochs other than 6; n on the boundaries of the
epoch kernel's 64-sample chunk and of the generator kernel's 64 steps per thread / 16 384 per block; seeds; data that is not
positive scores.  The cases are ocsvm_ref.CASES, which tests/test_ocsvm_ref_cpu.py pins on the CPU (the restatement equals
scikit-learn bit for bit on them, and each fixture exercises the branch it is there for).

Every assertion is equality: coef_ as bits, offset_, n_iter_, t_, score_samples and decision_function of 64 query rows as float32
and as float64.  n_iter_no_change in {1, 2, 8} has no scikit-learn side (its class has no such argument) and is held to the
restatement.

Checked once against two deliberately wrong builds of the epoch kernel -- the rescale branch left out, and the rescale done as
`(float)((double)w * wscale)` instead of `w * (float)wscale` -- : the six rescale cases fail on both, and nothing else in this file
or in tests/test_gpu_ocsvm.py notices either."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ocsvm_ref as R

gpu = pytest.mark.gpu
WITH_SKLEARN = [c for c in R.CASES if c.n_iter_no_change == 5]
PATIENCE = [c for c in R.CASES if c.group == "patience"]


@functools.lru_cache(maxsize=None)
def sk(name):
    return R.sklearn_fit(R.BY_NAME[name])


def device_fit(case, X=None):
    from cmdiad_amd.ocsvm import DeviceSGDOneClassSVM
    X = torch.from_numpy(R.make_X(case)).cuda() if X is None else X
    return DeviceSGDOneClassSVM(nu=case.nu, max_iter=case.max_iter, tol=case.tol, random_state=R.random_state(case),
                                n_iter_no_change=case.n_iter_no_change).fit(X)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_model(dev, coef, offset, n_iter, t):
    assert dev.coef_.dtype == np.float32 and dev.coef_.shape == coef.shape
    np.testing.assert_array_equal(bits(dev.coef_), bits(coef))
    assert dev.offset_.shape == (1,) and dev.offset_[0] == offset
    assert dev.n_iter_ == n_iter and dev.t_ == t


@gpu
@pytest.mark.parametrize("case", WITH_SKLEARN, ids=[c.name for c in WITH_SKLEARN])
def test_device_fit_equals_sklearn(case):
    ref = sk(case.name)
    dev = device_fit(case)
    assert_same_model(dev, ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)
    q32 = R.queries(case)
    for q in (q32, q32.astype(np.float64)):
        for method in ("score_samples", "decision_function"):
            a, b = getattr(dev, method)(q), getattr(ref, method)(q)
            assert a.dtype == b.dtype and a.shape == b.shape == (64,)      # float64 on both sides: offset_ is a double
            np.testing.assert_array_equal(bits(a), bits(b))


@gpu
@pytest.mark.parametrize("case", PATIENCE, ids=[c.name for c in PATIENCE])
def test_device_patience_equals_the_restatement(case):
    """n_iter_no_change is an argument of the device class alone: the restatement (pinned to scikit-learn at 5) is the reference."""
    coef, offset, n_iter, st = R.run(case)
    assert_same_model(device_fit(case), coef, offset, n_iter, st.t)


# ------------------------------------------------------------------------------------------------------------- the C entry point
def c_fit(Xd, nu, max_iter, tol, n_iter_no_change, seed):
    from cmdiad_amd import _native, ops
    from cmdiad_amd.ocsvm import xorshift32_pow2_table
    n, F = Xd.shape
    ws, wsb = ops._workspace("cmdiad_ocsvm_fit_workspace_bytes", Xd.device, n, F)
    tab = np.ascontiguousarray(xorshift32_pow2_table())
    coef = np.full(F, np.nan, dtype=np.float32)
    offset, n_iter = ctypes.c_double(np.nan), ctypes.c_int(-1)
    rc = _native.lib().cmdiad_ocsvm_fit(Xd.data_ptr(), n, F, nu, max_iter, tol, n_iter_no_change, seed, tab.ctypes.data_as(ctypes.c_void_p),
                                        coef.ctypes.data_as(ctypes.c_void_p), ctypes.byref(offset), ctypes.byref(n_iter), ws.data_ptr(), wsb,
                                        torch.cuda.current_stream(Xd.device).cuda_stream)
    _native.check(rc, "cmdiad_ocsvm_fit")
    return coef, offset.value, n_iter.value


@gpu
def test_seed_zero_is_seed_one_through_the_c_entry():
    """our_rand_r replaces a zero state by 1.  No random_state makes DeviceSGDOneClassSVM draw 0, so the C entry point is called."""
    case = R.BY_NAME["seed-0"]
    X = R.make_X(case)
    Xd = torch.from_numpy(X).cuda()
    zero, one = (c_fit(Xd, case.nu, case.max_iter, case.tol, 5, seed) for seed in (0, 1))
    coef, offset, n_iter, _ = R.fit(X, case.nu, case.max_iter, case.tol, None, seed=0)
    for got in (zero, one):
        np.testing.assert_array_equal(bits(got[0]), bits(coef))
        assert got[1:] == (offset, n_iter)


def test_the_c_entry_rejects_bad_arguments_without_a_launch():
    """cmdiad_ocsvm_fit validates before its first HIP call: -1 and a message, on a machine without a GPU too."""
    from cmdiad_amd import _native as nat
    L = nat.lib()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(X=p, n=8, F=2, nu=0.5, max_iter=3, pow2=p, coef=p, offset=p, n_iter=p, ws=p)

    def call(**kw):
        a = {**good, **kw}
        return L.cmdiad_ocsvm_fit(a["X"], a["n"], a["F"], a["nu"], a["max_iter"], 1e-3, 5, 42, a["pow2"], a["coef"], a["offset"], a["n_iter"],
                                  a["ws"], 1 << 20, None)

    for kw, text in ((dict(n=1), b"need n >= 2"), (dict(n=0), b"need n >= 2"), (dict(F=0), b"F=0"), (dict(F=5), b"F=5"), (dict(nu=0.0), b"need n >= 2"),
                     (dict(nu=-0.5), b"need n >= 2"), (dict(max_iter=0), b"need n >= 2"), (dict(X=None), b"null pointer"), (dict(pow2=None), b"null pointer"),
                     (dict(coef=None), b"null pointer"), (dict(offset=None), b"null pointer"), (dict(n_iter=None), b"null pointer"),
                     (dict(ws=None), b"null pointer")):
        assert call(**kw) == -1 and text in L.cmdiad_last_error(), (kw, L.cmdiad_last_error())
    assert not any(buf)                                 # no output was written


# ------------------------------------------------------------------------------------------------------------- non-finite parity
@gpu
def test_non_finite_rows_raise_like_sklearn_and_leave_nothing_fitted():
    """Rows of 3e38: the first update overflows the float32 weights (all arithmetic stays in registers; the host reads the state
    after the epoch).  scikit-learn raises ValueError at epoch #1; the device fit raises NativeError naming epoch 1."""
    from sklearn.linear_model import SGDOneClassSVM
    from cmdiad_amd import _native
    from cmdiad_amd.ocsvm import DeviceSGDOneClassSVM
    X = np.full((256, 2), 3e38, dtype=np.float32)
    with pytest.raises(ValueError, match="epoch #1"):
        SGDOneClassSVM(nu=0.5, random_state=42).fit(X)
    dev = DeviceSGDOneClassSVM(nu=0.5, random_state=42)
    with pytest.raises(_native.NativeError, match=r"under-/overflow at epoch 1 "):
        dev.fit(torch.from_numpy(X).cuda())
    assert not any(hasattr(dev, a) for a in ("coef_", "offset_", "n_iter_", "t_", "n_features_in_"))
    torch.cuda.synchronize()
    case = R.BY_NAME["seed-42"]                         # the library and the object are as usable as before
    ref = sk(case.name)
    assert_same_model(dev.fit(torch.from_numpy(R.make_X(case)).cuda()), ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)


# ------------------------------------------------------------------------------------------------------------- surface
@gpu
def test_input_kinds_give_the_contiguous_device_tensors_result():
    case = R.BY_NAME["n129-b"]
    X = R.make_X(case)
    ref = sk(case.name)
    X2 = np.zeros((case.n, 2 * case.F), dtype=np.float32)
    X2[:, ::2] = X
    X2[:, 1::2] = 7.0
    kinds = {"device tensor": torch.from_numpy(X).cuda(), "numpy": X, "cpu tensor": torch.from_numpy(X), "numpy view": X2[:, ::2],
             "cpu tensor view": torch.from_numpy(X2)[:, ::2], "device tensor view": torch.from_numpy(X2).cuda()[:, ::2]}
    assert not kinds["numpy view"].flags.c_contiguous and not kinds["device tensor view"].is_contiguous()
    for kind, x in kinds.items():
        dev = device_fit(case, X=x)
        assert_same_model(dev, ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)
        assert dev.n_features_in_ == case.F, kind


@gpu
def test_float64_rows_are_refused():
    from cmdiad_amd.ocsvm import DeviceSGDOneClassSVM
    X = R.make_X(R.BY_NAME["n129-b"]).astype(np.float64)
    for x in (X, torch.from_numpy(X), torch.from_numpy(X).cuda()):
        dev = DeviceSGDOneClassSVM(random_state=42)
        with pytest.raises(NotImplementedError, match="float32"):
            dev.fit(x)
        assert not hasattr(dev, "coef_")


@gpu
def test_fitting_twice_gives_the_same_bits():
    from cmdiad_amd.ocsvm import DeviceSGDOneClassSVM
    case = R.BY_NAME["stop-500x4"]
    ref = sk(case.name)
    Xd = torch.from_numpy(R.make_X(case)).cuda()
    dev = DeviceSGDOneClassSVM(nu=case.nu, max_iter=case.max_iter, tol=case.tol, random_state=case.rs)
    for _ in range(2):
        assert dev.fit(Xd) is dev
        assert_same_model(dev, ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)
    other = R.BY_NAME["data-negative"]                   # and a fit of other rows, other F, replaces every attribute
    o = sk(other.name)
    dev.fit(torch.from_numpy(R.make_X(other)).cuda())
    assert_same_model(dev, o.coef_, o.offset_[0], o.n_iter_, o.t_)
    assert dev.n_features_in_ == other.F


@gpu
def test_a_fit_on_a_side_stream_equals_the_default_stream_fit():
    case = R.BY_NAME["n16385-a"]
    ref = sk(case.name)
    Xd = torch.from_numpy(R.make_X(case)).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev = device_fit(case, X=Xd)
    side.synchronize()
    assert_same_model(dev, ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)
    assert_same_model(device_fit(case, X=Xd), ref.coef_, ref.offset_[0], ref.n_iter_, ref.t_)
