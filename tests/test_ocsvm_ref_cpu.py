"""tests/ocsvm_ref.py -- the restatement of scikit-learn's float32 one-class SGD that tests/test_gpu_ocsvm_edges.py holds
cmdiad_ocsvm_fit to -- against the INSTALLED scikit-learn, bit for bit, on every entry of ocsvm_ref.CASES; and the conditions under
which a fixture exercises its branch, asserted on the fixture itself (statistics of the restatement run), so that a changed
generator or library version cannot quietly turn a rescale case into one that never rescales.

Two kinds of case are not run through both sides: n_iter_no_change != 5 (scikit-learn's SGDOneClassSVM has no such argument: those
cases are held to the restatement alone, here only checked for what they make the rule do) and the production-nu rescale case
(1.86 M steps: scikit-learn and `rescale_steps`, not the Python loop).  Every case prints one line of the table in ocsvm_ref's
docstring (pytest -s shows them)."""
import functools

import numpy as np
import pytest

import ocsvm_ref as R

WITH_SKLEARN = [c for c in R.CASES if c.n_iter_no_change == 5]
LOOPED = [c for c in R.CASES if c.name not in R.LOOP_FREE]
RESCALE = [c for c in R.CASES if c.group == "rescale"]
STOP = [c for c in R.CASES if c.group == "stop"]
ids = lambda cases: [c.name for c in cases]   # noqa: E731


@functools.lru_cache(maxsize=None)
def restated(name, rescale=True):
    return R.run(R.BY_NAME[name], rescale=rescale)


@functools.lru_cache(maxsize=None)
def sk(name):
    return R.sklearn_fit(R.BY_NAME[name])


def test_the_first_rescale_steps_are_the_recorded_ones():
    """Data-independent: the running product of the float32 factors, which depend on t and nu alone (docs/history.md section 7)."""
    assert R.rescale_steps(1.0, 700000) == [R.NU1_FIRST_RESCALE] == [681755]
    assert R.rescale_steps(0.5, 1856512) == [R.NU05_FIRST_RESCALE] == [1829034]
    assert R.rescale_steps(0.3, 3200000) == [R.NU03_FIRST_RESCALE] == [3147809]
    assert R.rescale_steps(0.5, 1800000) == []          # the longest earlier case (300 000 rows, 6 epochs) ended before it
    # the factors are ~ 1 - 1/t, their product from step a to step b ~ a/b: after the first rescale the next is 10^6 times further
    assert R.rescale_steps(1.0, 4 * 10 ** 6) == [681755]


@pytest.mark.parametrize("case", WITH_SKLEARN, ids=ids(WITH_SKLEARN))
def test_restatement_equals_sklearn_bit_for_bit(case):
    ref = sk(case.name)
    if case.name in R.LOOP_FREE:
        print("\n" + R.table_line(case, ref.n_iter_, None))
        assert ref.n_iter_ == case.max_iter and ref.t_ == 1.0 + case.max_iter * case.n
        return
    coef, offset, n_iter, st = restated(case.name)
    print("\n" + R.table_line(case, n_iter, st))
    assert ref.coef_.dtype == np.float32 and ref.coef_.shape == coef.shape
    np.testing.assert_array_equal(coef.view(np.uint32), ref.coef_.view(np.uint32))
    assert ref.offset_.shape == (1,) and offset == ref.offset_[0]
    assert n_iter == ref.n_iter_ and st.t == ref.t_
    assert len(st.sumloss) == len(st.counter) == n_iter and st.hits + st.misses == n_iter * case.n


@pytest.mark.parametrize("case", LOOPED, ids=ids(LOOPED))
def test_every_case_has_hits_and_misses(case):
    st = restated(case.name)[3]
    assert st.hits > 0 and st.misses > 0, (st.hits, st.misses)
    if case.data == "zeros":                             # p = intercept for every sample: only the intercept moves
        coef, _, n_iter, _ = restated(case.name)
        assert not coef.any() and n_iter == 7


# ---------------------------------------------------------------------------------------------------------------- rescale group
@pytest.mark.parametrize("case", RESCALE, ids=ids(RESCALE))
def test_rescale_cases_rescale_where_predicted(case):
    assert case.tol is None
    predicted = R.rescale_steps(case.nu, case.max_iter * case.n)
    assert len(predicted) >= 1
    if case.nu == 1.0:
        assert case.max_iter == -(-681755 // case.n) + 2 and predicted[0] == 681755
    else:
        assert (case.nu, case.n, case.F, case.max_iter) == (0.5, 50176, 2, 37) and predicted == [1829034]
    if case.name in R.LOOP_FREE:
        return
    st = restated(case.name)[3]
    assert [s for s, _ in st.rescales] == predicted
    assert all(pos == (s - 1) % case.n for s, pos in st.rescales)


@pytest.mark.parametrize("case", [c for c in RESCALE if c.name not in R.LOOP_FREE], ids=ids([c for c in RESCALE if c.name not in R.LOOP_FREE]))
def test_a_fit_without_the_rescale_differs_from_sklearn(case):
    """What makes the bit-exact comparison a test of the branch: leaving it out changes coef_."""
    coef = restated(case.name, False)[0]
    assert not np.array_equal(coef.view(np.uint32), sk(case.name).coef_.view(np.uint32))


def test_rescale_positions_cover_the_chunk_and_both_epoch_ends():
    """Where step 681 755 falls in ocsvm_epoch_kernel's 64-sample chunks: lane 0 and lane 63 of a full chunk, inside the ragged
    last chunk, the last sample of an epoch and the first of the next (5 * 136 351 = 681 755, 2 * 340 877 = 681 754: both exist)."""
    def where(name):
        c = R.BY_NAME[name]
        (step, pos), = restated(name)[3].rescales
        assert step == 681755
        return c.n, pos
    n, pos = where("rescale-lane0")
    assert pos % 64 == 0 and pos + 64 <= n and pos > 0
    n, pos = where("rescale-lane63")
    assert pos % 64 == 63 and pos + 1 < n
    n, pos = where("rescale-ragged")
    assert n % 64 != 0 and pos >= n - n % 64 and 0 < pos % 64 < n % 64 - 1 and (n, pos) == (2228, 2214)
    n, pos = where("rescale-epoch-last")
    assert pos == n - 1 and 681755 % n == 0
    n, pos = where("rescale-epoch-first")
    assert pos == 0 and 681754 % n == 0
    assert sorted(R.BY_NAME[k].F for k in ("rescale-lane0", "rescale-lane63", "rescale-ragged", "rescale-epoch-last")) == [1, 2, 3, 4]


# ---------------------------------------------------------------------------------------------------------------- stop-rule group
def test_stop_rule_cases_stop_at_different_epochs():
    n_iters = {c.name: restated(c.name)[2] for c in STOP}
    late = {v for k, v in n_iters.items() if v != 6 and v != R.BY_NAME[k].max_iter}
    assert len(late) >= 4, n_iters
    fell_back = [c.name for c in STOP if any(a > 0 and b == 0 for a, b in zip(restated(c.name)[3].counter, restated(c.name)[3].counter[1:]))]
    assert fell_back, "no case where a later improvement resets the counter"
    assert n_iters["stop-tol0.1"] == 6


def test_stop_rule_and_max_iter_cases():
    free, capped = restated("stop-129x3"), restated("stop-at-max-iter")
    assert R.BY_NAME["stop-at-max-iter"].max_iter == free[2] == capped[2] and capped[3].stop == "rule" == free[3].stop
    np.testing.assert_array_equal(free[0], capped[0])
    one = restated("stop-max-iter-1")
    assert one[2] == 1 and one[3].stop == "max_iter" and one[3].counter == [0]
    c = R.BY_NAME["stop-tol-none-7"]
    seven = restated(c.name)
    assert c.tol is None and seven[2] == 7 and seven[3].stop == "max_iter" and seven[3].counter == [0] * 7
    assert restated("stop-64x2")[2] > 7                  # with the default tol the same rows go on past epoch 7


@pytest.mark.parametrize("k", [1, 2, 8])
def test_patience_cases_change_the_stopping_epoch(k):
    """n_iter_no_change in {1, 2, 8}: no scikit-learn side (its class has no such argument).  The restatement's counter logic is the
    one pinned above at 5; here: the fit stops at the first epoch whose counter reaches k, and the three differ from the default."""
    c = R.BY_NAME["patience-%d" % k]
    assert c.n_iter_no_change == k
    coef, _, n_iter, st = restated(c.name)
    print("\n" + R.table_line(c, n_iter, st))
    assert st.stop == "rule" and st.counter[-1] == k and max(st.counter[:-1], default=0) < k
    default = restated("stop-500x4")
    assert n_iter != default[2] and st.sumloss[:min(n_iter, default[2])] == default[3].sumloss[:min(n_iter, default[2])]


# ---------------------------------------------------------------------------------------------------------------- the other groups
def test_boundary_and_seed_groups_are_what_the_kernels_split_on():
    b = [c for c in R.CASES if c.group == "boundary"]
    assert sorted({c.n for c in b}) == [2, 3, 63, 64, 65, 66, 127, 128, 129, 16384, 16385, 16386, 16449]
    assert all(len({c.rs for c in b if c.n == n}) == 2 for n in R.BOUNDARY_N) and {c.F for c in b} == {1, 2, 3, 4}
    assert all(c.tol == 1e-3 and c.max_iter == 1000 for c in b)
    # n - 1 generator steps: 64 per thread, 16 384 per block
    assert {R.FY_THREAD, R.FY_THREAD + 1, R.FY_THREAD + 2, R.FY_BLOCK, R.FY_BLOCK + 1, R.FY_BLOCK + 2} <= {c.n for c in b}
    s = [c for c in R.CASES if c.group == "seed"]
    assert [c.rs for c in s] == [0, 1, 7, 42, 12345, 2 ** 31 - 2, (R.RNG_INSTANCE, 99)] and all(c.n == 1000 for c in s)
    seeds = [R.sgd_seed(R.random_state(c)) for c in s]
    assert len(set(seeds)) == len(seeds) and 0 not in seeds
    assert R.swap_targets(50, 0) == R.swap_targets(50, 1)   # our_rand_r: a zero state becomes 1


def test_tiny_scales_make_subnormal_products():
    for name in ("data-x1e-20", "data-x1e-22"):
        assert restated(name)[3].subnormal > 0, name
    assert restated("data-x1e3")[3].subnormal == 0
    big = restated("data-x1e19")[0]
    assert np.all(np.isfinite(big)) and np.abs(big).max() > 1e15


def test_non_finite_rows_raise_at_epoch_one_on_both_sides():
    from sklearn.linear_model import SGDOneClassSVM
    X = np.full((256, 2), 3e38, dtype=np.float32)
    with pytest.raises(ValueError, match="epoch #1"):
        SGDOneClassSVM(nu=0.5, random_state=42).fit(X)
    with pytest.raises(ValueError, match="epoch #1"):
        R.fit(X, 0.5, 1000, 1e-3, 42)
