"""CPU: the float64 reference of the score head / tail / re-score kernels (tests/score_ref.py) against the project's restatement of
the reference composition, oracle.scoring.single_s_s_map, fed a float64 distance matrix -- the proof of the yardstick that
tests/test_gpu_score_tail.py holds the HIP kernels to.  No GPU, no cmdiad_amd import.

What is compared: s_idx and nn_idx exactly; min_idx exactly; s_star, m_star_knn and s to float32 round-off (the oracle takes
sqrt(D) as a float32 tensor, scoring.py:82, so its exponent arguments carry one float32 rounding: |arg| * 2^-24 relative on each
exp, which the bound on s below states).  The same data is then run through the reference's SHARDED composition (d2_pair summed
over the shards + choose, m_star and knn_d summed over their owners): identical to the unsharded one, because exactly one shard
contributes a non-zero to every sum."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

U = 2.0 ** -24
CASES = [(16, 3, 4, 0), (16, 50, 100, 1), (49, 300, 768, 2), (49, 7, 260, 3), (4, 129, 1152, 4)]


def _data(Q, Nb, D, seed, dup_max=False):
    g = np.random.default_rng(seed)
    bank = g.standard_normal((Nb, D)).astype(np.float32)
    q = (bank[g.integers(0, Nb, Q)] + 0.4 * g.standard_normal((Q, D))).astype(np.float32)
    if dup_max:   # the farthest query twice more: the maximum of min_val then occurs three times, the first one must win
        d = np.sqrt(((q[:, None].astype(np.float64) - bank[None].astype(np.float64)) ** 2).sum(-1)).min(1)
        far = int(np.argmax(d))
        lo, hi = (far + 1) % Q, (far + Q // 2) % Q
        q[lo] = q[far]
        q[hi] = q[far]
    return q, bank


def _keys_from_dist(d2):
    """Best and runner-up (by float64 squared distance, ties to the lower row) as packed keys; a library of one row has no
    runner-up."""
    Q, Nb = d2.shape
    order = np.lexsort((np.broadcast_to(np.arange(Nb), d2.shape), d2), axis=1)
    keys = np.full((2, Q), 0x7FFFFFFFFFFFFFFF, dtype=np.int64)
    for r in range(Q):
        keys[0, r] = sr.pack_key(d2[r, order[r, 0]], order[r, 0])
        if Nb > 1:
            keys[1, r] = sr.pack_key(d2[r, order[r, 1]], order[r, 1])
    return keys


def _top3(m_star, bank):
    d2 = ((m_star[:, None].astype(np.float64) - bank[None].astype(np.float64)) ** 2).sum(-1)
    B, Nb = d2.shape
    top = np.full((B, 3), 0x7FFFFFFFFFFFFFFF, dtype=np.int64)
    for b in range(B):
        order = np.lexsort((np.arange(Nb), d2[b]))[:3]
        for k, row in enumerate(order):
            top[b, k] = sr.pack_key(d2[b, row], row)
    return top


def _compose(q, bank, keys, shards):
    """The reference helpers in the order the engine calls the kernels, over `shards` = [(row_offset, Nb), ...]."""
    Q, D = q.shape
    d2 = np.zeros((2, Q))
    owners = np.zeros((2, Q), dtype=int)
    for off, n in shards:
        part, wr = sr.pair_d2(q, bank[off:off + n], keys, off, n, np.zeros((2, Q)))
        d2 += part
        owners += wr
    mv, mi, wr = sr.choose(keys, d2.astype(np.float32), (np.zeros(Q, np.float32), np.full(Q, -1, np.int64)))
    assert wr.all() and (owners[0] == 1).all()          # every best candidate has exactly one owner
    m_star = np.zeros((1, D), np.float32)
    writers = 0
    for off, n in shards:
        h = sr.head(mv[None].astype(np.float32), mi[None], q[None], bank[off:off + n], off, n, np.zeros((1, D), np.float32))
        m_star += h["m_star"]
        writers += int(h["m_star_written"][0])
    assert writers == 1
    top3 = _top3(m_star, bank)
    knn = np.zeros((1, 2))
    for off, n in shards:
        part, wr = sr.tail(h["m_test"], top3, bank[off:off + n], off, n, np.zeros((1, 2)))
        knn += part
    s, w, ratio = sr.final(h["s_star"], knn, D)
    return dict(min_val=mv, min_idx=mi, s_idx=h["s_idx"][0], s_star=h["s_star"][0], nn_idx=sr.split_keys(top3)[1][0].astype(np.int64),
                knn=knn[0], s=s[0], ratio=ratio[0])


@pytest.mark.parametrize("Q,Nb,D,seed", CASES)
@pytest.mark.parametrize("dup_max", [False, True])
def test_reference_equals_oracle_composition(Q, Nb, D, seed, dup_max):
    from oracle import scoring
    q, bank = _data(Q, Nb, D, seed, dup_max)
    d2 = ((q[:, None].astype(np.float64) - bank[None].astype(np.float64)) ** 2).sum(-1)
    keys = _keys_from_dist(d2)
    side = int(round(Q ** 0.5))
    tq, tb = torch.from_numpy(q).double(), torch.from_numpy(bank).double()
    want = scoring.single_s_s_map(tq, torch.from_numpy(np.sqrt(d2)), tb, (side, side), gt_size=8, blur=False)
    got = _compose(q, bank, keys, [(0, Nb)])
    assert got["s_idx"] == int(want["s_idx"])
    if dup_max:
        assert (np.sqrt(d2).min(1) == np.sqrt(d2).min(1).max()).sum() == 3       # the case is what it claims to be
    np.testing.assert_array_equal(got["min_idx"], want["min_idx"].numpy())
    np.testing.assert_array_equal(got["nn_idx"], want["nn_idx"].numpy())
    # min_val went through the float32 d2_pair of the sharded protocol: one rounding of the squared distance
    np.testing.assert_allclose(got["min_val"], want["min_val"].numpy(), rtol=2 * U, atol=0)
    np.testing.assert_allclose(got["s_star"], float(want["s_star"]), rtol=2 * U, atol=0)
    np.testing.assert_allclose(got["knn"], want["m_star_knn"].numpy(), rtol=2 * U, atol=0)
    # s = (1 - ratio) s*: s* and the knn distances carry 2u, the oracle's float32 sqrt(D) one more u on every exponent argument
    arg = max(abs(got["s_star"]), *np.abs(got["knn"])) / np.sqrt(D)
    bound = abs(got["s_star"]) * (got["ratio"] * 2 * (3 * arg * U) + 2 * U * abs(1 - got["ratio"])) + 1e-300
    assert abs(got["s"] - float(want["s"])) <= bound, (got["s"], float(want["s"]), bound)
    # the sharded composition is the unsharded one
    for W in (2, 3):
        per = -(-Nb // W)
        shards = [(min(w * per, Nb), min((w + 1) * per, Nb) - min(w * per, Nb)) for w in range(W)] + [(Nb, 0)]
        sh = _compose(q, bank, keys, shards)
        for k in got:
            np.testing.assert_array_equal(sh[k], got[k], err_msg=k)


def test_rescore_contract_windows_and_absent_candidates():
    """Hand-built keys: ownership windows, absent candidates, the tie rule -- the rules of csrc/search_post.hip's header comment,
    on numbers small enough to check by eye."""
    E = 0x7FFFFFFFFFFFFFFF
    bank = np.array([[0, 0, 0, 0], [3, 4, 0, 0], [5, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    q = np.zeros((5, 4), np.float32)
    k = sr.pack_key
    keys = np.array([[k(25, 2), k(25, 1), k(1, 3), E, k(0, 0)],
                     [k(25, 1), k(25, 2), E, k(1, 3), k(1, 3)]], dtype=np.int64)
    pre = (np.full(5, -7.0, np.float32), np.full(5, -9, np.int64))
    mv, mi, wr = sr.rescore2(q, bank, keys, 0, 4, pre)
    np.testing.assert_array_equal(wr, [True, True, True, False, True])
    np.testing.assert_array_equal(mi, [1, 1, 3, -9, 0])          # rows 1 and 2 are both at distance 5: the lower row
    np.testing.assert_array_equal(mv, [5, 5, 1, -7, 0])
    # window [1, 3): owns rows 1 and 2 only
    d2, w2 = sr.pair_d2(q, bank[1:3], keys, 1, 2, np.full((2, 5), -1.0, np.float32))
    np.testing.assert_array_equal(w2, [[True, True, False, False, False], [True, True, False, False, False]])
    np.testing.assert_array_equal(d2, [[25, 25, -1, -1, -1], [25, 25, -1, -1, -1]])
    mv, mi, wr = sr.rescore2(q, bank[1:3], keys, 1, 2, pre)
    np.testing.assert_array_equal(wr, [True, True, False, False, False])
    mv, mi, wr = sr.rescore(q, bank[1:3], keys[0], 1, 2, pre)
    np.testing.assert_array_equal(mi, [2, 1, -9, -9, -9])
    np.testing.assert_array_equal(mv, [5, 5, -7, -7, -7])
    mv, mi, wr = sr.choose(keys, np.array([[25, 25, 1, 99, 0], [25, 25, 99, 1, 1]], np.float32), pre)
    np.testing.assert_array_equal(mi, [1, 1, 3, -9, 0])
    np.testing.assert_array_equal(mv, [5, 5, 1, -7, 0])


def test_head_first_argmax_clamp_and_nan():
    mv = np.array([[1, 7, 7, 2], [-3, -1, -2, -5], [np.nan, 2, np.nan, 2], [-0.0, 0, 0, 0]], np.float32)
    mi = np.array([[0, 1, 2, 0], [2, 2, 2, 2], [0, 3, 0, 0], [-1, 0, 0, 0]], np.int64)
    patch = np.arange(4 * 4 * 2, dtype=np.float32).reshape(4, 4, 2)
    bank = 100 + np.arange(8, dtype=np.float32).reshape(4, 2)
    h = sr.head(mv, mi, patch, bank[1:3], 1, 2, np.full((4, 2), -1, np.float32))
    np.testing.assert_array_equal(h["s_idx"], [1, 0, 1, 0])
    np.testing.assert_array_equal(h["s_star"], [7, -3, 2, 0])            # the raw value, not the clamped one
    assert np.signbit(h["s_star"][3])
    np.testing.assert_array_equal(h["m_test"], patch[np.arange(4), [1, 0, 1, 0]])
    np.testing.assert_array_equal(h["m_star_written"], [True, True, False, False])   # row 3: outside; -1: nobody's
    np.testing.assert_array_equal(h["m_star"], [bank[1], bank[2], [-1, -1], [-1, -1]])
