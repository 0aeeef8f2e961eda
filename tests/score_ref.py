"""Float64 restatements of what runs after the nearest-neighbour keys exist (csrc/search_post.hip: cmdiad_l2_rescore,
cmdiad_l2_rescore2, cmdiad_l2_choose, cmdiad_score_head / _tail / _final; reference features.py:225-290).  TEST INFRASTRUCTURE
ONLY: plain numpy, one row at a time where that is the clearest way to say it, no code shared with cmdiad_amd.

Every function takes what the entry point takes -- keys as int64 planes (value bits << 32 | global row), the shard's window
[row_offset, row_offset + Nb) over GLOBAL rows, `bank` = the Nb rows of that window -- and the caller's PREFILLED outputs.  It
returns new arrays: the prefill where the contract says "untouched", float64 values elsewhere, plus a boolean mask of what was
written, so a test can compare the untouched part bit for bit and the written part within a bound.

Proved against oracle.scoring.single_s_s_map in tests/test_score_ref_cpu.py before it judges a kernel."""
import numpy as np

NO_CANDIDATE = 0x7F800000          # value fields at or above the bits of +inf: "no candidate" (ops.KEY_EMPTY is one of them)


def _np(x, dtype=None):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return x.astype(dtype) if dtype is not None else x


def split_keys(keys):
    """int64 keys -> (value field, global row), both as Python-int-safe uint64 arrays."""
    k = _np(keys, np.int64).view(np.uint64)
    return k >> np.uint64(32), k & np.uint64(0xFFFFFFFF)


def pack_key(d2, row):
    """(fp32 squared distance >= 0, global row) -> the int64 key the search would leave."""
    bits = int(np.array(d2, dtype=np.float32).view(np.uint32))
    return (bits << 32) | int(row)


def _owned(row, row_offset, Nb):
    return (row >= np.uint64(row_offset)) & (row < np.uint64(row_offset + Nb))


def _d2(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.dot(d, d))


def rescore(q, bank, keys, row_offset, Nb, prefill):
    """cmdiad_l2_rescore: rows whose key's low 32 bits lie in the window get (sqrt(sum (q - b)^2), that row); others stay.
    prefill = (min_val, min_idx) -> (min_val f64, min_idx i64, written bool)."""
    q, bank = _np(q), _np(bank)
    _, row = split_keys(keys)
    mv, mi = _np(prefill[0]).astype(np.float64), _np(prefill[1], np.int64).copy()
    own = _owned(row, row_offset, Nb)
    for r in np.nonzero(own)[0]:
        g = int(row[r])
        mv[r] = np.sqrt(_d2(q[r], bank[g - row_offset]))
        mi[r] = g
    return mv, mi, own


def pair_d2(q, bank, keys2, row_offset, Nb, prefill):
    """The d2_pair output of cmdiad_l2_rescore2: [2, Q] squared distances of the candidates that exist AND whose rows lie in
    the window; the rest stays.  -> (d2 f64 [2, Q], written bool [2, Q])."""
    q, bank = _np(q), _np(bank)
    keys2 = _np(keys2, np.int64)
    out = _np(prefill).astype(np.float64)
    written = np.zeros(out.shape, dtype=bool)
    for pl in range(2):
        val, row = split_keys(keys2[pl])
        own = (val < np.uint64(NO_CANDIDATE)) & _owned(row, row_offset, Nb)
        for r in np.nonzero(own)[0]:
            out[pl, r] = _d2(q[r], bank[int(row[r]) - row_offset])
        written[pl] = own
    return out, written


def decide(keys2, d2, usable2):
    """Which candidate wins per query: the nearer one, of equal squared distances the lower global row; the runner-up only
    where usable2 says it may be looked at.  -> bool [Q], True = the runner-up."""
    _, g1 = split_keys(_np(keys2, np.int64)[0])
    _, g2 = split_keys(_np(keys2, np.int64)[1])
    return usable2 & ((d2[1] < d2[0]) | ((d2[1] == d2[0]) & (g2 < g1)))


def rescore2(q, bank, keys2, row_offset, Nb, prefill):
    """The min_val / min_idx output of cmdiad_l2_rescore2: written only where the BEST candidate exists and is owned; the
    runner-up takes part only where it exists and is owned too.  -> (min_val f64, min_idx i64, written)."""
    keys2 = _np(keys2, np.int64)
    Q = keys2.shape[1]
    d2, wr = pair_d2(q, bank, keys2, row_offset, Nb, np.zeros((2, Q)))
    second = decide(keys2, d2, wr[1])
    rows = np.stack([split_keys(keys2[0])[1], split_keys(keys2[1])[1]]).astype(np.int64)
    mv, mi = _np(prefill[0]).astype(np.float64), _np(prefill[1], np.int64).copy()
    w = wr[0]
    pick = second.astype(np.int64)
    ar = np.arange(Q)
    mv[w] = np.sqrt(d2[pick, ar])[w]
    mi[w] = rows[pick, ar][w]
    return mv, mi, w


def choose(keys2, d2_pair, prefill):
    """cmdiad_l2_choose: the same decision from squared distances summed over the shards (compared as the fp32 numbers they
    are); rows without a best candidate stay.  -> (min_val f64, min_idx i64, written)."""
    keys2 = _np(keys2, np.int64)
    Q = keys2.shape[1]
    d2 = _np(d2_pair).astype(np.float64)
    has1 = split_keys(keys2[0])[0] < np.uint64(NO_CANDIDATE)
    has2 = split_keys(keys2[1])[0] < np.uint64(NO_CANDIDATE)
    second = decide(keys2, d2, has2)
    rows = np.stack([split_keys(keys2[0])[1], split_keys(keys2[1])[1]]).astype(np.int64)
    mv, mi = _np(prefill[0]).astype(np.float64), _np(prefill[1], np.int64).copy()
    pick = second.astype(np.int64)
    ar = np.arange(Q)
    mv[has1] = np.sqrt(d2[pick, ar])[has1]
    mi[has1] = rows[pick, ar][has1]
    return mv, mi, has1


def head(min_val, min_idx, patch, bank, row_offset, Nb, m_star_prefill):
    """cmdiad_score_head for [B, Q] minima: s_idx = FIRST arg-max of max(min_val, 0) (a NaN entry counts as 0, as fmax does),
    s_star = the RAW value there, m_test = patch[b, s_idx]; m_star[b] = bank[min_idx[b, s_idx] - row_offset] only where that row
    lies in the window.  -> dict(s_idx, s_star, m_test, m_star, m_star_written [B])."""
    mv, mi, patch, bank = _np(min_val), _np(min_idx, np.int64), _np(patch), _np(bank)
    B = mv.shape[0]
    m_star = _np(m_star_prefill).copy()
    key = np.fmax(mv.astype(np.float64), 0.0)
    s_idx = np.array([int(np.argmax(key[b])) for b in range(B)], dtype=np.int64)
    s_star = mv[np.arange(B), s_idx]
    m_test = patch[np.arange(B), s_idx]
    g = mi[np.arange(B), s_idx] - row_offset
    wr = (g >= 0) & (g < Nb)
    for b in np.nonzero(wr)[0]:
        m_star[b] = bank[g[b]]
    return dict(s_idx=s_idx, s_star=s_star, m_test=m_test, m_star=m_star, m_star_written=wr)


def tail(m_test, top3, bank, row_offset, Nb, prefill):
    """cmdiad_score_tail: knn_d[b, k - 1] = || m_test[b] - bank[row(top3[b, k])] || for k = 1, 2 where that row lies in the
    window (features.py:285); the rest stays.  -> (knn_d f64 [B, 2], written bool [B, 2])."""
    m_test, bank = _np(m_test), _np(bank)
    _, row = split_keys(top3)
    out = _np(prefill).astype(np.float64)
    wr = _owned(row[:, 1:], row_offset, Nb)
    for b, k in zip(*np.nonzero(wr)):
        out[b, k] = np.sqrt(_d2(m_test[b], bank[int(row[b, k + 1]) - row_offset]))
    return out, wr


def final(s_star, knn_d, D):
    """features.py:286-290 in float64: s = (1 - exp(s* / sqrt(D)) / sum_k exp(knn_k / sqrt(D))) * s*.  -> (s, w, ratio)."""
    s_star, knn = _np(s_star).astype(np.float64), _np(knn_d).astype(np.float64)
    rd = np.sqrt(np.float64(D))
    with np.errstate(over="ignore", invalid="ignore"):
        ratio = np.exp(s_star / rd) / np.exp(knn / rd).sum(axis=1)
        w = 1.0 - ratio
    return w * s_star, w, ratio
