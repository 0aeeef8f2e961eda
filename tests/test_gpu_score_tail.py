"""GPU: what runs after the nearest-neighbour keys exist (csrc/search_post.hip) -- cmdiad_l2_rescore / _rescore2 / _choose and
cmdiad_score_head / _tail / _final -- called DIRECTLY with hand-built keys (ops.new_keys, KEY_EMPTY, tests/score_ref.pack_key), not
with searched ones, against the float64 restatement tests/score_ref.py (itself proved in tests/test_score_ref_cpu.py).  Every output
buffer is prefilled with a canary; wherever the contract says "untouched" the canary must still be there, bit for bit.

Everything that is a copy, an index or a decision is compared EXACTLY (s_idx, min_idx, m_test, m_star, s_star, which entries a
shard writes, sharded == unsharded).  The arithmetic is compared within bounds DERIVED from fp32, u = 2^-24, none read off the kernels:

  Squared distance, sum_{c < D} (a_c - b_c)^2 in any order, with or without FMA.  a_c - b_c is rounded once (1 + u), the square
  carries that twice plus its own rounding, a sum of D non-negative terms adds at most (D - 1) roundings to each: relative error
  <= (D + 3) u (first order; the terms are non-negative, so there is no cancellation).                                   D2_REL(D)
  The distance: sqrt halves the relative error and rounds once more:  (D + 3) u / 2 + u.                                 DIST_REL(D)

  score_final, s = w s*, w = 1 - r, r = exp(a) / (exp(b0) + exp(b1)), a = s*/sqrt(D), b_k = knn_k/sqrt(D):
    sqrtf((float)D) and the division are correctly rounded: each argument x carries 2u relative, i.e. 2|x|u ABSOLUTE, which exp
    turns into 2|x|u RELATIVE;  expf itself is within 1 ulp = 2u relative (HIP math API reference, single precision floating-point
    table: "expf -- maximum ULP error 1"; that table is part of the published HIP documentation, the ROCm tree ships the
    functions without it);  the sum of two positive numbers keeps the larger of their relative errors and adds u;  the division adds
    u.  So r has relative error <= (2|a| + 2) u + (2 max|b| + 2) u + 2u, rounded up to (2|a| + 2 max|b| + 8) u for the second-order
    terms;  1 - r adds u |w| absolutely, the last product u |w s*|:
        |w_kernel - w| <= r (2|a| + 2 max|b| + 8) u + u |w|          -- proportional to the ratio
        |s_kernel - s| <= |s*| (r (2|a| + 2 max|b| + 8) u + 2u |w|)                                                       final_bound()
    Beyond the range of fp32 exp (an argument above 88.72, or a sum above FLT_MAX) the expected value is what the reference's own
    fp32 expression (oracle/scoring.py:82-84) gives on the CPU, compared with equal_nan; the cases are built so that this value is
    NaN, -inf or s* itself -- it does not depend on the last bit of any exp.

The derived bounds are loose (a squared distance of D = 1920 terms is allowed 1.1e-4 relative, the kernels' pairwise order achieves
far less); they stay as derived."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ref as sr  # noqa: E402

from cmdiad_amd import engine as eng  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
E = ops.KEY_EMPTY
CANARY_F, CANARY_I = -12345.5, -777
FLT_MAX = float(np.finfo(np.float32).max)


def D2_REL(D):
    return (D + 3) * U


def DIST_REL(D):
    return (D + 3) * U / 2 + U


def _dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _bits(t):
    """float32 tensor / array -> int32 bit patterns on the host (NaN- and sign-of-zero-safe equality)."""
    a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.int32)


def _same_bits(got, want, what=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _close(got, want, rel, what, floor=0.0):
    """|got - want| <= rel * |want| (+ floor) element-wise; prints the achieved maximum (information only)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.size == 0:
        return
    err = np.abs(got - want)
    lim = rel * np.abs(want) + floor
    with np.errstate(divide="ignore", invalid="ignore"):
        ach = np.nanmax(np.where(want != 0, err / np.abs(want), 0.0))
    print(f"ACHIEVED {what}: max rel err {ach:.3e} (bound {np.max(rel):.3e})")
    assert (err <= lim).all(), (what, float(err.max()), float(lim[np.argmax(err - lim)]))


def _shards(Nb, W):
    """W contiguous shards of Nb rows and one EMPTY shard at the end: [(row_offset, rows), ...]."""
    per = -(-Nb // W)
    out = [(min(w * per, Nb), min((w + 1) * per, Nb) - min(w * per, Nb)) for w in range(W)]
    return out + [(Nb, 0)]


# ------------------------------------------------------------------------------------------------------------ re-score family
NB = 37
DUP_LO, DUP_HI, TIE_LO, TIE_HI = 5, 20, 9, 30
NKIND = 12


def _rescore_case(Q, D, rot, seed):
    """bank [NB, D], q [Q, D], keys [2, Q]; query r is of kind (r + rot) % NKIND:
      0 best = first row, runner-up = last row     1 the other way round       2 best and runner-up name the SAME row
      3 runner-up empty (odd queries: absent by its value field, +inf bits, while naming the row NEAREST to the query)
                                                   4 both empty                5 best absent (value field = +inf bits), runner-up real
      6 exact duplicate rows, g2 < g1              7 duplicates, g1 < g2
      8 / 9 rows that DIFFER but are equally far in fp32: the query is an integer vector c, the rows are c + (3, 4, 0, 0, ...) and
            c + (5, 0, 0, 0, ...) with |c_i| <= 8: every difference, square and partial sum is a small integer, exact in fp32 AND
            in float64 in any summation order -- both squared distances are exactly 25, a tie in both arithmetics (8: g2 < g1)
      10 / 11 two random rows (11: the best key's value field is the largest FINITE pattern 0x7F7FFFFF: still a candidate)"""
    g = np.random.default_rng(seed)
    bank = g.standard_normal((NB, D)).astype(np.float32)
    bank[DUP_HI] = bank[DUP_LO]
    c = g.integers(-8, 9, D).astype(np.float32)
    bank[TIE_LO] = c
    bank[TIE_LO, :2] += (3, 4)
    bank[TIE_HI] = c
    bank[TIE_HI, 0] += 5
    q = (bank[g.integers(0, NB, Q)] + 0.5 * g.standard_normal((Q, D))).astype(np.float32)
    keys = np.full((2, Q), E, dtype=np.int64)
    free = [r for r in range(NB) if r not in (DUP_LO, DUP_HI, TIE_LO, TIE_HI)]
    for r in range(Q):
        kind = (r + rot) % NKIND
        v1, v2 = np.float32(1.0 + r % 97), np.float32(0.25 + r % 89)       # the search's 16-bit estimates: must not matter
        a, b = (int(x) for x in g.choice(free, 2, replace=False))
        pairs = {0: (0, NB - 1), 1: (NB - 1, 0), 2: (a, a), 3: (a, None), 4: (None, None), 5: (a, b), 6: (DUP_HI, DUP_LO),
                 7: (DUP_LO, DUP_HI), 8: (TIE_HI, TIE_LO), 9: (TIE_LO, TIE_HI), 10: (a, b), 11: (a, b)}[kind]
        if kind in (8, 9):
            q[r] = c
        if pairs[0] is not None:
            keys[0, r] = sr.pack_key(v1, pairs[0])
        if pairs[1] is not None:
            keys[1, r] = sr.pack_key(v2, pairs[1])
        if kind == 5:
            keys[0, r] = (0x7F800000 << 32) | a
        if kind == 3 and r % 2:
            q[r] = bank[b] + np.float32(0.01) * g.standard_normal(D).astype(np.float32)
            keys[1, r] = (0x7F800000 << 32) | b
        if kind == 11:
            keys[0, r] = (0x7F7FFFFF << 32) | a
    # "min_idx is exact" needs candidates that are either exactly as far in float64 or further apart than the summation bound
    # can bridge (the test asserts it on the input): a query that sits too close to the bisector is moved towards its runner-up
    for _ in range(8):
        d2, has = sr.pair_d2(q, bank, keys, 0, NB, np.zeros((2, Q)))
        gap = np.abs(d2[0] - d2[1])
        bad = has[0] & has[1] & (gap != 0) & (gap <= 4 * D2_REL(D) * np.maximum(d2[0], d2[1]))
        if not bad.any():
            break
        rows = sr.split_keys(keys)[1].astype(np.int64)
        q[bad] += np.float32(0.25) * (bank[rows[1, bad]] - bank[rows[0, bad]])
    return bank, q, keys


def _raw_rescore2(q, bank_view, rows, keys, off, d2, mv, mi):
    """cmdiad_l2_rescore2 with an explicit window [off, off + rows) whose rows start at bank_view (a view INTO the whole library)."""
    ops._call("cmdiad_l2_rescore2", ops._p(q), ops._p(bank_view), ops._p(keys[0]), ops._p(keys[1]), q.shape[0], rows, q.shape[1], off,
              ops._p(d2), ops._p(mv), ops._p(mi), ops._stream())


@pytest.mark.parametrize("Q", [1, 3, 5, 784, 3137])
@pytest.mark.parametrize("D", [4, 64, 260, 768, 1152, 1920])
def test_rescore_family_hand_built_keys(D, Q):
    for rot in range(0, NKIND, min(Q, NKIND)):
        bank, q, keys = _rescore_case(Q, D, rot, 1000 * D + Q)
        # precondition of "min_idx is exact", asserted on the INPUT: two candidates are either exactly as far in float64 or further
        # apart than twice the summation bound, so no correct fp32 summation order can decide differently
        d2_all, has = sr.pair_d2(q, bank, keys, 0, NB, np.zeros((2, Q)))
        both = has[0] & has[1]
        gap = np.abs(d2_all[0] - d2_all[1])[both]
        assert ((gap == 0) | (gap > 2 * D2_REL(D) * np.maximum(d2_all[0], d2_all[1])[both])).all()
        tq, tb, tk = _dev(q), _dev(bank), _dev(keys)
        canary = lambda: (torch.full((Q,), CANARY_F, device=DEV), torch.full((Q,), CANARY_I, dtype=torch.int64, device=DEV))  # noqa: E731
        pre = (np.full(Q, CANARY_F, np.float32), np.full(Q, CANARY_I, np.int64))

        # --- both candidates, one device: ops.l2_rescore on [2, Q] keys
        mv, mi = canary()
        ops.l2_rescore(tq, tb, tk, mv, mi)
        wv, wi, wr = sr.rescore2(q, bank, keys, 0, NB, pre)
        np.testing.assert_array_equal(mi.cpu().numpy(), wi)                     # rows AND canaries
        _same_bits(mv.cpu().numpy()[~wr], wv[~wr], "rescore2 min_val canary")
        _close(mv.cpu().numpy()[wr], wv[wr], DIST_REL(D), f"rescore2 min_val D={D} Q={Q}")
        kinds = (np.arange(Q) + rot) % NKIND
        assert not wr[(kinds == 4) | (kinds == 5)].any() and wr[(kinds != 4) & (kinds != 5)].all()
        for kk, row in ((6, DUP_LO), (7, DUP_LO), (8, TIE_LO), (9, TIE_LO)):    # the lower row of equals
            assert (mi.cpu().numpy()[kinds == kk] == row).all()

        # --- the d2_pair mode
        d2 = torch.full((2, Q), CANARY_F, device=DEV)
        ops.l2_rescore_pair_d2(tq, tb, tk, d2)
        w2, w2r = sr.pair_d2(q, bank, keys, 0, NB, np.full((2, Q), CANARY_F, np.float32))
        _same_bits(d2.cpu().numpy()[~w2r], w2[~w2r], "d2_pair canary")
        _close(d2.cpu().numpy()[w2r], w2[w2r], D2_REL(D), f"d2_pair D={D} Q={Q}")
        assert not w2r[:, kinds == 4].any()

        # --- the winner alone: ops.l2_rescore on [Q] keys (only the low 32 bits of a key matter)
        mv1, mi1 = canary()
        k0 = tk[0].contiguous()
        ops.l2_rescore(tq, tb, k0, mv1, mi1)
        wv1, wi1, wr1 = sr.rescore(q, bank, keys[0], 0, NB, pre)
        np.testing.assert_array_equal(mi1.cpu().numpy(), wi1)
        _same_bits(mv1.cpu().numpy()[~wr1], wv1[~wr1], "rescore min_val canary")
        _close(mv1.cpu().numpy()[wr1], wv1[wr1], DIST_REL(D), f"rescore min_val D={D} Q={Q}")

        # --- shards: every shard writes exactly what it owns; sum + choose == the unsharded decision, bit for bit
        for W in (2, 3, 8):
            total = torch.zeros((2, Q), device=DEV)
            seen = np.zeros((2, Q), dtype=int)
            for off, n in _shards(NB, W):
                view = tb[off:off + n] if n else tb          # (an empty window: the pointer is not used)
                part = torch.full((2, Q), CANARY_F, device=DEV)
                _raw_rescore2(tq, view, n, tk, off, part, None, None)
                ws, wsr = sr.pair_d2(q, bank[off:off + n], keys, off, n, np.full((2, Q), CANARY_F, np.float32))
                got = part.cpu().numpy()
                np.testing.assert_array_equal(got != np.float32(CANARY_F), wsr)             # ownership, exactly
                _close(got[wsr], ws[wsr], D2_REL(D), f"shard d2 W={W} off={off}")
                seen += wsr
                total += torch.where(part == CANARY_F, torch.zeros_like(part), part)
                # the decision of a shard: only where it owns the best candidate
                smv, smi = canary()
                _raw_rescore2(tq, view, n, tk, off, None, smv, smi)
                _, wsi, wsw = sr.rescore2(q, bank[off:off + n], keys, off, n, pre)
                np.testing.assert_array_equal(smi.cpu().numpy(), wsi)
                _same_bits(smv.cpu().numpy()[~wsw], pre[0][~wsw], "shard min_val canary")
                # single-plane re-score of the shard
                rmv, rmi = canary()
                ops._call("cmdiad_l2_rescore", ops._p(tq), ops._p(view), ops._p(k0), Q, n, D, off, ops._p(rmv), ops._p(rmi),
                          ops._stream())
                _, rwi, rww = sr.rescore(q, bank[off:off + n], keys[0], off, n, pre)
                np.testing.assert_array_equal(rmi.cpu().numpy(), rwi)
                _same_bits(rmv.cpu().numpy()[~rww], pre[0][~rww], "shard rescore canary")
            np.testing.assert_array_equal(seen, has.astype(int))        # every existing candidate: exactly one owner
            cmv, cmi = canary()
            ops.l2_choose(tk, total, cmv, cmi)
            assert torch.equal(cmi, mi)
            _same_bits(cmv, mv, f"sum over {W} shards + choose vs unsharded")
            xv, xi, xw = sr.choose(keys, total.cpu().numpy(), pre)
            np.testing.assert_array_equal(cmi.cpu().numpy(), xi)
            _close(cmv.cpu().numpy()[xw], xv[xw], 2 * U, "choose sqrt")


# ------------------------------------------------------------------------------------------------------------------ score_head
NB_HEAD, HK = 50, 10
WIN = (13, 20)           # a shard's window [13, 33)
OUTSIDE, INSIDE = 40, 17


def _head_case(B, Q, rot, seed):
    g = np.random.default_rng(seed)
    mv = (3.0 * g.standard_normal((B, Q)) + 10.0).astype(np.float32)
    mv[:, ::7] *= -1                                                     # negative entries everywhere
    mi = g.integers(0, NB_HEAD, (B, Q)).astype(np.int64)
    top = np.float32(1000.0)
    for b in range(B):
        kind = (b + rot) % HK
        i = (7 * b + 3) % max(1, Q - 256)
        if kind == 0 and Q > 256 + i:          # twice on ONE thread's stride
            pos = (i, i + 256)
        elif kind == 1 and Q > 64 + (i % 64):  # twice, in different waves
            pos = (i % 64, i % 64 + 64)
        elif kind in (0, 1, 2):
            pos = (0, Q - 1)
        elif kind == 3:                        # all equal
            mv[b] = 4.25
            pos = ()
        elif kind == 4:                        # all zero
            mv[b] = 0.0
            pos = ()
        elif kind == 5:                        # nothing positive, one -0.0 behind index 0: the clamp makes them all equal
            mv[b] = -np.abs(mv[b]) - 1
            mv[b, min(1, Q - 1)] = -0.0
            pos = ()
        elif kind == 6:                        # a unique maximum, in the block's LAST wave where the row is long enough
            pos = (min(Q - 1, 192 + b % 64),) if Q > 192 else (Q // 2,)
        elif kind == 7:                        # NaN among finite ones, in front of, between and behind the two maxima
            pos = (Q // 3, Q - 1) if Q > 2 else (0, Q - 1)
            mv[b, ::5] = np.nan
        else:                                  # 8: the winner names no row; 9: the winner's row lies outside the window
            pos = (Q // 4, (Q // 4 + 64) % Q)
        for p in pos:
            mv[b, p] = top
        if pos:
            first = min(pos)
            mi[b, list(pos)] = g.choice(NB_HEAD, len(set(pos)), replace=False) if len(set(pos)) > 1 else INSIDE
            if kind == 8:
                mi[b, first] = -1
            elif kind == 9:
                mi[b, first] = OUTSIDE
                if max(pos) != first:
                    mi[b, max(pos)] = INSIDE
    return mv, mi


@pytest.mark.parametrize("D", [4, 100, 768, 1152])
@pytest.mark.parametrize("Q", [1, 63, 255, 256, 257, 784, 1369, 3136])
@pytest.mark.parametrize("B", [1, 6, 33])
def test_score_head_first_argmax_and_gathers(B, Q, D):
    gen = torch.Generator(device=DEV).manual_seed(B * 100000 + Q * 10 + D)
    patch = torch.randn((B, Q, D), generator=gen, device=DEV)
    bank = torch.randn((NB_HEAD, D), generator=gen, device=DEV)
    hp, hb = patch.cpu().numpy(), bank.cpu().numpy()
    for rot in range(0, HK, min(B, HK)):
        mv, mi = _head_case(B, Q, rot, B * 7 + Q * 3 + D + rot)
        tmv, tmi = _dev(mv.reshape(-1)), _dev(mi.reshape(-1))
        for off, n in ((0, NB_HEAD), WIN, (NB_HEAD, 0)):
            view = bank[off:off + n] if n else bank
            m_star = torch.full((B, D), CANARY_F, device=DEV)
            s_star, s_idx, m_test = ops.score_head(tmv, tmi, patch, view, m_star, off, n)
            want = sr.head(mv, mi, hp, hb[off:off + n], off, n, np.full((B, D), CANARY_F, np.float32))
            ctx = f"B={B} Q={Q} D={D} rot={rot} window=({off},{n})"
            np.testing.assert_array_equal(s_idx.cpu().numpy(), want["s_idx"], err_msg=ctx)
            _same_bits(s_star, want["s_star"], ctx + " s_star")
            _same_bits(m_test, want["m_test"], ctx + " m_test")
            _same_bits(m_star, want["m_star"], ctx + " m_star (rows of their owner, canary elsewhere)")
            kinds = (np.arange(B) + rot) % HK
            assert not want["m_star_written"][kinds == 8].any()
            if (off, n) == WIN:
                assert not want["m_star_written"][kinds == 9].any()


# ------------------------------------------------------------------------------------------------------------------ score_tail
NB_TAIL = 41


@pytest.mark.parametrize("D", [4, 100, 320, 768, 1152])
def test_score_tail_windows_and_empty_keys(D):
    g = np.random.default_rng(D)
    bank = g.standard_normal((NB_TAIL, D)).astype(np.float32)
    L = NB_TAIL - 1
    rows = [(3, 0, L), (3, L, 0), (3, None, None), (3, 5, None), (None, 7, 8), (2, 19, 20), (2, 20, 19), (0, 13, 14), (L, 27, 28),
            (1, 12, 12), (4, None, 33)]
    B = len(rows)
    m_test = (bank[g.integers(0, NB_TAIL, B)] + 0.7 * g.standard_normal((B, D))).astype(np.float32)
    top3 = np.array([[E if r is None else sr.pack_key(0.5 + k, r) for k, r in enumerate(t)] for t in rows], dtype=np.int64)
    s_star = _dev(np.full(B, 3.0, np.float32))
    tm, tt, tb = _dev(m_test), _dev(top3), _dev(bank)
    # one device: canary where a key is empty
    knn = torch.full((B, 2), CANARY_F, device=DEV)
    ops.score_tail(s_star, tm, tt, tb, knn)
    want, wr = sr.tail(m_test, top3, bank, 0, NB_TAIL, np.full((B, 2), CANARY_F, np.float32))
    np.testing.assert_array_equal(wr, [[r is not None for r in t[1:]] for t in rows])
    _same_bits(knn.cpu().numpy()[~wr], want[~wr], "knn_d canary (KEY_EMPTY)")
    _close(knn.cpu().numpy()[wr], want[wr], DIST_REL(D), f"knn_d D={D}")
    whole = ops.score_tail(s_star, tm, tt, tb, torch.zeros((B, 2), device=DEV))
    # shards: [0,20)+[20,41) splits image 5's and 6's rows; three shards split 13|14 and 27|28
    for shards in ([(0, 20), (20, 21), (NB_TAIL, 0)], [(0, 14), (14, 14), (28, 13), (NB_TAIL, 0)], _shards(NB_TAIL, 8)):
        total = torch.zeros((B, 2), device=DEV)
        seen = np.zeros((B, 2), dtype=int)
        for off, n in shards:
            view = tb[off:off + n] if n else tb
            part = torch.full((B, 2), CANARY_F, device=DEV)
            ops.score_tail(s_star, tm, tt, view, part, off, n)
            ws, wsr = sr.tail(m_test, top3, bank[off:off + n], off, n, np.full((B, 2), CANARY_F, np.float32))
            got = part.cpu().numpy()
            np.testing.assert_array_equal(got != np.float32(CANARY_F), wsr)
            _close(got[wsr], ws[wsr], DIST_REL(D), f"shard knn_d off={off}")
            seen += wsr
            total += torch.where(part == CANARY_F, torch.zeros_like(part), part)
        np.testing.assert_array_equal(seen, wr.astype(int))
        _same_bits(total, whole, "knn_d summed over the shards vs one device")


# ----------------------------------------------------------------------------------------------------------------- score_final
# (a, b0, b1) = the exponent arguments s*/sqrt(D), knn0/sqrt(D), knn1/sqrt(D); the inputs are these times sqrt(D), rounded to fp32
LN2 = float(np.log(2.0))
FINITE = [
    (0.44, 0.40, 0.50), (0.29, 0.34, 0.26), (1.08, 0.90, 1.01), (0.0, 0.3, 0.4), (-0.2, 0.3, 0.1), (2.5, 2.0, 3.5),       # ordinary: O(10)
    (0.5, 0.5 - LN2, 0.5 - LN2), (3.0, 3.0 - LN2, 3.0 - LN2), (0.7, 0.7 - 1e-4, 0.7 - 12.0), (20.0, 20.0 - LN2, 20.0 - LN2),  # r ~ 1
    (1.0, 1.0 - LN2 + 1e-5, 1.0 - LN2 - 1e-5), (6.0, 1.0, 2.0), (40.0, 40.0, 40.0 - 1e-3),
    (88.0, 87.9, 87.5), (87.0, 88.0, 50.0), (88.0, 10.0, 20.0), (-20.0, -22.0, -30.0),                                      # near the end of exp's range
]
OVERFLOW = [
    (89.0, 10.0, 10.0), (10.0, 89.0, 10.0), (10.0, 10.0, 89.0), (89.0, 89.0, 10.0), (100.0, 100.0, 100.0), (1000.0, 1.0, 2000.0),
    (80.0, 88.5, 88.5), (88.5, 88.5, 88.5), (120.0, 95.0, 0.0),
]


def final_bound(s_star, knn, D):
    s_star, knn = np.asarray(s_star, np.float64), np.asarray(knn, np.float64)
    _, w, r = sr.final(s_star, knn, D)
    rd = np.sqrt(float(D))
    x = 2 * np.abs(s_star) / rd + 2 * np.abs(knn).max(axis=1) / rd + 8
    return np.abs(s_star) * (r * x * U + 2 * U * np.abs(w))


def _oracle_fp32(s_star, knn, D):
    """oracle/scoring.py:82-84 on the CPU, per image."""
    out = []
    for b in range(len(s_star)):
        ss, kk = torch.tensor(s_star[b]), torch.from_numpy(knn[b])
        Dt = torch.sqrt(torch.tensor(D))
        w = 1 - (torch.exp(ss / Dt) / (torch.sum(torch.exp(kk / Dt))))
        out.append(float(w * ss))
    return np.array(out, np.float32)


@pytest.mark.parametrize("D", [128, 768, 1152])
@pytest.mark.parametrize("B", [1, 64, 65])
def test_score_final_three_regimes(B, D):
    rd = np.sqrt(float(D))
    cases = FINITE + OVERFLOW
    for rot in range(0, len(cases), B):
        pick = [(rot + b) % len(cases) for b in range(B)]
        args = np.array([cases[i] for i in pick], np.float64)
        finite = np.array([i < len(FINITE) for i in pick])
        s_star = (args[:, 0] * rd).astype(np.float32)
        knn = (args[:, 1:] * rd).astype(np.float32)
        # the regimes are what they claim to be (on the INPUTS, in float64, from the fp32 arguments as the kernel forms them)
        a32 = np.concatenate([s_star[:, None], knn], axis=1).astype(np.float64) / rd
        assert (a32[finite] <= 88.01).all() and (np.exp(a32[finite, 1:]).sum(1) < 0.99 * FLT_MAX).all()
        assert ((a32[~finite] <= 88.51) | (a32[~finite] >= 88.99)).all()
        got = ops.score_final(_dev(s_star), _dev(knn), D).cpu().numpy()
        want, _, _ = sr.final(s_star, knn, D)
        lim = final_bound(s_star, knn, D)
        err = np.abs(got.astype(np.float64) - want)
        if finite.any():
            worst = np.argmax((err / np.maximum(lim, 1e-300))[finite])
            print(f"ACHIEVED score_final B={B} D={D}: worst err/bound {(err / np.maximum(lim, 1e-300))[finite][worst]:.3e}")
            assert (err[finite] <= lim[finite]).all(), (args[finite][worst], got[finite][worst], want[finite][worst], lim[finite][worst])
        if (~finite).any():
            ref = _oracle_fp32(s_star, knn, D)
            assert (~np.isfinite(ref[~finite]) | (ref[~finite] == s_star[~finite])).all()    # independent of exp's last bit
            assert np.array_equal(got[~finite], ref[~finite], equal_nan=True), (args[~finite], got[~finite], ref[~finite])


# ---------------------------------------------------------------------------------------------------------------- engine level
def _poison_allocator(D):
    """Leaves NaN in the blocks torch.empty() will hand out next: a value computed from an unwritten buffer becomes visible."""
    junk = [torch.full(shape, float("nan"), device=DEV) for shape in ((2, D), (2, 2), (2,), (2, D), (2, 2), (512,), (4096,)) for _ in range(4)]
    del junk


def _engine_inputs(Nb, D=128, B=2, Q=4, seed=0):
    g = np.random.default_rng(seed + Nb)
    rows = g.standard_normal((Nb, D)).astype(np.float32)
    patch = (rows[g.integers(0, Nb, (B, Q))] + 0.5 * g.standard_normal((B, Q, D))).astype(np.float32)
    return rows, patch


def _check_scored(r, patch, rows, keys2, pair=""):
    """Every output of score_patches_from_keys against the float64 reference UNDER THE ZERO-PREFILL CONTRACT of its docstring."""
    B, Q, D = patch.shape
    Nb = rows.shape[0]
    flat = patch.reshape(B * Q, D)
    zf, zi = np.zeros(B * Q, np.float32), np.full(B * Q, -1, np.int64)
    wv, wi, ww = sr.rescore2(flat, rows, keys2, 0, Nb, (zf, zi))
    got_mv = r["min_val"].reshape(-1).cpu().numpy()
    np.testing.assert_array_equal(r["min_idx"].reshape(-1).cpu().numpy(), wi, err_msg=pair)
    assert (got_mv[~ww] == 0).all()
    _close(got_mv[ww], wv[ww], DIST_REL(D), f"engine min_val Nb={Nb}{pair}")
    h = sr.head(got_mv.reshape(B, Q), wi.reshape(B, Q), patch, rows, 0, Nb, np.zeros((B, D), np.float32))
    np.testing.assert_array_equal(r["s_idx"].cpu().numpy(), h["s_idx"])
    _same_bits(r["s_star"], h["s_star"], "engine s_star")
    # top3: the (up to three) nearest rows of m_star, the rest KEY_EMPTY
    d2 = ((h["m_star"][:, None].astype(np.float64) - rows[None].astype(np.float64)) ** 2).sum(-1)
    top = r["top3"].cpu().numpy()
    want_rows = np.argsort(d2, axis=1, kind="stable")[:, :3]
    for b in range(B):
        np.testing.assert_array_equal(sr.split_keys(top[b, :min(3, Nb)])[1].astype(np.int64), want_rows[b, :min(3, Nb)])
        assert (top[b, min(3, Nb):] == E).all()
    knn, kw = sr.tail(h["m_test"], top, rows, 0, Nb, np.zeros((B, 2)))
    got_knn = r["knn_d"].cpu().numpy()
    assert (got_knn[~kw] == 0).all(), got_knn                           # missing neighbours: exactly zero, never stale memory
    _close(got_knn[kw], knn[kw], DIST_REL(D), f"engine knn_d Nb={Nb}{pair}")
    s, _, _ = sr.final(r["s_star"].cpu().numpy(), got_knn, D)
    got_s = r["s"].cpu().numpy().astype(np.float64)
    assert np.isfinite(got_s).all(), got_s
    assert (np.abs(got_s - s) <= final_bound(r["s_star"].cpu().numpy(), got_knn, D)).all(), (got_s, s)
    return h


@pytest.mark.parametrize("Nb", [1, 2])
def test_engine_library_of_fewer_than_three_rows(Nb):
    """The reference's topk(k=3) raises here; score_patches_from_keys DEFINES the answer by a zero prefill (its docstring): the
    missing neighbours keep KEY_EMPTY in top3 and 0 in knn_d.  Same on the unsharded, the pair and the sharded path."""
    rows, patch = _engine_inputs(Nb)
    B, Q, D = patch.shape
    keys2 = np.full((2, B * Q), E, dtype=np.int64)
    for r_ in range(B * Q):
        keys2[0, r_] = sr.pack_key(1.0, r_ % Nb)
        if Nb > 1:
            keys2[1, r_] = sr.pack_key(2.0, (r_ + 1) % Nb)
    tp, tk = _dev(patch), _dev(keys2)
    bank = eng.Bank(_dev(rows))
    bank.blk16
    _poison_allocator(D)
    r = eng.score_patches_from_keys(tp, tk, bank, (2, 2), gt_size=8)
    _check_scored(r, patch, rows, keys2)
    _poison_allocator(D)
    ra, rb = eng.score_patches_from_keys_pair(tp, tk, bank, (2, 2), tp, tk, bank, (2, 2), gt_size=8)
    for x in (ra, rb):
        _check_scored(x, patch, rows, keys2, " pair")
        for k in ("min_val", "min_idx", "s_idx", "s_star", "s", "top3", "knn_d"):
            assert torch.equal(x[k], r[k]), k
    # the sharded path (one rank that owns everything), driven in lock-step without a process group
    sb = eng.Bank(_dev(rows), replicate_f32=False)
    _poison_allocator(D)
    gen = eng._sharded_score_steps(tp, tk, sb, (2, 2), 8)
    try:
        kind, t = next(gen)
        while True:
            kind, t = gen.send(t if kind == "sum" else t.unsqueeze(0))
    except StopIteration as done:
        rs = done.value
    for k in ("min_val", "min_idx", "s_idx", "s_star", "s", "top3", "knn_d"):
        assert torch.equal(rs[k], r[k]), k


def test_engine_image_without_any_candidate():
    """An image all of whose keys are KEY_EMPTY (every shard of the search was empty for it): min_val 0, min_idx -1, s_idx 0,
    s_star 0, nobody writes m_star -> the zero vector is the probe of the re-weighting scan, and s = 0 -- not NaN, not stale memory.
    The image next to it is scored as usual."""
    Nb = 9
    rows, patch = _engine_inputs(Nb, seed=5)
    B, Q, D = patch.shape
    keys2 = np.full((2, B * Q), E, dtype=np.int64)
    for r_ in range(Q, B * Q):                 # image 0: nothing; image 1: real candidates
        keys2[0, r_] = sr.pack_key(1.0, r_ % Nb)
        keys2[1, r_] = sr.pack_key(2.0, (r_ + 4) % Nb)
    tp, tk = _dev(patch), _dev(keys2)
    bank = eng.Bank(_dev(rows))
    bank.blk16
    _poison_allocator(D)
    r = eng.score_patches_from_keys(tp, tk, bank, (2, 2), gt_size=8)
    h = _check_scored(r, patch, rows, keys2)
    assert not h["m_star_written"][0] and h["m_star_written"][1]
    assert (r["min_val"][0] == 0).all() and (r["min_idx"][0] == -1).all()
    assert int(r["s_idx"][0]) == 0 and float(r["s_star"][0]) == 0.0 and float(r["s"][0]) == 0.0
    _poison_allocator(D)
    ra, rb = eng.score_patches_from_keys_pair(tp, tk, bank, (2, 2), tp, tk, bank, (2, 2), gt_size=8)
    for x in (ra, rb):
        for k in ("min_val", "min_idx", "s_idx", "s_star", "s", "top3", "knn_d"):
            assert torch.equal(x[k], r[k]), k


# ------------------------------------------------------------------------------------ engine level: ordinary sizes, searched keys
ALL_KEYS = ("min_val", "min_idx", "s_idx", "s_star", "s", "s_map_pre", "top3", "knn_d")


def _searched_library(Nb, Q, **bank_kw):
    """A seeded Gaussian library with B = 3 images of Q patches (no ties), its Bank, and the two-plane keys of a REAL search."""
    rows, patch = _engine_inputs(Nb, B=3, Q=Q)
    tp = _dev(patch)
    bank = eng.Bank(_dev(rows), **bank_kw)
    bank.blk16
    q16, _, qsq = ops.normalize_cast(tp.reshape(-1, tp.shape[2]))
    keys = ops.l2_min_keys(q16, qsq, bank.bf16, bank.sqnorm, ops.new_keys(q16.shape[0], DEV, runner=True), bank.row_offset)
    return tp, keys, bank


@pytest.mark.parametrize("scan_pair", ["1", "0"])
def test_engine_pair_of_two_different_libraries(scan_pair, monkeypatch):
    """The two halves of score_patches_from_keys_pair differ in EVERYTHING -- library (300 and 40 rows), patches ([3, 4, 128] and
    [3, 9, 128]), dims, keys -- so a bank, a `dims` or a `top3` that crossed from one half to the other cannot go unnoticed: each half
    is, bit for bit and in every key of the result, what the single-library call returns.  CMDIAD_SCAN_PAIR=0: the fallback."""
    pa, ka, bank_a = _searched_library(300, 4)
    pb, kb, bank_b = _searched_library(40, 9)
    D = pa.shape[2]
    launched = []
    pair_scan = ops.reweight_scan_pair
    monkeypatch.setattr(ops, "reweight_scan_pair", lambda *a, **k: launched.append(1) or pair_scan(*a, **k))
    monkeypatch.setenv("CMDIAD_SCAN_PAIR", scan_pair)
    _poison_allocator(D)
    want_a = eng.score_patches_from_keys(pa, ka, bank_a, (2, 2), gt_size=8)
    _poison_allocator(D)
    want_b = eng.score_patches_from_keys(pb, kb, bank_b, (3, 3), gt_size=8)
    _poison_allocator(D)
    ra, rb = eng.score_patches_from_keys_pair(pa, ka, bank_a, (2, 2), pb, kb, bank_b, (3, 3), gt_size=8)
    assert len(launched) == int(scan_pair)          # the pair scan really ran / really did not
    for got, want, half in ((ra, want_a, "a"), (rb, want_b, "b")):
        assert sorted(got) == sorted(want) == sorted(ALL_KEYS)
        for k in ALL_KEYS:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (half, k)
    assert ra["s_map_pre"].shape == rb["s_map_pre"].shape == (3, 8, 8) and not torch.equal(ra["s_map_pre"], rb["s_map_pre"])


def test_engine_sharded_tail_at_an_ordinary_size():
    """The tail of a library whose fp32 rows are sharded (one rank that owns all 300 of them), driven in lock-step without a process
    group, on searched keys: every key of the result, the score map included, is bit for bit the single-library result."""
    tp, keys, bank = _searched_library(300, 4)
    D = tp.shape[2]
    _poison_allocator(D)
    want = eng.score_patches_from_keys(tp, keys, bank, (2, 2), gt_size=8)
    _, keys_s, sharded = _searched_library(300, 4, replicate_f32=False)
    assert sharded.f32_sharded and torch.equal(keys_s, keys)
    _poison_allocator(D)
    gen = eng._sharded_score_steps(tp, keys_s, sharded, (2, 2), 8)
    kinds = []
    try:
        kind, t = next(gen)
        while True:
            kinds.append(kind)
            kind, t = gen.send(t if kind == "sum" else t.unsqueeze(0))
    except StopIteration as done:
        got = done.value
    assert kinds == ["sum", "sum", "gather", "sum"]
    assert sorted(got) == sorted(want) == sorted(ALL_KEYS)
    for k in ALL_KEYS:
        assert torch.equal(got[k], want[k]), k
