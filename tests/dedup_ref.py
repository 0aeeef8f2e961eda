"""A numpy restatement of the query-row dedup plan (cmdiad_amd/csrc/dedup.hip, include/cmdiad_hip.h), the means to build rows
that collide in its 32-bit tag, and the case table shared by tests/test_dedup_ref_cpu.py and tests/test_gpu_dedup_edges.py.

The plan's promise: a row is dropped only if its tag and the bits of its squared norm equal the representative's AND all D elements
compare equal.  Random rows never share a tag, so they never reach the norm or the element comparison.  The tag is invertible --
odd multipliers and xor-shifts are bijections of 32-bit words -- so rows that do share it are solved for here, on the host:

    chunk c of a row = four 32-bit words (x, y, z, w), eight 16-bit elements
    m    = x * K0 ^ y * K1 ^ z * K2 ^ w * K3
    h    = SUM over c of (m ^ m >> 15) * (2 c + 1) + c * KC          (wrapping)
    tag  = h ^ h >> 13

Given any x', y' = (m' ^ x' * K0 ^ z * K2 ^ w * K3) * K1^-1 gives the chunk any chosen m'; x' is drawn until both halves of y' are
finite 16-bit floats of magnitude below 8 (DRAWS records how many draws each call needed).

Everything is compared bit for bit; there is no tolerance anywhere in these files."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

K0, K1, K2, K3, KC = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F, 0x165667B1
M32 = 0xFFFFFFFF
K1_INV = pow(K1, -1, 1 << 32)
SAMPLE = 8192            # pick_rep_kernel: rows sampled
BLOCK = 1024             # compact_*_kernel: rows per block
KINDS = ("f16", "bf16")
WEAKENINGS = ("no_elements", "first64", "no_norm", "leading_sample", "no_block_base")

DRAWS = []               # draws of x' per crafted row, in call order (a function of the seeds alone)
CASE_DRAWS = ()          # those of all_cases()


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def row_tags(q_u16):
    """[Q] uint32: hash_rows_kernel."""
    q = np.ascontiguousarray(q_u16, dtype=np.uint16)
    Q, D = q.shape
    assert D % 8 == 0
    w = q.view("<u4").reshape(Q, D // 8, 4)
    m = (w[..., 0] * np.uint32(K0)) ^ (w[..., 1] * np.uint32(K1)) ^ (w[..., 2] * np.uint32(K2)) ^ (w[..., 3] * np.uint32(K3))
    c = np.arange(D // 8, dtype=np.uint32)
    t = (m ^ (m >> np.uint32(15))) * (np.uint32(2) * c + np.uint32(1)) + c * np.uint32(KC)
    h = t.sum(axis=1, dtype=np.uint32)
    return h ^ (h >> np.uint32(13))


def sample_positions(Q, leading=False):
    """The rows pick_rep_kernel counts: i * Q // ns for i < ns = min(Q, 8192).  (leading: the weakened form, rows i.)"""
    ns = min(Q, SAMPLE)
    i = np.arange(ns, dtype=np.int64)
    return i if leading or ns == 0 else i * Q // ns


def pick_rep(tags, leading=False):
    """-> (full tag of the first sampled row with the winning 24-bit prefix, that prefix was counted at least twice).
    Two rounds of 4 096 counters over the sampled rows: bits 0-11, then bits 12-23 inside the winning bucket; the highest count
    wins and the lowest bucket breaks ties."""
    pos = sample_positions(len(tags), leading)
    if len(pos) == 0:
        return 0, False
    g = tags[pos]
    lo = int(np.argmax(np.bincount(g & np.uint32(4095), minlength=4096)))           # argmax: the first = lowest index of the ties
    inside = g[(g & np.uint32(4095)) == lo]
    cnt = np.bincount((inside >> np.uint32(12)) & np.uint32(4095), minlength=4096)
    win = int(np.argmax(cnt))
    want = lo | (win << 12)
    first = int(np.nonzero((g & np.uint32(0xFFFFFF)) == want)[0][0])
    return int(g[first]), bool(cnt[win] >= 2)


def plan(q_u16, qsq_bits, weak=None):
    """-> (slot [Q] int32, rows [count] int32, count).  The representative is the first row carrying pick_rep's tag; a row repeats
    it iff tag, squared-norm bits and all D elements are equal; the other rows are compacted in their order; slot of a dropped row
    is the representative's index (nothing in front of the first occurrence is dropped, so that is its slot too).
    weak: one of WEAKENINGS -- a deliberately wrong plan, for the teeth checks."""
    assert weak is None or weak in WEAKENINGS
    q = np.ascontiguousarray(q_u16, dtype=np.uint16)
    sq = np.asarray(qsq_bits, dtype=np.uint32)
    Q = q.shape[0]
    tags = row_tags(q)
    full, twice = pick_rep(tags, leading=weak == "leading_sample")
    dup = np.zeros(Q, bool)
    rep = Q
    if twice:
        rep = int(np.nonzero(tags == np.uint32(full))[0][0])
        dup = tags == tags[rep]
        if weak != "no_norm":
            dup &= sq == sq[rep]
        if weak == "first64":
            dup &= (q[:, :512] == q[rep, :512]).all(axis=1)
        elif weak != "no_elements":
            dup &= (q == q[rep]).all(axis=1)
        dup[rep] = False
    slot = np.empty(Q, np.int32)
    if weak == "no_block_base":                        # every block of 1 024 rows compacts from 0; the count is the last block's
        rows = np.full(Q, -1, np.int32)
        count = 0
        for b in range(0, Q, BLOCK):
            kept = b + np.nonzero(~dup[b:b + BLOCK])[0]
            rows[:len(kept)] = kept
            slot[kept] = np.arange(len(kept))
            count = len(kept)
        rows = rows[:count]
    else:
        rows = np.nonzero(~dup)[0].astype(np.int32)
        count = len(rows)
        slot[rows] = np.arange(count)
    slot[dup] = rep
    return slot, rows, count


def as_plan(slot, rows, count, q16, qsq):
    """The reference plan in the shape of ops.DedupPlan (host tensors), for check_plan."""
    Q = q16.shape[0]
    r = torch.zeros(Q, dtype=torch.int32)
    r[:count] = torch.from_numpy(np.asarray(rows[:count], dtype=np.int32))
    p = SimpleNamespace(slot=torch.from_numpy(slot.copy()), rows=r, count=torch.tensor([count], dtype=torch.int32),
                        q16=torch.zeros_like(q16), q_sq=torch.zeros_like(qsq))
    if count and 0 <= int(r[:count].min()) and int(r[:count].max()) < Q:
        p.q16[:count] = q16[r[:count].long()]
        p.q_sq[:count] = qsq[r[:count].long()]
    return p


def check_plan(plan, q16, qsq, n_repeats):
    """The plan is valid -- the rows kept are the others in their order, every dropped row is bit for bit its representative (16-bit
    row and squared norm: everything the distance kernel reads) -- and it dropped the n_repeats - 1 later occurrences of the most
    repeated row (None: whatever it found; a pair among a few hundred rows can hide behind a hash-bucket tie, which costs nothing
    but the saving)."""
    q = q16.view(torch.int16).cpu().numpy()
    sq = qsq.cpu().numpy().view(np.uint32)
    Q = q.shape[0]
    n = int(plan.count.item())
    rows = plan.rows[:n].cpu().numpy()
    slot = plan.slot.cpu().numpy()
    assert 0 <= n <= Q and (np.diff(rows) > 0).all() and (n == 0 or (0 <= rows[0] and rows[-1] < Q))
    kept = np.zeros(Q, bool)
    kept[rows] = True
    assert np.array_equal(slot[rows], np.arange(n))
    dropped = np.nonzero(~kept)[0]
    if len(dropped):
        rep = rows[slot[dropped]]
        assert len(set(rep.tolist())) == 1 and (rep < dropped).all(), "one representative, the first occurrence"
        assert (q[dropped] == q[rep]).all() and (sq[dropped] == sq[rep]).all()
    if n_repeats is not None:
        assert len(dropped) == max(n_repeats - 1, 0), (len(dropped), n_repeats)
    idx = torch.from_numpy(rows).to(q16.device)
    assert torch.equal(plan.q16[:n], q16[idx]) and torch.equal(plan.q_sq[:n], qsq[idx])
    return n


# ---- 16-bit rows on the host -----------------------------------------------------------------------------------------------------
def to_u16(x, kind):
    """float32 -> the bits of the nearest fp16 / bf16 (ties to even)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if kind == "f16":
        return x.astype(np.float16).view(np.uint16)
    u = x.view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def from_u16(u, kind):
    u = np.ascontiguousarray(u, dtype=np.uint16)
    if kind == "f16":
        return u.view(np.float16).astype(np.float32)
    return (u.astype(np.uint32) << np.uint32(16)).view(np.float32)


def sqnorm_bits(q_u16, kind):
    """The bits of the fp32 squared norm of every row (any finite value serves: every search of a case reads the same one)."""
    x = from_u16(q_u16, kind)
    return (x * x).sum(axis=1, dtype=np.float32).view(np.uint32)


def _limit(kinds):
    """Magnitude bits (the low 15) below this bound are finite and below 8.0: exponent field <= 17 of 5 (fp16), <= 129 of 8 (bf16)."""
    return min({"f16": 18 << 10, "bf16": 130 << 7}[k] for k in kinds)


def small_and_finite(u16, kinds=KINDS):
    return bool(((np.asarray(u16, dtype=np.uint16) & np.uint16(0x7FFF)) < _limit(kinds)).all())


def _halves_ok(word, lim):
    return (word & 0x7FFF) < lim and ((word >> 16) & 0x7FFF) < lim


def _solve_chunk(words, m_want, rng, kinds):
    """(x', y') with x' * K0 ^ y' * K1 ^ z * K2 ^ w * K3 == m_want, all four halves finite and below 8, (x', y') != (x, y)."""
    x, y, z, w = (int(v) for v in words)
    rest = m_want ^ (z * K2 & M32) ^ (w * K3 & M32)
    lim = _limit(kinds)
    for draws in range(1, 10001):
        xn = int(rng.integers(0, lim)) | (int(rng.integers(0, 2)) << 15) | (int(rng.integers(0, lim)) << 16) | (int(rng.integers(0, 2)) << 31)
        yn = ((rest ^ (xn * K0 & M32)) * K1_INV) & M32
        if _halves_ok(yn, lim) and (xn, yn) != (x, y):
            DRAWS.append(draws)
            return xn, yn
    raise AssertionError("no finite solution in 10 000 draws")


def _chunk_m(words):
    x, y, z, w = (int(v) for v in words)
    return (x * K0 & M32) ^ (y * K1 & M32) ^ (z * K2 & M32) ^ (w * K3 & M32)


def same_tag_twin(row, chunk, rng, kinds=KINDS):
    """A row that differs from `row` only in the first two 32-bit words of `chunk` and has the same tag (the chunk keeps its m)."""
    out = np.array(row, dtype=np.uint16)
    w = out.view("<u4")
    w[4 * chunk], w[4 * chunk + 1] = _solve_chunk(w[4 * chunk:4 * chunk + 4], _chunk_m(w[4 * chunk:4 * chunk + 4]), rng, kinds)
    return out


def _unshift(t, s):
    h = t
    for _ in range(32 // s + 1):
        h = t ^ (h >> s)
    return h


def row_with_tag(row, tag, rng, chunk=0, kinds=KINDS):
    """A row that differs from `row` only in the first two 32-bit words of `chunk` and carries the full 32-bit `tag`."""
    out = np.array(row, dtype=np.uint16)
    w = out.view("<u4")
    cw = w[4 * chunk:4 * chunk + 4]
    m = _chunk_m(cw)
    h_now = _unshift(int(row_tags(out[None])[0]), 13)
    term_now = ((m ^ (m >> 15)) * (2 * chunk + 1) + chunk * KC) & M32
    term = (_unshift(int(tag), 13) - h_now + term_now) & M32
    m_want = _unshift(((term - chunk * KC) * pow(2 * chunk + 1, -1, 1 << 32)) & M32, 15)
    w[4 * chunk], w[4 * chunk + 1] = _solve_chunk(cw, m_want, rng, kinds)
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# A case: name, kind, q [Q, D] uint16, sq [Q] uint32, dropped (rows the plan must drop: the stated outcome), search (run the search
# equality on it), bites (weakenings that must give a rejected or another plan; every case needs one unless `toothless` says why).
def _random_rows(Q, D, kind, rng):
    return to_u16(np.clip(rng.standard_normal((Q, D), dtype=np.float32), -7.5, 7.5), kind)


class _Build:
    """Random distinct rows; put() overwrites rows with a value and (optionally) another row's norm bits."""

    def __init__(self, name, Q, D, kind, seed):
        self.name, self.kind, self.D = name, kind, D
        self.rng = np.random.default_rng(seed)
        self.q = _random_rows(Q, D, kind, self.rng)
        self.sq = sqnorm_bits(self.q, kind)

    def row(self):
        return _random_rows(1, self.D, self.kind, self.rng)[0]

    def put(self, at, row, sq=None):
        at = np.atleast_1d(np.asarray(at, dtype=np.int64))
        self.q[at] = row
        self.sq[at] = sqnorm_bits(row[None], self.kind)[0] if sq is None else sq
        return int(self.sq[at[0]]) if len(at) else None

    def twin(self, at, row, chunk, sq):
        t = same_tag_twin(row, chunk, self.rng, (self.kind,))
        self.put(at, t, sq)
        return t

    def done(self, dropped, bites, search=False, toothless=None, **extra):
        assert small_and_finite(self.q, (self.kind,))
        return SimpleNamespace(name=self.name, kind=self.kind, q=self.q, sq=self.sq, Q=self.q.shape[0], D=self.D, dropped=dropped,
                               search=search, bites=frozenset(bites), toothless=toothless, **extra)


def _behind(rng, first, Q, n, taken=()):
    """n distinct rows behind `first`, none of `taken`, ascending."""
    pool = np.setdiff1d(np.arange(first + 1, Q), np.asarray(list(taken), dtype=np.int64))
    return np.sort(rng.choice(pool, size=n, replace=False))


def twin_chunks(D):
    C = D // 8
    return sorted({c for c in (0, 63, 64, 128, C - 1) if c < C})


def _twins_case(name, Q, D, kind, n_rep, seed, search):
    """A row at `first` and n_rep - 1 times behind it; behind `first` also one same-tag twin per chunk of twin_chunks(D), with the
    representative's norm bits: the twins must be kept and answer for themselves."""
    b = _Build(name, Q, D, kind, seed)
    chunks = twin_chunks(D)
    first = int(b.rng.integers(0, 8))
    spots = _behind(b.rng, first, Q, n_rep - 1 + len(chunks))
    at_twin = b.rng.choice(len(spots), size=len(chunks), replace=False)
    R = b.row()
    sq = b.put(np.concatenate([[first], np.delete(spots, at_twin)]), R)
    for c, i in zip(chunks, at_twin):
        b.twin(spots[i], R, c, sq)
    bites = {"no_elements"} | ({"first64"} if D > 512 else set()) | ({"no_block_base"} if Q > BLOCK else set())
    return b.done(n_rep - 1, bites, search)


def _twin_in_front_case(kind, seed):
    """The twin stands in front of the first occurrence: it carries the tag first, so IT is the representative, nothing repeats it,
    and nothing is saved (the documented cost of a collision: the saving, never an answer)."""
    b = _Build(f"twin_in_front-{kind}", 1024, 768, kind, seed)
    R = b.row()
    spots = _behind(b.rng, 5, 1024, 400)
    sq = b.put(spots, R)
    b.twin(5, R, 95, sq)
    return b.done(0, {"no_elements", "first64"}, search=True)


def _norm_case(kind, seed):
    """Rows equal to the representative in all 16-bit elements whose squared norm is one ulp away must be kept."""
    b = _Build(f"norm_one_ulp-{kind}", 1500, 768, kind, seed)
    R = b.row()
    spots = _behind(b.rng, 2, 1500, 303)
    sq = b.put(np.concatenate([[2], spots[3:]]), R)
    b.put(spots[0], R, sq + 1)
    b.put(spots[1], R, sq - 1)
    b.put(spots[2], R, sq + 1)
    return b.done(300, {"no_norm", "no_block_base"})


def _block_q_case(Q, D, kind, seed):
    """Q around the 1 024-row blocks of the compaction: the row at `first`, on ~40 % of the rows behind it and on the last row; a
    twin right behind `first`."""
    b = _Build(f"block_Q{Q}-D{D}-{kind}", Q, D, kind, seed)
    if Q <= 1:
        return b.done(0, (), search=Q > 0, toothless="fewer than two rows: no comparison, sample or block base to get wrong")
    first = Q // 3 if Q >= 1000 else 0
    R = b.row()
    rest = np.arange(first + 2, Q)
    rep = np.concatenate([[first], rest[b.rng.random(len(rest)) < 0.4], rest[-1:]]) if len(rest) else np.array([first])
    rep = np.unique(rep)
    sq = b.put(rep, R)
    b.twin(first + 1, R, D // 8 - 1, sq)
    return b.done(len(rep) - 1, {"no_elements"} | ({"no_block_base"} if Q > BLOCK else set()), search=True)


def _rep_at_case(first, Q, D, kind, seed, only=None):
    """The representative at `first`; its repeats on ~30 % of the rows behind it (only: exactly these rows), a twin among them."""
    b = _Build(f"rep_at_{first}_of_{Q}-D{D}-{kind}", Q, D, kind, seed)
    R = b.row()
    rest = np.arange(first + 1, Q)
    rep = np.asarray(only) if only is not None else np.unique(np.concatenate([rest[b.rng.random(len(rest)) < 0.3],
                                                                                  [r for r in (1023, 1024, 2047, 2048, Q - 1) if r > first]]))
    sq = b.put(np.concatenate([[first], rep]), R)
    dropped = len(rep)
    if only is None:
        b.twin(rep[len(rep) // 2], R, D // 8 - 1, sq)
        dropped -= 1
    return b.done(dropped, {"no_block_base"} | ({"no_elements"} if only is None else set()), search=True)


def _later_block_case(kind, seed):
    """The representative in block 0, its repeats in block 2 only, a twin in block 1."""
    b = _Build(f"repeats_two_blocks_later-{kind}", 3072, 128, kind, seed)
    R = b.row()
    rep = _behind(b.rng, 2047, 3072, 350)
    sq = b.put(np.concatenate([[500], rep]), R)
    b.twin(1500, R, 7, sq)
    return b.done(350, {"no_elements", "no_block_base"}, search=True)


def _all_identical_case(Q, D, kind, seed):
    b = _Build(f"all_identical_Q{Q}-{kind}", Q, D, kind, seed)
    b.put(np.arange(Q), b.row())
    return b.done(Q - 1, {"no_block_base"}, search=True)


def _shares_case(Q, D, kind, seed):
    """Row A on 30 % of the rows, row B on 20 %.  All of B stands in the leading 8 192 rows, where it outnumbers A: sampled at
    i * Q // ns, A wins.  A twin of A keeps the element compare in play where the two samplings are the same rows (Q <= 8 193)."""
    b = _Build(f"shares_30_20_Q{Q}-D{D}-{kind}", Q, D, kind, seed)
    nA, nB = Q * 3 // 10, Q // 5
    lead = min(Q, SAMPLE)
    at_b = np.sort(b.rng.choice(lead, size=nB, replace=False))
    free = np.setdiff1d(np.arange(Q), at_b)
    lead_free = free[free < lead]
    n_lead = min(len(lead_free), nA) if Q <= SAMPLE + 1 else nB // 4         # A in the leading rows: a quarter of B's where it matters
    late = free[free >= lead]
    n_lead = max(n_lead, nA - len(late))
    at_a = np.sort(np.concatenate([b.rng.choice(lead_free, size=n_lead, replace=False), b.rng.choice(late, size=nA - n_lead, replace=False)]))
    A, B = b.row(), b.row()
    sq = b.put(at_a, A)
    b.put(at_b, B)
    b.twin(at_a[len(at_a) // 2], A, D // 8 - 1, sq)
    bites = {"no_elements", "no_block_base"} | ({"leading_sample"} if Q > SAMPLE + 1 else set())
    return b.done(nA - 2, bites, search=True)


def _tie_case(name, kind, seed, winner_later, round2):
    """Two rows with exactly equal sampled counts (Q = 4 096: every row is sampled): the lower bucket wins -- of bits 0-11, or,
    round2, of bits 12-23 with bits 0-11 equal.  winner_later: the loser occurs first, so 'first seen' is the wrong rule.  The
    winner has a twin, which counts in its bucket: 299 + 1 against 300; no other row counts in either bucket."""
    b = _Build(name, 4096, 128, kind, seed)
    X, Y = b.row(), b.row()
    tx = int(row_tags(X[None])[0])
    if round2:
        Y = row_with_tag(Y, (tx & 0xFFF) | ((tx ^ 0x5A5000) & 0xFFF000) | (int(row_tags(Y[None])[0]) & 0xFF000000), b.rng, 3, (kind,))
    ty = int(row_tags(Y[None])[0])
    key = (lambda t: (t >> 12) & 0xFFF) if round2 else (lambda t: t & 0xFFF)
    assert key(tx) != key(ty) and (not round2 or (tx & 0xFFF) == (ty & 0xFFF))
    W, L = (X, Y) if key(tx) < key(ty) else (Y, X)
    spots = b.rng.permutation(np.arange(2, 4096))[:600]
    at_w, at_l = np.sort(spots[:300]), np.sort(spots[300:])
    at_l = np.concatenate([[0 if winner_later else 1], at_l[1:]])
    at_w = np.concatenate([[1 if winner_later else 0], at_w[1:]])
    sq = b.put(at_w, W)
    b.put(at_l, L)
    b.twin(at_w[150], W, 15, sq)
    # no other row may count in the two buckets (bits 0-11 decide which rows round two sees, so they are kept clear in both forms)
    others = np.setdiff1d(np.arange(4096), np.concatenate([at_w, at_l]))
    while True:
        stray = others[np.isin(row_tags(b.q[others]) & np.uint32(0xFFF), [tx & 0xFFF, ty & 0xFFF])]
        if len(stray) == 0:
            break
        for r in stray:
            b.put(r, b.row())
    return b.done(298, {"no_elements", "no_block_base"}, tie=(int(row_tags(W[None])[0]), int(row_tags(L[None])[0]), round2))


def _odd_rows_case(kind, seed):
    """Q = 16 384: the sample is the even rows; the repeated row stands on odd rows only and is never seen.  Nothing is saved."""
    b = _Build(f"repeats_on_unsampled_rows-{kind}", 16384, 64, kind, seed)
    odd = np.arange(1, 16384, 2)
    b.put(odd[b.rng.random(len(odd)) < 0.6], b.row())
    return b.done(0, {"leading_sample"})


def _prefix_mate_case(kind, seed):
    """A row S with the repeated row's low 24 tag bits and other top 8 stands in front of it: S is the first sampled row with the
    winning prefix, its full tag is chosen, and the repeated row is not found.  Nothing is saved.  (S' behind it carries S's full
    tag and norm bits with other elements, so the plan still has a comparison to get right.)"""
    b = _Build(f"prefix_mate_in_front-{kind}", 3000, 768, kind, seed)
    R = b.row()
    b.put(_behind(b.rng, 10, 3000, 900), R)
    S = row_with_tag(b.row(), int(row_tags(R[None])[0]) ^ 0x81000000, b.rng, 40, (kind,))
    sq = b.put(7, S)
    b.twin(2500, S, 95, sq)
    return b.done(0, {"no_elements", "first64"})


def _no_repeats_case(Q, D, kind, seed):
    b = _Build(f"no_repeats_Q{Q}-D{D}-{kind}", Q, D, kind, seed)
    return b.done(0, (), toothless="distinct random rows: the second batch of the reuse case, whose outcome (count == Q) is stated")


LIVE = (255, 256, 257)            # live rows of the 1 024-row twin cases: either side of a 256-row tile of the counted search


@functools.lru_cache(maxsize=None)
def all_cases():
    global CASE_DRAWS
    cases, seed, drawn = [], 1000, len(DRAWS)
    for D in (128, 768):
        for kind in KINDS:
            for live in LIVE:         # Q - (n_rep - 1) = live
                seed += 1
                cases.append(_twins_case(f"twins_D{D}-{kind}-live{live}", 1024, D, kind, 1024 - live + 1, seed, True))
    for D in (8, 64, 320, 1152):
        for kind in KINDS:
            seed += 1
            cases.append(_twins_case(f"twins_D{D}-{kind}", 1500, D, kind, 400, seed, False))
    for kind in KINDS:
        cases += [_twin_in_front_case(kind, seed + 1), _norm_case(kind, seed + 2)]
        seed += 2
    for i, Q in enumerate((0, 1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049)):
        seed += 1
        cases.append(_block_q_case(Q, (128, 768)[i % 2], KINDS[(i // 2) % 2], seed))
    for i, first in enumerate((0, 1023, 1024)):
        seed += 1
        cases.append(_rep_at_case(first, 2500, (768, 128)[i % 2], KINDS[i % 2], seed))
    # a representative needs repeats behind it (enough to outnumber the chance collisions of bits 0-11 among 2 048 random rows), so
    # the last row cannot be one: the representative opens the last block and its repeats fill the block up to the last row
    cases.append(_rep_at_case(2048, 2088, 128, "bf16", seed + 1, only=np.arange(2049, 2088)))
    cases += [_later_block_case("f16", seed + 2), _later_block_case("bf16", seed + 3)]
    cases += [_all_identical_case(1025, 768, "f16", seed + 4), _all_identical_case(4096, 128, "bf16", seed + 5)]
    seed += 5
    for i, Q in enumerate((8191, 8192, 8193, 20011)):
        seed += 1
        cases.append(_shares_case(Q, (128, 768)[i % 2], KINDS[i % 2], seed))
    cases += [_tie_case("tie_low_bits_winner_first-f16", "f16", seed + 1, False, False),
              _tie_case("tie_low_bits_winner_later-bf16", "bf16", seed + 2, True, False),
              _tie_case("tie_high_bits_winner_later-f16", "f16", seed + 3, True, True),
              _odd_rows_case("f16", seed + 4), _odd_rows_case("bf16", seed + 5),
              _prefix_mate_case("f16", seed + 6), _prefix_mate_case("bf16", seed + 7),
              _no_repeats_case(1024, 768, "f16", seed + 8)]
    assert len({c.name for c in cases}) == len(cases)
    CASE_DRAWS = tuple(DRAWS[drawn:])
    return tuple(cases)


def case(name):
    return next(c for c in all_cases() if c.name == name)


def case_tensors(c, device="cpu"):
    """(q16 [Q, D] fp16 / bf16, q_sq [Q] f32) of a case."""
    dt = torch.float16 if c.kind == "f16" else torch.bfloat16
    q16 = torch.from_numpy(c.q.view(np.int16).copy()).view(dt).reshape(c.Q, c.D)
    qsq = torch.from_numpy(c.sq.view(np.float32).copy())
    return q16.to(device), qsq.to(device)
