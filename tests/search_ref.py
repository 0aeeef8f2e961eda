"""Lattice operands, case tables and integer references of the library search (csrc/l2min.hip cmdiad_l2_min_keys, _counted,
_segments) and of the re-weighting scan (csrc/scan.hip cmdiad_reweight_scan), shared by tests/test_gpu_search_exact.py and pinned by
tests/test_search_ref_cpu.py; tests/test_host_cpu.py puts the case tables through csrc/gemm_plan.h.  No GPU, no cmdiad_amd import.

The definition, restated (csrc/l2min.hip: the RowMin comment and the keys2 paragraph above rowmin_tag):
  q [Q, D], b [Nb, D];   d2[i][r] = sum_k (q[i][k] - b[r][k])^2;   R = row_offset + r;   group(R) = (R >> 6, (R >> 2) & 3)
  plane 0 = the lexicographic minimum of (d2[i][r], R) over all r
  plane 1 = the lexicographic minimum of (d2[i][r], R) over the rows whose group differs from the group of plane 0's row;
            KEY_EMPTY where there is none
  key     = (bits of float32(d2)) << 32 | R
  scan    = the three lexicographically smallest (d2, R); KEY_EMPTY in the slots a library of fewer than three rows leaves

The lattice: operands are integers with |x| <= 4 and D <= 1024, exact in bf16 and in fp16; |q|^2 and |b|^2 are integers <= 16384,
handed to the kernels as float32.  Every value the search's accumulator -(|q|^2 + |b|^2) / 2 + q.b can take on the way is a
multiple of 1/2 below 2^16 in magnitude: at most 17 significant bits, exact in fp32 in ANY order of addition, and with its low
four mantissa bits zero, so the truncation of rowmin_tag gives nothing up.  The finished accumulator IS -d2 / 2 and both key planes
have ONE correct value per query.  The scan's |p|^2 + |b|^2 - 2 p.b is an integer below 2^24 throughout: exact as well.

Libraries: uniform integers in [-amp, amp]; 30 % of the rows are then overwritten with copies of other rows, a third of the copies
going to src ^ 1 (the same quad of four rows), a third to src ^ 16 (the same group of 16 rows where that stays inside the 64-block)
and a third to a random row.  Queries are library rows; in the second half about 10 % of the entries move by +-1 (clipped to the
lattice).  Exact ties therefore occur in quantity, and often the second-nearest row lies INSIDE the winner's group, where "nearest
outside the group" and "second nearest" are different rows (tests/test_search_ref_cpu.py asserts both shares for every case).
Random queries alone would leave a particular row -- the last of a ragged tile, the first after a range boundary -- without any
query that it wins, and a kernel that drops it unnoticed: the first Q / 8 queries are edge_rows() of the library, rows that the
copying leaves alone, so that each is the only row at distance 0 of its query."""
import collections
import functools

import torch

KEY_EMPTY = 0x7FFFFFFFFFFFFFFF          # "no candidate": what the caller's arrays hold before a search (ops.KEY_EMPTY)
MAX_ABS = 4                             # the lattice
MAX_D = 1024

# ------------------------------------------------------------------------------------------------ case tables
# plan: what csrc/gemm_plan.h plan_l2 does with the case under CMDIAD_L2_TILE unset / 0 / 5 / 2 (2: the test-only build), one
# launch per "+" term: tile[library rows] nq nbt splits empty -- empty = the library ranges that hold no tile (their blocks leave at
# ntc <= 0).  tests/test_host_cpu.py asserts every label against the header.
Case = collections.namedtuple("Case", "Q Nb D amp plan")
SETTINGS = (None, "0", "5")             # CMDIAD_L2_TILE of the production build; "2" = the lock-step shape of the test-only build
AB_SETTING = "2"


def _plans(default, t0, t5, t2):
    return {None: default, "0": t0, "5": t5, "2": t2}


def _one(tile, Nb, nq, nbt, splits, empty=0):
    return f"{tile}[0:{Nb}] nq={nq} nbt={nbt} splits={splits} empty={empty}"


def _same(label, t2):                   # the 128 x 128 kernel whatever is asked for (D < 192, or Q < 512 and tile 0)
    return _plans(label, label, label, t2)


EDGE_CASES = [
    # one row, one query
    Case(1, 1, 64, 1, _same(_one("t128", 1, 1, 1, 1), _one("lockstep256", 1, 1, 1, 1))),
    # one group: plane 1 stays KEY_EMPTY
    Case(1, 4, 64, 1, _same(_one("t128", 4, 1, 1, 1), _one("lockstep256", 4, 1, 1, 1))),
    # first row of a second group
    Case(1, 5, 64, 1, _same(_one("t128", 5, 1, 1, 1), _one("lockstep256", 5, 1, 1, 1))),
    Case(17, 17, 128, 1, _same(_one("t128", 17, 1, 1, 1), _one("lockstep256", 17, 1, 1, 1))),
    Case(127, 63, 64, 1, _same(_one("t128", 63, 1, 1, 1), _one("lockstep256", 63, 1, 1, 1))),
    Case(128, 64, 128, 1, _same(_one("t128", 64, 1, 1, 1), _one("lockstep256", 64, 1, 1, 1))),
    Case(129, 65, 192, 2, _plans(_one("t128", 65, 2, 1, 1), _one("t128", 65, 2, 1, 1), _one("t128", 65, 2, 1, 1),
                                 _one("lockstep256", 65, 1, 1, 1))),
    Case(255, 255, 192, 2, _plans(_one("t128", 255, 2, 2, 2), _one("t128", 255, 2, 2, 2), _one("t128", 255, 2, 2, 2),
                                  _one("lockstep256", 255, 1, 1, 1))),
    # tile 5: one tile, one range, three K-tiles -- the two-group kernel's prologue is longer than the stream
    Case(256, 256, 192, 2, _plans(_one("t128", 256, 2, 2, 2), _one("t128", 256, 2, 2, 2), _one("two_group256", 256, 1, 1, 1),
                                  _one("lockstep256", 256, 1, 1, 1))),
    # tile 5: one full tile plus one row through the 128 kernel
    Case(257, 257, 256, 2, _plans(_one("t128", 257, 3, 3, 3), _one("t128", 257, 3, 3, 3),
                                  "two_group256[0:256] nq=2 nbt=1 splits=1 empty=0 + t128[256:257] nq=3 nbt=1 splits=1 empty=0",
                                  _one("lockstep256", 257, 2, 2, 2))),
    Case(511, 511, 320, 2, _plans(_one("t128", 511, 4, 4, 4), _one("t128", 511, 4, 4, 4),
                                  "two_group256[0:256] nq=2 nbt=1 splits=1 empty=0 + t128[256:511] nq=4 nbt=2 splits=2 empty=0",
                                  _one("lockstep256", 511, 2, 2, 2))),
    # the production switch: Q >= 512 takes the two-group kernel by default
    Case(512, 512, 192, 2, _plans(_one("two_group256", 512, 2, 2, 1), _one("t128", 512, 4, 4, 4), _one("two_group256", 512, 2, 2, 1),
                                  _one("lockstep256", 512, 2, 2, 2))),
    Case(513, 513, 320, 2, _plans("two_group256[0:512] nq=3 nbt=2 splits=1 empty=0 + t128[512:513] nq=5 nbt=1 splits=1 empty=0",
                                  _one("t128", 513, 5, 5, 5),
                                  "two_group256[0:512] nq=3 nbt=2 splits=1 empty=0 + t128[512:513] nq=5 nbt=1 splits=1 empty=0",
                                  _one("lockstep256", 513, 3, 3, 3))),
    # 128 kernel: 9 tiles over 8 ranges of 2, three ranges empty
    Case(300, 1025, 64, 1, _same(_one("t128", 1025, 3, 9, 8, 3), _one("lockstep256", 1025, 2, 5, 5))),
    # 4 whole tiles plus 255 rows
    Case(513, 1279, 256, 2, _plans("two_group256[0:1024] nq=3 nbt=4 splits=1 empty=0 + t128[1024:1279] nq=5 nbt=2 splits=2 empty=0",
                                   _one("t128", 1279, 5, 10, 8, 3),
                                   "two_group256[0:1024] nq=3 nbt=4 splits=1 empty=0 + t128[1024:1279] nq=5 nbt=2 splits=2 empty=0",
                                   _one("lockstep256", 1279, 3, 5, 5))),
    # 9 tiles in 2 ranges of 5 and 4, plus 1 row
    Case(769, 2305, 192, 2, _plans("two_group256[0:2304] nq=4 nbt=9 splits=2 empty=0 + t128[2304:2305] nq=7 nbt=1 splits=1 empty=0",
                                   _one("t128", 2305, 7, 19, 8, 1),
                                   "two_group256[0:2304] nq=4 nbt=9 splits=2 empty=0 + t128[2304:2305] nq=7 nbt=1 splits=1 empty=0",
                                   _one("lockstep256", 2305, 4, 10, 8, 3))),
    # 23 tiles in 5 ranges of 5, the last one short (3), plus 130 rows
    Case(513, 6018, 192, 2, _plans("two_group256[0:5888] nq=3 nbt=23 splits=5 empty=0 + t128[5888:6018] nq=5 nbt=2 splits=2 empty=0",
                                   _one("t128", 6018, 5, 48, 8),
                                   "two_group256[0:5888] nq=3 nbt=23 splits=5 empty=0 + t128[5888:6018] nq=5 nbt=2 splits=2 empty=0",
                                   _one("lockstep256", 6018, 3, 24, 8))),
    # 16 K-tiles, amp 4
    Case(260, 1024, 1024, 4, _plans(_one("t128", 1024, 3, 8, 8), _one("t128", 1024, 3, 8, 8), _one("two_group256", 1024, 2, 4, 1),
                                    _one("lockstep256", 1024, 2, 4, 4))),
    Case(1, 2305, 256, 2, _plans(_one("t128", 2305, 1, 19, 8, 1), _one("t128", 2305, 1, 19, 8, 1),
                                 "two_group256[0:2304] nq=1 nbt=9 splits=2 empty=0 + t128[2304:2305] nq=1 nbt=1 splits=1 empty=0",
                                 _one("lockstep256", 2305, 1, 10, 8, 3))),
]


def case_of(Q, Nb, D):
    return next(c for c in EDGE_CASES if (c.Q, c.Nb, c.D) == (Q, Nb, D))


# shards of a library, cut at multiples of 64: one of exactly 64 rows, one empty, a ragged last one
SHARD_CASES = [((769, 2305, 192), (0, 64, 64, 1088, 2304, 2305)), ((513, 1279, 256), (0, 512, 576, 576, 1279))]

# counted launch: the grid is sized for Q_MAX rows, the live count is known on the device only
COUNTED_CASE = (513, 1279, 256)
COUNTED_Q_MAX = 513
COUNTED_COUNTS = (0, 1, 127, 128, 129, 255, 256, 257, 512, 513)

# segments launch: query segment w = rows [w * stride, w * stride + min(max(count[w], 0), stride)); the stride is no multiple of
# either tile, so a segment's first row falls inside a 16-row fragment of the tile before it
SEGMENT_CASE = (513, 1279, 256)
SEGMENT_STRIDE = 300
SEGMENT_COUNTS = ((0, 300, 1, 257, 129), (300, -3, 999, 256, 0))
SEGMENT_SETTINGS = (None, "0")
SEGMENT_PLAN = {
    None: "two_group256[0:1024] nq=10 nbt=4 splits=1 empty=0 + t128[1024:1279] nq=15 nbt=2 splits=2 empty=0",
    "0": "t128[0:1279] nq=15 nbt=10 splits=8 empty=3",
}

# the re-weighting scan
SCAN_NB = (1, 2, 3, 15, 16, 17, 257, 4001)
SCAN_D = (128, 768)
SCAN_R = (1, 5, 32)
SCAN_AMP = 2
SCAN_COPIES = 9                          # rows equal to probe 0: more than the eight candidates the scan keeps per probe
SCAN_SHARDS = ((257, 130), (4001, 1999))  # (Nb, first row of the second shard)

# seeds: a case that misses a condition of tests/test_search_ref_cpu.py gets another seed here, never a weaker condition
SEEDS = {}


def seed_of(*shape):
    return SEEDS.get(tuple(shape), sum(s * p for s, p in zip(shape, (1000003, 1009, 17, 5))) % (2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------ operands
def edge_rows(Nb, most):
    """Up to `most` library rows at which a tiling can lose a row, the likeliest first: the last row, row 0, the rows on either
    side of every multiple of 256 from the top down (the two-group kernel's tiles, the cut between its launch and the remainder
    launch, the range boundaries of both kernels), then of the odd multiples of 128.  operands() keeps these rows out of the
    copying and makes each of them a query, so every one of them IS the unique winner of some query: a kernel that drops one
    cannot pass."""
    rows = [Nb - 1, 0]
    for step in (range(Nb // 256 * 256, 0, -256), range((Nb // 128 - 1 + Nb // 128 % 2) * 128, 0, -256)):
        for t in step:
            rows += [t - 1, t]
    rows = [r for r in dict.fromkeys(rows) if 0 <= r < Nb]
    return rows[:most]


def library(g, Nb, D, amp, keep=()):
    """int64 [Nb, D] on the lattice, 30 % of the rows copies of other rows (module docstring); the rows in `keep` are neither
    copied nor overwritten"""
    b = torch.randint(-amp, amp + 1, (Nb, D), generator=g, dtype=torch.int64)
    n = int(0.3 * Nb) if Nb >= 2 else 0
    if n:
        src = torch.randint(0, Nb, (n,), generator=g)
        rnd = torch.randint(0, Nb, (n,), generator=g)
        kind = torch.arange(n) % 3
        dst = torch.where(kind == 0, src ^ 1, torch.where(kind == 1, src ^ 16, rnd))
        dst = torch.where(dst < Nb, dst, rnd)
        keep = set(keep)
        for s, d in zip(src.tolist(), dst.tolist()):          # in turn: a copy of a copy is a copy
            if s not in keep and d not in keep:
                b[d] = b[s]
    return b


def queries(g, b, Q, amp, first=()):
    """int64 [Q, D]: library rows, the rows `first` in front; in the second half ~10 % of the entries moved by +-1 and clipped to
    the lattice"""
    idx = torch.randint(0, b.shape[0], (Q,), generator=g)
    idx[:len(first)] = torch.tensor(list(first), dtype=torch.int64)
    q = b[idx].clone()
    h = Q // 2
    assert len(first) <= h
    move = (torch.rand(q[h:].shape, generator=g) < 0.1).long() * (2 * torch.randint(0, 2, q[h:].shape, generator=g) - 1)
    q[h:] = (q[h:] + move).clamp(-amp, amp)
    return q


@functools.lru_cache(maxsize=None)
def operands(Q, Nb, D, amp):
    """(q [Q, D], b [Nb, D]) int64 on the lattice; query i < len(edge_rows(Nb, Q // 8)) is that edge row of the library"""
    g = torch.Generator().manual_seed(seed_of(Q, Nb, D))
    edges = edge_rows(Nb, Q // 8)
    b = library(g, Nb, D, amp, keep=edges)
    return queries(g, b, Q, amp, first=edges), b


def sqnorm(x):
    """|row|^2 as the kernels get it: float32 of the integer"""
    return (x * x).sum(1).float()


@functools.lru_cache(maxsize=None)
def scan_operands(Nb, D, R):
    """(probes [R, D], library [Nb, D]) int64: probe 0 equals SCAN_COPIES library rows (as many as the library has, if fewer), the
    other probes are library rows, the later half of them moved off the library by +-1 entries.  Where the library has more rows
    than the copies take, its LAST row is like no other and probe 1 (if there is one) equals it: the scan masks the rows past Nb
    of the last group of 16 by row index, and must not mask that one."""
    g = torch.Generator().manual_seed(seed_of(Nb, D, R, 3))
    last = Nb > SCAN_COPIES
    b = library(g, Nb, D, SCAN_AMP, keep=[Nb - 1] if last else ())
    rows = torch.randperm(Nb - last, generator=g)[:SCAN_COPIES]
    b[rows] = b[rows[0]].clone()
    p = queries(g, b, R, SCAN_AMP)
    p[0] = b[rows[0]]
    if last and R >= 2:
        p[1] = b[Nb - 1]
    return p, b


# ------------------------------------------------------------------------------------------------ references
def distances(q, b):
    """int64 [Q, Nb] squared distances through |q|^2 + |b|^2 - 2 q.b^T, the form the kernels compute in"""
    q, b = q.long(), b.long()
    return (q * q).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (q @ b.T)


def group_of(R):
    """the 16 rows {64 a + 16 j + 4 g + r: j, r = 0..3} form group (a, g), as ONE integer"""
    return (R >> 6) * 4 + ((R >> 2) & 3)


def pack(d2, R):
    """key = (bits of float32(d2)) << 32 | R for int64 tensors d2 >= 0 and R < 2^32"""
    bits = d2.float().contiguous().view(torch.int32).long()
    return (bits << 32) | R


def _ordered(q, b, row_offset):
    """int64 [Q, Nb]: d2 << 32 | R -- integer order = the lexicographic order of (d2, R)"""
    R = row_offset + torch.arange(b.shape[0], dtype=torch.int64)
    return (distances(q, b) << 32) | R[None, :], R


def reference_keys(q, b, row_offset=0):
    """int64 [2, Q]: both key planes of the definition above for integer operands q [Q, D] and b [Nb, D], Nb >= 1"""
    c, R = _ordered(q, b, row_offset)
    best = c.min(1).values
    outside = group_of(R)[None, :] != group_of(best & 0xFFFFFFFF)[:, None]
    runner = torch.where(outside, c, torch.full_like(c, KEY_EMPTY)).min(1).values
    k0 = pack(best >> 32, best & 0xFFFFFFFF)
    k1 = torch.where(outside.any(1), pack(runner >> 32, runner & 0xFFFFFFFF), torch.full_like(runner, KEY_EMPTY))
    return torch.stack([k0, k1])


def reference_top3(p, b, row_offset=0):
    """int64 [R, 3]: the three lexicographically smallest (d2, row) of every probe, KEY_EMPTY where the library has no more rows"""
    c, _ = _ordered(p, b, row_offset)
    k = min(3, b.shape[0])
    low = c.topk(k, dim=1, largest=False, sorted=True).values
    out = torch.full((p.shape[0], 3), KEY_EMPTY, dtype=torch.int64)
    out[:, :k] = pack(low >> 32, low & 0xFFFFFFFF)
    return out


def tie_shares(q, b, row_offset=0):
    """(share of the queries whose minimum d2 is reached by two or more rows, share of the queries whose second-smallest
    (d2, R) lies inside the winner's group -- there the runner-up is NOT the second-nearest row); Nb >= 2"""
    c, _ = _ordered(q, b, row_offset)
    low = c.topk(2, dim=1, largest=False, sorted=True).values
    tied = (low[:, 0] >> 32) == (low[:, 1] >> 32)
    inside = group_of(low[:, 0] & 0xFFFFFFFF) == group_of(low[:, 1] & 0xFFFFFFFF)
    return tied.float().mean().item(), inside.float().mean().item()


@functools.lru_cache(maxsize=None)
def case_reference(Q, Nb, D):
    """reference_keys of a table case at row_offset 0 (cached: computed once, never modified -- use shifted() for an offset)"""
    c = case_of(Q, Nb, D)
    return reference_keys(*operands(c.Q, c.Nb, c.D, c.amp))


def shifted(keys, row_offset):
    """reference keys of the same library searched at `row_offset` -- for BOTH planes only where row_offset % 64 == 0 (the
    groups move with the rows); plane 0 at any offset"""
    return torch.where(keys == KEY_EMPTY, keys, keys + row_offset)


def describe(got, want):
    """None when the two int64 key tensors are equal, else the first differing entry as (d2, row) pairs"""
    if got.shape == want.shape and torch.equal(got, want):
        return None
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} against {tuple(want.shape)}"
    bad = (got != want).nonzero()
    at = tuple(int(v) for v in bad[0])

    def show(k):
        k = int(k)
        return "KEY_EMPTY" if k == KEY_EMPTY else f"(d2 bits {k >> 32:#x}, row {k & 0xFFFFFFFF})"
    return f"{len(bad)} of {got.numel()} keys differ; first at {at}: got {show(got[at])}, want {show(want[at])}"
