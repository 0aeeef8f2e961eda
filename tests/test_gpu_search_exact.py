"""GPU: the library search (csrc/l2min.hip cmdiad_l2_min_keys, _counted, _segments) and the re-weighting scan (csrc/scan.hip
cmdiad_reweight_scan) held KEY FOR KEY to the integer references of tests/search_ref.py on lattice operands, at the shapes where
these kernels can go wrong: one row, one group of 16 rows (no runner-up), one library tile on the two-group kernel (a prologue
longer than the stream), more library ranges than tiles (blocks that leave), short and uneven ranges, a remainder launch of one
row, D = 64 ... 1024, every live count around the tile edges of the counted launch, a segment stride that is no multiple of the
tile.  On the lattice every value the accumulator takes is exact in fp32 whatever the order of addition and loses nothing to
RowMin's truncation, so both key planes have ONE correct value per query; exact ties occur in quantity and the second-nearest row
often lies inside the winner's group (tests/test_search_ref_cpu.py asserts all of that without a GPU, tests/test_host_cpu.py that
each case reaches the launch its label names).  Every assertion is torch.equal; a failure names the first differing key.

Every key array carries GUARD more entries than the launch has query rows: they must keep what the caller put there."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import search_ref as sr  # noqa: E402
from conftest import need_ab_variants  # noqa: E402

from cmdiad_amd import engine as eng  # noqa: E402
from cmdiad_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 64
DTYPES = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "fp16"]
SHAPES = [(c.Q, c.Nb, c.D) for c in sr.EDGE_CASES]
SHAPE_IDS = [f"{Q}x{Nb}x{D}" for Q, Nb, D in SHAPES]


def _tile(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("CMDIAD_L2_TILE", raising=False)
    else:
        monkeypatch.setenv("CMDIAD_L2_TILE", setting)


@functools.lru_cache(maxsize=None)
def _device_operands(shape, dt):
    """(q16, |q|^2, b16, |b|^2) of a table case on the device: the integers cast to the operand type, the norms computed from the
    integers (not through normalize_cast: test_operand_producer_returns_the_lattice_bit_for_bit ties the two)"""
    c = sr.case_of(*shape)
    q, b = sr.operands(c.Q, c.Nb, c.D, c.amp)
    return q.to(dt).to(DEV), sr.sqnorm(q).to(DEV), b.to(dt).to(DEV), sr.sqnorm(b).to(DEV)


def _keys(Q, runner):
    return ops.new_keys(Q + GUARD, DEV, runner=runner)


def _check(keys, want, Q, what):
    """keys [.., Q + GUARD] from the device against the reference [.., Q]; the guard entries untouched"""
    keys = keys.cpu()
    assert sr.describe(keys[..., :Q], want) is None, f"{what}: {sr.describe(keys[..., :Q], want)}"
    assert bool((keys[..., Q:] == sr.KEY_EMPTY).all()), f"{what}: keys past the {Q} query rows were written"


def _edge_case(shape, dt, setting, monkeypatch):
    _tile(monkeypatch, setting)
    Q = shape[0]
    q16, qsq, b16, bsq = _device_operands(shape, dt)
    ref = sr.case_reference(*shape)
    for row_offset in (0, 192):
        keys = ops.l2_min_keys(q16, qsq, b16, bsq, _keys(Q, True), row_offset=row_offset)
        _check(keys, sr.shifted(ref, row_offset), Q, f"both planes, row_offset {row_offset}")
    for row_offset in (0, 192, 7):
        keys = ops.l2_min_keys(q16, qsq, b16, bsq, _keys(Q, False), row_offset=row_offset)
        _check(keys, sr.shifted(ref[0], row_offset), Q, f"single plane, row_offset {row_offset}")


# ------------------------------------------------------------------------------------------------ 1. the edge table
def test_references_restate_the_key_sentinel():
    assert sr.KEY_EMPTY == ops.KEY_EMPTY


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("setting", sr.SETTINGS, ids=["default", "tile0", "tile5"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_l2_keys_equal_the_definition_at_edge_shapes(shape, setting, dt, monkeypatch):
    _edge_case(shape, dt, setting, monkeypatch)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_l2_keys_equal_the_definition_exact_variant(shape, dt, monkeypatch):
    """the lock-step 256 x 256 formulation of the test-only build (tests/test_gpu_variants.py runs it there)"""
    need_ab_variants(f"CMDIAD_L2_TILE={sr.AB_SETTING}")
    _edge_case(shape, dt, sr.AB_SETTING, monkeypatch)


@pytest.mark.parametrize("runner", [True, False], ids=["two_planes", "one_plane"])
@pytest.mark.parametrize("setting", sr.SETTINGS, ids=["default", "tile0", "tile5"])
def test_l2_empty_inputs_return_the_keys_as_given(setting, runner, monkeypatch):
    """Q = 0 and Nb = 0 (an empty row shard): nothing is launched, the caller's keys stay"""
    _tile(monkeypatch, setting)
    q16, qsq, b16, bsq = _device_operands((129, 65, 192), torch.float16)
    given = torch.arange(2 * 129, dtype=torch.int64, device=DEV).reshape(2, 129) + (1 << 40)
    given = given if runner else given[0].clone()
    keys = ops.l2_min_keys(q16, qsq, b16[:0], bsq[:0], given.clone(), row_offset=64)
    assert torch.equal(keys, given)
    none = given[..., :0].contiguous()
    assert ops.l2_min_keys(q16[:0], qsq[:0], b16, bsq, none.clone()).shape == none.shape
    keys = given.clone()                               # a 0-row query set in front of live keys: none of them is touched
    ops.l2_min_keys(q16[:0], qsq[:0], b16, bsq, keys)
    assert torch.equal(keys, given)


@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("setting", sr.SETTINGS, ids=["default", "tile0", "tile5"])
def test_l2_all_zero_rows_score_zero_and_tie_to_the_lowest(setting, dt, monkeypatch):
    """All-zero rows (background patches) in the library and among the queries: their accumulators start at -0.0 and every product
    is a signed zero, and RowMin compares accumulator BITS -- a zero query against a zero row must still be the smallest value there
    is, tie to the lowest zero row, and name the nearest zero row of another group as its runner-up."""
    _tile(monkeypatch, setting)
    c = sr.case_of(513, 1279, 256)
    q, b = (t.clone() for t in sr.operands(c.Q, c.Nb, c.D, c.amp))
    zero_rows, zero_queries = [6, 7, 22, 300, 1023, 1024, 1278], [0, 100, 512]
    b[zero_rows] = 0
    q[zero_queries] = 0
    ref = sr.reference_keys(q, b)
    assert ref[:, zero_queries].tolist() == [[6] * 3, [300] * 3]         # d2 bits 0: rows 6, 7 and 22 share group (0, 1)
    keys = ops.l2_min_keys(q.to(dt).to(DEV), sr.sqnorm(q).to(DEV), b.to(dt).to(DEV), sr.sqnorm(b).to(DEV), _keys(c.Q, True))
    _check(keys, ref, c.Q, "zero rows")


# ------------------------------------------------------------------------------------------------ 2. shards
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("setting", sr.SETTINGS, ids=["default", "tile0", "tile5"])
@pytest.mark.parametrize("shape,cuts", sr.SHARD_CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}" for s, _ in sr.SHARD_CASES])
def test_l2_shards_merge_to_the_whole_library(shape, cuts, setting, dt, monkeypatch):
    """shards cut at multiples of 64 -- one of exactly 64 rows, one empty, a ragged last one -- each searched on its own with its
    row_offset and merged with engine.merge_key_planes: the whole library's reference on both planes (plane 0 alone: torch.minimum)"""
    _tile(monkeypatch, setting)
    Q = shape[0]
    q16, qsq, b16, bsq = _device_operands(shape, dt)
    ref = sr.case_reference(*shape)
    for runner in (True, False):
        merged = None
        for lo, hi in zip(cuts, cuts[1:]):
            k = ops.l2_min_keys(q16, qsq, b16[lo:hi].contiguous(), bsq[lo:hi].contiguous(), _keys(Q, runner), row_offset=lo)
            if hi == lo:
                assert bool((k == ops.KEY_EMPTY).all()), "an empty shard finds nothing"
            merged = k if merged is None else eng.merge_key_planes(merged, k)
        _check(merged, ref if runner else ref[0], Q, f"{len(cuts) - 1} shards, {'both planes' if runner else 'plane 0'}")


# ------------------------------------------------------------------------------------------------ 3. the counted launch
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("setting", ["0", "5"], ids=["tile0", "tile5"])
def test_l2_counted_launch_searches_the_live_rows_only(setting, dt, monkeypatch):
    """rows < count hold the reference, rows >= count what new_keys put there, for every count around the tile edges of both
    kernels (counts stay <= Q_max: the caller's contract, L2Params::q_count)"""
    _tile(monkeypatch, setting)
    Q = sr.COUNTED_Q_MAX
    q16, qsq, b16, bsq = _device_operands(sr.COUNTED_CASE, dt)
    ref = sr.case_reference(*sr.COUNTED_CASE)
    for count in sr.COUNTED_COUNTS:
        cnt = torch.tensor([count], dtype=torch.int32, device=DEV)
        for runner in (True, False):
            want = (ref if runner else ref[0]).clone()
            want[..., count:] = sr.KEY_EMPTY
            keys = ops.l2_min_keys_counted(q16, qsq, cnt, b16, bsq, _keys(Q, runner))
            _check(keys, want, Q, f"count {count}, {'both planes' if runner else 'plane 0'}")


# ------------------------------------------------------------------------------------------------ 4. the segments launch
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("row_offset", [0, 192])
@pytest.mark.parametrize("setting", sr.SEGMENT_SETTINGS, ids=["default", "tile0"])
@pytest.mark.parametrize("counts", sr.SEGMENT_COUNTS, ids=["in_range", "clamped"])
def test_l2_segments_launch_searches_each_segments_live_rows(counts, setting, row_offset, dt, monkeypatch):
    """query rows [w * stride, w * stride + min(max(count[w], 0), stride)) hold the reference of their own rows, every other row
    keeps the (distinct) value the caller put there; the stride is a multiple of neither tile"""
    _tile(monkeypatch, setting)
    stride, n_seg = sr.SEGMENT_STRIDE, len(counts)
    Q = n_seg * stride
    q16, qsq, b16, bsq = _device_operands(sr.SEGMENT_CASE, dt)
    ref = sr.shifted(sr.case_reference(*sr.SEGMENT_CASE), row_offset)
    src = torch.arange(Q) % q16.shape[0]                  # query row i of the launch is row i mod 513 of the case
    qa, qa_sq = q16[src.to(DEV)].contiguous(), qsq[src.to(DEV)].contiguous()
    live = torch.zeros(Q, dtype=torch.bool)
    for w, c in enumerate(counts):
        live[w * stride:w * stride + min(max(c, 0), stride)] = True
    seg = torch.tensor(counts, dtype=torch.int32, device=DEV)
    for runner in (True, False):
        given = sr.KEY_EMPTY - 1 - torch.arange(2 * Q, dtype=torch.int64).reshape(2, Q)    # above every key a search can write
        given[:, live] = sr.KEY_EMPTY
        r = ref[:, src]
        want = torch.where(live[None, :], r, given)
        given, want = (given, want) if runner else (given[0].clone(), want[0].clone())
        keys = _keys(Q, runner)
        keys[..., :Q] = given.to(DEV)
        ops.l2_min_keys_segments(qa, qa_sq, seg, stride, b16, bsq, keys, row_offset=row_offset)
        _check(keys, want, Q, f"counts {counts}, {'both planes' if runner else 'plane 0'}")


# ------------------------------------------------------------------------------------------------ 5. the operand producer
@pytest.mark.parametrize("dt", DTYPES, ids=DT_IDS)
def test_operand_producer_returns_the_lattice_bit_for_bit(dt):
    """ops.normalize_cast, the engine's only producer of search operands, on the integer-valued fp32 rows: the same 16-bit rows
    and the same squared norms as the tests above feed, bit for bit"""
    c = sr.case_of(513, 1279, 256)
    q16, qsq, b16, bsq = _device_operands((c.Q, c.Nb, c.D), dt)
    for x, x16, xsq in zip(sr.operands(c.Q, c.Nb, c.D, c.amp), (q16, b16), (qsq, bsq)):
        o16, _, sq = ops.normalize_cast(x.float().to(DEV), 0.0, 1.0, dtype=dt)
        assert o16.dtype == dt and torch.equal(o16.view(torch.int16), x16.view(torch.int16))
        assert torch.equal(sq.view(torch.int32), xsq.view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6. the re-weighting scan
@pytest.mark.parametrize("R", sr.SCAN_R)
@pytest.mark.parametrize("D", sr.SCAN_D)
@pytest.mark.parametrize("Nb", sr.SCAN_NB)
def test_reweight_scan_returns_the_three_smallest_keys(Nb, D, R):
    """the scan's approximate keys are exact on the lattice: the three lexicographically smallest (d2, row) of every probe, with
    KEY_EMPTY where the library has fewer than three rows; probe 0 equals nine library rows (more than the eight candidates kept)"""
    p, b = sr.scan_operands(Nb, D, R)
    dp, db = p.float().to(DEV), b.float().to(DEV)
    for row_offset in (0, 1000):
        top3 = ops.reweight_scan(dp, db, row_offset=row_offset).cpu()
        want = sr.reference_top3(p, b, row_offset)
        assert sr.describe(top3, want) is None, f"row_offset {row_offset}: {sr.describe(top3, want)}"


@pytest.mark.parametrize("D", sr.SCAN_D)
@pytest.mark.parametrize("Nb,cut", sr.SCAN_SHARDS)
def test_reweight_scan_shards_chain_to_the_whole_library(Nb, cut, D):
    p, b = sr.scan_operands(Nb, D, 32)
    dp, db = p.float().to(DEV), b.float().to(DEV)
    want = sr.reference_top3(p, b)
    for first, second in (((0, cut), (cut, Nb)), ((cut, Nb), (0, cut))):       # in either order
        top3 = ops.reweight_scan(dp, db[first[0]:first[1]].contiguous(), row_offset=first[0])
        top3 = ops.reweight_scan(dp, db[second[0]:second[1]].contiguous(), top3=top3, row_offset=second[0]).cpu()
        assert sr.describe(top3, want) is None, sr.describe(top3, want)


def test_reweight_scan_pair_equals_two_single_calls_and_the_reference():
    (p0, b0), (p1, b1) = sr.scan_operands(257, 128, 5), sr.scan_operands(17, 128, 1)
    d = [t.float().to(DEV) for t in (p0, b0, p1, b1)]
    blk0, blk1 = ops.bank_block16(d[1]), ops.bank_block16(d[3])
    t0, t1 = ops.reweight_scan_pair(d[0], d[1], blk0, d[2], d[3], blk1, row_offset0=0, row_offset1=64)
    assert torch.equal(t0, ops.reweight_scan(d[0], d[1], blk0)) and torch.equal(t1, ops.reweight_scan(d[2], d[3], blk1, row_offset=64))
    assert sr.describe(t0.cpu(), sr.reference_top3(p0, b0)) is None, sr.describe(t0.cpu(), sr.reference_top3(p0, b0))
    assert sr.describe(t1.cpu(), sr.reference_top3(p1, b1, 64)) is None, sr.describe(t1.cpu(), sr.reference_top3(p1, b1, 64))
