"""CPU: tests/encoder_ref.py pinned without a GPU.  The float32 reference equals a float64 and an int64 evaluation of the same
chain (so the lattice really is exact), the preconditions of the exact GPU comparison hold on every grid case, and the reference
differs on every grid case from each mutant of itself that models a defect the GPU tests are there to catch: the inputs would
show it."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as er  # noqa: E402

IDS = [f"{g}x{m}" for g, m in er.GRID]


RAGGED = [c for c in er.GRID if c[0] * c[1] % 128]


@functools.lru_cache(maxsize=1)
def _kept(groups, Mg):
    return er.reference(groups, Mg, keep=True)


@pytest.fixture(scope="module", params=er.GRID, ids=IDS)
def kept(request):
    """one grid case with the values before rounding and before the maximum kept; shared by the tests below, left unchanged"""
    groups, Mg = request.param
    return groups, Mg, _kept(groups, Mg)


def test_preconditions_hold(kept):
    groups, Mg, r = kept
    print(r["stats"])
    er.check_preconditions(r["stats"], Mg)


@pytest.mark.parametrize("groups,Mg", er.GRID, ids=IDS)
def test_float32_equals_float64_and_int64(groups, Mg):
    r = er.case(groups, Mg)
    r64 = er.reference(groups, Mg, dtype=torch.float64)
    for k in ("h2", "g16", "h3"):
        assert torch.equal(r[k].view(torch.int16), r64[k].view(torch.int16)), k
    for k in ("g32", "gb", "tok"):
        assert r64[k].dtype == torch.float64 and torch.equal(r[k].double(), r64[k]), k
    if groups * Mg > 40000:      # (int64 matrix products run unblocked on the CPU: the two largest cases would take a minute)
        return
    ri = er.reference_int(groups, Mg)
    for k in ("h2", "g32", "g16", "gb", "h3", "tok"):
        assert torch.equal((r[k].double() * 8).long(), ri[k]) and torch.equal(ri[k].double() / 8, r[k].double()), k


def test_bf16_roundings_and_ties():
    x = torch.tensor([257.0, 258.0, 259.0, 3.0, -257.0, -259.0, 1.00390625, 1.01171875, 0.0])    # 257 and 259 are ties at step 2
    assert er.bf16_rne(x).tolist() == [256.0, 258.0, 260.0, 3.0, -256.0, -260.0, 1.0, 1.015625, 0.0]
    assert er.bf16_trunc(x).tolist() == [256.0, 258.0, 258.0, 3.0, -256.0, -258.0, 1.0, 1.0078125, 0.0]
    assert er.bf16_half_up(x).tolist() == [258.0, 258.0, 260.0, 3.0, -258.0, -260.0, 1.0078125, 1.015625, 0.0]
    assert er.is_tie(x).tolist() == [True, False, True, False, True, True, True, True, False]
    v = (x[:6] * 8).long()
    assert (er.bf16_rne_int(v).double() / 8).tolist() == er.bf16_rne(x[:6]).tolist()


@pytest.mark.parametrize("mode", er.MAX_MUTANTS)
def test_reference_differs_from_maximum_mutants(kept, mode):
    """a maximum that skips row 0, row Mg - 1 or rows 16-31 of a group, is seeded with 0, or has its boundaries 32 rows off: the
    stage-1 maxima AND the tokens (384 and 256 wide) change"""
    groups, Mg, r = kept
    w = er.weights()
    assert not torch.equal(er.group_max(r["h2p"], groups, Mg, mode), r["g32"])
    assert not torch.equal(er.tokens(w, r["acc4"], groups, Mg, mode), r["tok"])
    assert not torch.equal(er.tokens(w, r["acc4"][:, :256], groups, Mg, mode), r["tok"][:, :256])
    if mode.startswith("skip"):     # row coverage: EVERY checked group shows a dropped row, in both maxima
        for gi in er.checked_groups(groups, Mg):
            assert not torch.equal(er.group_max(r["h2p"], groups, Mg, mode)[gi], r["g32"][gi]), gi
            assert not torch.equal(er.tokens(w, r["acc4"][:, :256], groups, Mg, mode)[gi], r["tok"][gi, :256]), gi


@pytest.mark.parametrize("rnd", [er.bf16_trunc, er.bf16_half_up], ids=["trunc", "half_up"])
def test_reference_differs_from_rounding_mutants(kept, rnd):
    """bf16 by truncation / by round-half-up, in h2 alone and in h3 alone: the stored tensor and the tokens change"""
    groups, Mg, r = kept
    w = er.weights()
    h2m = rnd(r["h2p"])
    assert not torch.equal(h2m, r["h2"])
    _, h3m = er.conv3(w, h2m, r["gb"], Mg)
    assert not torch.equal(er.tokens(w, er.conv4(w, h3m), groups, Mg), r["tok"])
    h3m = rnd(r["h3p"])
    assert not torch.equal(h3m, r["h3"])
    assert not torch.equal(er.tokens(w, er.conv4(w, h3m), groups, Mg), r["tok"])
    assert not torch.equal(rnd(r["g32"]), r["g16"])


def test_reference_differs_from_maximum_after_rounding(kept):
    groups, Mg, r = kept
    late = er.group_max(r["h2"].float(), groups, Mg)
    assert not torch.equal(late, r["g32"])
    assert torch.equal(late.to(torch.bfloat16), r["g16"])       # (rounding is monotone: only the fp32 maxima can tell)


def test_reference_differs_without_b4(kept):
    groups, Mg, r = kept
    assert not torch.equal(er.tokens(er.weights(), r["acc4"], groups, Mg, use_b4=False), r["tok"])


@pytest.mark.parametrize("groups,Mg", RAGGED, ids=[f"{g}x{m}" for g, m in RAGGED])
def test_reference_differs_from_padded_ragged_tile(groups, Mg):
    """copies of the last row in the ragged tile's unused rows, taking part in the last stored group's maximum.  With the last
    group's bias they are that row again and change nothing; without one (rows past the last group have none) the tokens change."""
    r, w = _kept(groups, Mg), er.weights()
    assert torch.equal(torch.maximum(r["tok"][-1], r["acc4"][-1] + w["b4"]), r["tok"][-1])
    for n_out in er.N_OUT:
        assert not torch.equal(er.padded_tail_tokens(w, r["h2"], r["gb"], groups, Mg, n_out), r["tok"][:, :n_out])


@pytest.mark.parametrize("N,K,groups,Mg", er.GROUPMAX_GRID)
def test_groupmax_cases(N, K, groups, Mg):
    c = er.groupmax_case(N, K, groups, Mg)
    er.check_groupmax_preconditions(c["stats"], N, Mg)
    er.check_groupmax_preconditions(c["stats_nb"], N, Mg)
    acc64 = c["A"].double() @ c["W"].double().T
    assert torch.equal(acc64, c["acc"].double())
    assert torch.equal(er.group_max(acc64, groups, Mg) + c["bias"].double(), c["out"].double())
    for mode in er.MAX_MUTANTS[:4] + (("shift32",) if groups > 1 else ()):
        assert not torch.equal(er.group_max(c["acc"], groups, Mg, mode), c["out_nb"]), mode
