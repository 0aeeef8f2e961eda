"""CPU: the preconditions of tests/test_gpu_gemm_edges.py, checked on the very operands and references of tests/gemm_ref.py.

The GPU file compares bit patterns.  That is only a statement about the kernels if (1) fp32 accumulation of these operands is exact
in every order, (2) no reference carries a sentinel bit pattern, (3) the bf16 outputs really need rounding, with truncation and
round-half-up each giving another answer than nearest-even, and (4) the slab bookkeeping of the split-K references is the kernels'
per = ceil(KT / split) rule, with an empty slab where a case claims one."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_ref as er  # noqa: E402
import gemm_ref as gr  # noqa: E402

CASES = gr.all_cases()
SHAPES = list(dict.fromkeys(s for s, _ in CASES))


def _on_lattice(x, step):
    return bool((x.double() / step == (x.double() / step).round()).all())


def test_case_tables_hold_what_the_issue_lists():
    assert len(gr.GENERAL_SHAPES) == 9 and len(gr.WIDE256_SHAPES) == 5 and len(gr.SETTINGS) == 3
    assert sorted({s[2] // gr.BK for s in gr.GENERAL_SHAPES}) == [1, 2, 3, 4, 5, 8, 16]          # K-tiles against the 3-stage pipeline
    assert {f.split for f in gr.GENERAL_FORMS} == {1, 2, 3, 5} and {f.group_rows for f in gr.GENERAL_FORMS} == {0, 1, 32}
    assert all(s[1] % 256 == 0 and s[2] >= 192 for s in gr.WIDE256_SHAPES) and min(s[0] for s in gr.WIDE256_SHAPES) < 128
    assert {k for k, _, _, _ in gr.PITCHED_CASES} == {"general", "res_rows", "ln", "pp3", "res_wide"}
    assert all(s[1] % 64 == 0 for k, _, s, _ in gr.PITCHED_CASES if k in ("res_rows", "ln"))
    p = gr.PITCHED
    assert p.a % 8 == 0 and p.w % 8 == 0 and p.r % 4 == 0 and p.o32 % 4 == 0 and p.o16 % 8 == 0 and p.xb % 4 == 0 and p.add2 % 4 == 0
    assert len({p.r, p.o32, p.o16}) == 3 and p.a != p.w and min(p) > 0
    assert all(K <= 1024 for _, _, K in SHAPES) and all(c[0] <= 1024 and c[0] % 64 == 0 for c in gr.TN_CASES)
    assert all(M * N <= 1.2e6 for M, N, _ in SHAPES)


@pytest.mark.parametrize("shape", SHAPES)
def test_operands_sit_on_their_lattices(shape):
    o = gr.operands(*shape)
    assert _on_lattice(o.A, 1) and o.A.abs().max() <= 4 and _on_lattice(o.W, 1) and o.W.abs().max() <= 2
    for t in (o.bias, o.gb1, o.gb32):
        assert _on_lattice(t, 0.25) and t.abs().max() <= 8
    for t in (o.res, o.add2):
        assert _on_lattice(t, 0.5) and t.abs().max() <= 32
    assert set(o.rscale.tolist()) <= {0.25, 0.5, 1.0, 2.0}
    for t in (o.A, o.W):                                        # the GEMM operands are exact in bf16
        assert torch.equal(t.bfloat16().float(), t)
    assert torch.equal(torch.tensor(gr.PAD_VALUE).bfloat16().float().isfinite(), torch.tensor(True))
    # the worst partial sum of ANY order is bounded by sum |a| |w|: with the largest scale and every addend, far below 2^24 / 16
    worst = float((o.A.double().abs() @ o.W.double().abs().T).max()) * 2 + 8 + 8 + 32 + 32
    assert worst < 2 ** 15 < 2 ** 24 / 16


@pytest.mark.parametrize("shape", SHAPES)
def test_fp32_accumulation_is_exact_in_two_orders(shape):
    o = gr.operands(*shape)
    fwd, rev = gr.fp32_product_two_orders(o.A, o.W)
    ref = o.A.double() @ o.W.double().T
    assert torch.equal(fwd.double(), ref) and torch.equal(rev.double(), ref)


@pytest.mark.parametrize("shape,form", CASES, ids=lambda v: v.name if hasattr(v, "name") else "x".join(map(str, v)))
def test_references_are_exact_in_fp32_and_free_of_sentinels(shape, form):
    o = gr.operands(*shape)
    for add2 in ((False, True) if form.residual and form.outs == "f32" else (False,)):
        pre, out = gr.reference(o, form, add2=add2)
        assert torch.equal(pre.float().double(), pre) and _on_lattice(pre, 1 / 16)
        if form.act != gr.ACT_GELU:
            assert torch.equal(out.float().double(), out) and _on_lattice(out, 1 / 16)     # the reference equals its own fp32 cast
        assert not gr.has_sentinel(out) and not gr.has_sentinel(pre)
        assert not (out == 0).logical_and(torch.signbit(out)).any()
        if form.split > 1:
            assert torch.equal(out.sum(0), o.A.double() @ o.W.double().T)


def test_bf16_outputs_need_rounding_and_the_rounding_mutants_differ():
    """Over all bf16-output cases of M N >= 256 at least 1 % of the reference values are not bf16 numbers, and on each case whose
    values leave the integers (a bias: quarters) truncation and round-half-up each differ from nearest-even somewhere.  The one
    form without a bias holds integers, |sum| of standard deviation 3.7 sqrt(K): below 256, where every integer IS a bf16 number,
    for all but a handful of elements even at K = 1024 -- that form is held to the same f2bf through the cases next to it."""
    total = inexact = 0
    for shape, form in CASES:
        M, N, _ = shape
        if form.outs == "f32" or M * N < 256:
            continue
        _, out = gr.reference(gr.operands(*shape), form)
        if form.act == gr.ACT_GELU:
            out = out.float().double()                          # what an exact fp32 GELU would hand to the cast
        bad = gr.bf16_inexact(out)
        total += out.numel()
        inexact += int(bad.sum())
        if not form.bias:
            continue
        rne = er.bf16_rne(out.float())
        assert not torch.equal(er.bf16_trunc(out.float()), rne), (shape, form.name, "truncation")
        assert not torch.equal(er.bf16_half_up(out.float()), rne), (shape, form.name, "half-up")
    assert total > 0 and inexact >= 0.01 * total


def test_slab_rule_is_the_kernels_and_the_empty_slabs_exist():
    for KT in range(1, 40):
        for split in range(1, 12):
            per = -(-KT // split)
            got = gr.slab_ranges(KT, split)
            assert len(got) == split and sum(n for _, n in got) == KT
            for y, (k0, n) in enumerate(got):
                assert k0 == y * per and n == max(0, min(per, KT - k0))      # gemm_std_kernel / gemm_tn_kernel: kt_begin, kt_count
            used = -(-KT // per)                                              # cmdiad_gemm_bf16 zeroes slabs used .. split - 1
            assert [n > 0 for _, n in got] == [y < used for y in range(split)]
    # the cases that claim an empty slab have one
    assert gr.slab_ranges(576 // 64, 4) == [(0, 3), (3, 3), (6, 3), (9, 0)] and (576, 200, 328, 4, False) in gr.TN_CASES
    empty = [(s, f.split) for s in gr.GENERAL_SHAPES for f in gr.GENERAL_FORMS if f.split > 1 and gr.slab_ranges(s[2] // 64, f.split)[-1][1] == 0]
    assert ((255, 260, 256), 3) in empty and len({sp for _, sp in empty}) == 3
    pitched_split = [(s, f) for k, _, s, f in gr.PITCHED_CASES if f.split > 1]
    assert pitched_split and all(gr.slab_ranges(s[2] // 64, f.split)[-1][1] == 0 for s, f in pitched_split)
    # gemm_tn refuses split > M / 64, so every slab but those cut off by the ceil rule has a K-step
    assert all(split <= M // 64 for M, _, _, split, _ in gr.TN_CASES)


@pytest.mark.parametrize("case", gr.TN_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_gemm_tn_references(case):
    M, N1, N2, split, _ = case
    P, Q = gr.tn_operands(M, N1, N2)
    assert _on_lattice(P, 1) and P.abs().max() <= 4 and _on_lattice(Q, 1) and Q.abs().max() <= 2
    slabs, cs = gr.tn_reference(P, Q, split)
    assert slabs.shape == (split, N1, N2) and cs.shape == (split, N1)
    full = P.double().T @ Q.double()
    assert torch.equal(slabs.sum(0), full) and torch.equal(cs.sum(0), P.double().sum(0))
    fwd, rev = gr.fp32_product_two_orders(P.T.contiguous(), Q.T.contiguous())
    assert torch.equal(fwd.double(), full) and torch.equal(rev.double(), full)
    assert torch.equal(slabs.float().double(), slabs) and not gr.has_sentinel(slabs) and not gr.has_sentinel(cs)
    # asymmetric: the transposed product is another matrix (or another shape)
    assert N1 != N2 or not torch.equal(full, full.T)
    assert float((P.double().abs().T @ Q.double().abs()).max()) < 2 ** 14


def test_streamk_edge_shapes_are_what_they_claim():
    tiles = [((M + 255) // 256) * (N // 256) for M, N, _ in gr.STREAMK_SHAPES]
    assert tiles == [257, 511, 258, 511] and [M % 256 for M, _, _ in gr.STREAMK_SHAPES] == [1, 1, 156, 0]
    for (M, N, K), t in zip(gr.STREAMK_SHAPES, tiles):            # cmdiad_gemm_streamk_eligible, restated
        KT = K // 64
        assert N % 256 == 0 and K % 64 == 0 and K >= 192 and t * KT // 256 >= KT and 256 < t < 512
