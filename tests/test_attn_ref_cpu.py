"""tests/attn_ref.py on its own: the float64 tile model against plain float64 softmax attention, and the fp32 emulation of the
kernel's loop on the routing inputs, whose expected outputs must come out bit for bit.  No GPU, no cmdiad_amd import."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402


@pytest.mark.parametrize("T", [1, 63, 65, 257])
def test_tile_model_vs_plain_float64_softmax(T):
    """The model differs from softmax_2(q k^T) v only by the bf16 rounding of P (the lazy reference and the tiling cancel in
    O / l).  Two bounds: what that rounding can do at most, 2^-8 x sum_i w_i |v_i| per (query, column) (every P within 2^-8 of
    itself, relative); and the slack the stage-by-stage test grants the kernel against the model, 2^-7 x the query's largest
    weight x the column's largest |v|, plus 1e-5 of the output scale.  The second is not implied by the first under near-uniform
    attention (it holds outright only where sum w |v| <= 2 x largest weight x largest |v|); with these operands -- scores with a
    spread of ~2.4 log2 units -- it is met with the ratio printed below (0.99 at T = 257)."""
    B, H = 3, 2
    q, k, v = ar.spiked_operands(B, H, T, 100 + T)
    stats = {}
    out, peak, l_run = ar.attention_tile_model(q, k, v, T, stats)
    sc = q.double() @ k.double().transpose(-2, -1)
    w = torch.softmax(sc * torch.log(torch.tensor(2.0, dtype=torch.float64)), -1)
    ref = w @ v.double()
    assert torch.allclose(peak, w.amax(-1), rtol=1e-12, atol=0)
    bound = 2.0 ** -7 * w.amax(-1)[..., None] * v.double().abs().amax(2)[:, :, None, :] + 1e-5 * float(ref.abs().mean())
    err = (out - ref).abs()
    assert bool((err <= 2.0 ** -8 * (w @ v.double().abs()) * (1 + 1e-9) + 1e-12).all())          # (+ float64's own noise)
    print(f"T = {T}: reference moved in {stats['moved']} (head, later tile) pairs; largest |model - exact| / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    if T > 64:
        assert stats["moved"] >= 1          # the planted spike exercised the moving reference
    assert bool((l_run > 0).all())


def test_emulate_fp32_vs_tile_model_pooled_share():
    """The baseline the device's figure is read against (tests/test_gpu_attention_edges.py, same grid, same operands): the fp32
    emulation against the float64 model, every element within the stage test's bound, and the share of elements that are not the
    nearest bf16 of the model's value, pooled over the grid, below the stage's threshold."""
    miss = total = 0
    for B, H in ar.EDGE_BH:
        for T in ar.EDGE_T:
            q, k, v = ar.spiked_operands(B, H, T, ar.edge_seed(B, H, T))
            a_ref, peak, _ = ar.attention_tile_model(q, k, v, T)
            out, _ = ar.emulate_fp32(q, k, v, T)
            off = ar._ulp_check(out.to(torch.bfloat16), a_ref, f"emulation B={B} H={H} T={T}", max_ulps=1.05, frac_off=1.0,
                                abs_slack=ar.attention_slack(peak, v.double(), a_ref))
            miss, total = miss + off * a_ref.numel(), total + a_ref.numel()
    print(f"fp32 emulation, not the nearest bf16 of the model's value, pooled over the grid: {miss / total:.2e} ({round(miss)} of {total})")
    assert miss / total <= 5e-3


@pytest.mark.parametrize("B,H,T,kind", ar.routing_cases(), ids=lambda v: str(v))
def test_emulate_fp32_routing_bit_exact(B, H, T, kind):
    q, k, v, want = ar.routing_inputs(B, H, T, kind, ar.routing_seed(B, H, T))
    for t in (q, k, v, want):
        assert torch.equal(ar.r16(t), t)                                     # bf16 holds every operand and result exactly
    sc = q.double() @ k.double().transpose(-2, -1)
    hot = 220.0 if kind == "one_hot" else 200.0
    top = sc.amax(-1)
    assert bool(((top == hot) | (top == 220.0)).all())                       # (a two-hot query without a partner stays one-hot)
    n_hot = (sc == top[..., None]).sum(-1)
    assert bool((n_hot <= 2).all()) and bool(((sc == top[..., None]) | (sc <= top[..., None] - 40.0)).all())
    out, l = ar.emulate_fp32(q, k, v, T)
    assert torch.equal(l, n_hot.float())                                     # l is exactly 1 or 2
    assert torch.equal(out, want)
    if kind != "one_hot":
        assert int((n_hot == 2).sum()) > 0                                   # the tie really occurs
    if kind == "one_hot":                                                   # a permutation with the forced ends
        j = (sc == 220.0).double().argmax(-1)
        assert bool((j[..., 0] == T - 1).all()) and bool((j[..., -1] == 0).all())
        assert bool((j.sort(-1).values == torch.arange(T)).all())
