"""GPU: the training-step kernels one at a time against a plain float64 restatement on the CPU, computed on the same fp32 / bf16
inputs the kernel reads (loss head, Adam, the deterministic reductions, LayerNorm / BatchNorm parameter gradients, the layout
kernels, the GEMM training epilogues) -- and the shared erf-GELU over the whole fp32 range.  The whole-network training tests
(test_gpu_train.py, test_gpu_conv_train.py) compare at cosine 0.93 .. 0.995; these bound each kernel to its own rounding."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cmdiad_amd import ops, train  # noqa: E402

DEV = "cuda"
U32 = 2.0 ** -24          # fp32 unit roundoff
GELU_ABS = 5.3e-7         # common.h: |gelu_erf - GELU| for every finite x
CANARY = 12345.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _p(t):
    return ops._p(t)


def _s():
    return ops._stream()


def _d(t):
    return t.detach().cpu().double()


def _gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def _gelu_grad64(x):
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _assert_within(got, ref, tol, what):
    got, ref = _d(got), _d(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        t = tol.reshape(-1)[i] if torch.is_tensor(tol) and tol.numel() > 1 else tol
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} outside the bound; first at flat index {i}: "
                             f"got {got.reshape(-1)[i].item()!r} ref {ref.reshape(-1)[i].item()!r} bound {float(t)!r}")


def _bf16_bound(ref, extra=0.0):
    """|bf16(v) - ref| for a v within `extra` of ref: half a bf16 ulp (<= 2^-8 |v|) + extra."""
    return 2.0 ** -8 * (ref.abs() + extra) + extra


# ---------------------------------------------------------------------------------------------------------------- loss head
_MODES = {"l2": 0, "cos_dist": 1, "smooth_l1": 2}
_ACTS = {"gelu": 0, "none": 1, "sigmoid": 2}


def _act64(z, act):
    return _gelu64(z) if act == "gelu" else z if act == "none" else torch.sigmoid(z)


def _loss_ref(z, t, mode, act, inv_b):
    """float64 torch: (row_loss, dL/dz of inv_b * sum(row_loss), y) on the kernel's fp32 inputs."""
    z = z.double().requires_grad_(True)
    t = t.double()
    y = _act64(z, act)
    tv = torch.sigmoid(t) if act == "sigmoid" else t
    if mode == "l2":
        rl = torch.linalg.norm(y - tv, dim=1)
    elif mode == "cos_dist":
        rl = 1.0 - torch.cosine_similarity(y, tv, dim=1)
    else:
        rl = torch.nn.SmoothL1Loss(reduction="none")(y, tv).sum(1)
    (g,) = torch.autograd.grad(rl.sum() * inv_b, z)
    return rl.detach(), g, y.detach()


def _loss_head(z, t, mode, act, inv_b, want_dz=True, want_y=True):
    M, D = z.shape
    rl = torch.full((M + 4,), CANARY, dtype=torch.float32, device=DEV)
    dz = torch.empty((M, D), dtype=torch.bfloat16, device=DEV) if want_dz else None
    y = torch.empty((M, D), dtype=torch.float32, device=DEV) if want_y else None
    code = _MODES[mode] | (_ACTS[act] << 8)
    ops._call("cmdiad_loss_head", _p(z), _p(t), M, D, code, float(inv_b), _p(rl), _p(dz), _p(y), _s())
    torch.cuda.synchronize()
    assert torch.all(rl[M:] == CANARY), "row_loss written past M"
    return rl[:M], dz, y


@pytest.mark.parametrize("D", [4, 60, 256, 772])
def test_loss_head_against_float64(D):
    M, inv_b = 7, 1.0 / 3.0                       # M % 4 != 0: the last block holds three rows
    g = _gen(100 + D)
    z = (1.5 * torch.randn(M, D, generator=g)).float()
    t = torch.randn(M, D, generator=g).float()
    zd, td = z.to(DEV), t.to(DEV)
    for mode in _MODES:
        for act in _ACTS:
            what = f"{mode}/{act}/D={D}"
            rl, dz, y = _loss_head(zd, td, mode, act, inv_b)
            rl_ref, g_ref, y_ref = _loss_ref(z, t, mode, act, inv_b)
            # 1 - cos cancels: the cosine itself carries fp32 rounding of its three dot products, an absolute error
            np.testing.assert_allclose(rl.cpu().numpy(), rl_ref.numpy(), rtol=1e-5, atol=1e-6 if mode == "cos_dist" else 0.0,
                                       err_msg=what)
            if act == "gelu":
                _assert_within(y, y_ref, GELU_ABS, f"{what} y_out")
            elif act == "sigmoid":
                _assert_within(y, y_ref, 1e-6, f"{what} y_out")
            else:
                assert torch.equal(y.cpu(), z), f"{what}: y_out of the identity activation"
            _assert_within(dz, g_ref, _bf16_bound(g_ref) + 1e-5 * g_ref.abs().max(), f"{what} dz3")
            rl2, _, _ = _loss_head(zd, td, mode, act, inv_b, want_dz=False, want_y=False)
            assert torch.equal(rl2, rl), f"{what}: row_loss differs without the dz3 / y_out outputs"


def test_loss_and_grad_is_loss_head_then_sum_vector():
    """ops.loss_and_grad is ops.loss_head followed by ops.sum_vector with 1 / batch in both -- the same two launches, so the loss
    and the gradient are theirs bit for bit, with and without the gradient; and the names of ops are this file's mode numbers."""
    assert (ops.LOSS_L2, ops.LOSS_COS_DIST, ops.LOSS_SMOOTH_L1) == tuple(_MODES[k] for k in ("l2", "cos_dist", "smooth_l1"))
    assert (ops.LOSS_OUT_GELU, ops.LOSS_OUT_NONE, ops.LOSS_OUT_SIGMOID) == tuple(_ACTS[k] << 8 for k in ("gelu", "none", "sigmoid"))
    M, D, batch = 7, 4, 3
    g = _gen(100 + D)
    z = (1.5 * torch.randn(M, D, generator=g)).float().to(DEV)
    t = torch.randn(M, D, generator=g).float().to(DEV)
    for mode in _MODES.values():
        for act in _ACTS.values():
            rl, dz = ops.loss_head(z, t, mode, act << 8, 1.0 / batch)
            want = ops.sum_vector(rl, 1.0 / batch)
            assert want.dim() == 0 and dz.dtype == torch.bfloat16 and dz.shape == z.shape
            for need_grad in (True, False):
                loss, grad = ops.loss_and_grad(z, t, mode, batch, need_grad, out_act=act << 8)
                assert loss.shape == want.shape and torch.equal(loss.view(torch.int32), want.view(torch.int32)), (mode, act, need_grad)
                if need_grad:
                    assert torch.equal(grad.view(torch.int16), dz.view(torch.int16)), (mode, act)
                else:
                    assert grad is None


def test_loss_head_edges():
    D = 64
    inv_b = 0.5
    one = np.float32(1.0)
    # smooth_l1 at |d| == 1 and one fp32 ulp either side (identity activation: y = z exactly, t = 0)
    d = torch.tensor([1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                      -1.0, -np.nextafter(one, np.float32(0)), -np.nextafter(one, np.float32(2))], dtype=torch.float32)
    z = torch.zeros(6, D)
    z[:, 5] = d
    t = torch.zeros(6, D)
    rl, dz, _ = _loss_head(z.to(DEV), t.to(DEV), "smooth_l1", "none", inv_b)
    rl_ref, g_ref, _ = _loss_ref(z, t, "smooth_l1", "none", inv_b)
    np.testing.assert_allclose(rl.cpu().numpy(), rl_ref.numpy(), rtol=1e-6)
    assert torch.equal(_d(dz), g_ref.to(torch.bfloat16).double()), "smooth_l1 gradient at |d| = 1 +- 1 ulp"
    assert torch.equal(dz[:, 5].float().cpu(), (inv_b * d.double().clamp(-1, 1)).bfloat16().float())
    # l2 with y == t: loss 0 and gradient 0 (torch's norm backward at 0)
    g = _gen(7)
    t = torch.randn(5, D, generator=g)
    z = t.clone()
    z[1] += 0.25
    rl, dz, _ = _loss_head(z.to(DEV), t.to(DEV), "l2", "none", inv_b)
    rl_ref, g_ref, _ = _loss_ref(z, t, "l2", "none", inv_b)
    assert rl[0].item() == 0.0 and rl[2].item() == 0.0 and torch.all(dz[[0, 2, 3, 4]].float() == 0)
    assert torch.all(g_ref[[0, 2, 3, 4]] == 0)
    np.testing.assert_allclose(rl.cpu().numpy(), rl_ref.numpy(), rtol=1e-5)
    # cos_dist on a zero row (identity and GELU, whose value at 0 is 0): loss 1, gradient -inv_b / (1e-8 |t|) t (* GELU'(0))
    for act, dact in (("none", 1.0), ("gelu", 0.5)):
        z = torch.randn(3, D, generator=g)
        z[1] = 0.0
        rl, dz, _ = _loss_head(z.to(DEV), t[:3].contiguous().to(DEV), "cos_dist", act, inv_b)
        rl_ref, g_ref, _ = _loss_ref(z, t[:3], "cos_dist", act, inv_b)
        assert rl[1].item() == 1.0 and rl_ref[1].item() == 1.0
        want = -inv_b / (1e-8 * torch.linalg.norm(t[1].double())) * t[1].double() * dact
        _assert_within(dz[1], want, _bf16_bound(want) + 1e-6 * want.abs().max(), f"cos_dist zero row ({act})")
        _assert_within(dz[1], g_ref[1], _bf16_bound(g_ref[1]) + 1e-6 * want.abs().max(), f"cos_dist zero row vs autograd ({act})")
        np.testing.assert_allclose(rl.cpu().numpy(), rl_ref.numpy(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------- GELU, whole range
def _gelu_inputs():
    grid = torch.arange(-8 * 4096, 8 * 4096, dtype=torch.float64) / 4096.0           # [-8, 8) at step 2^-12
    mags = torch.logspace(math.log10(1e-30), math.log10(3e38), 2000, dtype=torch.float64)
    x = torch.cat([grid, mags, -mags, torch.tensor([-1000.0, -1e5, -6.08, -6.0811529, -6.09, 6.09, 1000.0])]).float()
    n = (x.numel() + 255) // 256 * 256
    return torch.cat([x, torch.zeros(n - x.numel())])


def test_gelu_whole_range_scalar_and_vector_forms():
    x = _gelu_inputs()
    n = x.numel()
    ref = _gelu64(x.double())
    # scalar form: the loss head's y_out (GELU output activation); smooth_l1 against t = -3e38 makes dL/dy = inv_b = 1 for every
    # element, so dz3 = bf16(GELU'(x))
    z = x.reshape(-1, 256).to(DEV)
    t = torch.full_like(z, -3e38)
    _, dz, y = _loss_head(z, t, "smooth_l1", "gelu", 1.0)
    y = y.reshape(-1).cpu()
    # 4-wide form: the GEMM epilogue on a zero product, the values in the bias
    A = torch.zeros((1, 64), dtype=torch.bfloat16, device=DEV)
    W = torch.zeros((n, 64), dtype=torch.bfloat16, device=DEV)
    y4, _ = ops.gemm(A, W, bias=x.to(DEV), act=ops.ACT_GELU, want_f32=True, want_bf16=False)
    y4 = y4.reshape(-1).cpu()
    for form, v in (("gelu_erf (loss head y_out)", y), ("gelu_erf4 (GEMM epilogue)", y4)):
        err = (v.double() - ref).abs()
        i = int(err.argmax())
        assert err.max().item() <= GELU_ABS, f"{form}: |GELU - float64| = {err.max().item():.3g} at x = {x[i].item()!r} (got {v[i].item()!r})"
    assert torch.equal(y.view(torch.int32), y4.view(torch.int32)), \
        f"gelu_erf and gelu_erf4 differ at {int((y.view(torch.int32) != y4.view(torch.int32)).sum())} inputs"
    gref = _gelu_grad64(x.double())
    _assert_within(dz.reshape(-1), gref, _bf16_bound(gref, 2e-7), "GELU' (loss head dz3)")


# ---------------------------------------------------------------------------------------------------------------- Adam
_B1, _B2, _EPS = 0.9, 0.999, 1e-8
_B1F, _B2F = float(np.float32(_B1)), float(np.float32(_B2))


def _ulp(x):
    """one fp32 ulp at the top of x's binade: 2^-23 |x|"""
    return 2.0 ** -23 * x.abs()


def _spacing(x):
    return torch.from_numpy(np.spacing(np.abs(x.detach().cpu().numpy().astype(np.float32)))).double()


def _adam_call(p, g, m, v, n, lr, step, gscale=1.0, pb=None):
    ops._call("cmdiad_adam_step", _p(p), _p(g), _p(m), _p(v), n, float(lr), _B1, _B2, _EPS, int(step), float(gscale), _p(pb), _s())


def _check_adam_step(before, after, g, lr, step, gscale, n, what):
    p0, m0, v0 = (_d(a)[:n] for a in before)
    p1, m1, v1 = (_d(a)[:n] for a in after)
    gi = (g[:n] * gscale).cpu().double()         # the fp32 scaled gradient (exact when grad_scale = 1)
    m_ref = _B1F * m0 + (1.0 - _B1F) * gi
    v_ref = _B2F * v0 + (1.0 - _B2F) * gi * gi
    # 2 ulp of the terms' magnitude (m's two terms may cancel; v's are both >= 0)
    _assert_within(m1, m_ref, 2 * _ulp(_B1F * m0.abs() + (1.0 - _B1F) * gi.abs()), f"{what} m")
    _assert_within(v1, v_ref, 2 * _ulp(v_ref), f"{what} v")
    # the update from the kernel's own m, v: torch.optim.Adam in float64 (python betas: the fp32 powf bias corrections are
    # part of what the 2e-5 covers), plus half an ulp of the stored p
    u_ref = -lr / (1.0 - _B1 ** step) * m1 / (v1.sqrt() / math.sqrt(1.0 - _B2 ** step) + _EPS)
    _assert_within(p1 - p0, u_ref, 2e-5 * u_ref.abs() + 0.5 * _spacing(p1), f"{what} update")


@pytest.mark.parametrize("n", [1, 255, 257, 1_000_003])
def test_adam_step_against_float64(n):
    g = _gen(n)
    pad = 64
    p = torch.full((n + pad,), CANARY, device=DEV)
    p[:n] = (1e-3 * torch.randn(n, generator=g)).to(DEV)
    m = torch.full((n + pad,), CANARY, device=DEV); m[:n] = 0.0
    v = torch.full((n + pad,), CANARY, device=DEV); v[:n] = 0.0
    grads = [torch.randn(n, generator=g).float().to(DEV) * (1.0 + k) for k in range(10)]   # fixed synthetic sequence
    for step in range(1, 11):
        gscale = 1.0 if step % 2 else 0.37
        before = [a.clone() for a in (p, m, v)]
        _adam_call(p, grads[step - 1], m, v, n, 1e-3, step, gscale)
        torch.cuda.synchronize()
        if step in (1, 2, 10) or n < 1000:
            _check_adam_step(before, (p, m, v), grads[step - 1], 1e-3, step, gscale, n, f"n={n} step {step}")
    # step 10^4 from a synthetic state
    m[:n] = (0.1 * torch.randn(n, generator=g)).to(DEV)
    v[:n] = (torch.rand(n, generator=g) * 0.5 + 1e-4).to(DEV)
    before = [a.clone() for a in (p, m, v)]
    _adam_call(p, grads[0], m, v, n, 3e-4, 10_000, 0.37)
    torch.cuda.synchronize()
    _check_adam_step(before, (p, m, v), grads[0], 3e-4, 10_000, 0.37, n, f"n={n} step 1e4")
    # lr = 0 leaves p bit-identical; the bf16 copy is p's round-to-nearest-even cast
    p_keep = p.clone()
    pb = torch.full((n + pad,), 7.0, dtype=torch.bfloat16, device=DEV)
    _adam_call(p, grads[1], m, v, n, 0.0, 11, 1.0, pb)
    torch.cuda.synchronize()
    assert torch.equal(p, p_keep), "lr = 0 changed p"
    _adam_call(p, grads[2], m, v, n, 1e-3, 12, 1.0, pb)
    torch.cuda.synchronize()
    assert torch.equal(pb[:n], p[:n].bfloat16()), "p_bf16 is not the bf16 cast of p"
    for a in (p, m, v):
        assert torch.all(a[n:] == CANARY), "Adam wrote past n"
    assert torch.all(pb[n:] == 7.0), "p_bf16 written past n"


def test_fused_adam_matches_torch_adam_with_lr_schedule():
    g = _gen(5)
    shapes = [(257,), (33, 65), (4,)]
    p0 = [(0.01 * torch.randn(s, generator=g)).float() for s in shapes]
    sign = [torch.where(torch.rand(s, generator=g) < 0.5, -1.0, 1.0) for s in shapes]
    mine = [torch.nn.Parameter(a.clone().to(DEV)) for a in p0]
    ref = [torch.nn.Parameter(a.clone().double()) for a in p0]
    opt = train.FusedAdam(mine, lr=1e-3)
    opt_ref = torch.optim.Adam(ref, lr=1e-3, betas=(_B1, _B2), eps=_EPS, foreach=False)
    for k in range(20):
        lr = 1e-3 * 0.5 * (1.0 + math.cos(math.pi * k / 20))           # changed between steps, as lr_sched does
        for o in (opt, opt_ref):
            for pg in o.param_groups:
                pg["lr"] = lr
        for a, b, s in zip(mine, ref, sign):
            gr = (s * (0.5 + torch.rand(s.shape, generator=g))).float()    # one sign per element: updates do not cancel
            a.grad = gr.to(DEV)
            b.grad = gr.double()
        opt.step()
        opt_ref.step()
    for a, b, a0 in zip(mine, ref, p0):
        upd = b.detach() - a0.double()
        _assert_within(a.detach(), b.detach(), 1e-5 * upd.abs(), "FusedAdam vs torch.optim.Adam")


# ---------------------------------------------------------------------------------------------------------------- reductions
def _sum_bound(k, abs_sum):
    return k * U32 * abs_sum


def test_reduce_slabs():
    g = _gen(11)
    for n in (4, 252, 64 * 256 + 4):
        for S in (1, 3, 4, 5, 64, 65):
            stride = n + 8
            scale = 0.37
            slabs = torch.randn(S, stride, generator=g).float()
            slabs[:, n:] = float("nan")                        # the gap between slabs is never read
            sd = slabs.to(DEV)
            out = torch.full((n + 64,), CANARY, device=DEV)
            ops._call("cmdiad_reduce_slabs", _p(sd), S, n, stride, scale, _p(out), _s())
            out2 = torch.full((n + 64,), CANARY, device=DEV)
            ops._call("cmdiad_reduce_slabs", _p(sd), S, n, stride, scale, _p(out2), _s())
            torch.cuda.synchronize()
            assert torch.equal(out, out2), f"reduce_slabs S={S} n={n}: two calls differ"
            assert torch.all(out[n:] == CANARY), f"reduce_slabs S={S} n={n}: written past n"
            s64 = slabs[:, :n].double()
            ref = s64.sum(0) * scale
            _assert_within(out[:n], ref, _sum_bound(S + 3, s64.abs().sum(0) * scale), f"reduce_slabs S={S} n={n}")


def test_sum_vector():
    g = _gen(12)
    for n in (0, 1, 1023, 1024, 1025, 1_000_003):
        x = torch.randn(max(n, 1), generator=g).float()[:n].contiguous()
        xd = x.to(DEV) if n else torch.empty(4, device=DEV)
        out = torch.full((2,), CANARY, device=DEV)
        ops._call("cmdiad_sum_vector", _p(xd), n, 0.25, _p(out), _s())
        out2 = torch.full((2,), CANARY, device=DEV)
        ops._call("cmdiad_sum_vector", _p(xd), n, 0.25, _p(out2), _s())
        torch.cuda.synchronize()
        assert torch.equal(out, out2) and out[1].item() == CANARY, f"sum_vector n={n}"
        ref = x.double().sum() * 0.25
        bound = _sum_bound((n + 1023) // 1024 + 4 + 2 + 16 + 1, x.double().abs().sum().item() * 0.25)
        assert abs(out[0].item() - ref.item()) <= bound, f"sum_vector n={n}: {out[0].item()} vs {ref.item()}"


def test_colsum_bf16():
    g = _gen(13)
    for M, N in ((37, 100), (1000, 36), (5, 68)):
        x = torch.randn(M, N, generator=g).bfloat16()
        xd = x.to(DEV)
        for chunks in (1, 64, M + 3):
            part = torch.full((chunks, N), float("nan"), device=DEV)
            ops._call("cmdiad_colsum_bf16", _p(xd), M, N, chunks, _p(part), _s())
            part = part.cpu()
            rpc = (M + chunks - 1) // chunks
            x64 = x.double()
            for c in range(chunks):
                rows = x64[c * rpc: (c + 1) * rpc]
                ref = rows.sum(0) if rows.shape[0] else torch.zeros(N, dtype=torch.float64)
                _assert_within(part[c], ref, _sum_bound(rows.shape[0] // 4 + 3, rows.abs().sum(0)), f"colsum M={M} N={N} chunks={chunks} #{c}")
                if not rows.shape[0]:
                    assert torch.all(part[c] == 0), "an empty chunk's partial is not zero"


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("C", [64, 100, 768])
def test_ln_param_grad(C):
    g = _gen(200 + C)
    M = 203
    x = (torch.randn(M, C, generator=g) * 2.0 + torch.randn(M, 1, generator=g) * 3.0).float()
    dh = torch.randn(M, C, generator=g).float()
    x64 = x.double()
    mean64 = x64.mean(1)
    rstd64 = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + 1e-5)
    mean, rstd = mean64.float(), rstd64.float()            # the saved row statistics the kernel reads
    xd, dhd, md, rd = x.to(DEV), dh.to(DEV), mean.to(DEV), rstd.to(DEV)
    xhat = (x64 - mean.double()[:, None]) * rstd.double()[:, None]
    terms_g, terms_b = dh.double() * xhat, dh.double()
    # end result: fp64 autograd of F.layer_norm; the fp32 statistics differ from it by their own rounding
    w = torch.ones(C, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.layer_norm(x64, (C,), w, b, 1e-5).backward(dh.double())
    stat_err = (dh.double().abs() * ((mean.double() - mean64).abs()[:, None] * rstd64[:, None] +
                                     (x64 - mean64[:, None]).abs() * (rstd.double() - rstd64).abs()[:, None])).sum(0)
    for chunks in (64, M + 5):
        pg = torch.full((chunks, C), float("nan"), device=DEV)
        pb = torch.full((chunks, C), float("nan"), device=DEV)
        ops._call("cmdiad_ln_param_grad", _p(dhd), _p(xd), _p(md), _p(rd), M, C, chunks, _p(pg), _p(pb), _s())
        pg_h, pb_h = pg.cpu(), pb.cpu()
        rpc = (M + chunks - 1) // chunks
        for c in range(chunks):
            sl = slice(c * rpc, (c + 1) * rpc)
            k = max(0, min(M, (c + 1) * rpc) - c * rpc) // 4 + 3
            _assert_within(pg_h[c], terms_g[sl].sum(0), _sum_bound(k + 3, terms_g[sl].abs().sum(0)), f"ln partial_g C={C} chunks={chunks}")
            _assert_within(pb_h[c], terms_b[sl].sum(0), _sum_bound(k, terms_b[sl].abs().sum(0)), f"ln partial_b C={C} chunks={chunks}")
        dg = torch.empty(C, device=DEV)
        db = torch.empty(C, device=DEV)
        ops.reduce_slabs(pg, chunks, C, dg)
        ops.reduce_slabs(pb, chunks, C, db)
        torch.cuda.synchronize()
        kk = rpc // 4 + 3 + chunks // 4 + 3 + 3
        _assert_within(dg, w.grad, _sum_bound(kk, terms_g.abs().sum(0)) + stat_err, f"LayerNorm dgamma C={C} chunks={chunks}")
        _assert_within(db, b.grad, _sum_bound(kk, terms_b.abs().sum(0)), f"LayerNorm dbeta C={C} chunks={chunks}")


@pytest.mark.parametrize("C", [384, 768])
def test_layernorm_stats(C):
    g = _gen(300 + C)
    M = 37
    x = torch.randn(M, C, generator=g)
    x[::3] += 1e3                                           # rows with a large common offset
    x[1::5] -= 1e4
    x = x.float()
    gamma = torch.randn(C, generator=g).float().to(DEV)
    beta = torch.randn(C, generator=g).float().to(DEV)
    mean = torch.full((M + 4,), CANARY, device=DEV)
    rstd = torch.full((M + 4,), CANARY, device=DEV)
    ops.layernorm(x.to(DEV), gamma, beta, 1e-5, stats=(mean[:M], rstd[:M]))
    torch.cuda.synchronize()
    assert torch.all(mean[M:] == CANARY) and torch.all(rstd[M:] == CANARY)
    x64 = x.double()
    m64 = x64.mean(1)
    var64 = x64.var(1, unbiased=False)
    r64 = 1.0 / torch.sqrt(var64 + 1e-5)
    k = C // 64 + 12                                        # per-lane run + the 64-lane tree + the row total
    dm = _sum_bound(k, x64.abs().mean(1))
    _assert_within(mean[:M], m64, dm, f"LayerNorm mean C={C}")
    # two-pass variance about the fp32 mean: its error dm adds dm^2 / var; the squares' sum carries k roundings; rsqrt ~1 ulp
    rel = k * U32 + 0.5 * dm * dm / (var64 + 1e-5) + 2 * U32
    _assert_within(rstd[:M], r64, rel * r64, f"LayerNorm rstd C={C}")


# ---------------------------------------------------------------------------------------------------------------- BatchNorm
def test_bn_affine():
    g = _gen(400)
    rows, C = 4099, 40
    x = torch.randn(rows, C, generator=g)
    x[:, :8] = x[:, :8] * 0.1 + 1e3                         # mean 1e3, std 1e-1: one-pass variance cancels 1e8 : 1
    x[:, 8:16] = x[:, 8:16] * 30.0 - 5.0
    x = x.float()
    x64 = x.double()
    s, sq = x64.sum(0), (x64 * x64).sum(0)
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    beta = torch.randn(C, generator=g).float()
    eps = 1e-5
    outs64 = [torch.full((C + 1,), CANARY, dtype=torch.float64, device=DEV) for _ in range(2)]
    outs32 = [torch.full((C + 1,), CANARY, device=DEV) for _ in range(4)]
    ins = [a.to(DEV) for a in (s, sq, gamma, beta)]         # held until the kernel has run: no temporaries behind a raw pointer
    ops._call("cmdiad_bn_affine", *[_p(a) for a in ins], rows, eps, C, *[_p(o) for o in outs64], *[_p(o) for o in outs32], _s())
    torch.cuda.synchronize()
    for o in outs64 + outs32:
        assert o[C].item() == CANARY, "bn_affine wrote past C"
    mean64, var64 = (o[:C].cpu() for o in outs64)
    scale, shift, mean, rstd = (o[:C].cpu() for o in outs32)
    m_ref, v_ref = x64.mean(0), x64.var(0, unbiased=False)
    # the float64 sums the kernel reads carry ~rows u64 of E[x^2]; E[x^2] - mean^2 turns that into an absolute variance error
    u64 = 2.0 ** -53
    dv = 4 * rows * u64 * sq / rows
    _assert_within(mean64, m_ref, 4 * u64 * m_ref.abs() + rows * u64 * x64.abs().mean(0), "bn_affine mean64")
    _assert_within(var64, v_ref, dv, "bn_affine var64")
    r_ref = 1.0 / torch.sqrt(v_ref + eps)
    rel = 0.5 * dv / (v_ref + eps)
    _assert_within(rstd, r_ref, (U32 + rel) * r_ref, "bn_affine rstd")
    _assert_within(mean, m_ref, U32 * m_ref.abs() + 4 * u64 * m_ref.abs(), "bn_affine mean")
    sc_ref = gamma.double() * r_ref
    _assert_within(scale, sc_ref, (U32 + rel) * sc_ref.abs(), "bn_affine scale")
    sh_ref = beta.double() - m_ref * scale.double()          # y = z * scale + shift == (z - mean) * scale + beta
    _assert_within(shift, sh_ref, U32 * sh_ref.abs() + 8 * u64 * (m_ref * scale.double()).abs() + rows * u64 * x64.abs().mean(0) *
                   scale.double().abs(), "bn_affine shift")


def _bn_consts(z, gamma, beta, eps=1e-5):
    z64 = z.double()
    m, v = z64.mean(0), z64.var(0, unbiased=False)
    r = 1.0 / torch.sqrt(v + eps)
    scale = (gamma.double() * r).float()
    shift = (beta.double() - m * scale.double()).float()
    return scale, shift, m.float(), r.float()


@pytest.mark.parametrize("C", [8, 72])
def test_bn_relu_fwd(C):
    g = _gen(500 + C)
    M = 37
    z = (torch.randn(M, C, generator=g) * 2 + 0.5).float()
    res = torch.randn(M, C, generator=g).float()
    scale, shift, _, _ = _bn_consts(z, torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g))
    zd, sd, hd, rd = z.to(DEV), scale.to(DEV), shift.to(DEV), res.to(DEV)
    for residual in (None, rd):
        for relu in (False, True):
            y, y32 = ops.bn_relu_fwd(zd, sd, hd, residual=residual, relu=relu, want_f32=True)
            torch.cuda.synchronize()
            pre = z.double() * scale.double() + shift.double()
            ref = pre + (res.double() if residual is not None else 0.0)
            if relu:
                ref = ref.clamp(min=0.0)
            what = f"bn_relu_fwd C={C} residual={residual is not None} relu={relu}"
            _assert_within(y32, ref, U32 * (pre.abs() + ref.abs()), what)
            assert torch.equal(y, y32.bfloat16()), f"{what}: bf16 output is not the cast of the f32 one"


@pytest.mark.parametrize("M,C,chunks", [(37, 72, None), (10, 8, None), (37, 72, 64), (200, 8, 16)])
def test_bn_relu_bwd(M, C, chunks):
    g = _gen(600 + M + C)
    eps = 1e-5
    z = (torch.randn(M, C, generator=g) * 1.5 + 0.3).float()
    gamma = (torch.rand(C, generator=g) + 0.5).float()
    beta = (0.3 * torch.randn(C, generator=g)).float()
    res = torch.randn(M, C, generator=g).float()
    scale, shift, mean, rstd = _bn_consts(z, gamma, beta, eps)
    # no upstream gradient where the layer's own ReLU sits within rounding of its threshold (masked=True decides it in fp32)
    near = (z.double() * scale.double() + shift.double()).abs() < 1e-4
    G = torch.randn(M, C, generator=g).masked_fill(near, 0.0).float()
    dev = [a.to(DEV) for a in (scale, shift, mean, rstd)]
    for masked in (False, True):
        # masked=False: Bottleneck bn3, relu(bn(z) + r) -- dy arrives masked by the ReLU after the sum
        # masked=True:  relu(bn(z)) -- the kernel masks with the layer's own ReLU
        zz = z.double().requires_grad_(True)
        gg = gamma.double().requires_grad_(True)
        bb = beta.double().requires_grad_(True)
        bn = F.batch_norm(zz, None, None, gg, bb, training=True, eps=eps)
        out = torch.relu(bn + res.double()) if not masked else torch.relu(bn)
        out.backward(G.double())
        dy = (G.double() * (out > 0)).float() if not masked else G
        dz, dgamma, dbeta = ops.bn_relu_bwd(dy.to(DEV), z.to(DEV), *dev, chunks=chunks, masked=masked)
        torch.cuda.synchronize()
        what = f"bn_relu_bwd M={M} C={C} chunks={chunks} masked={masked}"
        open_ = (z.double() * scale.double() + shift.double() > 0) if masked else torch.ones_like(z, dtype=torch.bool)
        gm = dy.double() * open_
        xhat = (z.double() - mean.double()) * rstd.double()
        _assert_within(dbeta, bb.grad, _sum_bound(M // 4 + 12, gm.abs().sum(0)), f"{what} dbeta")
        _assert_within(dgamma, gg.grad, _sum_bound(M // 4 + 14, (gm * xhat).abs().sum(0)) + 1e-6 * (gm * xhat).abs().sum(0),
                       f"{what} dgamma")
        ref = zz.grad
        _assert_within(dz, ref, _bf16_bound(ref) + 1e-5 * ref.abs().max(), f"{what} dz")


# ---------------------------------------------------------------------------------------------------------------- layout kernels
def test_pad_nhwc_bit_exact():
    g = _gen(700)
    for B, H, W, C in ((3, 5, 7, 8), (1, 9, 3, 16)):
        x = torch.randn(B, H, W, C, generator=g).bfloat16()
        buf, guard, rows = ops.pad_nhwc(x.to(DEV))
        torch.cuda.synchronize()
        ref = F.pad(x, (0, 0, 1, 1, 1, 1)).reshape(-1, C)
        body = buf[guard: guard + ref.shape[0]].cpu()
        assert torch.equal(body.view(torch.int16), ref.view(torch.int16)), f"pad_nhwc {B}x{H}x{W}x{C}"
        rest = torch.cat([buf[:guard], buf[guard + ref.shape[0]:]]).cpu()
        assert rest.shape[0] == 2 * guard + rows - ref.shape[0] and torch.all(rest.view(torch.int16) == 0), "guards / padding rows"
        # the raw kernel writes the interior only: a pre-filled border stays as it was
        out = torch.full((B, H + 2, W + 2, C), 3.0, dtype=torch.bfloat16, device=DEV)
        xd = x.to(DEV)
        ops._call("cmdiad_pad_nhwc_bf16", _p(xd), B, H, W, C, _p(out), _s())
        torch.cuda.synchronize()
        want = torch.full((B, H + 2, W + 2, C), 3.0, dtype=torch.bfloat16)
        want[:, 1:H + 1, 1:W + 1] = x
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), "pad_nhwc touched the border"


def test_im2col3x3_bit_exact():
    g = _gen(701)
    for stride in (1, 2):
        for C in (1, 3, 7):
            B, H, W = 2, 9, 7
            img = torch.randn(B, C, H, W, generator=g).float()
            for ld in ((9 * C + 7) // 8 * 8, (9 * C + 7) // 8 * 8 + 16):
                cols = ops.im2col3x3(img.to(DEV), stride=stride, ld=ld).cpu()
                ref = F.unfold(img, 3, padding=1, stride=stride).permute(0, 2, 1).reshape(-1, 9 * C).bfloat16()
                what = f"im2col3x3 stride={stride} C={C} ld={ld}"
                assert cols.shape[0] == ref.shape[0], what
                assert torch.equal(cols[:, :9 * C].view(torch.int16), ref.view(torch.int16)), what
                assert torch.all(cols[:, 9 * C:].view(torch.int16) == 0), f"{what}: columns past 9 C"


def test_cast_bf16_bit_exact():
    g = _gen(702)
    bits = [0x3F808000, 0x3F818000, 0x3F80_8001, 0x3F80_7FFF, 0xBF80_8000, 0xBF81_8000,     # ties to even either way, near ties
            0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x80000001, 0x807FFFFF, 0x00400000,  # subnormals
            0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F7FFF, 0x7F800000, 0xFF800000,  # +-0, +-max, +-inf
            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF]                                      # NaNs
    special = torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32))
    rnd = torch.randint(-2 ** 31, 2 ** 31 - 1, (4096,), generator=g, dtype=torch.int64).to(torch.int32)
    xi = torch.cat([special, rnd])
    xi = torch.cat([xi, torch.zeros((-xi.numel()) % 4, dtype=torch.int32)])
    x = xi.view(torch.float32)
    out = ops.cast_bf16(x.to(DEV)).cpu()
    ref = x.bfloat16()
    nan = torch.isnan(x)
    assert torch.equal(torch.isnan(out), nan), "NaN in, NaN out (and nothing else)"
    assert torch.equal(out[~nan].view(torch.int16), ref[~nan].view(torch.int16)), \
        f"cast_bf16 differs at bits {[hex(int(b) & 0xFFFFFFFF) for b in xi[~nan][out[~nan].view(torch.int16) != ref[~nan].view(torch.int16)][:8]]}"


def test_linear3_each_activation():
    g = _gen(703)
    M, N = 37, 136
    x = (torch.randn(M, 3, generator=g) * 2).float()
    wb = torch.randn(N, 4, generator=g).float()
    lin = x.double() @ wb[:, :3].double().T + wb[:, 3].double()
    terms = x.double().abs() @ wb[:, :3].double().abs().T + wb[:, 3].double().abs()
    for act in (ops.ACT_NONE, ops.ACT_GELU, ops.ACT_RELU):
        out = ops.linear3(x.to(DEV), wb.to(DEV), act=act)
        torch.cuda.synchronize()
        ref = _gelu64(lin) if act == ops.ACT_GELU else lin.clamp(min=0) if act == ops.ACT_RELU else lin
        err = 4 * U32 * terms * (1.13 if act == ops.ACT_GELU else 1.0) + (GELU_ABS if act == ops.ACT_GELU else 0.0)
        _assert_within(out, ref, _bf16_bound(ref, err), f"linear3 act={act}")


# ---------------------------------------------------------------------------------------------------------------- GEMM epilogues
def _operands(M, N, K, seed):
    g = _gen(seed)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).bfloat16()
    prod = A.double() @ W.double().T
    bound = K * U32 * (A.double().abs() @ W.double().abs().T)
    return A, W, prod, bound


@pytest.mark.parametrize("M,N", [(77, 100), (200, 36)])
def test_gemm_dact_of(M, N):
    K = 128
    A, W, prod, bound = _operands(M, N, K, 800 + M)
    z = (2 * torch.randn(M, N, generator=_gen(801))).bfloat16()
    _, out = ops.gemm(A.to(DEV), W.to(DEV), dact_of=z.to(DEV))
    torch.cuda.synchronize()
    dg = _gelu_grad64(z.double())
    ref = prod * dg
    _assert_within(out, ref, _bf16_bound(ref, bound * dg.abs() + 2e-7 * prod.abs()), f"dact_of M={M} N={N}")


@pytest.mark.parametrize("M,N", [(77, 100), (200, 36)])
def test_gemm_out_pre_bf16(M, N):
    K = 192
    A, W, prod, bound = _operands(M, N, K, 810 + M)
    bias = torch.randn(N, generator=_gen(811)).float().to(DEV)
    Ad, Wd = A.to(DEV), W.to(DEV)
    pre = torch.empty((M, N), dtype=torch.bfloat16, device=DEV)
    _, act = ops.gemm(Ad, Wd, bias=bias, act=ops.ACT_GELU, out_pre_bf16=pre)
    f32, _ = ops.gemm(Ad, Wd, bias=bias, act=ops.ACT_NONE, want_f32=True, want_bf16=False)
    torch.cuda.synchronize()
    assert torch.equal(pre.view(torch.int16), f32.bfloat16().view(torch.int16)), "out_pre_bf16 is not the bf16 cast of the product"
    z = f32.cpu().double()
    _assert_within(f32, prod + bias.cpu().double(), bound + U32 * z.abs(), "f32 product + bias")
    ref = _gelu64(z)
    _assert_within(act, ref, _bf16_bound(ref, GELU_ABS), "GELU output next to out_pre_bf16")


@pytest.mark.parametrize("K,split", [(512, 3), (512, 8), (64 * 33, 8), (512, 5)])
def test_gemm_split_k_slabs(K, split):
    M, N = 77, 100
    A, W, prod, bound = _operands(M, N, K, 820 + split)
    Ad, Wd = A.to(DEV), W.to(DEV)
    slabs = torch.full((split, M, N), float("nan"), device=DEV)   # every slab must be written, even one without a K tile
    ops.gemm(Ad, Wd, out_f32=slabs, want_bf16=False, split_k=split)
    full, _ = ops.gemm(Ad, Wd, want_f32=True, want_bf16=False)
    torch.cuda.synchronize()
    assert not torch.isnan(slabs).any(), f"split_k={split} K={K}: slabs {sorted(set(torch.nonzero(torch.isnan(slabs))[:, 0].tolist()))} not written"
    _assert_within(full, prod, bound, "unsplit f32 product")
    _assert_within(slabs.double().sum(0), prod, bound + split * U32 * (A.double().abs() @ W.double().abs().T), f"split_k={split} slab sum")
    out = torch.empty((M * N,), device=DEV)
    ops.reduce_slabs(slabs, split, M * N, out)
    torch.cuda.synchronize()
    _assert_within(out.reshape(M, N), _d(full), 2 * bound + (split + 3) * U32 * (A.double().abs() @ W.double().abs().T),
                   f"split_k={split}: reduced slabs vs the unsplit product")
