"""CPU references for csrc/attention.hip, shared by the GPU tests and pinned by tests/test_attn_ref_cpu.py.  No GPU, no cmdiad_amd import.

attention_tile_model  float64 model of the kernel's tile loop: keys in tiles of 64, P = bf16(exp2(S - reference)), row sum of the
                      unrounded exp2, a reference that moves per wave of 32 queries only when a score exceeds it by more than 8.
emulate_fp32          the same loop in float32 arithmetic, as the kernel evaluates it.
routing_inputs        operands for which that arithmetic is exact in any order, so the expected output holds bit for bit.
spiked_operands       random operands with one dominant key per head in the last key tile.
qkv_exact_*           integer operands and the bit-exact float32 reference of cmdiad_gemm_qkv's head-split stores.
_ulp_check            the bf16 nearest / neighbour criterion of the stage-by-stage tests.
The grids (ROUTING_*, EDGE_*, QKV_GRID) live here so that the CPU test runs exactly the cases the device runs."""
import torch

HD = 64            # head dimension
KEYS = 64          # keys per tile
WAVE = 32          # queries that share one decision to move the reference
LAZY = 8.0         # log2 units a score may exceed the reference before it moves (kLazy)
CODE_BITS = 11     # key indices below 2 048


def r16(x):
    """round-to-nearest-even to bf16, back in the dtype it came in"""
    return x.float().to(torch.bfloat16).to(x.dtype)


def _ulp_check(got, ref64, what, max_ulps=1.0, frac_off=2e-3, abs_slack=None):
    """got: bf16 tensor from the GPU; ref64: float64 values BEFORE rounding.  Every element must be one of the (at most two)
    bf16 neighbours of the exact value -- |got - exact| <= max_ulps * ulp(exact) + abs_slack -- and all but a fraction `frac_off`
    must be the NEAREST one (round(exact) == got).  abs_slack (default 1e-5 of the mean magnitude) covers the fp32 evaluation of
    values that are small by CANCELLATION (a LayerNorm output or a dot product near zero carries the absolute error of its
    terms, ~1e-7 of THEIR size, which is many bf16 steps of a result of 1e-4)."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().cpu()
    if abs_slack is None:
        abs_slack = 1e-5 * float(ref64.abs().mean())
    nearest = ref64.float().to(torch.bfloat16).double()
    ulp = torch.exp2(torch.floor(torch.log2(nearest.abs().clamp_min(1e-37))) - 7.0)       # the bf16 step at the exact value
    err = (got - ref64).abs()
    assert bool((err <= max_ulps * ulp + abs_slack).all()), (what, float(((err - abs_slack) / ulp).max()))
    off = float((got != nearest).double().mean())
    assert off <= frac_off, (what, off)
    return off


def _wave_any(flag, T):
    """flag [B,H,T] bool -> the same shape: true for every query whose wave (32 consecutive queries) has one that is set.
    Queries past T are zero rows (scores 0, like their first tile's maximum): they never set it."""
    B, H, _ = flag.shape
    over = torch.nn.functional.pad(flag, (0, (-T) % WAVE)).reshape(B, H, -1, WAVE).any(-1)
    return over.repeat_interleave(WAVE, -1)[..., :T]


def attention_tile_model(q, k, v, T, stats=None):
    """q, k, v [B,H,>=T,64] holding the bf16 values the kernel reads (q pre-scaled: softmax is exp2 of the raw q.k) ->
    (out64 [B,H,T,64] float64 before the output's rounding, peak [B,H,T] the query's largest weight, l_run [B,H,T]).
    The reference is the first tile's maximum and moves up only when some query of the WAVE meets a score more than 8 (log2
    units) above its own; then every query of that wave moves to its running maximum (csrc/attention.hip).  stats (a dict)
    receives `moved`: in how many (head, later tile) pairs some reference moved."""
    qd, kd, vd = q[:, :, :T].cpu().double(), k[:, :, :T].cpu().double(), v[:, :, :T].cpu().double()
    B, H = qd.shape[:2]
    sc = qd @ kd.transpose(-2, -1)
    m_run = torch.full((B, H, T), -float("inf"), dtype=torch.float64)
    l_run = torch.zeros((B, H, T), dtype=torch.float64)
    o = torch.zeros((B, H, T, HD), dtype=torch.float64)
    moved = 0
    for t0 in range(0, T, KEYS):
        st = sc[..., t0:t0 + KEYS]
        grow = st.amax(-1) - m_run                                           # [B,H,T]; +inf in the first tile
        move = _wave_any(grow > LAZY, T) | (t0 == 0)                         # the wave-uniform decision, per query
        moved += int(move.any(-1).sum()) if t0 else 0
        m_new = torch.where(move, torch.maximum(m_run, st.amax(-1)), m_run)
        alpha = torch.exp2(m_run - m_new)
        p = torch.exp2(st - m_new[..., None])
        l_run = l_run * alpha + p.sum(-1)
        o = o * alpha[..., None] + r16(p) @ vd[:, :, t0:t0 + KEYS]
        m_run = m_new
    if stats is not None:
        stats["moved"] = moved
    peak = (torch.exp2(sc - m_run[..., None]) / l_run[..., None]).amax(-1)
    return o / l_run[..., None], peak, l_run


def emulate_fp32(q, k, v, T):
    """The kernel's tile loop in float32: scores with one rounding (the MFMA accumulator starts at minus the reference, so a
    later tile arrives as fp32(S - reference)), exp2, the row sum, P rounded to bf16, O += P V, the rescale by exp2(-growth)
    and the final O * (1 / l) each in float32; the per-wave lazy reference as in attention_tile_model.  q, k, v [B,H,>=T,64]
    -> (out [B,H,T,64] float32 holding bf16 values, l [B,H,T] float32).  The order of the additions inside a tile is torch's,
    not the MFMA's: results that depend on it are not pinned by this function, only those that are exact in any order."""
    qd, kd = q[:, :, :T].cpu().double(), k[:, :, :T].cpu().double()
    vf = v[:, :, :T].cpu().float()
    B, H = qd.shape[:2]
    sc = qd @ kd.transpose(-2, -1)                                           # exact products, float64 sum
    m = torch.zeros((B, H, T), dtype=torch.float32)
    l = torch.zeros((B, H, T), dtype=torch.float32)
    o = torch.zeros((B, H, T, HD), dtype=torch.float32)
    one = torch.ones((), dtype=torch.float32)
    for t0 in range(0, T, KEYS):
        s = (sc[..., t0:t0 + KEYS] - m.double()[..., None]).float()          # first tile: m = 0
        mloc = s.amax(-1)
        if t0 == 0:
            move, delta, alpha = torch.ones_like(mloc, dtype=torch.bool), mloc, torch.zeros_like(mloc)
            m = mloc
        else:
            move = _wave_any(mloc > LAZY, T)
            delta = torch.where(move, mloc.clamp_min(0.0), torch.zeros_like(mloc))
            alpha = torch.where(move, torch.exp2(-delta), one)
            m = torch.where(move, m + delta, m)
        s = torch.where(move[..., None], s - delta[..., None], s)
        p = torch.exp2(s)
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + r16(p) @ vf[:, :, t0:t0 + KEYS]
    return r16(o * (1.0 / l)[..., None]), l


EDGE_T = (1, 33, 63, 64, 65, 127, 129, 197, 257)          # the random-operand grid of tests/test_gpu_attention_edges.py
EDGE_BH = ((3, 2), (1, 6))


def spiked_operands(B, H, T, seed):
    """q = 0.3 randn, k, v = randn, rounded to bf16, with one planted spike per head in the last key tile: k[j*] = 4 q[t*] (the
    score of that pair is ~20 log2 units above the rest, so the reference of t*'s wave moves in the last tile when T > 64).
    -> q, k, v [B,H,T,64] float32 holding bf16 values."""
    g = torch.Generator().manual_seed(seed)
    q = r16(0.3 * torch.randn((B, H, T, HD), generator=g))
    k = r16(torch.randn((B, H, T, HD), generator=g))
    v = r16(torch.randn((B, H, T, HD), generator=g))
    last = (T - 1) // KEYS * KEYS
    for b in range(B):
        for h in range(H):
            t = int(torch.randint(0, T, (1,), generator=g))
            j = last + int(torch.randint(0, T - last, (1,), generator=g))
            k[b, h, j] = r16(4.0 * q[b, h, t])
    return q, k, v


def attention_slack(peak, v, a_ref):
    """The slack of the stage-by-stage test per (query, column): 2^-7 x the query's largest weight x the column's largest |v|
    (two P elements whose rounding falls the other way), plus 1e-5 of the output scale.  peak [B,H,T], v [B,H,T,64] float64,
    a_ref [B,H,T,64] -> [B,H,T,64]."""
    return 2.0 ** -7 * peak[..., None] * v.abs().amax(2)[:, :, None, :] + 1e-5 * float(a_ref.abs().mean())


def code(idx):
    """idx int64 [...] -> [..., 11] float32 of +-1: bit i of the index as a sign"""
    return ((idx[..., None] >> torch.arange(CODE_BITS)) & 1).float() * 2.0 - 1.0


ROUTING_KINDS = ("one_hot", "two_hot2", "two_hot5", "two_hot6", "two_hot7")


def routing_bit(kind):
    """the tied bit of a two-hot kind; None for one_hot"""
    return None if kind == "one_hot" else int(kind[len("two_hot"):])


ROUTING_T = (1, 2, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 197, 257, 1025)
ROUTING_BH = ((1, 1), (3, 2), (9, 2), (1, 12))      # (9, 2): B H = 18, over 8 and no multiple of 8, with two query tiles from T = 129


def routing_cases():
    """(B, H, T, kind) of the routing grid: every (B, H) at every T, (1, 2) only at T = 1025; a tied bit only where the pair
    can exist ((1 << bit) < T)."""
    out = []
    for T in ROUTING_T:
        for B, H in (((1, 2),) if T == 1025 else ROUTING_BH):
            for kind in ROUTING_KINDS:
                bit = routing_bit(kind)
                if bit is None or (1 << bit) < T:
                    out.append((B, H, T, kind))
    return out


def routing_seed(B, H, T):
    return 1000 * T + 10 * B + H


def edge_seed(B, H, T):
    return 7000 + 100 * T + 10 * B + H


def routing_inputs(B, H, T, kind, seed):
    """-> (q, k, v, want), each [B,H,T,64] float32 with values bf16 holds exactly.  Keys carry 20 x the +-1 code of their index in
    the first 11 dimensions; v[j, d] = sign[d] * mag[j, d] with mag from {0.5, 1, 1.5, 2} and one sign per (b, h, column), so the
    sum of two rows never cancels.
      one_hot    q[t] = code(perm(t)), a permutation per (b, h) with perm(0) = T-1 and perm(T-1) = 0: score 220 at the hot key,
                 <= 180 elsewhere; want = v[perm(t)].
      two_hot<b> q[t] = code(j_t) with dimension b zeroed: keys j_t and j_t ^ (1 << b) tie at 200, the rest <= 160; want =
                 (v[j] + v[j']) / 2.  Where j' >= T the query stays one-hot.  j_0 = T-1 and j_{T-1} = 0.
    All scores are integers, so S - reference is exact in fp32 in any order; P is 1 at the hot keys and <= 2^-40 elsewhere, so l
    is 1 or 2 exactly and the other terms vanish when added to a value >= 0.5: want holds bit for bit."""
    if T > 1 << CODE_BITS:
        raise ValueError(f"routing_inputs: T = {T} needs more than {CODE_BITS} code bits")
    g = torch.Generator().manual_seed(seed)
    bit = routing_bit(kind)
    k = torch.zeros((B, H, T, HD))
    k[..., :CODE_BITS] = 20.0 * code(torch.arange(T))
    mag = torch.tensor([0.5, 1.0, 1.5, 2.0])[torch.randint(0, 4, (B, H, T, HD), generator=g)]
    sign = (torch.randint(0, 2, (B, H, 1, HD), generator=g) * 2 - 1).float()
    v = sign * mag
    if bit is None:
        j = torch.stack([torch.randperm(T, generator=g) for _ in range(B * H)]).reshape(B, H, T)
        if T > 1:      # swap the forced ends in, keeping a permutation
            for row in j.view(-1, T):
                for pos, val in ((0, T - 1), (T - 1, 0)):
                    at = int((row == val).nonzero())
                    row[at], row[pos] = row[pos].clone(), val
    else:
        j = torch.randint(0, T, (B, H, T), generator=g)
        j[..., 0], j[..., T - 1] = T - 1, 0
    cq = code(j)
    idx = j[..., None].expand(B, H, T, HD)
    want = torch.gather(v, 2, idx)
    if bit is not None:
        j2 = j ^ (1 << bit)
        tied = j2 < T
        cq[..., bit] = torch.where(tied, torch.zeros(()), cq[..., bit])
        pair = torch.gather(v, 2, j2.clamp_max(T - 1)[..., None].expand(B, H, T, HD))
        want = torch.where(tied[..., None], (want + pair) * 0.5, want)
    q = torch.zeros((B, H, T, HD))
    q[..., :CODE_BITS] = cq
    return q, k, v, want


# ------------------------------------------------------------------------------------------------ QKV head-split, exact
QKV_GRID = ((1, 1, 128), (3, 1, 128), (300, 1, 128),      # single-token images
            (40, 5, 128),                                 # 25 images per 128-row tile
            (7, 3, 128),                                  # T < 4: every V^T group of four tokens crosses an image
            (2, 63, 128), (2, 64, 128), (2, 65, 128),     # the row-store guard on both sides
            (3, 43, 128),                                 # M = 129
            (1, 127, 128), (1, 129, 128),                 # around one 128-row tile
            (2, 197, 128), (1, 257, 128),                 # ViT-S/16-like, DINOv2 at 224
            (1, 1025, 128),                               # Point-BERT with its class row
            (2, 65, 384), (1, 197, 768))                  # the wider geometries
Q_SCALE = float(torch.tensor(0.125 * 1.4426950408889634, dtype=torch.float32))   # head_dim^-0.5 * log2 e as the fp32 constant
PAD_FILL = 7.0                                            # what the padding of q, k, v^T holds before the launch


def qkv_exact_operands(B, T, C):
    """-> (A [B*T, C] bf16 of integers in [-4, 4], W [3C, C] bf16 of integers in [-2, 2], bias [3C] f32 of multiples of 0.25 in
    [-8, 8], row_scale [B*T rounded up to 256] f32 of powers of two in {0.25, 0.5, 1, 2}).  acc = A . W^T is an integer below
    2^13; acc + bias and fma(acc, row_scale, bias) are multiples of 1/4 below 2^14: exact in fp32 in any order."""
    g = torch.Generator().manual_seed(B * 100003 + T * 101 + C)
    M = B * T
    A = torch.randint(-4, 5, (M, C), generator=g).to(torch.bfloat16)
    W = torch.randint(-2, 3, (3 * C, C), generator=g).to(torch.bfloat16)
    bias = torch.randint(-32, 33, (3 * C,), generator=g).float() * 0.25
    rs = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, ((M + 255) // 256 * 256,), generator=g)]
    return A, W, bias, rs


def qkv_exact_reference(A, W, bias, row_scale, B, T):
    """float32 on the CPU, every step exact but the q scale's one fp32 rounding and the bf16 rounding behind it ->
    (q, k [B,H,T,64], vt [B,H,64,T]) bf16."""
    M, C = A.shape
    H = C // HD
    acc = A.float() @ W.float().T
    assert float(acc.abs().max()) < 2.0 ** 13
    if row_scale is not None:
        acc = acc * row_scale[:M, None]
    if bias is not None:
        acc = acc + bias
    qkv = acc.reshape(B, T, 3, H, HD).permute(2, 0, 3, 1, 4)               # [3,B,H,T,64]
    q = (qkv[0] * Q_SCALE).to(torch.bfloat16)
    return q.contiguous(), qkv[1].to(torch.bfloat16).contiguous(), qkv[2].to(torch.bfloat16).transpose(-1, -2).contiguous()


def qkv_filled_buffers(B, H, T, device):
    """q, k [B,H,Tp,64] and v^T [B,H,64,Tp] bf16 holding PAD_FILL everywhere (cmdiad_gemm_qkv never writes the padding)"""
    Tp = (T + KEYS - 1) // KEYS * KEYS
    q = torch.full((B, H, Tp, HD), PAD_FILL, dtype=torch.bfloat16, device=device)
    return q, q.clone(), torch.full((B, H, HD, Tp), PAD_FILL, dtype=torch.bfloat16, device=device)
