"""Lattice operands and the CPU reference of the point-group encoder (csrc/gemm.hip cmdiad_encoder_stage1, the group-bias
cmdiad_gemm_bf16, cmdiad_gemm_groupmax; csrc/encoder_tail.hip), shared by tests/test_gpu_encoder_exact.py and pinned by
tests/test_encoder_ref_cpu.py.  No GPU, no cmdiad_amd import.

Every operand sits on a lattice on which each product, each partial sum in any order, each `+ bias` and each `+ group bias` of
the chain is a multiple of 1/8 below 2^24 / 8 in magnitude, hence exact in fp32: whatever order a kernel adds in, its result is
determined bit for bit, and float32 on the CPU equals float64 (and int64 arithmetic on the values times 8).

  coordinates   multiples of 1/8 in [-2, 2]
  w1, b1        integers in [-2, 2] / [-3, 3]: conv1's ReLU output is <= 15 on the 1/8 grid, exact in bf16
  W2, b2        integers in [-2, 2], quarters
  W3a, W3b, W4  {-1, 0, 1}, about 3/4 zeros; b3, b4 quarters; W4's first eight rows non-positive with a negative bias

The arithmetic restated (csrc/gemm_core.h conv1_act, csrc/gemm.hip groupmax_epilogue, csrc/encoder_tail.hip):
  a1  = bf16(ReLU(fma(wz, z, fma(wy, y, fma(wx, x, b)))))     (exact here, so the FMA chain is a plain sum)
  h2' = W2 . a1 + b2          g32 = max over the group's rows of h2'  (BEFORE the rounding)      h2 = bf16(h2'), g16 = bf16(g32)
  gb  = W3a . g16 + b3  (fp32)                                  h3 = bf16(ReLU(W3b . h2 + gb[group]))
  tok = max over the group's rows of (W4 . h3) + b4

A random draw lets a row position win a column's maximum only by luck (110 of 128 positions over 256 columns), and a kernel that
drops one row of a group then passes.  So 128 of conv2's 256 columns, 128 of conv3's 512 and 128 of conv4's first 256 are
DETECTORS: column c_i of h2' is  beta_i - 2 |x - P_i|_1  (six conv1 channels ReLU(+-(2 x - 2 P_i)) per axis, P_i one of 128
points with half-integer coordinates in [-1.5, 1.5]), b3 lifts it so that it is positive (1/2 .. 3/4) only within 1/8 of P_i,
and one weight of W4 hands it to a token.  The rows of a CHECKED group (first, last, every group of the last 128-row tile) sit
on distinct P_i plus an offset of at most 1/8 on one axis (its own detector reads >= beta - 1/4, every other row's <= beta - 3/4):
row r is then the only maximiser of its detector column in h2' and in the tokens, wherever in the group it stands.  The other
half of every width, and every other group's coordinates, are drawn freely.  coverage() checks the property on the reference's
numbers alone, whatever produced them."""
import functools

import torch

C1, C2, C3 = 128, 256, 512           # conv1, conv2, conv3 widths (fixed in the kernels)
N_OUT = (384, 256)                   # conv4: Point-MAE, Point-BERT
GRANULE = 0.125
NDET = 128                           # detector columns = the largest group

# (groups, Mg): what the row count exercises is listed in tests/test_gpu_encoder_exact.py
GRID = [(1, 32), (1, 64), (1, 128), (4, 32), (2, 64), (3, 32), (5, 32), (3, 64), (7, 32), (9, 64), (257, 128), (1030, 32), (2052, 32)]
CHAIN = [(1, 32), (2, 64), (3, 32), (5, 32), (9, 64)]
GROUPMAX_GRID = [(N, K, g, Mg) for N in (4, 132, 384) for K in (64, 192, 512) for (g, Mg) in ((1, 32), (5, 32), (3, 64), (3, 128))]


# ------------------------------------------------------------------------------------------------ bf16 roundings
def bf16_rne(x):
    """nearest-even, through torch"""
    return x.to(torch.bfloat16)


def _bits(x):
    return x.float().contiguous().view(torch.int32)


def bf16_trunc(x):
    """mutant: the low 16 bits dropped"""
    return (_bits(x) & -65536).view(torch.float32).to(torch.bfloat16)


def bf16_half_up(x):
    """mutant: + 0x8000 and truncate (ties away from zero instead of to even)"""
    return ((_bits(x) + 0x8000) & -65536).view(torch.float32).to(torch.bfloat16)


def is_tie(x):
    """fp32 values exactly half way between two bf16 values"""
    return (_bits(x) & 0xFFFF) == 0x8000


# ------------------------------------------------------------------------------------------------ group maxima
def group_max(v, groups, Mg, mode=None):
    """v [groups * Mg, N] -> [groups, N].  mode: None, or one of the mutants of tests/test_encoder_ref_cpu.py."""
    x = v.reshape(groups, Mg, -1)
    if mode is None:
        return x.amax(1)
    if mode == "skip_row0":
        return x[:, 1:].amax(1)
    if mode == "skip_last":
        return x[:, :-1].amax(1)
    if mode == "skip_16_31":
        return torch.cat([x[:, :16], x[:, 32:]], 1).amax(1) if Mg > 32 else x[:, :16].amax(1)
    if mode == "seed0":
        return x.amax(1).clamp_min(0)
    if mode == "shift32":   # group g = rows [g Mg - 32, (g + 1) Mg - 32) of the matrix; nothing there: the identity of max
        pad = torch.full((32, v.shape[1]), float("-inf"), dtype=v.dtype)
        return torch.cat([pad, v[:-32]], 0).reshape(groups, Mg, -1).amax(1)
    raise ValueError(mode)


MAX_MUTANTS = ("skip_row0", "skip_last", "skip_16_31", "seed0", "shift32")


# ------------------------------------------------------------------------------------------------ operands
def _quarters(g, n, lo, hi):
    return torch.randint(int(lo * 4), int(hi * 4) + 1, (n,), generator=g).float() / 4


def _ternary(g, rows, cols):
    return (torch.randint(0, 8, (rows, cols), generator=g) == 0).float() - (torch.randint(0, 8, (rows, cols), generator=g) == 0).float()


@functools.lru_cache(maxsize=None)
def weights(seed=7):
    """The encoder's weights on the lattice (float32 on the CPU; W2, W3a, W3b, W4 are exact in bf16), W4 / b4 at 384 rows: the
    256-wide form uses the first 256.  Also P [128, 3], the detectors' points."""
    g = torch.Generator().manual_seed(seed)
    w1 = torch.randint(-2, 3, (C1, 3), generator=g).float()
    b1 = torch.randint(-3, 4, (C1,), generator=g).float()
    W2 = torch.randint(-2, 3, (C2, C1), generator=g).float()
    b2 = _quarters(g, C2, -4, 4)
    W3a, W3b, W4 = _ternary(g, C3, C2), _ternary(g, C3, C2), _ternary(g, 384, C3)
    b3, b4 = _quarters(g, C3, -4, 4), _quarters(g, 384, -4, 4)
    W4[:8] = -W4[:8].abs()
    W4[:8, :8] = -1.0
    b4[:8] = -b4[:8].abs() - 0.25
    # ---- detectors.  conv1 channels k1[axis, level, sign] = ReLU(sign (2 x_axis - level)), level = 2 P in -3 .. 3
    k1 = torch.randperm(C1, generator=g)[:42].reshape(3, 7, 2)
    for ax in range(3):
        for lv in range(7):
            for sg in range(2):
                k = k1[ax, lv, sg]
                w1[k] = 0.0
                w1[k, ax] = 2.0 if sg == 0 else -2.0
                b1[k] = float(-(lv - 3)) if sg == 0 else float(lv - 3)
    code = torch.randperm(343, generator=g)[:NDET]                       # 128 distinct points of the 7 x 7 x 7 half-integer cube
    lv = torch.stack([code // 49, code // 7 % 7, code % 7], 1)           # levels 0 .. 6
    P = (lv.float() - 3.0) / 2
    c2 = torch.randperm(C2, generator=g)[:NDET]
    c3 = torch.randperm(C3, generator=g)[:NDET]
    c4 = torch.randperm(248, generator=g)[:NDET] + 8                     # inside both output widths, past the eight negative rows
    beta = _quarters(g, NDET, -6, 6)
    for i in range(NDET):
        W2[c2[i]] = 0.0
        for ax in range(3):
            W2[c2[i], k1[ax, lv[i, ax]]] = -1.0                          # - ReLU(2 x - 2 P) - ReLU(2 P - 2 x) = - 2 |x - P|
        b2[c2[i]] = beta[i]
        W3a[c3[i]] = 0.0
        W3b[c3[i]] = 0.0
        W3b[c3[i], c2[i]] = 1.0
        b3[c3[i]] = 0.75 - beta[i]                                       # within 1/8 of P_i: 1/2 .. 3/4; within 1/8 of any other P_j: <= 0
        W4[c4[i]] = 0.0
        W4[c4[i], c3[i]] = 1.0
    b4[c4] = _quarters(g, NDET, -3, 0.5)
    return dict(w1b1=torch.cat([w1, b1[:, None]], 1).contiguous(), W2=W2, b2=b2, W3a=W3a, W3b=W3b, b3=b3, W4=W4, b4=b4, P=P)


def checked_groups(groups, Mg):
    """first, last, and every group of the last 128-row tile"""
    first_of_last_tile = ((groups * Mg - 1) // 128 * 128) // Mg
    return sorted({0, groups - 1, *range(first_of_last_tile, groups)})


def coordinates(groups, Mg, seed=None):
    """[groups * Mg, 3] on the 1/8 grid in [-2, 2]; the checked groups on distinct detector points (see the module docstring)"""
    g = torch.Generator().manual_seed(groups * 1000 + Mg if seed is None else seed)
    xyz = torch.randint(-16, 17, (groups, Mg, 3), generator=g).float() / 8
    P = weights()["P"]
    for gi in checked_groups(groups, Mg):
        pts = P[torch.randperm(NDET, generator=g)[:Mg]]
        off = torch.zeros(Mg, 3)
        axis = torch.randint(0, 3, (Mg,), generator=g)                   # one step of +-1/8 (or none) on one axis
        off[torch.arange(Mg), axis] = torch.randint(-1, 2, (Mg,), generator=g).float() / 8
        xyz[gi] = pts + off
    return xyz.reshape(-1, 3).contiguous()


# ------------------------------------------------------------------------------------------------ the reference
def stage1(w, xyz, groups, Mg, dtype=torch.float32, rnd=bf16_rne):
    """-> dict(a1, h2p [M,256] before the rounding, h2 bf16, g32, g16 bf16)"""
    w1b1 = w["w1b1"].to(dtype)
    x = xyz.to(dtype)
    a = w1b1[:, 3] + x[:, 0:1] * w1b1[:, 0]          # conv1_act's chain: fma(wz, z, fma(wy, y, fma(wx, x, b))); exact here
    a = a + x[:, 1:2] * w1b1[:, 1]
    a = (a + x[:, 2:3] * w1b1[:, 2]).clamp_min(0)
    a1 = rnd(a.float())
    h2p = a1.to(dtype) @ w["W2"].to(dtype).T + w["b2"].to(dtype)
    h2 = rnd(h2p.float())
    g32 = group_max(h2p, groups, Mg)
    return dict(a1=a1, h2p=h2p, h2=h2, g32=g32, g16=rnd(g32.float()))


def group_bias(w, g16, dtype=torch.float32):
    return g16.to(dtype) @ w["W3a"].to(dtype).T + w["b3"].to(dtype)


def conv3(w, h2, gb, Mg, dtype=torch.float32, rnd=bf16_rne):
    """-> (h3p before the rounding (after the ReLU), h3 bf16)"""
    h3p = (h2.to(dtype) @ w["W3b"].to(dtype).T + gb.to(dtype).repeat_interleave(Mg, 0)).clamp_min(0)
    return h3p, rnd(h3p.float())


def conv4(w, h3, n_out=384, dtype=torch.float32):
    """W4 . h3 before the maximum and the bias"""
    return h3.to(dtype) @ w["W4"][:n_out].to(dtype).T


def tokens(w, acc4, groups, Mg, max_mode=None, use_b4=True):
    t = group_max(acc4, groups, Mg, max_mode)
    return t + w["b4"][:t.shape[1]].to(t.dtype) if use_b4 else t


def padded_tail_tokens(w, h2, gb, groups, Mg, n_out=384):
    """mutant: the ragged last tile is filled up to 128 rows with copies of the last row, and those rows take part in the maximum of
    the last stored group.  A copy that also carries the last group's bias changes nothing (max is idempotent; asserted in the CPU
    test), so the copies here go through conv3 with NO group bias, as rows past the last group have none."""
    pad = (-groups * Mg) % 128
    assert pad
    _, h3 = conv3(w, h2, gb, Mg)
    acc = conv4(w, h3, n_out)
    _, h3x = conv3(w, h2[-1:], torch.zeros(1, C3), 1)
    tok = tokens(w, acc, groups, Mg)
    tok[-1] = torch.maximum(tok[-1], conv4(w, h3x, n_out)[0] + w["b4"][:n_out])
    return tok


def reference(groups, Mg, dtype=torch.float32, rnd=bf16_rne, keep=False):
    """The whole chain on the lattice case (groups, Mg) -> dict(xyz, h2, g32, g16, gb, h3, tok (384 wide; the 256-wide tokens
    are its first 256 columns), stats).  keep: also h2p, h3p, acc4 (the values before rounding / before the maximum)."""
    w = weights()
    xyz = coordinates(groups, Mg)
    s1 = stage1(w, xyz, groups, Mg, dtype, rnd)
    gb = group_bias(w, s1["g16"], dtype)
    h3p, h3 = conv3(w, s1["h2"], gb, Mg, dtype, rnd)
    acc4 = conv4(w, h3, 384, dtype)
    out = dict(xyz=xyz, h2=s1["h2"], g32=s1["g32"], g16=s1["g16"], gb=gb, h3=h3, tok=tokens(w, acc4, groups, Mg))
    if dtype == torch.float32 and rnd is bf16_rne:
        out["stats"] = preconditions(w, s1, gb, h3p, h3, acc4, out["tok"], groups, Mg)
    if keep:
        out.update(a1=s1["a1"], h2p=s1["h2p"], h3p=h3p, acc4=acc4)
    return out


@functools.lru_cache(maxsize=None)
def case(groups, Mg):
    """reference(groups, Mg) in float32, computed once per process and left unchanged"""
    return reference(groups, Mg)


# ------------------------------------------------------------------------------------------------ the same chain in integers
def bf16_rne_int(v, frac_bits=3):
    """bf16 nearest-even of the values v / 2^frac_bits, v int64, without a float in sight: keep the top 8 significant bits"""
    a = v.abs()
    shift = torch.zeros_like(a)
    for s in range(1, 40):
        shift = torch.where(a >= (1 << (7 + s)), torch.full_like(a, s), shift)
    q, rem, half = a >> shift, a & ((1 << shift) - 1), (1 << shift) >> 1
    up = (shift > 0) & ((rem > half) | ((rem == half) & (q & 1 == 1)))
    return torch.sign(v) * ((q + up.long()) << shift)


def reference_int(groups, Mg):
    """reference() in int64 on the values times 8 -> dict(h2, g32, g16, gb, h3, tok), each int64 = 8 x the value"""
    w = weights()
    i8 = lambda t: (t.double() * 8).round().long()      # noqa: E731 -- biases and coordinates: on the 1/8 grid
    wi = lambda t: t.long()                             # noqa: E731 -- weights: integers
    x = i8(coordinates(groups, Mg))
    a1 = bf16_rne_int((x @ wi(w["w1b1"][:, :3]).T + i8(w["w1b1"][:, 3])).clamp_min(0))
    h2p = a1 @ wi(w["W2"]).T + i8(w["b2"])
    h2, g32 = bf16_rne_int(h2p), h2p.reshape(groups, Mg, -1).amax(1)
    g16 = bf16_rne_int(g32)
    gb = g16 @ wi(w["W3a"]).T + i8(w["b3"])
    h3 = bf16_rne_int((h2 @ wi(w["W3b"]).T + gb.repeat_interleave(Mg, 0)).clamp_min(0))
    tok = (h3 @ wi(w["W4"]).T).reshape(groups, Mg, -1).amax(1) + i8(w["b4"])
    return dict(h2=h2, g32=g32, g16=g16, gb=gb, h3=h3, tok=tok)


# ------------------------------------------------------------------------------------------------ preconditions
def exactness(a, W, bias, gbias=None, Mg=1):
    """max over the outputs of (sum |a| |w| + |bias| + |group bias|) / granule, as a fraction of 2^24: below 1, every partial
    sum of the product in any order is an integer number of granules that fp32 holds exactly."""
    s = a.float().abs() @ W.float().abs().T
    if bias is not None:
        s = s + bias.abs()
    if gbias is not None:
        s = s + gbias.abs().repeat_interleave(Mg, 0)
    return float(s.max()) / GRANULE / 2 ** 24


def on_lattice(*ts):
    return all(bool((t.double() / GRANULE == (t.double() / GRANULE).round()).all()) for t in ts)


def coverage(v, groups, Mg, which=None):
    """v [groups * Mg, N] before the maximum -> over the checked groups, the smallest number of row positions that are the ONLY
    maximiser of at least one column."""
    x = v.reshape(groups, Mg, -1)
    worst = Mg
    for gi in (checked_groups(groups, Mg) if which is None else which):
        top = x[gi].amax(0)
        hit = x[gi] == top
        sole = hit.sum(0) == 1
        worst = min(worst, int(hit[:, sole].any(1).sum()))
    return worst


def preconditions(w, s1, gb, h3p, h3, acc4, tok, groups, Mg):
    """The figures the test files assert (check_preconditions): exactness margin per product, row coverage of both maxima (384
    and 256 wide), negative maxima, rounded elements and exact ties of h2 and h3."""
    h2p = s1["h2p"]
    return dict(
        margin=dict(conv2=exactness(s1["a1"], w["W2"], w["b2"]), gbias=exactness(s1["g16"], w["W3a"], w["b3"]),
                    conv3=exactness(s1["h2"], w["W3b"], None, gb, Mg), conv4=exactness(h3, w["W4"], w["b4"])),
        lattice=on_lattice(s1["a1"], h2p, gb, h3p, acc4, tok),
        cover1=coverage(h2p, groups, Mg), cover384=coverage(acc4, groups, Mg), cover256=coverage(acc4[:, :256], groups, Mg),
        neg_tok384=float((tok < 0).float().mean()), neg_tok256=float((tok[:, :256] < 0).float().mean()), neg_g32=int((s1["g32"] < 0).sum()),
        rounded_h2=float((s1["h2"].float() != h2p).float().mean()), rounded_h3=float((h3.float() != h3p).float().mean()),
        ties_h2=int(is_tie(h2p).sum()), ties_h3=int(is_tie(h3p).sum()))


def check_preconditions(st, Mg):
    """Conditions on the inputs, not tolerances: without them an exact comparison proves less than it seems to."""
    assert st["lattice"], st
    assert max(st["margin"].values()) < 1.0, st["margin"]
    assert st["cover1"] == Mg and st["cover384"] == Mg and st["cover256"] == Mg, st
    assert st["neg_tok384"] >= 0.05 and st["neg_tok256"] >= 0.05 and st["neg_g32"] >= 1, st
    assert st["rounded_h2"] >= 0.05 and st["rounded_h3"] >= 0.05, st
    assert st["ties_h2"] >= 100 and st["ties_h3"] >= 100, st


# ------------------------------------------------------------------------------------------------ gemm_groupmax off the encoder's shape
def _groupmax_draw(N, K, groups, Mg, attempt):
    """Lattice operands of cmdiad_gemm_groupmax at any (N, K): A [groups * Mg, K] in k / 8, k = 1 .. 64 (positive, like h3), W
    [N, K] in {-1, 0, 1}, bias quarters; the first ceil(N / 8) rows of W non-positive with a -1, so that their maxima are negative
    with and without the bias.  Row r of a group is given a column of its own where it can -- min(Mg, N) of them: a column has one
    maximiser, so N columns cannot single out more than N rows -- by a spike: 6 .. 8 where that column's weight is +1, at most 1/2 where it is -1; row 0, the last row and one of rows 16-31
    are served first.
    -> dict(A, W, bias, acc [M,N] before the maximum, out / out_nb [groups,N] with / without bias, stats / stats_nb)"""
    g = torch.Generator().manual_seed(N * 7919 + K * 31 + groups * 1000 + Mg + attempt * 1000003)
    M = groups * Mg
    A = torch.randint(1, 65, (M, K), generator=g).float() / 8
    W = _ternary(g, N, K)
    nneg = (N + 7) // 8
    W[:nneg] = -W[:nneg].abs()
    W[:nneg, :4] = -1.0
    bias = _quarters(g, N, -4, 4)
    bias[:nneg] = -bias[:nneg].abs()
    for gi in range(groups):
        # the rows a kernel is most likely to lose come first (row 0, the last row, one of rows 16-31), then any others
        first = [0, Mg - 1, 16 + int(torch.randint(0, 16, (1,), generator=g))]
        rows = (first + [r for r in torch.randperm(Mg, generator=g).tolist() if r not in first])[:min(Mg, N)]
        cols = torch.randperm(N, generator=g)[:min(Mg, N)]
        for r, c in zip(rows, cols.tolist()):   # (drawn per element, so that no two groups share a maximum)
            hi, lo = torch.randint(48, 65, (K,), generator=g).float() / 8, torch.randint(1, 5, (K,), generator=g).float() / 8
            A[gi * Mg + r] = torch.where(W[c] > 0, hi, torch.where(W[c] < 0, lo, A[gi * Mg + r]))
    acc = A @ W.T
    out_nb = group_max(acc, groups, Mg)
    res = dict(A=A, W=W, bias=bias, acc=acc, out=out_nb + bias, out_nb=out_nb)
    for key, b in (("stats", bias), ("stats_nb", None)):
        o = res["out"] if b is not None else out_nb
        res[key] = dict(margin=exactness(A, W, b), lattice=on_lattice(A, acc, o), cover=coverage(acc, groups, Mg, range(groups)),
                        neg=float((o < 0).float().mean()), rounded=float((o.to(torch.bfloat16).float() != o).float().mean()))
    return res


@functools.lru_cache(maxsize=None)
def groupmax_case(N, K, groups, Mg):
    """the first draw (of a fixed sequence of seeds) whose reference meets check_groupmax_preconditions: two spikes can shadow each
    other, and the conditions are on the reference's numbers, not on how they were planted"""
    for attempt in range(32):
        res = _groupmax_draw(N, K, groups, Mg, attempt)
        if all(st["cover"] == min(Mg, N) and st["neg"] >= 0.05 for st in (res["stats"], res["stats_nb"])):
            return res
    raise AssertionError(f"no lattice draw of gemm_groupmax N={N} K={K} {groups} x {Mg} covers min(Mg, N) row positions")


def check_groupmax_preconditions(st, N, Mg):
    assert st["lattice"] and st["margin"] < 1.0, st
    assert st["cover"] == min(Mg, N), st
    assert st["neg"] >= 0.05, st
