"""Lattice operands, case tables and float64 references of the GEMM family (csrc/gemm.hip cmdiad_gemm_bf16 and the five kernels
behind it, csrc/gemm_sk.hip cmdiad_gemm_streamk_bf16, csrc/gemm_tn.hip cmdiad_gemm_tn_bf16), shared by
tests/test_gpu_gemm_edges.py and pinned by tests/test_gemm_ref_cpu.py.  No GPU, no cmdiad_amd import.

Every operand sits on a lattice on which each product, each partial sum in ANY order and each epilogue value is a multiple of 1/16
far below 2^24 / 16 in magnitude, hence exact in fp32: whatever order a kernel adds in, its fp32 result is determined bit for bit
and equals the float64 reference; a bf16 output is the nearest-even cast of that value.

  A            integers in [-4, 4]            W          integers in [-2, 2]              (K <= 1024: |A . W^T| <= 2^13)
  bias, group_bias   multiples of 1/4 in [-8, 8]
  residual, add2     multiples of 1/2 in [-32, 32]
  row_scale    a power of two in {1/4, 1/2, 1, 2}
  gemm_tn      P integers in [-4, 4], Q integers in [-2, 2], M <= 1024; the column sum of P is an exact integer

GELU cases: the pre-activation is exact, the output is compared with float64 erf-GELU of it within GELU_ABS (csrc/common.h) and
one rounding of the output format.

The epilogue restated (csrc/gemm.hip gemm_std_kernel / gemm_std_pp3_kernel, csrc/gemm_core.h residual_rows_block):
  v = row_scale[m] * acc + bias[n]   (one FMA)   or   acc + bias[n];     v += group_bias[m / group_rows][n];
  v = act(v);     v += residual[m][n];     (+ add2[m][n]: the LayerNorm-fold producer only)
Split-K (cmdiad_gemm_bf16 split_k > 1, cmdiad_gemm_tn_bf16): slab y holds the K-tiles [y per, min((y + 1) per, KT)) with
per = ceil(KT / split); a slab left without a K-tile is all zeros."""
import collections
import functools
import math

import torch

BK = 64                               # K-tile of every kernel here (gemm_tn: 64 rows of m per step)
SENT32 = 0x4B3C5A69                   # sentinel bit patterns of tests/test_gpu_conv_edges.py (finite, in no reference here)
SENT16 = 0x5A69
PAD_VALUE = 3.0e4                     # what the pad columns of pitched operands hold: one read of it changes every result
GELU_ABS = 5.3e-7                     # csrc/common.h: |gelu_erf - GELU| for every finite x
ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2

# ------------------------------------------------------------------------------------------------ case tables
# 1, 2, 3, 4, 5, 8 and 16 K-tiles against the three-stage pipeline (both prologue branches), N below one tile, N = 128 t +- 4,
# M = 128 t - 1, 128 t, 128 t + 1
GENERAL_SHAPES = [(1, 4, 64), (5, 60, 128), (127, 124, 192), (128, 128, 64), (129, 132, 192), (255, 260, 256), (257, 8, 320),
                  (300, 1156, 512), (1025, 64, 1024)]
# dispatch settings of the 128 x 128 kernel: (name, environment)
SETTINGS = [("default", {}), ("panel", {"CMDIAD_GEMM_PANEL_MIN": "1"}), ("rowmajor", {"CMDIAD_GEMM_GROUPM": "1"})]

# outs: "f32", "bf16" or "both"; group_rows 0 = no group bias; split 1 = no split-K
Form = collections.namedtuple("Form", "name bias group_rows act residual row_scale split outs")
BIAS_RES_F32 = Form("bias_res_f32", True, 0, ACT_NONE, True, False, 1, "f32")   # N % 64 == 0: the residual-row epilogue; else general
GENERAL_FORMS = [
    Form("plain", False, 0, ACT_NONE, False, False, 1, "both"),
    Form("bias_relu", True, 0, ACT_RELU, False, False, 1, "bf16"),
    Form("bias_gb1_relu", True, 1, ACT_RELU, False, False, 1, "both"),
    Form("bias_gb32_relu", True, 32, ACT_RELU, False, False, 1, "both"),     # group boundaries at 32, 64, 96: inside the 128-row tile
    Form("bias_res", True, 0, ACT_NONE, True, False, 1, "both"),            # two outputs: the GENERAL epilogue's residual add at every N
    Form("bias_gelu", True, 0, ACT_GELU, False, False, 1, "both"),
    Form("rscale_bias", True, 0, ACT_NONE, False, True, 1, "both"),
    Form("split2", False, 0, ACT_NONE, False, False, 2, "f32"),
    Form("split3", False, 0, ACT_NONE, False, False, 3, "f32"),
    Form("split5", False, 0, ACT_NONE, False, False, 5, "f32"),
    BIAS_RES_F32,
]

# the 256-column kernels: M = 1 and 100 leave the wr = 1 half of the 256-row tile wholly past M; fewer jobs than blocks throughout
WIDE256_SHAPES = [(1, 256, 192), (100, 256, 192), (255, 512, 192), (257, 256, 256), (513, 768, 320)]
PP3_FORMS = [
    Form("bias", True, 0, ACT_NONE, False, False, 1, "bf16"),
    Form("bias_gelu", True, 0, ACT_GELU, False, False, 1, "bf16"),
    Form("bias_relu", True, 0, ACT_RELU, False, False, 1, "bf16"),
    Form("rscale_bias", True, 0, ACT_NONE, False, True, 1, "bf16"),
]
PP3_ENV = {"CMDIAD_GEMM_PP3": "1"}
RES_WIDE_ENV = {"CMDIAD_GEMM_RES_WIDE": "1"}

# the 4-wave shapes of the A/B build (CMDIAD_GEMM_WIDE = 4: 256 x 128, 8: 256 x 256): bias, group bias, activation, both outputs
AB_WIDE_SHAPES = [(1, 4, 64), (129, 132, 192), (255, 260, 256), (300, 1156, 512), (257, 256, 256)]
AB_WIDE_FORMS = [f for f in GENERAL_FORMS if not f.residual and not f.row_scale and f.split == 1]

# pitches in elements beyond the matrix width: (lda, ldw, ldr, ldo32, ldo16, ld_xb, ld_add2)
Pitch = collections.namedtuple("Pitch", "a w r o32 o16 xb add2", defaults=(0, 0, 0, 0, 0, 0, 0))
PITCHED = Pitch(8, 24, 4, 12, 8, 4, 8)
# (kernel, environment, shape, form): at least one shape per kernel; "ln" = the residual-row epilogue with ln_xb / ln_part / add2
PITCHED_CASES = [
    ("general", {}, (5, 60, 128), GENERAL_FORMS[0]),
    ("general", {}, (129, 132, 192), GENERAL_FORMS[3]),
    ("general", {}, (255, 260, 256), GENERAL_FORMS[4]),
    ("general", {}, (255, 260, 256), GENERAL_FORMS[5]),
    ("general", {}, (127, 124, 192), GENERAL_FORMS[6]),
    ("general", {}, (255, 260, 256), GENERAL_FORMS[8]),        # split 3 of four K-tiles: the empty third slab is zeroed at the pitch
    ("general", {"CMDIAD_GEMM_PANEL_MIN": "1"}, (300, 1156, 512), GENERAL_FORMS[1]),
    ("res_rows", {}, (1025, 64, 1024), BIAS_RES_F32),
    ("res_rows", {}, (257, 256, 256), BIAS_RES_F32),
    ("ln", {}, (257, 256, 256), BIAS_RES_F32),
    ("pp3", PP3_ENV, (100, 256, 192), PP3_FORMS[1]),
    ("pp3", PP3_ENV, (513, 768, 320), PP3_FORMS[3]),
    ("res_wide", RES_WIDE_ENV, (100, 256, 192), BIAS_RES_F32),
    ("res_wide", RES_WIDE_ENV, (513, 768, 320), BIAS_RES_F32),
]

# cmdiad_gemm_tn_bf16: (M, N1, N2, split, pitched).  (576, 200, 328, 4): nine K-steps in slabs of three, the fourth slab is empty
TN_CASES = [(64, 8, 8, 1, False), (128, 136, 72, 2, False), (576, 200, 328, 4, False), (640, 128, 128, 10, False),
            (1024, 264, 8, 3, False), (192, 136, 200, 2, True)]
TN_PITCH = (8, 16, 4)                 # ldp - N1, ldq - N2, ldo - N2

# stream-K at the edges of its eligibility (256 blocks): 257 tiles, the last with one row; 511 tiles, the last with one row;
# 258 tiles of four K-tiles; 511 whole tiles.  K = 192 is the minimum of three K-tiles.
STREAMK_SHAPES = [(65537, 256, 192), (130561, 256, 192), (32924, 512, 256), (130816, 256, 192)]

# seeds: a table entry that misses a precondition of tests/test_gemm_ref_cpu.py gets another seed here, never a weaker condition
SEEDS = {(1, 256, 192): 1}            # the default seed drew row_scale = 1/4 for the one row: every output below 64, exact in bf16


def seed_of(*shape):
    return SEEDS.get(tuple(shape), sum(s * p for s, p in zip(shape, (1000003, 1009, 17, 5))) % (2 ** 31 - 1))


# ------------------------------------------------------------------------------------------------ operands
def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


Operands = collections.namedtuple("Operands", "A W bias gb1 gb32 res add2 rscale")


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """float32 CPU tensors on the lattice (see the module docstring); gb1 / gb32: the group bias for group_rows = 1 / 32."""
    g = torch.Generator().manual_seed(seed_of(M, N, K))
    return Operands(A=_ints(g, -4, 4, (M, K)), W=_ints(g, -2, 2, (N, K)), bias=_ints(g, -32, 32, (N,)) / 4,
                    gb1=_ints(g, -32, 32, (M, N)) / 4, gb32=_ints(g, -32, 32, ((M + 31) // 32, N)) / 4,
                    res=_ints(g, -64, 64, (M, N)) / 2, add2=_ints(g, -64, 64, (M, N)) / 2,
                    rscale=2.0 ** _ints(g, -2, 1, (M,)))


@functools.lru_cache(maxsize=None)
def tn_operands(M, N1, N2):
    g = torch.Generator().manual_seed(seed_of(M, N1, N2, 7))
    return _ints(g, -4, 4, (M, N1)), _ints(g, -2, 2, (M, N2))


# ------------------------------------------------------------------------------------------------ references
def slab_ranges(KT, split):
    """[(first K-tile, K-tile count)] of the `split` slabs; count 0 = an empty slab (all zeros)."""
    per = (KT + split - 1) // split
    return [(y * per, max(0, min(per, KT - y * per))) for y in range(split)]


def gelu64(x):
    return 0.5 * x * torch.erfc(-x / math.sqrt(2.0))


def group_bias_of(o, form):
    return None if not form.group_rows else (o.gb1 if form.group_rows == 1 else o.gb32)


def reference(o, form, add2=False):
    """float64 (pre-activation, output) of cmdiad_gemm_bf16 on Operands o; split-K forms: the slabs [split, M, N] twice."""
    A, W = o.A.double(), o.W.double()
    if form.split > 1:
        slabs = torch.stack([A[:, k0 * BK:(k0 + n) * BK] @ W[:, k0 * BK:(k0 + n) * BK].T for k0, n in slab_ranges(A.shape[1] // BK, form.split)])
        return slabs, slabs
    v = A @ W.T
    if form.row_scale:
        v = v * o.rscale.double()[:, None]
    if form.bias:
        v = v + o.bias.double()
    if form.group_rows:
        v = v + group_bias_of(o, form).double().repeat_interleave(form.group_rows, 0)[:A.shape[0]]
    pre = v
    if form.act == ACT_GELU:
        v = gelu64(v)
    elif form.act == ACT_RELU:
        v = torch.relu(v)
    if form.residual:
        v = v + o.res.double()
    if add2:
        v = v + o.add2.double()
    return pre, v + 0.0                                           # (+ 0.0: no negative zero in a reference)


def tn_reference(P, Q, split):
    """float64 slabs [split, N1, N2] of P^T Q over each slab's own rows, and the column sums of P [split, N1] over the same rows."""
    out, cs = [], []
    for k0, n in slab_ranges(P.shape[0] // BK, split):
        p, q = P[k0 * BK:(k0 + n) * BK].double(), Q[k0 * BK:(k0 + n) * BK].double()
        out.append(p.T @ q)
        cs.append(p.sum(0))
    return torch.stack(out), torch.stack(cs)


def fp32_product_two_orders(X, Y):
    """X [M, K] . Y [N, K]^T in float32 two ways: K ascending in one matmul, and K-tile by K-tile added in DESCENDING order."""
    fwd = X @ Y.T
    rev = torch.zeros_like(fwd)
    for k0 in range(X.shape[1] - BK, -1, -BK):
        rev = rev + X[:, k0:k0 + BK].flip(1) @ Y[:, k0:k0 + BK].flip(1).T
    return fwd, rev


# ------------------------------------------------------------------------------------------------ roundings and bounds
def bf16_rne(x):
    return x.float().to(torch.bfloat16)


def bf16_inexact(x):
    """elements of the float64 tensor x that bf16 cannot hold"""
    return bf16_rne(x).double() != x


def gelu_bound_f32(ref):
    return GELU_ABS + 2.0 ** -24 * ref.abs()


def bf16_bound(ref, extra=0.0):
    """|bf16(v) - ref| for a v within `extra` of ref: half a bf16 ulp (<= 2^-8 |v|) + extra (tests/test_gpu_train_kernels.py)."""
    return 2.0 ** -8 * (ref.abs() + extra) + extra


def has_sentinel(x):
    """x float64: does its fp32 cast or its bf16 cast carry a sentinel bit pattern?"""
    return bool((x.float().contiguous().view(torch.int32) == SENT32).any() or (bf16_rne(x).contiguous().view(torch.int16) == SENT16).any())


def locate(row, col, bm=128, bn=128, wm=64, wn=64):
    """where an output element sits in a kernel's tiling: block tile (bm x bn) and wave (wm x wn) inside it"""
    return f"tile ({row // bm}, {col // bn}) of {bm} x {bn}, wave (wr {row % bm // wm}, wc {col % bn // wn}), row {row % wm} col {col % wn} of the wave"


def first_difference(got, want, tiling=(128, 128, 64, 64)):
    """None when the two 2-D tensors hold the same bits, else a description of the first differing element."""
    gi = got.contiguous().view(torch.int32 if got.dtype == torch.float32 else torch.int16)
    wi = want.contiguous().view(torch.int32 if want.dtype == torch.float32 else torch.int16)
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} against {tuple(want.shape)}"
    if torch.equal(gi, wi):
        return None
    bad = (gi != wi).nonzero()
    r, c = int(bad[0][0]), int(bad[0][1])
    return (f"{len(bad)} of {got.numel()} differ; first at ({r}, {c}): got {float(got[r, c])!r}, want {float(want[r, c])!r}; "
            + locate(r, c, *tiling))


def all_cases():
    """every (shape, form) that tests/test_gpu_gemm_edges.py launches through cmdiad_gemm_bf16, once"""
    cases = [(s, f) for s in GENERAL_SHAPES for f in GENERAL_FORMS]
    cases += [(s, f) for s in WIDE256_SHAPES for f in PP3_FORMS + [BIAS_RES_F32]]
    cases += [(s, f) for s in AB_WIDE_SHAPES for f in AB_WIDE_FORMS]
    cases += [(s, f) for _, _, s, f in PITCHED_CASES]
    return list(dict.fromkeys(cases))
