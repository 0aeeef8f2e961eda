// Shared device helpers for the gfx950 (CDNA4, wave64) kernels of cmdiad_amd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmdiad_hip.h"
#include "gemm_plan.h"   // host only: the plans of the GEMM family
#include "workspace.h"   // host only: Carve, workspace_ok

using plan::aligned16;
using plan::kPersistCUs;
using plan::ln_out_operands_ok;

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define CMDIAD_WAVE 64

// Last error text, returned through cmdiad_last_error().  Never throws across the C ABI.
void cmdiad_set_error(const char* fmt, ...);

#define CMDIAD_REQUIRE(cond, code, ...)        \
    do {                                       \
        if (!(cond)) {                         \
            cmdiad_set_error(__VA_ARGS__);     \
            return (code);                     \
        }                                      \
    } while (0)

#define CMDIAD_CHECK_LAUNCH()                                                  \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess) {                                                \
            cmdiad_set_error("%s:%d launch: %s", __FILE__, __LINE__, hipGetErrorString(e_)); \
            return CMDIAD_ERR_LAUNCH;                                          \
        }                                                                      \
    } while (0)

__device__ __forceinline__ float bf2f(bf16_t v) { return (float)v; }
__device__ __forceinline__ bf16_t f2bf(float v) { return (bf16_t)v; }

// erf-GELU (nn.GELU() default, utils/utils.py:97, models/models.py:129):  GELU(x) = x - h for x > 0, h otherwise, with
// h = 0.5 x erfc(|x| / sqrt 2) and erfc(z) = 2^(-q(z)), q a degree-6 polynomial fitted to -log2 erfc on [0, 4.3] (beyond it
// erfc < 2e-9).  Past the clamp (x < -4.3 sqrt 2) 2^(-q) stays at erfc(4.3), so the x that multiplies it is clamped there too
// (NaN-propagating v_maximum3_f32, one VALU op): h then stays at -3.6e-9 for every x below instead of growing with |x| (-6e-7
// at x = -1000, -1.8e29 at -3e38), and nothing changes for x >= -4.3 sqrt 2.  |error| <= 5.3e-7 absolute on the GELU value for
// every finite x -- a tenth of a bf16 half-ulp, the same bound as the Abramowitz-Stegun 7.1.26 form it replaces -- with ONE
// transcendental (v_exp_f32, quarter rate) instead of two (rcp + exp): ~17 VALU issue slots per element instead of ~22, and the
// Horner steps are plain FMAs that the 4-wide form below hands to v_pk_fma_f32 two elements at a time.  The fc1 epilogues run
// this on 77 M activations per ViT layer; in the two-group persistent GEMM both waves of a SIMD evaluate it between the same two
// barriers, where it is not hidden by anything.
#define CMDIAD_GELU_Q6 -2.3885208886e-04f
#define CMDIAD_GELU_Q5 4.0851729330e-03f
#define CMDIAD_GELU_Q4 -3.1410888601e-02f
#define CMDIAD_GELU_Q3 1.4969202041e-01f
#define CMDIAD_GELU_Q2 9.1851604883e-01f
#define CMDIAD_GELU_Q1 1.6277476882e+00f
#define CMDIAD_GELU_Q0 2.2232231590e-05f
#define CMDIAD_GELU_XMIN -6.0811529f   // -4.3 sqrt 2: below it z is clamped

__device__ __forceinline__ float gelu_erf(float x)
{
    const float z = fminf(fabsf(x) * 0.70710678118654752440f, 4.3f);
    float q = fmaf(CMDIAD_GELU_Q6, z, CMDIAD_GELU_Q5);
    q = fmaf(q, z, CMDIAD_GELU_Q4);
    q = fmaf(q, z, CMDIAD_GELU_Q3);
    q = fmaf(q, z, CMDIAD_GELU_Q2);
    q = fmaf(q, z, CMDIAD_GELU_Q1);
    q = fmaf(q, z, CMDIAD_GELU_Q0);
    const float h = (0.5f * __builtin_elementwise_maximum(x, CMDIAD_GELU_XMIN)) * __builtin_amdgcn_exp2f(-q);
    return x > 0.0f ? x - h : h;
}

// the same on four values: identical arithmetic per element (so every kernel gives the same bits whichever form it uses)
__device__ __forceinline__ f32x4 gelu_erf4(f32x4 x)
{
    f32x4 z;
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = fminf(fabsf(x[i]) * 0.70710678118654752440f, 4.3f);
    const f32x4 c5 = {CMDIAD_GELU_Q5, CMDIAD_GELU_Q5, CMDIAD_GELU_Q5, CMDIAD_GELU_Q5};
    const f32x4 c4 = {CMDIAD_GELU_Q4, CMDIAD_GELU_Q4, CMDIAD_GELU_Q4, CMDIAD_GELU_Q4};
    const f32x4 c3 = {CMDIAD_GELU_Q3, CMDIAD_GELU_Q3, CMDIAD_GELU_Q3, CMDIAD_GELU_Q3};
    const f32x4 c2 = {CMDIAD_GELU_Q2, CMDIAD_GELU_Q2, CMDIAD_GELU_Q2, CMDIAD_GELU_Q2};
    const f32x4 c1 = {CMDIAD_GELU_Q1, CMDIAD_GELU_Q1, CMDIAD_GELU_Q1, CMDIAD_GELU_Q1};
    const f32x4 c0 = {CMDIAD_GELU_Q0, CMDIAD_GELU_Q0, CMDIAD_GELU_Q0, CMDIAD_GELU_Q0};
    f32x4 q = __builtin_elementwise_fma(f32x4{CMDIAD_GELU_Q6, CMDIAD_GELU_Q6, CMDIAD_GELU_Q6, CMDIAD_GELU_Q6}, z, c5);
    q = __builtin_elementwise_fma(q, z, c4);
    q = __builtin_elementwise_fma(q, z, c3);
    q = __builtin_elementwise_fma(q, z, c2);
    q = __builtin_elementwise_fma(q, z, c1);
    q = __builtin_elementwise_fma(q, z, c0);
    const f32x4 hx = __builtin_elementwise_maximum(x, f32x4{CMDIAD_GELU_XMIN, CMDIAD_GELU_XMIN, CMDIAD_GELU_XMIN, CMDIAD_GELU_XMIN}) * 0.5f;
    f32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float h = hx[i] * __builtin_amdgcn_exp2f(-q[i]);
        out[i] = x[i] > 0.0f ? x[i] - h : h;
    }
    return out;
}

// d/dx of the above: Phi(x) + x phi(x), sharing the one exponential (exp(-x^2/2) = exp(-z^2))
__device__ __forceinline__ float gelu_erf_grad(float x)
{
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __expf(-z * z);
    const float erfa = 1.0f - p * t * e;
    return 0.5f * (1.0f + copysignf(erfa, x)) + x * 0.39894228040143267794f * e;
}

// 64-bit key: high word = fp32 bits of a NON-NEGATIVE value, low word = index.  Integer order of
// the key == (value, index) lexicographic order, so min over keys = smallest value, lowest index.
__device__ __forceinline__ unsigned long long pack_key(float v, unsigned idx)
{
    return ((unsigned long long)__float_as_uint(v) << 32) | idx;
}

// Order keys of ANY float: the unsigned order of the key is the order of the values, so integer atomicMin / atomicMax, sorts and
// binary searches work on them.  f2ord / d2ord keep -0.0 below +0.0 (two keys); f64_key folds -0.0 into +0.0 (one key), which is
// what a comparison of scores needs (docs/metrics.md).
__device__ __forceinline__ uint32_t f2ord(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__device__ __forceinline__ unsigned long long d2ord(double d)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord2d(unsigned long long u)
{
    return __longlong_as_double((long long)((u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u));
}

constexpr unsigned long long kSign = 0x8000000000000000ull;
__device__ __forceinline__ unsigned long long f64_key(double x)
{
    unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (b == kSign) b = 0;
    return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double key_f64(unsigned long long k) { return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k)); }

// max over the 16 lanes of a DPP row (lanes 16 r .. 16 r + 15), result in all 16: quad xor 1, quad xor 2, half-row mirror,
// row mirror -- VALU only (four __shfl_xor steps are four ds_bpermute round trips through the LDS pipeline).
__device__ __forceinline__ float row16_max(float v)
{
    int i = __builtin_bit_cast(int, v);
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0xB1, 0xF, 0xF, false)));
    i = __builtin_bit_cast(int, v);
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x4E, 0xF, 0xF, false)));
    i = __builtin_bit_cast(int, v);
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x141, 0xF, 0xF, false)));
    i = __builtin_bit_cast(int, v);
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, 0x140, 0xF, 0xF, false)));
    return v;
}

// The same for N >= 4 values at once, ONE instruction per value and step (v_max_f32 with the DPP modifier on its first
// source): the builtin form above costs a copy, the DPP move, a quieting v_max v, v, v and the max.  Inline asm is outside
// the compiler's hazard tracking: a DPP read needs two wait states after the VALU write of its source -- the s_nop covers
// the values' producers, and inside the batch consecutive steps of one value are N - 1 >= 3 instructions apart (the
// statements are volatile: their order is kept).  No NaN inputs.
template <int N>
__device__ __forceinline__ void row16_max_batch(float (&v)[N])
{
    static_assert(N >= 4, "spacing between dependent DPP steps");
    asm volatile("s_nop 1");
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_max_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_max_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_max_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
#pragma unroll
    for (int k = 0; k < N; ++k) asm volatile("v_max_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(v[k]));
    asm volatile("s_nop 1");   // nothing the compiler places next may read a lane-crossed result too early either
}

// Sum over the 64 lanes, result wave-uniform: four DPP steps inside the rows of 16 (as row16_max), then the four row sums are
// read as scalars and added in row order -- ~11 VALU instructions against six ds_bpermute round trips for the xor butterfly
// (whose summation order differs: results agree to fp32 rounding, not bitwise).
__device__ __forceinline__ float wave_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
    const int i = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(i, 48));
    return ((r0 + r1) + r2) + r3;
}

// (a, b) = (v, v) -> v_permlane32_swap exchanges a's upper 32 lanes with b's lower 32: afterwards {a, b} = {v[lane], v[lane ^ 32]}
// in some order on every lane, so max(a, b) / a + b are the cross-half reductions -- one VALU instruction instead of the
// ds_bpermute round trip of __shfl_xor(v, 32).  (Inline asm: the builtin folds the two results of equal inputs into one;
// two wait states between the VALU write of the sources and the permlane read, outside the compiler's hazard tracking.)
__device__ __forceinline__ void half_swap(float v, float& a, float& b)
{
    a = v;
    b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float half_max(float v) { float a, b; half_swap(v, a, b); return fmaxf(a, b); }
__device__ __forceinline__ float half_sum(float v) { float a, b; half_swap(v, a, b); return a + b; }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return ((unsigned long long)hi << 32) | lo;
}
