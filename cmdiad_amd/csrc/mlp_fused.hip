// Point-MAE MLP as one kernel (C = 384, hidden = 1 536, folded LayerNorm):  x += fc2(GELU(rstd o (xb . W1''^T) + b1')) + b2
// on the fp32 residual stream, in place.  The [M, 1 536] bf16 hidden never leaves the CU: the pair of products it replaces
// (gemm_std_pp3_kernel<GELU, true> + the 128 x 128 residual-row gemm_std_kernel) writes it and reads it back, 100 MB per layer
// at M = 32 768 -- 2.4 GB per Point-MAE forward of pure round trip.
//
// One block of 8 waves per 128-row tile (M = 32 768: 256 tiles, one per CU).  Every wave owns 16 rows, end to end:
//   * its rows of the block input xb (16 x 384 bf16, 12 KiB) are staged into LDS once and stay there;
//   * the hidden is produced in chunks of 64 columns: fc1 over K = 384 into 16 accumulators, then row_scale, bias, erf-GELU,
//     bf16, parked in a private 2 KiB LDS tile in the fragment layout of the 128 x 128 kernel's A stage;
//   * fc2 adds that chunk's 64-deep contribution to all 384 output columns (96 accumulators per lane).
// Only the weights stream, as 8 KiB pieces of [64 rows][64 k] (W1 rows c*64.. at K-tile s; W2 rows nb*64.. at K-tile c) through
// a ring of six LDS slots, five pieces ahead (one LDS-DMA instruction per wave and piece, counted vmcnt(4), one barrier per
// piece).  Per tile 2.36 MB of weights from L2 (both matrices, shared by the 32 CUs of an XCD) against ~302 MFLOP.
//
// Results are bit-identical to the two launches: every accumulator sees the same v_mfma_f32_16x16x32_bf16 chain as in the
// products it replaces -- swapped orientation (weights as the MFMA A operand), the same k of each lane's fragment, K blocks
// of 32 in increasing order from zero (fc1 over K = 384; fc2 over the chunks in order, i.e. K = 1 536 in order) -- and the
// epilogues are the same code: act_bf16<GELU, true> (fma(acc, rstd, b1) -> gelu_erf4 -> bf16) for the hidden, as in
// gemm_std_pp3_kernel; residual_rows_block (RowStore32, the residual-row arithmetic and the 64-column ln_part sums in their
// lane order), as in gemm_std_kernel<..., RES_ROWS, LN_OUT>, for the output.  Both live in gemm_core.h.
//
// LDS: xb 8 x 12 KiB + hidden 8 x 2 KiB + ring 6 x 8 KiB = 160 KiB.
#include "gemm_core.h"
#include "launch.h"

namespace {

using namespace gemm;

constexpr int kC = 384, kHid = 1536, kBM = 128, kWaves = 8;
constexpr int kChunks = kHid / 64;          // 24 hidden chunks of 64 columns
constexpr int kKT1 = kC / BK;               // 6 fc1 K-tiles per chunk
constexpr int kPer = kKT1 + kC / 64;        // 12 weight pieces per chunk: 6 of W1, then 6 of W2
constexpr int kSlots = 6, kAhead = kSlots - 1;
static_assert(kPer % kSlots == 0, "the slot of a piece depends on its place in the chunk only");
constexpr int kPieceBytes = 64 * BK * 2;    // 8 KiB
constexpr int kXbWave = kKT1 * 16 * BK * 2; // 12 KiB of xb per wave
constexpr int kHOff = kWaves * kXbWave;     // 96 KiB
constexpr int kRingOff = kHOff + kWaves * 2048;
constexpr int kLdsBytes = kRingOff + kSlots * kPieceBytes;
static_assert(kLdsBytes == 160 * 1024, "LDS budget");

struct MlpParams {
    int M;
    const bf16_t* xb;        // [M, 384] raw rows of the block input as bf16 (proj's ln_xb)
    const float* row_scale;  // [M] 1 / sigma (fc1's LayerNorm fold)
    const bf16_t* w1;        // [1536, 384] folded fc1 weights
    const float* b1;         // [1536]
    const bf16_t* w2;        // [384, 1536]
    const float* b2;         // [384]
    float* x;                // [M, 384] residual stream, updated in place
    bf16_t* ln_xb;           // LN_OUT: bf16 copy of the new rows ...
    float* ln_part;          // ... and (sum, M2) of every 64-column chunk [6][M][2]
    const float* add2;       // LN_OUT: added after the residual (the next block's pos), or null
};

__device__ __forceinline__ void mlp_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <bool LN_OUT>
__global__ __launch_bounds__(512, 1) void pmae_mlp_fused_kernel(MlpParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, r16 = lane & 15;
    const int mw = (int)blockIdx.x * kBM + wave * 16;   // first row of this wave
    char* xs = lds + wave * kXbWave;
    char* hs = lds + kHOff + wave * 2048;
    char* ring = lds + kRingOff;

    // Epilogue operands come by inline asm (the compiler then places no vmcnt of its own, which in this loop would be a
    // vmcnt(0): a drain of the ring).  1 / sigma of the lane's row (rows past M: clamped, computed, never stored) and the
    // fc1 bias of chunk 0 land with the prologue's wait; the bias of chunk c + 1 is fetched in step 7 of chunk c.
    float rsc;
    f32x4 b1v[4];   // fc1 bias of the current chunk: the lane's four columns of each 16-column block
    auto load_b1 = [&](int c) {
        const float* bp = p.b1 + c * 64 + g * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(b1v[j]) : "v"(bp + j * 16) : "memory");
    };
    {
        const float* rp = p.row_scale + min(mw + r16, p.M - 1);
        asm volatile("global_load_dword %0, %1, off" : "=v"(rsc) : "v"(rp) : "memory");
    }
    load_b1(0);
    // the wave's 16 rows of xb: 6 K-tiles x 2 pieces of 8 rows; lane l lands on row l >> 3, physical chunk l & 7
    const int sw_chunk = (lane & 7) ^ (lane >> 3);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const bf16_t* src = p.xb + (size_t)min(mw + e * 8 + (lane >> 3), p.M - 1) * kC + sw_chunk * 8;
#pragma unroll
        for (int s = 0; s < kKT1; ++s)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + s * BK),
                                             (__attribute__((address_space(3))) void*)(xs + s * 2048 + e * 1024), 16, 0, 0);
    }
    // weight pieces: wave w stages rows 8 w .. 8 w + 7 of the piece
    const char* w1l = reinterpret_cast<const char*>(p.w1 + (size_t)(wave * 8 + (lane >> 3)) * kC + sw_chunk * 8);
    const char* w2l = reinterpret_cast<const char*>(p.w2 + (size_t)(wave * 8 + (lane >> 3)) * kHid + sw_chunk * 8);
    auto issue = [&](int c, int q) {   // piece q of chunk c (q compile-time after unrolling)
        const char* src = q < kKT1 ? w1l + ((size_t)c * 64 * kC + q * BK) * 2 : w2l + ((size_t)(q - kKT1) * 64 * kHid + c * BK) * 2;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(ring + (q % kSlots) * kPieceBytes + wave * 1024), 16, 0, 0);
    };
#pragma unroll
    for (int q = 0; q < kAhead; ++q) issue(0, q);
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // rsc, the bias, xb and piece 0 have landed
    mlp_barrier();

    // fragments: row (lane & 15), k = kk * 32 + (lane >> 4) * 8 .. + 7 of the 64-deep tile
    auto ldf = [&](const char* tile, int row, int kk) { return *reinterpret_cast<const bf16x8*>(tile + lds_off(row, kk * 4 + g)); };
    auto step = [&](const char* wt, const bf16x8& a0, const bf16x8& a1, f32x4 (&acc)[4]) {
        bf16x8 wf[2][4];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[kk][j] = ldf(wt, j * 16 + r16, kk);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = mfma16(wf[kk][j], kk ? a1 : a0, acc[j]);
        __builtin_amdgcn_s_setprio(0);
    };

    f32x4 acc2[kC / 64][4];
#pragma unroll
    for (int nb = 0; nb < kC / 64; ++nb)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc2[nb][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c = 0; c < kChunks; ++c) {
        f32x4 acc1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        bf16x8 h0, h1;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            // the piece kAhead ahead goes into the slot read in the previous step, which every wave has left
            const int qn = q + kAhead < kPer ? q + kAhead : q + kAhead - kPer;
            const int cn = q + kAhead < kPer ? c : c + 1;
            const bool more = cn < kChunks;
            // the next chunk's bias (4 loads, older than this step's piece): the waits of steps 7-10 leave them in flight
            // (vmcnt(8) = the four youngest pieces + them), step 11's vmcnt(4) retires them
            if (q == 7 && more) load_b1(c + 1);
            if (more) issue(cn, qn);
            const char* wt = ring + (q % kSlots) * kPieceBytes;
            if (q < kKT1) step(wt, ldf(xs + q * 2048, r16, 0), ldf(xs + q * 2048, r16, 1), acc1);
            else step(wt, h0, h1, acc2[q - kKT1]);
            // the next piece must be in LDS before anyone reads it; the younger ones stay in flight across the barrier
            if (!more) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (q >= 7 && q <= 10) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            mlp_barrier();
            if (q == kKT1 - 1) {
                // hidden chunk: act_bf16 (gemm_core.h), the expression of gemm_std_pp3_kernel<GELU, true>, parked as bf16 at
                // row r16, columns j * 16 + 4 g .. + 3 of the wave's [16][64] tile, read back as fc2's A fragments
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<bf16x4*>(hs + lds_off(r16, 2 * j + (g >> 1)) + (g & 1) * 8) = act_bf16<CMDIAD_ACT_GELU, true>(acc1[j], rsc, b1v[j]);
                h0 = ldf(hs, r16, 0);
                h1 = ldf(hs, r16, 1);
            }
        }
    }

    // out = ((acc + b2) + x) (+ add2) through residual_rows_block (gemm_core.h), the epilogue of gemm_std_kernel<S128, NONE, false,
    // true, LN_OUT>: per 64-column chunk nb, rows R and R + 8 of the wave's 16
    RowStore32 rs;
    rs.init(hs, lane);   // (the hidden tile is no longer read)
    const ResRows o{p.x, kC, p.x, kC, p.ln_xb, kC, p.ln_part, p.add2, kC, p.M};
    const bool full = mw + 16 <= p.M;
#pragma unroll
    for (int nb = 0; nb < kC / 64; ++nb) {
        f32x4 bj[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bj[j] = *reinterpret_cast<const f32x4*>(p.b2 + nb * 64 + j * 16 + g * 4);
        residual_rows_block<LN_OUT>(rs, acc2[nb], bj, o, mw + rs.R, nb * 64, full);
    }
}

}  // namespace

// Launch sequencing entry for blocks.cpp (not part of the C ABI).  ln_xb / ln_part / add2: the PREP_NEXT outputs, or null.
int cmdiad_pmae_mlp_fused(float* x, const uint16_t* xb, const float* rstd, const uint16_t* w1, const float* b1, const uint16_t* w2,
                          const float* b2, int M, uint16_t* ln_xb, float* ln_part, const float* add2, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(x && xb && rstd && w1 && b1 && w2 && b2 && M > 0, CMDIAD_ERR_ARG, "cmdiad_pmae_mlp_fused: null operand");
    CMDIAD_REQUIRE(aligned16(x) && aligned16(xb) && aligned16(w1) && aligned16(w2) && aligned16(b1) && aligned16(b2) && (!add2 || aligned16(add2)), CMDIAD_ERR_ARG,
                   "cmdiad_pmae_mlp_fused: operands must be 16-byte aligned");
    CMDIAD_REQUIRE(ln_out_operands_ok(ln_xb, kC, ln_part, add2, kC), CMDIAD_ERR_ARG,
                   "cmdiad_pmae_mlp_fused: ln_xb and ln_part come together (8-byte aligned); add2 only with them");
    MlpParams p{M, (const bf16_t*)xb, rstd, (const bf16_t*)w1, b1, (const bf16_t*)w2, b2, x, (bf16_t*)ln_xb, ln_part, add2};
    const dim3 grid((unsigned)((M + kBM - 1) / kBM)), block(kWaves * 64);
    const int rc = ln_xb ? launch_lds<pmae_mlp_fused_kernel<true>>("cmdiad_pmae_mlp_fused", grid, block, kLdsBytes, (hipStream_t)stream, p)
                         : launch_lds<pmae_mlp_fused_kernel<false>>("cmdiad_pmae_mlp_fused", grid, block, kLdsBytes, (hipStream_t)stream, p);
    if (rc) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
