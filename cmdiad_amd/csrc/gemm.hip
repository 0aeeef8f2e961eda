// GEMM entry points built on gemm_core.h: generic Linear with fused epilogue, QKV with head-split
// stores, and the Point-MAE encoder stages (on-the-fly first conv, per-group max pooling).
#include <type_traits>

#ifdef CMDIAD_AB_VARIANTS
#include "gemm_wide.h"  // 4-wave 256-row shapes: A/B references, test-only build (make ab)
#else
#include "gemm_core.h"
#endif
#include "gemm_pp3.h"
#include "launch.h"

namespace {

using namespace gemm;

// ------------------------------------------------------------------------------------------------
// Generic:  out = act(A.W^T + bias + group_bias[row/group_rows]) + residual
// ------------------------------------------------------------------------------------------------
struct StdParams {
    int M, N, K;
    const float* bias;
    const float* group_bias;
    int group_rows;
    int act;
    const float* residual; int ldr;
    float* out_f32; int ldo32;
    bf16_t* out_bf16; int ldo16;
    bf16_t* out_pre_bf16;         // pre-activation copy (training keeps z for the GELU backward)
    const bf16_t* dact_of;        // acc *= GELU'(dact_of[m][n]) first (backward through an activation)
    int split_k;                  // > 1: block y handles K/split_k, writes slab y of out_f32 (no epilogue terms)
    int panel;                    // N tiles walked by one block (gemm_plan.h panel_tiles)
    int group_m;                  // M tiles per L2 group (Coord)
    const int* m_count;           // device-resident live row count (rows >= it are neither computed nor stored), or null
    // LayerNorm folded into the products on either side of it (see "LayerNorm fold" below)
    const float* row_scale;       // consumer: out = act(row_scale[m] * acc + bias) (1 / sigma of row m), or null
    bf16_t* ln_xb; int ld_xb;     // producer (residual-row epilogue): bf16 copy of the new residual rows ...
    float* ln_part;               // ... and [N/64][M] (sum, M2 about the chunk mean) of every 64-column chunk of them
    const float* add2; int ld_add2;  // producer: a second fp32 addend (Point-MAE's positional embedding of the NEXT block), or null
};

// (sum, M2 about the chunk mean) of `chunks` 64-column chunks of row m -> 1 / sqrt(var + eps); merged in chunk order (Chan et al.)
__device__ __forceinline__ float ln_merge_chunks(const float2* __restrict__ part, int M, int chunks, int m, float eps, float* mean_out)
{
    float sum = 0.0f;
    for (int c = 0; c < chunks; ++c) sum += part[(size_t)c * M + m].x;
    const float mean = sum / (float)(chunks * 64);
    float m2 = 0.0f;
    for (int c = 0; c < chunks; ++c) {
        const float2 v = part[(size_t)c * M + m];
        const float d = v.x * (1.0f / 64) - mean;
        m2 += v.y + 64.0f * d * d;
    }
    if (mean_out) *mean_out = mean;
    return rsqrtf(m2 / (float)(chunks * 64) + eps);
}

// rows the launch really has: the caller's M, or the device-side count of a compacted row set (block-uniform)
__device__ __forceinline__ void live_m(StdParams& p, GlobalTile& A)
{
    if (p.m_count) {
        p.M = min(p.M, __builtin_amdgcn_readfirstlane(*p.m_count));
        A.rows = max(p.M, 1);
    }
}

__device__ __forceinline__ float gelu_grad_f(float x) { return gelu_erf_grad(x); }

// block -> (m tile, n tile) with the XCD remap; lane/wave coordinates shared by every epilogue
template <class S>
struct Coord {
    int m0, nt, count, lane, wr, wc;
    // panel > 1: the block owns `panel` consecutive N tiles of its M panel and runs them as ONE flattened
    // pipeline (A comes from HBM once, from L2 afterwards; the fill/drain latency is paid once per panel).
    // group_m > 1: L2-aware order.  Walking all N tiles of one M tile before the next M tile makes the blocks that are
    // co-resident on an XCD (64 of them) touch ~3 A tiles and EVERY W tile: for fc1 (24 W tiles = 4.7 MB) that alone exceeds
    // the 4 MB L2 and the PMC pass shows each launch fetching 10x its operands from beyond L2.  In groups of `group_m` M tiles
    // walked M-fastest, 64 consecutive blocks cover group_m A tiles x 64/group_m W tiles (8 + 8 tiles = 3 MB at group_m = 8).
    // nwg: workgroups that have a tile (default: the launched grid).  A launch sized for more rows than are live (m_count)
    // remaps over the LIVE count: the remap hands every XCD a contiguous range of the tile order, so over the launched grid the
    // live row tiles would all land on the first XCDs and the others would idle.
    __device__ __forceinline__ Coord(int n_tiles_n, int panel = 1, int group_m = 1, int m_tiles = 0, int nwg = -1)
    {
        const int wg = xcd_remap(blockIdx.x, nwg < 0 ? (int)gridDim.x : nwg);
        const int groups = (n_tiles_n + panel - 1) / panel;
        if (group_m > 1) {
            const int per_group = group_m * groups;
            const int g = wg / per_group, within = wg - g * per_group;
            const int rows = min(group_m, m_tiles - g * group_m);  // the last group may be short
            m0 = (g * group_m + within % rows) * S::BM;
            nt = (within / rows) * panel;
        } else {
            m0 = (wg / groups) * S::BM;
            nt = (wg % groups) * panel;
        }
        count = min(panel, n_tiles_n - nt);
        lane = threadIdx.x & 63;
        const int wave = threadIdx.x >> 6;
        wr = wave / S::WN;
        wc = wave % S::WN;
    }
    // swapped orientation: lane holds row m(i), columns n(j) .. n(j)+3
    __device__ __forceinline__ int m(int i) const { return m0 + wr * (S::MI * 16) + i * 16 + (lane & 15); }
    __device__ __forceinline__ int n(int ntile, int j) const { return ntile * S::BN + wc * 64 + j * 16 + (lane >> 4) * 4; }
};

// The epilogue is specialised at compile time.  With every optional term as a run-time branch the 16 unrolled
// (row tile, column tile) bodies carried 64 inlined erff/expf expansions -- ~40 KB of code that even the skipped
// branches had to fetch through the instruction cache (measured: the plain 4.2M x 512 x 256 product spent as long
// in that epilogue as in its MFMA loop).  ACT = CMDIAD_ACT_*; EXTRAS = the training-only terms (dact_of, out_pre).
// LayerNorm fold (models/models.py:177-180: x = x + attn(norm1(x)); x = x + mlp(norm2(x))).  A stand-alone LayerNorm reads the
// fp32 residual rows the previous product has just written and writes their normalised bf16 copy: 6 bytes per element of pure
// traffic, 25 launches per network, 24 us each.  With  LN(x) . W^T = rstd (x - mean) . (gamma o W)^T + beta . W^T  and weights
// centred over k (W''[n,k] = gamma[k] W[n,k] - mean_k(gamma[k] W[n,k]), so that sum_k x[k] W''[n,k] = sum_k (x[k] - mean) gamma[k] W[n,k]
// for ANY row mean), the consumer multiplies the RAW rows: out = rstd[m] * (xb . W''^T) + (b + W beta).  The producer's
// residual-row epilogue (LN_OUT) therefore also stores the rows as bf16 (xb) and, per 64-column chunk, their sum and their
// squared deviation from the chunk mean; cmdiad_ln_stats_finalize merges the chunks (Chan's formula: no E[x^2] - mean^2
// cancellation, no atomics: bit-reproducible) into rstd[m], which the consumer's epilogue applies (row_scale).
// Rounding: x is rounded to bf16 instead of LN(x): the operand's rounding noise is sqrt(1 + (mean / sigma)^2) times that of
// the unfused form -- the same for the zero-mean-ish rows of a pre-LN residual stream.
template <class S, int ACT, bool EXTRAS, bool RES_ROWS = false, bool LN_OUT = false>
__global__ __launch_bounds__(S::THREADS, S::WAVES_PER_SIMD) void gemm_std_kernel(GlobalTile A, GlobalTile W, StdParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    live_m(p, A);                                                 // the grid was sized for the caller's M; p.M is the live row count now
    const int n_tiles_n = (p.N + S::BN - 1) / S::BN, m_tiles = (p.M + S::BM - 1) / S::BM;
    const int nwg = m_tiles * ((n_tiles_n + p.panel - 1) / p.panel);
    if ((int)blockIdx.x >= nwg) return;                           // block-uniform: no tile left for this workgroup
    const Coord<S> c(n_tiles_n, p.panel, p.group_m, m_tiles, nwg);
    const int kt_per = (p.K / BK + p.split_k - 1) / p.split_k;
    const int kt_begin = blockIdx.y * kt_per;
    const int kt_count = min(kt_per, p.K / BK - kt_begin);
    float* out32 = p.out_f32 ? p.out_f32 + (size_t)blockIdx.y * p.M * p.ldo32 : nullptr;
    if (kt_count <= 0) return;

    // fp32 residual stream in place (proj / fc2 of every transformer block): out_f32 = acc + bias + residual.  In the
    // accumulator layout its 16-byte loads and stores touch 16 rows x 64 bytes per instruction; on the short-K products the
    // texture addresser, not the MFMAs, then bounds the block (proj 25120 x 768 x 768: 417 TFLOP/s against fc2's 710 on the
    // same kernel).  RowStore32: 8 rows x 128 contiguous bytes per load / store.
    // RES_ROWS is its own instantiation, chosen on the host (gemm_plan.h res_rows_form()): with both epilogues in one kernel the
    // compiler ran out of registers and spilled the general path's row pointers (tools/isa_lint.py).
    static_assert(!RES_ROWS || (!EXTRAS && ACT == CMDIAD_ACT_NONE), "residual-row epilogue: no activation, no training terms");
    static_assert(!LN_OUT || RES_ROWS, "the LayerNorm statistics come from the residual-row epilogue");
    RowStore32 rs;
    rs.init(lds + S::LDS_BYTES + (threadIdx.x >> 6) * kRowStoreScratch, c.lane);

    run<S, true>(A, W, c.m0, c.nt, c.count, kt_count, lds, [&](auto& acc, int ntile, char*) {
        if constexpr (RES_ROWS) {
            const int n0 = ntile * S::BN + c.wc * 64;
            if (n0 >= p.N) return;   // N = 64 (2 t + 1): the last tile's second wave column has nothing to store (wave-uniform)
            f32x4 bj[4];
            if constexpr (!LN_OUT) {
#pragma unroll
                for (int j = 0; j < 4; ++j) bj[j] = *reinterpret_cast<const f32x4*>(p.bias + n0 + j * 16 + (c.lane >> 4) * 4);
            }
            // full tiles run without a per-row test (a branch per row = a basic block per store group = s_waitcnt vmcnt(0)
            // in front of each: stores count in vmcnt on gfx9)
            auto emit = [&](auto FULL) {
                constexpr bool full = decltype(FULL)::value;
                if constexpr (LN_OUT) {
                    // loaded INSIDE each of the two paths: fetched ahead of the full / ragged branch, the compiler's counter
                    // model sees them pending on the way back to the loop header and puts s_waitcnt vmcnt(0) between the
                    // LDS-DMA issue and the fragment reads of EVERY K-step (tools/isa_lint.py)
                    // (the two empty asm statements differ, so the identical loads of the two paths are not merged and hoisted back)
                    const float* bp = p.bias + n0 + (c.lane >> 4) * 4;
                    if constexpr (full) asm volatile("; bias of a full tile" : "+v"(bp));
                    else asm volatile("; bias of the ragged tile" : "+v"(bp));
#pragma unroll
                    for (int j = 0; j < 4; ++j) bj[j] = *reinterpret_cast<const f32x4*>(bp + j * 16);
                }
                // (built here, not ahead of the K loop: see m0r below)
                const ResRows o{p.residual, p.ldr, out32, p.ldo32, p.ln_xb, p.ld_xb, p.ln_part, p.add2, p.ld_add2, p.M};
#pragma unroll
                for (int i = 0; i < S::MI; ++i) {
                    int m0r = c.m0 + c.wr * (S::MI * 16) + i * 16 + rs.R;
                    // (LN_OUT has twice the row pointers: computed ahead of the K loop, as the compiler would, they spill)
                    if constexpr (LN_OUT) asm volatile("" : "+v"(m0r));
                    residual_rows_block<LN_OUT>(rs, acc[i], bj, o, m0r, n0, full);
                    if constexpr (LN_OUT) __builtin_amdgcn_sched_barrier(0);   // keep the next row block's loads behind this one's: 64 more live VGPRs spill
                }
            };
            if (c.m0 + S::BM <= p.M) emit(std::true_type{});
            else emit(std::false_type{});
        } else {
        // (do NOT hoist the bias loads above the row loop: the compiler then speculates them into the K loop and
        //  guards the fragment reads with s_waitcnt vmcnt(0), which also waits for the LDS-DMA of the next stage --
        //  15 % slower on every shape; tools/isa_lint.py checks the main loops for that pattern)
#pragma unroll
        for (int i = 0; i < S::MI; ++i) {
            const int m = c.m(i);
            if (m >= p.M) continue;
            const float* gb = p.group_bias ? p.group_bias + (size_t)(m / p.group_rows) * p.N : nullptr;
            const float* res = p.residual ? p.residual + (size_t)m * p.ldr : nullptr;
            float* o32 = out32 ? out32 + (size_t)m * p.ldo32 : nullptr;
            bf16_t* o16 = p.out_bf16 ? p.out_bf16 + (size_t)m * p.ldo16 : nullptr;
            const float rsc = p.row_scale ? p.row_scale[m] : 1.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = c.n(ntile, j);
                if (n >= p.N) continue;
                f32x4 v = acc[i][j];
                if constexpr (EXTRAS) {
                    if (p.dact_of) {
                        const bf16x4 z = *reinterpret_cast<const bf16x4*>(p.dact_of + (size_t)m * p.N + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] *= gelu_grad_f(bf2f(z[r]));
                    }
                }
                if (p.row_scale) {   // one fused multiply-add per element, as the persistent kernel's epilogue: identical bits
                    const f32x4 b = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f};
                    v = __builtin_elementwise_fma(v, f32x4{rsc, rsc, rsc, rsc}, b);
                } else if (p.bias) { const float4 b = *reinterpret_cast<const float4*>(p.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
                if (gb) { const float4 b = *reinterpret_cast<const float4*>(gb + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
                if constexpr (EXTRAS) {
                    if (p.out_pre_bf16) {
                        bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                        *reinterpret_cast<bf16x4*>(p.out_pre_bf16 + (size_t)m * p.N + n) = o;
                    }
                }
                if constexpr (ACT == CMDIAD_ACT_GELU) {
v = gelu_erf4(v);
                } else if constexpr (ACT == CMDIAD_ACT_RELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaxf(v[r], 0.0f);
                }
                if (res) { const float4 b = *reinterpret_cast<const float4*>(res + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
                if (o32) *reinterpret_cast<f32x4*>(o32 + n) = v;
                if (o16) {
                    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                    *reinterpret_cast<bf16x4*>(o16 + n) = o;
                }
            }
        }
        }
    }, kt_begin);
}

// Persistent form for the wide transformer products (fc1-like: whole 256-column tiles, bias, bf16 output): one block per CU
// walks a contiguous range of the (M tile, N tile) list, N tile fastest, on the two-group pipeline (run_two_group in gemm_pp3.h,
// where the schedule, its staging and its counted waits are derived; the distance GEMM of l2min.hip runs the same schedule).  The
// 128 x 128 shape moves 32 KiB through the L1 -> LDS path per 512 MFMA cycles, which IS that path's 64 B/clk: two co-resident
// blocks can never exceed half the MFMA rate; 256 x 256 halves the bytes per FLOP, the job walk removes the per-tile
// fill / drain and the partial last round (a lock-step 256 x 256 persistent kernel without the two-group schedule gained
// 12 % on fc1 and nothing on qkv, profiles/r2_notes.md; this one gains 18-40 %).
// Three W buffers + three A half slots, per-stream issuer waves, counted waits that are never drained: 7 phases of W lead.
//   out_bf16 = act(acc + bias)      (qkv-like products, fc1 + GELU; the N = 768 residual products stay on 128 x 128:
//                                    3 x 99 tiles on 256 CUs are two rounds for a 256 x 256 tile)
// Epilogue.  In the MFMA accumulator layout a lane holds 4 columns of ONE row, so a store instruction touches 16 rows x 32
// bytes: 64 separate line accesses for the texture-addresser, ~2 000 cycles of store issue per wave and tile -- measured:
// the stores, not the arithmetic (GELU included), cost 30 % of fc1 (profiles/r2_notes.md).  Every wave therefore
// transposes its 16-row blocks through a private 2 KiB LDS scratch (XOR-swizzled 16-byte units: conflict-free both ways)
// and stores 8 rows x 128 contiguous bytes per instruction.  The scratch is read back by inline asm: a compiler-visible
// LDS read after LDS-DMA gets an s_waitcnt vmcnt(0), i.e. a drain of the whole prefetch queue per tile.  The bias arrives
// by inline-asm loads issued in phase 0 of the tile's last K-tile (gemm_pp3.h `pre`), with a counted wait.
constexpr int kPp3Scratch = kRowStoreScratch;   // per wave
#ifndef CMDIAD_PP3_ABL
#define CMDIAD_PP3_ABL 0   // timing-only ablations of the epilogue: tools/pp3_grid.py builds them with -DCMDIAD_PP3_ABL=n
#endif

// RSCALE: out = act(row_scale[m] * acc + bias), the consumer side of the LayerNorm fold; row_scale must be readable up to the
// row count rounded up to 256 (the ragged last tile reads, and never uses, the rows past M).
template <int ACT, bool RSCALE = false>
__global__ __launch_bounds__(512, 1) void gemm_std_pp3_kernel(GlobalTile A, GlobalTile W, StdParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    live_m(p, A);
    const int NT = p.N / SPP3::BN, MT = (p.M + SPP3::BM - 1) / SPP3::BM;
    const int jobs = MT * NT;
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int j0 = (int)((long)jobs * vb / gridDim.x), j1 = (int)((long)jobs * (vb + 1) / gridDim.x);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 2, wc = wave & 3;
    RowStore16 rs;
    rs.init(lds + SPP3::LDS_BYTES + wave * kPp3Scratch, lane);
    const int g = rs.g, R = rs.R, u = rs.u;
    // vector-memory operations of a FULL-tile epilogue per wave (the four bias loads come earlier and are not counted)
    constexpr int kEpiOps = 16;
    f32x4 bias[4];
    float rsc[8];   // RSCALE: 1 / sigma of the lane's row in each of its eight 16-row blocks
    run_pp3_jobs<false, kEpiOps>(A, W, j0, j1, NT, p.K / BK, lds, [&](int mt, int ntile) {
        const float* bp = p.bias + ntile * SPP3::BN + wc * 64 + g * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bias[j]) : "v"(bp + j * 16) : "memory");
        if constexpr (RSCALE) {   // one VGPR offset + immediates: rows mt * 256 + wr * 128 + 16 i + (lane & 15)
            const unsigned off = (unsigned)(mt * SPP3::BM + wr * 128 + (lane & 15)) * 4u;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(rsc[i]) : "v"(off), "s"(p.row_scale), "n"(i * 64) : "memory");
        }
    }, [&](auto& acc, int mt, int ntile) -> int {
        const int nw = ntile * SPP3::BN + wc * 64;                  // first column of this wave's 64
        const int mw = mt * SPP3::BM + wr * 128;                    // first row of this wave's 128
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");            // the bias fetched in phase 0
#if CMDIAD_PP3_ABL == 3      // timing only: no epilogue (accumulators kept live)
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][1]), "v"(acc[i][j][2]), "v"(acc[i][j][3]));
        return 0;
#endif
        __builtin_amdgcn_sched_barrier(0);
        // FULL tiles (all but the last M tile) store without a per-row test: a branch per row makes every group of stores
        // its own basic block, and the compiler then guards each with s_waitcnt vmcnt(0) -- stores count in vmcnt on gfx9,
        // so every group would wait for the previous group's stores to complete
        auto emit = [&](auto FULL) {
            constexpr bool full = decltype(FULL)::value;
            bf16_t* o0 = p.out_bf16 + (size_t)(mw + R) * p.ldo16 + nw + u * 8;
            // act(acc + bias) of 16-row block i as bf16, in the MFMA layout
            auto compute = [&](int i, bf16x4 (&h)[4]) {
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = act_bf16<ACT, RSCALE>(acc[i][j], RSCALE ? rsc[i] : 1.0f, bias[j]);
            };
            // software pipeline over the eight blocks: the arithmetic of block i + 1 (the GELU is ~20 VALU operations per
            // element) runs while block i makes its round trip through the scratch
            bf16x4 h[4];
            compute(0, h);
            rs.park(h);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                uint4 t0, t1;
                rs.fetch_issue(t0, t1);
                if (i < 7) compute(i + 1, h);
                rs.fetch_wait();
                const int m = mw + i * 16 + R;
#if CMDIAD_PP3_ABL == 1      // timing only: no stores (the transposed rows stay live through an empty asm)
                asm volatile("" ::"v"(t0.x), "v"(t0.y), "v"(t0.z), "v"(t0.w), "v"(t1.x), "v"(t1.y), "v"(t1.z), "v"(t1.w));
#elif CMDIAD_PP3_ABL == 2    // timing only: every tile of a block stores to the same L2-resident window
                bf16_t* w0 = p.out_bf16 + (size_t)((blockIdx.x & 63) * 256 + wr * 128 + R) * p.ldo16 + (blockIdx.x >> 6) * 256 + wc * 64 + u * 8;
                *reinterpret_cast<uint4*>(w0 + (size_t)(i * 16) * p.ldo16) = t0;
                *reinterpret_cast<uint4*>(w0 + (size_t)(i * 16 + 8) * p.ldo16) = t1;
#else
                if (full || m < p.M) *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16) * p.ldo16) = t0;
                if (full || m + 8 < p.M) *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16 + 8) * p.ldo16) = t1;
#endif
                if (i < 7) rs.park(h);
            }
        };
        if (mt * SPP3::BM + SPP3::BM <= p.M) {
            emit(std::true_type{});
            return CMDIAD_PP3_ABL == 1 ? 0 : kEpiOps;
        }
        emit(std::false_type{});
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// QKV projection, head-split stores (head_dim 64).  Q and K tiles run swapped (4 consecutive d per
// lane -> 8-byte stores into [B,H,Tp,64]); V tiles run un-swapped (4 consecutive tokens per lane)
// and are stored transposed into [B,H,64,Tp] so the attention kernel reads keys contiguously.
// ------------------------------------------------------------------------------------------------
struct QkvParams {
    int M, T, Tp, C, H, group_m;
    const float* bias;
    bf16_t *q, *k, *vt;
    const float* row_scale;   // LayerNorm fold (see gemm_std_kernel): qkv = row_scale[m] * (A . W^T) + bias, or null
    int v_rows;               // V tiles leave through the wave's LDS scratch as 128-byte token rows (see the kernel)
};

template <class S, bool RSCALE = false>
__global__ __launch_bounds__(S::THREADS, S::WAVES_PER_SIMD) void gemm_qkv_kernel(GlobalTile A, GlobalTile W, QkvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const Coord<S> c((3 * p.C) / S::BN, 1, p.group_m, (p.M + S::BM - 1) / S::BM);
    const int which = (c.nt * S::BN) / p.C;  // 0 q, 1 k, 2 v : block-uniform because C % BN == 0

    if (which < 2) {
        bf16_t* dst = which == 0 ? p.q : p.k;
        // q carries head_dim^-0.5 (models.py:153) AND log2(e), so the attention kernel's softmax is a bare exp2
        const float scale = which == 0 ? 0.125f * 1.4426950408889634f : 1.0f;
        // a wave's 64 columns are ONE head: its 16-token blocks leave as 8 tokens x 128 contiguous bytes per store (RowStore16)
        RowStore16 rs;
        rs.init(lds + S::LDS_BYTES + (threadIdx.x >> 6) * kRowStoreScratch, c.lane);
        run<S, true>(A, W, c.m0, c.nt, 1, p.C / BK, lds, [&](auto& acc, int ntile, char*) {
            const int n0 = ntile * S::BN + c.wc * 64;              // first column of the wave: a head boundary
            const int hh = (n0 - which * p.C) >> 6;
            f32x4 bj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bj[j] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + n0 + j * 16 + (c.lane >> 4) * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < S::MI; ++i) {
                bf16x4 h[4];
                float rsc = 1.0f;
                if constexpr (RSCALE) {
                    int mi = min(c.m(i), p.M - 1);
                    asm volatile("" : "+v"(mi));   // address arithmetic stays in the epilogue (hoisted above the K loop it spills)
                    rsc = p.row_scale[mi];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = (RSCALE ? __builtin_elementwise_fma(acc[i][j], f32x4{rsc, rsc, rsc, rsc}, bj[j]) : acc[i][j] + bj[j]) * scale;
                    h[j] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                }
                rs.park(h);
                uint4 t0, t1;
                rs.fetch_issue(t0, t1);
                rs.fetch_wait();
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int m = c.m0 + c.wr * (S::MI * 16) + i * 16 + rs.R + 8 * half;
                    if (m >= p.M) continue;
                    const int b = m / p.T, t = m - b * p.T;
                    *reinterpret_cast<uint4*>(dst + (((size_t)b * p.H + hh) * p.Tp + t) * 64 + rs.u * 8) = half ? t1 : t0;
                }
            }
        });
    } else {
        // V^T [B, H, 64, Tp]: in this orientation a lane holds FOUR CONSECUTIVE TOKENS of one channel -- 8 contiguous bytes of a V^T
        // row -- so a 16-token x 16-channel block leaves as one 8-byte store per lane (16 rows x 32 bytes per instruction; the
        // token offset inside an image is arbitrary, so the stores are 2-byte aligned: fine on this device, tools/
        // unaligned_store_test.hip).  The scalar form (64 two-byte stores and 64 divisions by T per lane and tile) stays for the
        // four-token groups that straddle two images or the end of the matrix.
        // A wave's 64 tokens x 64 channels (one head) lie in ONE image almost always (the tile straddles two images, or the end of the
        // matrix, in 64 of every T rows): then each 16-channel block goes through the wave's LDS scratch -- the lane's four-token pieces
        // of the four row blocks are the 8-byte slots 4 i + g of channel row (lane & 15), exactly RowStore16's layout with the row
        // block in place of the column block -- and leaves as 8 channel rows x 128 contiguous bytes (64 tokens) per store instead
        // of 16 rows x 32 bytes: a quarter of the line accesses (CMDIAD_QKV_VROWS=0: the direct form, A/B).
        run<S, false>(A, W, c.m0, c.nt, 1, p.C / BK, lds, [&](auto& acc, int ntile, char*) {
            static_assert(S::MI == 4, "RowStore16 takes four 8-byte pieces per lane");
            int m0w = c.m0 + c.wr * (S::MI * 16);
            int ln = c.lane;
            asm volatile("" : "+v"(m0w), "+v"(ln));   // everything below is computed HERE: hoisted above the K loop it spills
            const int b0 = m0w / p.T, t0w = m0w - b0 * p.T;
            if (!RSCALE && p.v_rows && m0w + 63 < p.M && t0w + 63 < p.T) {   // (the folded-LayerNorm variant has no registers to spare: direct form)
                RowStore16 rsv;
                rsv.init(lds + S::LDS_BYTES + (threadIdx.x >> 6) * kRowStoreScratch, ln);
                const int hd = (ntile * S::BN + c.wc * 64 - 2 * p.C) >> 6;
                bf16_t* base = p.vt + ((size_t)b0 * p.H + hd) * 64 * p.Tp + t0w + rsv.u * 8;
                f32x4 rs4[S::MI];
                if constexpr (RSCALE) {
#pragma unroll
                    for (int i = 0; i < S::MI; ++i) {
                        rs4[i] = *reinterpret_cast<const f32x4*>(p.row_scale + m0w + i * 16 + (ln >> 4) * 4);      // (rows < M here; row_scale is 16-byte aligned)
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float bb = p.bias ? p.bias[ntile * S::BN + c.wc * 64 + j * 16 + (ln & 15)] : 0.0f;
                    bf16x4 h[4];
#pragma unroll
                    for (int i = 0; i < S::MI; ++i) {
                        const f32x4 v = RSCALE ? __builtin_elementwise_fma(acc[i][j], rs4[i], f32x4{bb, bb, bb, bb}) : acc[i][j] + bb;
                        h[i] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                    }
                    rsv.park(h);
                    uint4 t0, t1;
                    rsv.fetch_issue(t0, t1);
                    rsv.fetch_wait();
                    __builtin_memcpy(base + (size_t)(j * 16 + rsv.R) * p.Tp, &t0, 16);       // 2-byte aligned (the token offset is arbitrary)
                    __builtin_memcpy(base + (size_t)(j * 16 + rsv.R + 8) * p.Tp, &t1, 16);
                }
                return;
            }
            int tb[S::MI], tt[S::MI];   // image and token of the lane's first token in row block i
            f32x4 rsc[S::MI];           // 1 / sigma of the lane's four tokens
#pragma unroll
            for (int i = 0; i < S::MI; ++i) {
                const int m = m0w + i * 16 + (ln >> 4) * 4;
                tb[i] = m / p.T;
                tt[i] = m - tb[i] * p.T;
                rsc[i] = f32x4{1.f, 1.f, 1.f, 1.f};
                if constexpr (RSCALE) {
                    int mm = m;
                    asm volatile("" : "+v"(mm));
#pragma unroll
                    for (int r = 0; r < 4; ++r) rsc[i][r] = p.row_scale[min(mm + r, p.M - 1)];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = ntile * S::BN + c.wc * 64 + j * 16 + (ln & 15);
                const int cc = n - 2 * p.C;
                const int h = cc >> 6, d = cc & 63;
                const float bb = p.bias ? p.bias[n] : 0.0f;
#pragma unroll
                for (int i = 0; i < S::MI; ++i) {
                    const int m = m0w + i * 16 + (ln >> 4) * 4;
                    if (m + 3 < p.M && tt[i] + 3 < p.T) {
                        const f32x4 v = RSCALE ? __builtin_elementwise_fma(acc[i][j], rsc[i], f32x4{bb, bb, bb, bb}) : acc[i][j] + bb;
                        const bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                        __builtin_memcpy(p.vt + (((size_t)tb[i] * p.H + h) * 64 + d) * p.Tp + tt[i], &o, 8);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            if (m + r >= p.M) continue;
                            const int b = (m + r) / p.T, t = m + r - b * p.T;
                            p.vt[(((size_t)b * p.H + h) * 64 + d) * p.Tp + t] = f2bf(RSCALE ? __builtin_fmaf(acc[i][j][r], rsc[i][r], bb) : acc[i][j][r] + bb);
                        }
                    }
                }
            }
        });
    }
}

// ------------------------------------------------------------------------------------------------
// Per-group max pooling epilogue shared by the two encoder stages.  The BM-row tile holds BM/Mg whole
// groups.  Column max: in-lane over pairs of row tiles (32 rows), xor-shuffle over the 16 row lanes,
// then a [BM/32][BN] LDS table (one row per 32-row block) combined by the first BN threads.
// ------------------------------------------------------------------------------------------------
struct GroupMaxParams {
    int M, N, K, Mg, panel;
    const float* bias;
    bf16_t* full_bf16; int ldf;  // optional full activations [M,N]
    float* max_f32;
    bf16_t* max_bf16;
};

// epilogue of one finished BM x BN tile: + bias, optional full store, per-group column maxima (see above)
template <class S, class Acc>
__device__ __forceinline__ void groupmax_epilogue(Acc& acc, int ntile, const Coord<S>& c, const GroupMaxParams& p,
                                                  float (*s_max)[S::BN], int tid, const f32x4* pre_bias = nullptr,
                                                  const RowStore16* rs = nullptr)
{
        if (rs && p.full_bf16) {   // full activations, row-contiguous (8 rows x 128 bytes per store): see RowStore16
            f32x4 bj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = ntile * S::BN + c.wc * 64 + j * 16 + (c.lane >> 4) * 4;
                bj[j] = pre_bias ? pre_bias[j] : (p.bias && n < p.N ? *reinterpret_cast<const f32x4*>(p.bias + n) : f32x4{0.f, 0.f, 0.f, 0.f});
            }
            const int mrow = c.m0 + c.wr * (S::MI * 16) + rs->R;
            bf16_t* o0 = p.full_bf16 + (size_t)mrow * p.ldf + ntile * S::BN + c.wc * 64 + rs->u * 8;
#pragma unroll
            for (int i = 0; i < S::MI; ++i) {
                bf16x4 h[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 v = acc[i][j] + bj[j];
                    h[j] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                }
                rs->park(h);
                uint4 t0, t1;
                rs->fetch_issue(t0, t1);
                rs->fetch_wait();
                const int m = mrow + i * 16;
                if (m < p.M) *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16) * p.ldf) = t0;
                if (m + 8 < p.M) *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16 + 8) * p.ldf) = t1;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nl = c.wc * 64 + j * 16 + (c.lane >> 4) * 4;  // column within the tile
            const int n = ntile * S::BN + nl;
            float4 b = {0.f, 0.f, 0.f, 0.f};
            if (pre_bias) b = float4{pre_bias[j][0], pre_bias[j][1], pre_bias[j][2], pre_bias[j][3]};  // fetched by the caller
            else if (p.bias && n < p.N) b = *reinterpret_cast<const float4*>(p.bias + n);
            f32x4 mx[S::MI / 2];
#pragma unroll
            for (int i = 0; i < S::MI; ++i) {
                f32x4 v = acc[i][j];
                v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
                const int m = c.m(i);
                if (!rs && p.full_bf16 && m < p.M && n < p.N) {
                    bf16x4 o = {f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                    *reinterpret_cast<bf16x4*>(p.full_bf16 + (size_t)m * p.ldf + n) = o;
                }
                if ((i & 1) == 0) mx[i >> 1] = v;
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx[i >> 1][r] = fmaxf(mx[i >> 1][r], v[r]);
                }
            }
#pragma unroll
            for (int hb = 0; hb < S::MI / 2; ++hb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = mx[hb][r];
                    v = row16_max(v);
                    if ((c.lane & 15) == 0) s_max[c.wr * (S::MI / 2) + hb][nl + r] = v;
                }
            }
        }
        __syncthreads();
        if (tid < S::BN) {
            const int n = ntile * S::BN + tid;
            const int per = p.Mg / 32;  // 32-row blocks per group: 1, 2 or 4
            for (int g = 0; g < (S::BM / 32) / per; ++g) {
                float v = s_max[g * per][tid];
                for (int q = 1; q < per; ++q) v = fmaxf(v, s_max[g * per + q][tid]);
                const int grp = (c.m0 + g * p.Mg) / p.Mg;
                if (n < p.N && c.m0 + g * p.Mg < p.M) {
                    if (p.max_f32) p.max_f32[(size_t)grp * p.N + n] = v;
                    if (p.max_bf16) p.max_bf16[(size_t)grp * p.N + n] = f2bf(v);
                }
            }
        }
}

template <class S, class ALoader>
__device__ __forceinline__ void groupmax_body(const ALoader& A, const GlobalTile& W, const GroupMaxParams& p, char* lds)
{
    float(*s_max)[S::BN] = reinterpret_cast<float(*)[S::BN]>(lds + S::LDS_BYTES);
    const Coord<S> c((p.N + S::BN - 1) / S::BN, p.panel);
    const int tid = threadIdx.x;

    run<S, true>(A, W, c.m0, c.nt, c.count, p.K / BK, lds, [&](auto& acc, int ntile, char*) { groupmax_epilogue<S>(acc, ntile, c, p, s_max, tid); });
}

template <class S>
__global__ __launch_bounds__(S::THREADS, S::WAVES_PER_SIMD) void gemm_groupmax_kernel(GlobalTile A, GlobalTile W, GroupMaxParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    groupmax_body<S>(A, W, p, lds);
}

#ifdef CMDIAD_AB_VARIANTS  // generic-pipeline form of the encoder's first stage (conv1 re-staged per step): A/B reference
template <class S>
__global__ __launch_bounds__(S::THREADS, S::WAVES_PER_SIMD) void encoder_stage1_kernel(Conv1Tile A, GlobalTile W, GroupMaxParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    groupmax_body<S>(A, W, p, lds);
}
#endif

// ------------------------------------------------------------------------------------------------
// Encoder first stage, dedicated form: a block's 128 x 128 conv1 activations are computed ONCE into LDS (both K tiles)
// and the four 128 x 64 weight tiles of conv2 stream past them -- the generic pipeline above re-stages (re-computes) the A
// tile for every (N tile, K tile) step, i.e. conv1 runs twice per block with a dependent round trip for its weights and
// coordinates in front of every step.  Same arithmetic in the same order (conv1 formula, K order, epilogue): identical
// h2 / group maxima.  LDS: A 32 KiB + 2 weight stages 32 KiB + max table 2 KiB.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void encoder_stage1_once_kernel(Conv1Tile A, GlobalTile W, GroupMaxParams p)
{
    using S = S128;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int KT_BYTES = S::BM * BK * 2;  // one [128][64] bf16 tile: 16 KiB
    char* a_lds = lds;                        // [2 K tiles]
    char* w_lds = lds + 2 * KT_BYTES;         // [2 stages]
    float(*s_max)[S::BN] = reinterpret_cast<float(*)[S::BN]>(lds + 4 * KT_BYTES);
    const Coord<S> c(1);                      // block = one M tile; both N tiles are walked here
    const int tid = threadIdx.x;
    RowStore16 rs;                            // h2 (2.2 GB per batch of 32) leaves as 128-byte row pieces
    rs.init(lds + 4 * KT_BYTES + (S::BM / 32) * S::BN * (int)sizeof(float) + (tid >> 6) * kRowStoreScratch, tid & 63);

    // conv2's bias for both N tiles, by inline asm before anything else: loaded by the compiler where the epilogue uses it, it
    // is hoisted above the MFMA steps and guarded with s_waitcnt vmcnt(0) in front of their fragment reads (tools/isa_lint.py)
    f32x4 bias[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(bias[nt][j]) : "v"(p.bias + nt * S::BN + c.wc * 64 + j * 16 + (c.lane >> 4) * 4) : "memory");
    W.stage<S::BN, S::WAVES>(w_lds, 0, 0, tid);  // step 0's weights fly while conv1 runs on the VALU
    A.stage<S::BM, S::WAVES>(a_lds, c.m0, 0, tid);
    A.stage<S::BM, S::WAVES>(a_lds + KT_BYTES, c.m0, BK, tid);
    wait_vmcnt<0>();
    block_barrier();

    f32x4 acc[S::MI][4];
#pragma unroll
    for (int i = 0; i < S::MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int step = 0; step < 4; ++step) {  // (N tile, K tile) = (0,0) (0,1) (1,0) (1,1)
        const int nt = step >> 1, kt = step & 1;
        if (step < 3) W.stage<S::BN, S::WAVES>(w_lds + ((step + 1) & 1) * KT_BYTES, ((step + 1) >> 1) * S::BN, ((step + 1) & 1) * BK, tid);
        compute_stage<S, true, false>(acc, a_lds + kt * KT_BYTES, w_lds + (step & 1) * KT_BYTES, c.wr, c.wc, c.lane);
        if (kt == 1) {
            groupmax_epilogue<S>(acc, nt, c, p, s_max, tid, bias[nt], &rs);
#pragma unroll
            for (int i = 0; i < S::MI; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        wait_vmcnt<0>();
        block_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// Encoder first stage, PERSISTENT form (M % 128 == 0): the once-per-block kernel above lives ~21 us per 128-row block for 1 us
// of MFMA (coordinates -> conv1 -> four weight tiles, each behind a full wait, 32 768 blocks per batch of 32).  Here a block
// of 8 waves (2 x 4 grid of 64 x 64 wave tiles = 128 rows x all 256 conv2 channels) stays on its CU and walks tiles
// blockIdx, + gridDim, ...: conv2's weights never touch LDS -- every wave keeps its 64 x 128 slice as MFMA fragments in 64
// VGPRs for the whole launch -- the conv1 activations of tile t+1 are computed into the other half of a double buffer
// while nothing waits on memory, and the coordinates of tile t+2 are fetched a full iteration ahead (an inline-asm load
// older than the iteration's eight stores per wave: s_waitcnt vmcnt(8) never waits for a store).  What is left per tile is
// its 64 KiB of h2 stores: the kernel is bound by the HBM write stream (2.15 GB per batch of 32).
// Same arithmetic in the same order as the kernels above (conv1 expression, K order, + bias, bf16, maxima): identical bits.
// LDS: conv1 tiles 2 x 32 KiB | coordinates 2 x 1.5 KiB | max tables 2 x 4 KiB | 8 store scratches of 2 KiB | conv1 weights 2 KiB.
// ------------------------------------------------------------------------------------------------
struct Stage1Persist {
    static constexpr int KT_BYTES = 128 * BK * 2;
    static constexpr int C_OFF = 4 * KT_BYTES, MAX_OFF = C_OFF + 2 * 384 * 4, SCR_OFF = MAX_OFF + 2 * 4 * 256 * 4;
    static constexpr int W1_OFF = SCR_OFF + 8 * kRowStoreScratch, LDS_BYTES = W1_OFF + 128 * 16;
};

template <bool G64>   // G64: Mg is 64 or 128 -- a wave's 64 rows are one group, their maximum is taken in-lane first
__global__ __launch_bounds__(512, 1) void encoder_stage1_persist_kernel(const float* __restrict__ neigh, const float4* __restrict__ wb,
                                                                        const bf16_t* __restrict__ W2, GroupMaxParams p, int n_tiles)
{
    using L = Stage1Persist;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    float* cbuf = reinterpret_cast<float*>(lds + L::C_OFF);
    float(*s_max)[4][256] = reinterpret_cast<float(*)[4][256]>(lds + L::MAX_OFF);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    RowStore16 rs;
    rs.init(lds + L::SCR_OFF + wave * kRowStoreScratch, lane);

    // conv2 weights of this wave's 64 channels as MFMA fragments (row = channel, 8 consecutive k per lane), resident
    bf16x8 wf[4][4];
#pragma unroll
    for (int kc = 0; kc < 4; ++kc)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            wf[kc][j] = *reinterpret_cast<const bf16x8*>(W2 + (size_t)(wc * 64 + j * 16 + (lane & 15)) * 128 + kc * 32 + (lane >> 4) * 8);
    f32x4 bias[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bias[j] = *reinterpret_cast<const f32x4*>(p.bias + wc * 64 + j * 16 + (lane >> 4) * 4);
    // conv1: a thread owns 8 channels (16-byte chunk c16 of the 128) of rows (tid >> 4) + 32 i; the folded weights sit in LDS
    const int c16 = tid & 15;
    float4* wl = reinterpret_cast<float4*>(lds + L::W1_OFF);
    if (tid < 128) wl[(tid & 7) * 16 + (tid >> 3)] = wb[tid];   // [e][chunk]: the 16 chunks a wave touches at once are 256 contiguous bytes (bank-conflict-free)
    char* const a_dst = lds + (c16 >> 3) * L::KT_BYTES;
    auto conv1 = [&](int par) {
        const float* cb = cbuf + par * 384 + (tid >> 4) * 3;
        float xs[4], ys[4], zs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { xs[i] = cb[i * 96]; ys[i] = cb[i * 96 + 1]; zs[i] = cb[i * 96 + 2]; }
        bf16x8 h[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {   // two rows per v_pk_fma_f32: the same FMA chain as conv1_act, element-wise
            const float4 w = wl[e * 16 + c16];
#pragma unroll
            for (int i = 0; i < 4; i += 2) {
                f32x2 a = __builtin_elementwise_fma(f32x2{w.x, w.x}, f32x2{xs[i], xs[i + 1]}, f32x2{w.w, w.w});
                a = __builtin_elementwise_fma(f32x2{w.y, w.y}, f32x2{ys[i], ys[i + 1]}, a);
                a = __builtin_elementwise_fma(f32x2{w.z, w.z}, f32x2{zs[i], zs[i + 1]}, a);
                h[i][e] = f2bf(fmaxf(a[0], 0.0f));
                h[i + 1][e] = f2bf(fmaxf(a[1], 0.0f));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<bf16x8*>(a_dst + par * 2 * L::KT_BYTES + lds_off((tid >> 4) + 32 * i, c16 & 7)) = h[i];
    };
    const int my = (n_tiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // tiles blockIdx + t gridDim
    const float4* n4 = reinterpret_cast<const float4*>(neigh);                           // a tile = 384 floats = 96 float4
    f32x4 cnext = {0.f, 0.f, 0.f, 0.f};
    if (tid < 96) {
        *reinterpret_cast<float4*>(cbuf + tid * 4) = n4[(size_t)blockIdx.x * 96 + tid];
        if (my > 1) *reinterpret_cast<float4*>(cbuf + 384 + tid * 4) = n4[(size_t)(blockIdx.x + gridDim.x) * 96 + tid];
    }
    __syncthreads();
    conv1(0);
    __syncthreads();

    const int a_frag = (wr * 64 + (lane & 15)) * 128, swz = lane & 7, g4 = lane >> 4;
    for (int t = 0; t < my; ++t) {
        const int par = t & 1;
        const size_t m0 = (size_t)(blockIdx.x + (size_t)t * gridDim.x) * 128;
        const bool fetch = t + 2 < my;   // block-uniform
        if (fetch && tid < 96)
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(cnext) : "v"(n4 + (size_t)(blockIdx.x + (size_t)(t + 2) * gridDim.x) * 96 + tid) : "memory");
        if (t + 1 < my) conv1(par ^ 1);
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const char* at = lds + par * 2 * L::KT_BYTES + a_frag;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            bf16x8 af[2][4];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    af[kk][i] = *reinterpret_cast<const bf16x8*>(at + kt * L::KT_BYTES + i * 2048 + (((kk * 4 + g4) ^ swz) << 4));
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(wf[kt * 2 + kk][j], af[kk][i], acc[i][j]);
        }
        // ---- epilogue: + bias, h2 as 8 rows x 128 contiguous bytes per store, column maxima of the 32-row blocks
        bf16_t* o0 = p.full_bf16 + (m0 + wr * 64 + rs.R) * 256 + wc * 64 + rs.u * 8;
        f32x4 mx[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x4 h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = acc[i][j] + bias[j];
                h[j] = bf16x4{f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
                const int hb = G64 ? 0 : i >> 1;
                if (i == 0 || (!G64 && i == 2)) mx[hb][j] = v;
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) mx[hb][j][r] = fmaxf(mx[hb][j][r], v[r]);
                }
            }
            rs.park(h);
            uint4 t0, t1;
            rs.fetch_issue(t0, t1);
            rs.fetch_wait();
            *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16) * 256) = t0;
            *reinterpret_cast<uint4*>(o0 + (size_t)(i * 16 + 8) * 256) = t1;
        }
        {
            constexpr int NV = (G64 ? 1 : 2) * 16;
            float red[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) red[q] = mx[q >> 4][(q >> 2) & 3][q & 3];
            row16_max_batch(red);
#pragma unroll
            for (int q = 0; q < NV; ++q) mx[q >> 4][(q >> 2) & 3][q & 3] = red[q];
        }
        if ((lane & 15) == 0) {   // table row = 32-row block (both halves of a 64-row wave tile carry the same value under G64)
#pragma unroll
            for (int hb = 0; hb < 2; ++hb)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *reinterpret_cast<f32x4*>(&s_max[par][wr * 2 + hb][wc * 64 + j * 16 + g4 * 4]) = mx[G64 ? 0 : hb][j];
        }
        // coordinates of tile t+2: the load is older than this iteration's eight stores
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        if (fetch && tid < 96) *reinterpret_cast<f32x4*>(cbuf + par * 384 + tid * 4) = cnext;
        __syncthreads();
        if (tid < 256) {
            const int per = p.Mg >> 5;  // 32-row blocks per group: 1, 2 or 4
            for (int g = 0; g < 4 / per; ++g) {
                float v = s_max[par][g * per][tid];
                for (int q = 1; q < per; ++q) v = fmaxf(v, s_max[par][g * per + q][tid]);
                const size_t grp = (m0 + (size_t)g * p.Mg) / p.Mg;
                if (p.max_f32) p.max_f32[grp * 256 + tid] = v;
                if (p.max_bf16) p.max_bf16[grp * 256 + tid] = f2bf(v);
            }
        }
    }
}

template <class S> constexpr int group_max_lds() { return S::LDS_BYTES + (S::BM / 32) * S::BN * (int)sizeof(float); }

#ifdef CMDIAD_AB_VARIANTS
#include "ab/gemm_wide_kernels.inc"
#endif  // CMDIAD_AB_VARIANTS

// part [chunks][M] (sum, M2 about the chunk mean) of 64-column chunks -> rstd[m] = 1 / sqrt(var + eps) (and the row mean).
// The chunks are merged in chunk order by one thread per row (Chan et al.): the result does not depend on launch geometry.
__global__ __launch_bounds__(256) void ln_stats_finalize_kernel(const float2* __restrict__ part, int M, int chunks, float eps,
                                                                float* __restrict__ rstd, float* __restrict__ mean_out)
{
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    rstd[m] = ln_merge_chunks(part, M, chunks, m, eps, mean_out ? mean_out + m : nullptr);
}

// Every network GEMM runs the 128 x 128 shape unless its plan says otherwise (gemm_plan.h plan_gemm, where the rules and their
// measurements live); the larger shapes serve the distance GEMM (l2min.hip).
constexpr int kLdsStd = S128::LDS_BYTES + S128::WAVES * kRowStoreScratch;

// the run-time activation (none, GELU, ReLU) as a compile-time constant: f(std::integral_constant<int, CMDIAD_ACT_*>)
template <class F>
int with_act(int act, F f)
{
    return act == CMDIAD_ACT_GELU   ? f(std::integral_constant<int, CMDIAD_ACT_GELU>{})
           : act == CMDIAD_ACT_RELU ? f(std::integral_constant<int, CMDIAD_ACT_RELU>{})
                                    : f(std::integral_constant<int, CMDIAD_ACT_NONE>{});
}

#ifdef CMDIAD_AB_VARIANTS
template <int NJ, auto Kernel, class P>
int launch_wide(const char* who, plan::tile_grid g, P& p, const GlobalTile& A, const GlobalTile& W, hipStream_t s)
{
    p.panel = g.panel;
    return launch_lds<Kernel>(who, dim3(g.x), dim3(256), WideShape<NJ>::LDS_BYTES, s, A, W, p);
}
#endif  // CMDIAD_AB_VARIANTS

}  // namespace

int gemm_residual_tiles_launch(const cmdiad_gemm_args* a, unsigned tiles, hipStream_t stream);   // gemm_sk.hip

// plan (gemm_plan.h: every argument check, the kernel, its grid), zero what the plan says no block will write, launch
extern "C" int cmdiad_gemm_bf16(const cmdiad_gemm_args* a, cmdiad_stream_t stream)
{
    using K = plan::gemm_kernel;
    constexpr const char* who = "cmdiad_gemm_bf16";
    CMDIAD_REQUIRE(a, CMDIAD_ERR_ARG, "cmdiad_gemm_bf16: null operand");
    const plan::gemm_plan pl = plan::plan_gemm(*a, env_switches(), kAbBuild);
    CMDIAD_REQUIRE(!pl.err, pl.err, "%s", pl.text);
    hipStream_t s = (hipStream_t)stream;
    const int split = plan::split_of(*a);
    if (pl.first_empty_slab >= 0 &&
        hipMemset2DAsync(a->out_f32 + (size_t)pl.first_empty_slab * a->M * a->ldo32, (size_t)a->ldo32 * sizeof(float), 0,
                         (size_t)a->N * sizeof(float), (size_t)(split - pl.first_empty_slab) * a->M, s) != hipSuccess) {
        cmdiad_set_error("cmdiad_gemm_bf16: hipMemset2DAsync of the empty split-K slabs failed");
        return CMDIAD_ERR_LAUNCH;
    }
    if (pl.kernel == K::res_tiles) return gemm_residual_tiles_launch(a, pl.grid_x, s);
    GlobalTile A{(const bf16_t*)a->A, a->lda, a->M}, W{(const bf16_t*)a->W, a->ldw, a->N};
    StdParams p{a->M, a->N, a->K, a->bias, a->group_bias, a->group_rows, a->act, a->residual, a->ldr,
                a->out_f32, a->ldo32, (bf16_t*)a->out_bf16, a->ldo16, (bf16_t*)a->out_pre_bf16, (const bf16_t*)a->dact_of, split, pl.panel, pl.group_m, a->m_count,
                a->row_scale, (bf16_t*)a->ln_xb, a->ld_xb, a->ln_part, a->add2, a->ld_add2};
    const dim3 grid(pl.grid_x, pl.grid_y), block(S128::THREADS);
    constexpr int kLds3 = SPP3::LDS_BYTES + 8 * kPp3Scratch;
    int rc = CMDIAD_OK;
    switch (pl.kernel) {
    case K::general:
        rc = with_act(pl.act, [&](auto act) { return launch_lds<gemm_std_kernel<S128, decltype(act)::value, false>>(who, grid, block, kLdsStd, s, A, W, p); });
        break;
    case K::general_train:
        rc = with_act(pl.act, [&](auto act) { return launch_lds<gemm_std_kernel<S128, decltype(act)::value, true>>(who, grid, block, kLdsStd, s, A, W, p); });
        break;
    case K::res_rows: rc = launch_lds<gemm_std_kernel<S128, CMDIAD_ACT_NONE, false, true>>(who, grid, block, kLdsStd, s, A, W, p); break;
    case K::res_rows_ln: rc = launch_lds<gemm_std_kernel<S128, CMDIAD_ACT_NONE, false, true, true>>(who, grid, block, kLdsStd, s, A, W, p); break;
    case K::pp3:
        rc = with_act(pl.act, [&](auto act) { return launch_lds<gemm_std_pp3_kernel<decltype(act)::value>>(who, grid, dim3(512), kLds3, s, A, W, p); });
        break;
    case K::pp3_rscale:
        rc = with_act(pl.act, [&](auto act) { return launch_lds<gemm_std_pp3_kernel<decltype(act)::value, true>>(who, grid, dim3(512), kLds3, s, A, W, p); });
        break;
#ifdef CMDIAD_AB_VARIANTS
    case K::wide4:
        rc = with_act(pl.act, [&](auto act) { return launch_wide<4, gemm_std_wide_kernel<4, decltype(act)::value>>(who, {pl.grid_x, pl.panel}, p, A, W, s); });
        break;
    case K::wide8:
        rc = with_act(pl.act, [&](auto act) { return launch_wide<8, gemm_std_wide_kernel<8, decltype(act)::value>>(who, {pl.grid_x, pl.panel}, p, A, W, s); });
        break;
#else
    case K::wide4: case K::wide8:   // planned in the test-only build alone
        cmdiad_set_error("cmdiad_gemm_bf16: the plan names a kernel that only the test build (make ab) contains");
        return CMDIAD_ERR_ARG;
#endif
    case K::res_tiles: break;       // launched above
    }
    if (rc) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_ln_stats_finalize(const float* part, int M, int chunks, float eps, float* rstd, float* mean_out,
                                        cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(part && rstd && M > 0 && chunks > 0 && ((uintptr_t)part & 7) == 0, CMDIAD_ERR_ARG, "cmdiad_ln_stats_finalize: bad args");
    hipLaunchKernelGGL(ln_stats_finalize_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const float2*)part, M, chunks, eps, rstd, mean_out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_gemm_qkv(const uint16_t* A, const uint16_t* W, const float* bias, const float* row_scale, int B, int T, int C,
                               uint16_t* q_out, uint16_t* k_out, uint16_t* vt_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(A && W && q_out && k_out && vt_out, CMDIAD_ERR_ARG, "cmdiad_gemm_qkv: null pointer");
    CMDIAD_REQUIRE(B > 0 && T > 0 && C > 0 && C % 128 == 0, CMDIAD_ERR_ARG, "cmdiad_gemm_qkv: need C%%128==0 (C=%d)", C);
    CMDIAD_REQUIRE(aligned16(A) && aligned16(W) && aligned16(q_out) && aligned16(k_out) && (!bias || aligned16(bias)),
                   CMDIAD_ERR_ARG, "cmdiad_gemm_qkv: 16-byte alignment");
    const int M = B * T;
    GlobalTile At{(const bf16_t*)A, C, M}, Wt{(const bf16_t*)W, C, 3 * C};
    static const int v_rows = !env_is("CMDIAD_QKV_VROWS", '0');
    QkvParams p{M, T, (T + 63) / 64 * 64, C, C / 64, plan::group_m_tiles(env_switches()), bias, (bf16_t*)q_out, (bf16_t*)k_out, (bf16_t*)vt_out, row_scale, v_rows};
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(plan::grid128(M, 3 * C)), block(S128::THREADS);
    const int rc = row_scale ? launch_lds<gemm_qkv_kernel<S128, true>>("cmdiad_gemm_qkv", grid, block, kLdsStd, s, At, Wt, p)
                             : launch_lds<gemm_qkv_kernel<S128, false>>("cmdiad_gemm_qkv", grid, block, kLdsStd, s, At, Wt, p);
    if (rc) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_gemm_groupmax(const uint16_t* A, const uint16_t* W, const float* bias, int groups, int Mg,
                                    int N, int K, float* out_f32, uint16_t* out_bf16, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(A && W && (out_f32 || out_bf16), CMDIAD_ERR_ARG, "cmdiad_gemm_groupmax: null pointer");
    CMDIAD_REQUIRE(groups > 0 && (Mg == 32 || Mg == 64 || Mg == 128) && N % 4 == 0 && K % 64 == 0, CMDIAD_ERR_ARG,
                   "cmdiad_gemm_groupmax: Mg in {32,64,128}, N%%4==0, K%%64==0 (Mg=%d N=%d K=%d)", Mg, N, K);
    CMDIAD_REQUIRE(aligned16(A) && aligned16(W) && (!bias || aligned16(bias)), CMDIAD_ERR_ARG,
                   "cmdiad_gemm_groupmax: 16-byte alignment");
    const int M = groups * Mg;
    GlobalTile At{(const bf16_t*)A, K, M}, Wt{(const bf16_t*)W, K, N};
    GroupMaxParams p{M, N, K, Mg, 1, bias, nullptr, 0, out_f32, (bf16_t*)out_bf16};
    hipStream_t s = (hipStream_t)stream;
    const plan::switches sw = env_switches();
    const int wide = plan::wide_choice(true, 1, sw, kAbBuild);
    const plan::tile_grid g = plan::groupmax_grid(M, N, K, wide, sw);
    int rc;
#ifdef CMDIAD_AB_VARIANTS
    if (wide == 8) rc = launch_wide<8, gemm_groupmax_wide_kernel<8>>("cmdiad_gemm_groupmax", g, p, At, Wt, s);
    else if (wide == 4) rc = launch_wide<4, gemm_groupmax_wide_kernel<4>>("cmdiad_gemm_groupmax", g, p, At, Wt, s);
    else
#endif
    {
        p.panel = g.panel;
        rc = launch_lds<gemm_groupmax_kernel<S128>>("cmdiad_gemm_groupmax", dim3(g.x), dim3(S128::THREADS), group_max_lds<S128>(), s, At, Wt, p);
    }
    if (rc) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_encoder_stage1(const float* neigh, const float* w1, const uint16_t* W2, const float* b2,
                                     int groups, int Mg, uint16_t* h2_out, float* gmax_out,
                                     uint16_t* gmax_bf16_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(neigh && w1 && W2 && h2_out && gmax_out, CMDIAD_ERR_ARG, "cmdiad_encoder_stage1: null pointer");
    CMDIAD_REQUIRE(groups > 0 && (Mg == 32 || Mg == 64 || Mg == 128), CMDIAD_ERR_ARG,
                   "cmdiad_encoder_stage1: Mg in {32,64,128} (Mg=%d)", Mg);
    CMDIAD_REQUIRE(aligned16(w1) && aligned16(W2) && (!b2 || aligned16(b2)) && ((uintptr_t)h2_out & 7) == 0,
                   CMDIAD_ERR_ARG, "cmdiad_encoder_stage1: alignment");
    const int M = groups * Mg;
    Conv1Tile At{neigh, (const float4*)w1, M};
    GlobalTile Wt{(const bf16_t*)W2, 128, 256};
    GroupMaxParams p{M, 256, 128, Mg, 1, b2, (bf16_t*)h2_out, 256, gmax_out, (bf16_t*)gmax_bf16_out};
    hipStream_t s = (hipStream_t)stream;
    CMDIAD_REQUIRE(b2, CMDIAD_ERR_ARG, "cmdiad_encoder_stage1: the second convolution's bias is required");
    const plan::stage1_plan pl = plan::plan_stage1(M, Mg, env_switches(), kAbBuild);
    const dim3 grid(pl.grid_x);
    p.panel = pl.panel;
    int rc = CMDIAD_OK;
    switch (pl.kernel) {
    case plan::stage1_kernel::persist:
        if (pl.g64) rc = launch_lds<encoder_stage1_persist_kernel<true>>("cmdiad_encoder_stage1", grid, dim3(512), Stage1Persist::LDS_BYTES, s, neigh, (const float4*)w1, (const bf16_t*)W2, p, pl.n_tiles);
        else rc = launch_lds<encoder_stage1_persist_kernel<false>>("cmdiad_encoder_stage1", grid, dim3(512), Stage1Persist::LDS_BYTES, s, neigh, (const float4*)w1, (const bf16_t*)W2, p, pl.n_tiles);
        break;
    case plan::stage1_kernel::once:
        rc = launch_lds<encoder_stage1_once_kernel>("cmdiad_encoder_stage1", grid, dim3(S128::THREADS), group_max_lds<S128>() + 4 * kRowStoreScratch, s, At, Wt, p);
        break;
    case plan::stage1_kernel::generic:   // planned in the test-only build alone
#ifdef CMDIAD_AB_VARIANTS
        rc = launch_lds<encoder_stage1_kernel<S128>>("cmdiad_encoder_stage1", grid, dim3(S128::THREADS), group_max_lds<S128>(), s, At, Wt, p);
        break;
#else
        cmdiad_set_error("cmdiad_encoder_stage1: the plan names a kernel that only the test build (make ab) contains");
        return CMDIAD_ERR_ARG;
#endif
    }
    if (rc) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
