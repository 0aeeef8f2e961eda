// Stream-K form of the residual products of the transformer blocks (models/models.py:126-132,177-180: x = x + fc2(...), and the
// same algebra in timm's ViT block reached at models.py:48):   out_f32 = A . W^T + bias + residual,   N % 256 == 0.
//
// Why.  The N = 768 products of ViT-B/8 are 99 x 3 = 297 tiles of 256 x 256: on 256 CUs a tile walk is two rounds for 1.16 rounds
// of work, which is why they ran on the 128 x 128 kernel (1 188 tiles, three rounds for 2.3).  Here the unit of work is a K-STEP:
// the (tile, k-tile) list -- 297 x 48 = 14 256 steps for fc2 -- is cut into one contiguous range per CU (55.7 steps each), so
// every CU does the same amount of MFMA work on the two-group 256 x 256 pipeline (run_two_group, gemm_pp3.h: the schedule, its
// staging and its counted waits live there; this file supplies the job list and the job-end / job-start hooks).  A range covers the
// END of one tile, whole tiles, and the BEGINNING of another; a tile that two blocks share is finished IN ORDER:
//   * the block that owns the tile's first k-tiles accumulates from zero and parks its 256 x 256 fp32 accumulators in a
//     workspace slot (1 KiB per wave store: fully coalesced), then raises the slot's counter;
//   * the block that owns the rest loads them as the INITIAL accumulators and carries on -- the chain of MFMA accumulations per
//     output is exactly the one a single block would execute, so the result is bit-identical to the 128 x 128 kernel's
//     (tests/test_gpu_kernels.py), not a sum of two partial sums.
// Order inside a block: the head piece it must HAND OVER comes first, whole tiles next, the tail piece it must TAKE OVER last --
// its predecessor parked that piece at the very start of its own run, so nobody waits (ranges are at least one tile long: no
// block both takes and hands over the same tile).  Blocks use their hardware index (no XCD remap): dispatch is in index order,
// so a block's predecessor is resident before it is.
// Cross-XCD visibility: the parked accumulators are stored and loaded with sc0 sc1 (write-through / bypass: the L2 of an XCD is not
// coherent with the others'), the counters are agent-scope atomics; no cache-wide write-back or invalidate.
// The partial accumulators and the epilogue's residual rows arrive by inline-asm loads with explicit counted waits: a
// compiler-visible load inside the K loop gets an s_waitcnt vmcnt(0) in every iteration (tools/isa_lint.py).
#include "gemm_pp3.h"
#include "gemm_sk_jobs.h"
#include "launch.h"

namespace {

using namespace gemm;

struct SkParams {
    int M, N, K;
    const float* bias;
    const float* residual; int ldr;
    float* out; int ldo;
    float* partial;        // [blocks][8 waves][32][64 lanes] f32x4
    unsigned* counter;     // [blocks][2]: waves that have parked slot b / waves that have taken it over
};

constexpr int kSkSlotFloats = 256 * 256;
constexpr int kSkEpiOps = 32;   // vector-memory stores of one wave at the end of a job (partial hand-over or full epilogue)

__global__ __launch_bounds__(512, 1) void gemm_sk_kernel(GlobalTile A, GlobalTile W, SkParams p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using S = SPP3;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    const int b = blockIdx.x;
    // the block's jobs in execution order (gemm_sk_jobs.h): head piece to hand over | whole tiles | tail piece to take over
    const SkJob first((p.M + S::BM - 1) / S::BM, p.N / S::BN, p.K / BK, b, (int)gridDim.x);
    if (first.total <= 0) return;

    RowStore32 rs;
    rs.init(lds + S::LDS_BYTES + wave * kRowStoreScratch, lane);
    // hand-over slots: wave w, accumulator register q = 4 i + j, lane l at float4 index (w * 32 + q) * 64 + l -- addressed as
    // (uniform base of (slot, i) in SGPRs) + (per-lane byte offset) + (j * 1 KiB immediate): no per-access address registers
    const unsigned slot_voff = (unsigned)((wave * 32 * 64 + lane) * 16);
    const float* slot_out = p.partial + (size_t)b * kSkSlotFloats;
    const float* slot_in = p.partial + (size_t)(b - 1) * kSkSlotFloats;

    f32x4 acc[8][4];
    // a job that continues a tile: its first accumulators are what the previous block parked (inline asm: header comment)
    auto take_over = [&]() __attribute__((always_inline)) {
        if (lane == 0) {
            while (__hip_atomic_load(p.counter + 2 * (b - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 8u) __builtin_amdgcn_s_sleep(2);
        }
        // the parked values were written by another CU, maybe on another XCD (whose L2 is not this one's): sc0 sc1 loads go to the
        // coherence point instead of this XCD's L2 -- an acquire FENCE at agent scope would invalidate the whole L2 under every
        // block of the XCD (measured: +60 us per launch)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* base = slot_in + (size_t)i * 4 * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3 sc0 sc1" : "=v"(acc[i][j]) : "v"(slot_voff), "s"(base), "n"(j * 1024) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // the slot is free again once all 8 waves have taken their part: the last one clears both counters for the next launch
        if (lane == 0) {
            const unsigned got = __hip_atomic_fetch_add(p.counter + 2 * (b - 1) + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (got == 7u) {
                __hip_atomic_store(p.counter + 2 * (b - 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(p.counter + 2 * (b - 1) + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    };
    // a job that stops before the tile's last k-tile: park the accumulators for the next block
    auto hand_over = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float* base = slot_out + (size_t)i * 4 * 256;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 sc0 sc1" ::"v"(slot_voff), "v"(acc[i][j]), "s"(base), "n"(j * 1024) : "memory");
        }
        // write-through stores (sc0 sc1), complete at the coherence point when the counter says so: this wave's count goes up only
        // after they are (a release FENCE at agent scope would write back the whole L2 instead)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(p.counter + 2 * b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    // out = acc + bias + residual, rows through the per-wave LDS transposition (8 rows x 128 contiguous bytes per access);
    // residual rows of 16-row block i + 1 are in flight while block i is combined and stored.  Residual addresses: a uniform
    // base (the wave's 64 columns) in SGPRs + a 32-bit per-lane byte offset (row x pitch + 16 u; rows past M clamp to M - 1).
    auto epilogue = [&](int mt, int ntile) __attribute__((always_inline)) {
        const int nw = ntile * S::BN + wc * 64, mw = mt * S::BM + wr * 128;
        f32x4 bj[4];
        {
            const float* bp = p.bias + nw;
            const unsigned boff = (unsigned)((lane >> 4) * 16);
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(bj[j]) : "v"(boff), "s"(bp), "n"(j * 64) : "memory");
        }
        const bool full = mt * S::BM + S::BM <= p.M;
        const float* rbase = p.residual + nw;
        f32x4 res[2][4];   // [parity of the 16-row block][ch * 2 + (row R | row R + 8)]
        auto load_res = [&](int i) __attribute__((always_inline)) {
            const int m0r = mw + i * 16 + rs.R;
            const unsigned oa = (unsigned)min(m0r, p.M - 1) * (unsigned)(p.ldr * 4) + (unsigned)(rs.u * 16);
            const unsigned ob = (unsigned)min(m0r + 8, p.M - 1) * (unsigned)(p.ldr * 4) + (unsigned)(rs.u * 16);
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(res[i & 1][0]) : "v"(oa), "s"(rbase) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(res[i & 1][1]) : "v"(ob), "s"(rbase) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, %2 offset:128" : "=v"(res[i & 1][2]) : "v"(oa), "s"(rbase) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, %2 offset:128" : "=v"(res[i & 1][3]) : "v"(ob), "s"(rbase) : "memory");
        };
        load_res(0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (i < 7) load_res(i + 1);
            // operations issued after block i's loads: block i - 1's stores (4) and block i + 1's loads (4); a ragged tile skips
            // stores, so its count is not known: it waits for everything
            if (!full) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (i == 0) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");     // (the bias loads are older still)
            else if (i < 7) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            const int m0r = mw + i * 16 + rs.R;
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                const int col = nw + ch * 32 + rs.u * 4;
                rs.park(acc[i][2 * ch] + bj[2 * ch], acc[i][2 * ch + 1] + bj[2 * ch + 1]);
                f32x4 t0, t1;
                rs.fetch(t0, t1);
                const f32x4 o0 = t0 + res[i & 1][ch * 2], o1 = t1 + res[i & 1][ch * 2 + 1];
                if (full || m0r < p.M) *reinterpret_cast<f32x4*>(p.out + (size_t)m0r * p.ldo + col) = o0;
                if (full || m0r + 8 < p.M) *reinterpret_cast<f32x4*>(p.out + (size_t)(m0r + 8) * p.ldo + col) = o1;
            }
        }
        return full;
    };

    run_two_group<false, kSkEpiOps>(A, W, first, first.total, lds, acc, [](const SkJob&, int) {},
        [&](const SkJob& j) {   // job finished: park the accumulators for the next block, or the tile's epilogue
            if (j.hands_over()) { hand_over(); return true; }
            return epilogue(j.mt(), j.nt());
        },
        [&](const SkJob& j) {   // job started: the accumulators the previous block parked, or zeros
            if (j.takes_over()) take_over();
            else {
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        });
}

}  // namespace

// The same kernel with ONE WHOLE TILE per block (grid = tiles: every block's unit range is exactly one tile, so nothing is parked
// or taken over and the workspace is never touched).  Stand-alone this loses to the 128 x 128 kernel (294 tiles = a full round of
// 256 CUs and a round of 38), but per CU-second a 256 x 256 tile is cheaper (half the LDS-DMA pieces per FLOP, the bound of the
// 128 x 128 kernel: profiles/r4_notes.md section 12) -- and inside the pipeline the CUs its second round leaves idle are not idle:
// the other streams' kernels take them.  Planned by plan_gemm (gemm_plan.h: tiles = its grid) for the residual products it is legal for.
int gemm_residual_tiles_launch(const cmdiad_gemm_args* a, unsigned tiles, hipStream_t stream)
{
    constexpr int kLds = SPP3::LDS_BYTES + 8 * kRowStoreScratch;
    GlobalTile A{(const bf16_t*)a->A, a->lda, a->M}, W{(const bf16_t*)a->W, a->ldw, a->N};
    SkParams p{a->M, a->N, a->K, a->bias, a->residual, a->ldr, a->out_f32, a->ldo32, nullptr, nullptr};
    if (const int rc = launch_lds<gemm_sk_kernel>("cmdiad_gemm_bf16", dim3(tiles), dim3(512), kLds, stream, A, W, p)) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

// a hand-over slot per block | two counters per block
struct SkWs { float* partial; unsigned* counters; size_t total; };
static SkWs sk_layout(void* base)
{
    Carve c(base);
    return {c.take<float>((size_t)kPersistCUs * kSkSlotFloats), c.take<unsigned>((size_t)kPersistCUs * 2), c.total()};
}

extern "C" size_t cmdiad_gemm_streamk_workspace_bytes(void) { return sk_layout(nullptr).total; }

extern "C" int cmdiad_gemm_streamk_eligible(int M, int N, int K) { return plan::streamk_eligible(M, N, K) ? 1 : 0; }

extern "C" int cmdiad_gemm_streamk_bf16(const cmdiad_gemm_args* a, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(a && a->A && a->W && a->bias && a->residual && a->out_f32 && workspace, CMDIAD_ERR_ARG,
                   "cmdiad_gemm_streamk_bf16: needs A, W, bias, residual, out_f32 and a workspace");
    CMDIAD_REQUIRE(plan::residual_form_only(*a), CMDIAD_ERR_ARG, "cmdiad_gemm_streamk_bf16: the residual form only (out_f32 = A.W^T + bias + residual)");
    CMDIAD_REQUIRE(plan::streamk_eligible(a->M, a->N, a->K), CMDIAD_ERR_ARG,
                   "cmdiad_gemm_streamk_bf16: shape M=%d N=%d K=%d is not eligible (cmdiad_gemm_streamk_eligible)", a->M, a->N, a->K);
    CMDIAD_REQUIRE(a->lda % 8 == 0 && a->ldw % 8 == 0 && aligned16(a->A) && aligned16(a->W) && a->ldo32 % 4 == 0 && a->ldr % 4 == 0 &&
                       aligned16(a->out_f32) && aligned16(a->residual) && aligned16(a->bias) && aligned16(workspace),
                   CMDIAD_ERR_ARG, "cmdiad_gemm_streamk_bf16: 16-byte alignment, lda / ldw %% 8, ldo / ldr %% 4");
    const SkWs L = sk_layout(workspace);
    if (const int rc = workspace_ok("cmdiad_gemm_streamk_bf16", workspace, workspace_bytes, L.total)) return rc;
    constexpr int kLds = SPP3::LDS_BYTES + 8 * kRowStoreScratch;
    GlobalTile A{(const bf16_t*)a->A, a->lda, a->M}, W{(const bf16_t*)a->W, a->ldw, a->N};
    SkParams p{a->M, a->N, a->K, a->bias, a->residual, a->ldr, a->out_f32, a->ldo32, L.partial, L.counters};
    if (const int rc = launch_lds<gemm_sk_kernel>("cmdiad_gemm_streamk_bf16", dim3(kPersistCUs), dim3(512), kLds, (hipStream_t)stream, A, W, p)) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
