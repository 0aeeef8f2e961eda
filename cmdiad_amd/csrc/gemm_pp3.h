// The two-group ("ping-pong") 256 x 256 x 64 MFMA pipeline: THE one implementation of the schedule (run_two_group) that the
// persistent network GEMMs (gemm.hip: gemm_std_pp3_kernel through run_pp3_jobs) and the stream-K / one-tile residual kernel
// (gemm_sk.hip) instantiate with a job type and their hooks.  l2_min_pp3_kernel (l2min.hip) runs the same schedule from a
// hand-kept copy (its norm fetch / park hooks pushed the shared loop past 256 VGPRs: profiles/two_group_loop.md); a change to
// the schedule is made here and there.
//
//   * 8 waves of 128 x 64 in two groups of four (one wave of each group per SIMD) half a phase apart: one group's fragment
//     reads and LDS-DMA issue sit under the other group's MFMAs.  A K-tile = 4 phases of 16 MFMAs per wave.
//   * LDS (SPP3): three W buffers (3 x 32 KiB) + three A HALF slots (3 x 16 KiB: a tile's lo rows are read in phase 0 and its
//     hi rows in phase 2, so halves rotate through three slots) = 144 KiB.
//   * The two operands are issued by DIFFERENT waves -- waves 0-3 (the earlier group) feed the W stream, waves 4-7 the A
//     stream -- because s_waitcnt vmcnt retires in order per wave: in one queue the short-lead A pieces would force the
//     long-lead W pieces out early.  Each stream is a plain sequence of half-units (8 pieces = 4 waves x 2)
//     [lo h0, lo h1, hi h0, hi h1] per K-tile, one per phase:   W half-unit (P + 10) and A half-unit (P + 5) are issued in
//     phase P.
//       W:  lo(T') in phases 4T'-10, -9 (its buffer held K-tile T'-3, whose lo rows were last read in phase 4T'-12: an
//           earlier-group issuer needs two phases of distance), hi(T') in 4T'-8, -7 (last read 4T'-11); read in 4T', 4T'+1:
//           every half-unit has >= 7 phases, so vmcnt(14) (the 7 newest half-units) is the counted wait of the W waves;
//       A:  lo(T') in 4T'-5, -4 (slot of hi(T'-2), last read 4T'-6: a later-group issuer needs one phase), hi(T') in
//           4T'-3, -2 (slot of lo(T'-1), last read 4T'-4); the earlier group reads half a phase before the issuing group's
//           wait, so a half-unit issued in phase P is readable from P + 3: vmcnt(6) for the A waves.
//     The s_waitcnt counters are never drained inside a stream, and BOTH streams run on across job boundaries: the next job's
//     first K-tiles are in flight while the current job's last MFMAs and its end hook execute -- no per-tile fill or drain.
//   * Hooks of run_two_group (all called by every wave, on the consumer side's copy of the job):
//       phase0(job, left)  in phase 0 of every K-tile, `left` K-tiles of the job remaining including this one: the place to
//                          fetch the job end's operands by inline asm (eight DMA pieces are issued between phase 0 of the
//                          last K-tile and the job end, or the stream has ended and drained: the end can open with
//                          s_waitcnt vmcnt(8) instead of a compiler-placed vmcnt(0) that would drain the prefetch queue);
//       job_end(job)       after the job's last phase; returns true when it is GUARANTEED to have issued EPI_OPS
//                          vector-memory operations.  Loads and stores count in vmcnt like the DMA pieces and retire in order,
//                          so for the phases in which those operations are younger than the piece a counted wait protects (7
//                          phases for the W stream, 3 for the A stream) the wait's immediate is raised by EPI_OPS: vmcnt(14)
//                          right after 32 stores would wait for 20 of them to reach L2 -- with all eight waves of the CU at
//                          the next barrier;
//       job_start(job)     before the first job's first phase (after the prologue's DMA pieces) and after every job_end but
//                          the last: sets the accumulators.
//   * A job is a small value type: mt() / nt() its tile, k0() its first k-tile, kc() its k-tile count (>= 1), next() the step
//     to the block's next job.  The stream side and the consumer side each walk a copy.
// Whole 256-column tiles only (N % 256 == 0); ragged M is clamped on the A stream and masked by the caller; K >= 192.
#pragma once
#include "gemm_core.h"

namespace gemm {

struct SPP3 {
    static constexpr int BM = 256, BN = 256, THREADS = 512;
    static constexpr int BUF = 32768, HALF = 16384;
    static constexpr int A_OFF = 3 * BUF;
    static constexpr int LDS_BYTES = A_OFF + 3 * HALF;
};

__device__ __forceinline__ void pp3_barrier() { asm volatile("s_barrier" ::: "memory"); }

template <int N>
__device__ __forceinline__ void pp3_wait_vmcnt()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// acc[i][j][r]: row m = mt*256 + wr*128 + i*16 + (lane & 15), column n = nt*256 + wc*64 + j*16 + (lane >> 4)*4 + r
// (swapped orientation: a lane holds four consecutive columns of one row).
// T_total: K-tiles of all the block's jobs together.  EPI_OPS is compile time: it becomes an s_waitcnt immediate.
template <bool F16, int EPI_OPS, class Job, class Phase0, class JobEnd, class JobStart>
__device__ __forceinline__ void run_two_group(const GlobalTile& A, const GlobalTile& W, const Job& first, int T_total, char* lds,
                                              f32x4 (&acc)[8][4], Phase0&& phase0, JobEnd&& job_end, JobStart&& job_start)
{
    using S = SPP3;
    using frag = typename std::conditional<F16, f16x8, bf16x8>::type;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    if (T_total <= 0) return;  // block-uniform

    // Everything below is instantiated twice, once per stream: a wave only ever executes its own (lean) issue path.
    auto body = [&](auto BANK) {
    constexpr bool bank_wave = decltype(BANK)::value;
    const int sw = wave & 3;
    const int src_chunk = ((lane & 7) ^ (lane >> 3)) * 8;  // element offset of the 16-byte chunk this lane fetches
    const int row_w = bank_wave ? (sw >> 1) * 64 + (sw & 1) * 16 : sw * 16;  // this wave's share of every half-unit
    const size_t ld2 = (size_t)(bank_wave ? W.ld : A.ld) * 2;                  // row pitch in bytes
    Job sj = first;                                                            // the stream's current job
    int s_mt = sj.mt(), s_k = sj.k0(), s_left = sj.kc();
    auto tile_ptr = [&]() {
        return bank_wave ? reinterpret_cast<const char*>(W.base + (size_t)(sj.nt() * S::BN + row_w + (lane >> 3)) * W.ld + s_k * BK + src_chunk)
                         : reinterpret_cast<const char*>(A.base + (size_t)(s_mt * S::BM + row_w + (lane >> 3)) * A.ld + s_k * BK + src_chunk);
    };
    const char* ptr = tile_ptr();
    bool a_full = s_mt * S::BM + S::BM <= A.rows;
    int hT = 0;                    // stream cursor: K-tile index over the whole job range
    int slot_lo = 0, slot_hi = 1;  // W: both = buffer of K-tile hT;  A: half slots of (lo, hi) of K-tile hT
    if (bank_wave) slot_hi = 0;
    auto issue_part = [&](auto PART) {  // -> true when the half-unit was issued
        constexpr int part = decltype(PART)::value, hi = part >> 1, hsel = part & 1;
        if (hT >= T_total) return false;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const char* src;
            char* dst;
            if (bank_wave) {
                constexpr int rows = hsel * 128 + hi * 32;
                src = ptr + (size_t)(rows + e * 8) * ld2;
                dst = lds + slot_lo * S::BUF + (row_w + rows + e * 8) * 128;
            } else {
                constexpr int rows = hsel * 128 + hi * 64;
                if (a_full) src = ptr + (size_t)(rows + e * 8) * ld2;
                else src = reinterpret_cast<const char*>(A.base + (size_t)min(s_mt * S::BM + row_w + rows + e * 8 + (lane >> 3), A.rows - 1) * A.ld + s_k * BK + src_chunk);
                dst = lds + S::A_OFF + (hi ? slot_hi : slot_lo) * S::HALF + (row_w + hsel * 64 + e * 8) * 128;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
        }
        if constexpr (part == 3) {  // next K-tile of this stream
            ++hT;
            ++s_k;
            if (--s_left == 0 && hT < T_total) {   // next job
                sj.next();
                s_mt = sj.mt(); s_k = sj.k0(); s_left = sj.kc();
                ptr = tile_ptr();
                a_full = s_mt * S::BM + S::BM <= A.rows;
            } else ptr += BK * 2;
            if (bank_wave) { slot_lo = slot_lo == 2 ? 0 : slot_lo + 1; slot_hi = slot_lo; }
            else { slot_lo = slot_lo == 0 ? 2 : slot_lo - 1; slot_hi = slot_hi == 0 ? 2 : slot_hi - 1; }  // (x + 2) mod 3
        }
        return true;
    };
    // phase j issues W part (j + 2) % 4 and A part (j + 1) % 4 (W half-unit P + 10, A half-unit P + 5)
    auto issue_phase = [&](auto J) {
        constexpr int j = decltype(J)::value;
        return bank_wave ? issue_part(std::integral_constant<int, (j + 2) % 4>{}) : issue_part(std::integral_constant<int, (j + 1) % 4>{});
    };
    int ep_age = 1 << 20;  // phases since a job end that issued EPI_OPS operations (wave-uniform)
    auto phase_wait = [&](bool issued) {
        constexpr int lead = bank_wave ? 7 : 3, base = bank_wave ? 14 : 6;
        constexpr int raised = base + EPI_OPS > 63 ? 63 : base + EPI_OPS;
        if (!issued) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else if (ep_age < lead) pp3_wait_vmcnt<raised>();
        else pp3_wait_vmcnt<base>();
        ++ep_age;
    };
    {
        using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
        using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
        issue_part(I0{}); issue_part(I1{}); issue_part(I2{}); issue_part(I3{}); issue_part(I0{});  // half-units 0..4
        if (bank_wave) { issue_part(I1{}); issue_part(I2{}); issue_part(I3{}); issue_part(I0{}); issue_part(I1{}); }  // 5..9
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    pp3_barrier();
    if (wr == 1) pp3_barrier();  // the second group runs one barrier (half a phase) behind the first

    // fragment addresses: row*128 + ((chunk ^ (row & 7)) << 4), chunk = kk*4 + (lane >> 4); kk = 1 flips bit 6
    const int swz = (((lane >> 4)) ^ (lane & 7)) << 4;
    const int a_off = (wr * 64 + (lane & 15)) * 128 + swz, b_off = (wc * 64 + (lane & 15)) * 128 + swz;
    int a_lo = 0, a_hi = 0, b_base = 0;
    auto lda = [&](int i, int kk) { return *reinterpret_cast<const frag*>(lds + (((i < 4 ? a_lo : a_hi) + (i & 3) * 2048) ^ (kk << 6))); };
    auto ldb = [&](int j, int kk) { return *reinterpret_cast<const frag*>(lds + ((b_base + j * 2048) ^ (kk << 6))); };

    frag af[4][2], wlo[2][2], whi[2][2];
    Job cj = first;        // the consumer's current job
    int c_left = cj.kc();
    job_start(cj);
    for (int T = 0; T < T_total; ++T) {
        a_lo = S::A_OFF + ((2 * T) % 3) * S::HALF + a_off;
        a_hi = S::A_OFF + ((2 * T + 1) % 3) * S::HALF + a_off;
        b_base = (T % 3) * S::BUF + b_off;
        // ================= phase 0: W lo + A lo
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) wlo[j][kk] = ldb(j, kk);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) af[i][kk] = lda(i, kk);
        phase0(cj, c_left);
        phase_wait(issue_phase(std::integral_constant<int, 0>{}));
        pp3_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(wlo[j][kk], af[i][kk], acc[i][j]);
        __builtin_amdgcn_s_setprio(0);
        pp3_barrier();
        // ================= phase 1: W hi
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) whi[j][kk] = ldb(2 + j, kk);
        phase_wait(issue_phase(std::integral_constant<int, 1>{}));
        pp3_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][2 + j] = mfma16(whi[j][kk], af[i][kk], acc[i][2 + j]);
        __builtin_amdgcn_s_setprio(0);
        pp3_barrier();
        // ================= phase 2: A hi
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) af[i][kk] = lda(4 + i, kk);
        phase_wait(issue_phase(std::integral_constant<int, 2>{}));
        pp3_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[4 + i][2 + j] = mfma16(whi[j][kk], af[i][kk], acc[4 + i][2 + j]);
        __builtin_amdgcn_s_setprio(0);
        pp3_barrier();
        // ================= phase 3: no reads (W lo is still in registers)
        phase_wait(issue_phase(std::integral_constant<int, 3>{}));
        pp3_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[4 + i][j] = mfma16(wlo[j][kk], af[i][kk], acc[4 + i][j]);
        __builtin_amdgcn_s_setprio(0);
        if (--c_left == 0) {  // job finished
            __builtin_amdgcn_sched_barrier(0);
            ep_age = job_end(cj) ? 0 : 1 << 20;
            if (T + 1 < T_total) {
                cj.next();
                c_left = cj.kc();
                job_start(cj);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        pp3_barrier();
    }
    if (wr == 0) pp3_barrier();  // both groups execute the same number of barriers
    };
    if (wave < 4) body(std::true_type{});
    else body(std::false_type{});
}

// The persistent walk: jobs [j0, j1) of the (M tile, N tile) list, N tile fastest, every job a whole tile of KT k-tiles.
struct TileJob {
    int m, n, NT, KT;
    __device__ __forceinline__ int mt() const { return m; }
    __device__ __forceinline__ int nt() const { return n; }
    __device__ __forceinline__ int k0() const { return 0; }
    __device__ __forceinline__ int kc() const { return KT; }
    __device__ __forceinline__ void next() { if (++n == NT) { n = 0; ++m; } }
};

// pre(mt, nt) runs in phase 0 of a tile's LAST K-tile; epi(acc, mt, nt) after its last phase, returning the number of
// vector-memory operations it is guaranteed to have issued (EPI_OPS for a full tile, 0 when unsure).
template <bool F16, int EPI_OPS, class Pre, class Epi>
__device__ __forceinline__ void run_pp3_jobs(const GlobalTile& A, const GlobalTile& W, int j0, int j1, int NT, int KT, char* lds,
                                             Pre&& pre, Epi&& epi)
{
    f32x4 acc[8][4];
    run_two_group<F16, EPI_OPS>(A, W, TileJob{j0 / NT, j0 % NT, NT, KT}, (j1 - j0) * KT, lds, acc,
        [&](const TileJob& j, int left) { if (left == 1) pre(j.m, j.n); },
        [&](const TileJob& j) { return epi(acc, j.m, j.n) >= EPI_OPS; },
        [&](const TileJob&) {
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        });
}

}  // namespace gemm
