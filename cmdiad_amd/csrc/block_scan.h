// Integer prefix sums over the threads of a workgroup of WAVES waves (blockDim.x = WAVES * 64; every thread calls them).
// Each has ONE barrier inside, between the write of the WAVES wave totals to the LDS row the caller passes and their read.
// Reuse of that row is the caller's business: a second call on the same row needs a barrier of the caller's (or a second
// row, as unorganize_kernel alternates) between the reads of one call and the writes of the next.
// Beside them: the lane of a thread, the wave-aggregated table increment and the plain workgroup sum.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// table[idx] += 1 for every active lane; lanes of the wave with the same idx share one atomic.  Every lane of the wave calls it.
template <typename T, typename I>
__device__ __forceinline__ void wave_agg_inc(T* table, I idx, bool active)
{
    unsigned long long todo = __ballot(active);
    while (todo) {   // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const I lidx = __shfl(idx, leader, 64);
        const unsigned long long same = __ballot(active && idx == lidx);
        if (lane_id() == leader) atomicAdd(table + lidx, (T)__popcll(same));
        todo &= ~same;
    }
}

// sum over the workgroup of an int (256 threads); one barrier, sh: 4 ints
__device__ __forceinline__ int block_sum(int v, int* sh)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// inclusive sum over the lanes of a wave
__device__ __forceinline__ int wave_incl_scan(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// the wave totals of `row` in front of this wave, and all of them
template <int WAVES>
__device__ __forceinline__ int block_scan_base(const int* row, int& total)
{
    const int wave = threadIdx.x >> 6;
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int s = row[w];
        base += w < wave ? s : 0;
        tot += s;
    }
    total = tot;
    return base;
}

// exclusive sum of v over the block's threads in thread order; total = the sum over all of them.  sh: WAVES ints of LDS
template <int WAVES>
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total)
{
    const int incl = wave_incl_scan(v);
    if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = incl;
    __syncthreads();
    return block_scan_base<WAVES>(sh, total) + incl - v;
}

// the number of threads in front of this one whose `keep` is set (by ballots: no shuffles); total = all that keep
template <int WAVES>
__device__ __forceinline__ int block_ballot_rank(bool keep, int* s_wave, int& total)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) s_wave[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    return block_scan_base<WAVES>(s_wave, total) + __popcll(m & ((1ull << lane) - 1ull));
}
