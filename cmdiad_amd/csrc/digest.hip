// 64-bit content digest of a device buffer (cmdiad_digest64): what a stored fit (cmdiad_amd/fitted.py, docs/fitted.md) compares
// the backbone weights and the patch libraries in HBM against, without copying 450 MB + 300 MB per class to the host.
//
//   digest(buf, seed) = sum_i h( h(seed + i) ^ w_i )   mod 2^64,     w_i = the i-th little-endian 32-bit word of buf,
//   h = the splitmix64 finaliser (two xor-shift-multiply rounds and a closing xor-shift).
//
// A SUM of per-word terms, each keyed by the word's index: commutative and associative mod 2^64, so every reduction order --
// lanes, waves, workgroups, the order in which the workgroups' atomics land -- gives the same bits, and
// digest(a || b, s) = digest(a, s) + digest(b, s + len(a) / 4): a buffer can be hashed in pieces (a row shard by its offset).
// It guards against MISTAKES (another checkpoint, a truncated or bit-rotted file, a wrong shard), not against adversaries: the
// sum is linear in the per-word terms and anyone who wants a collision can build one.
//
// Cost: four 64 x 64-bit multiplies per word (v_mul_lo_u32 / v_mul_hi_u32 / v_mad_u64_u32 chains on the quarter-rate integer
// multiplier), so the kernel is bound by the VALU, not by HBM -- see profiles/fitted.md for the measured rate.
#include <algorithm>
#include "common.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ uint64_t term(uint64_t key, uint32_t w) { return mix64(mix64(key) ^ (uint64_t)w); }

constexpr int kDigestThreads = 256;

// words [0, head) one by one (head < 4: up to the first 16-byte boundary), then nvec uint4 (16-byte loads, grid-stride, two
// independent loads in flight per lane), then the last tail < 4 words one by one.  Every index stays below n = head + 4 nvec + tail.
__global__ __launch_bounds__(kDigestThreads) void digest64_kernel(const uint32_t* __restrict__ words, unsigned head, size_t nvec,
                                                                   unsigned tail, uint64_t seed, unsigned long long* __restrict__ acc)
{
    const uint4* __restrict__ vec = reinterpret_cast<const uint4*>(words + head);
    const size_t stride = (size_t)gridDim.x * kDigestThreads;
    const uint64_t base = seed + head;
    uint64_t s0 = 0, s1 = 0;
    size_t v = (size_t)blockIdx.x * kDigestThreads + threadIdx.x;
    for (; v + stride < nvec; v += 2 * stride) {
        const uint4 a = vec[v], b = vec[v + stride];
        const uint64_t ka = base + 4 * (uint64_t)v, kb = base + 4 * (uint64_t)(v + stride);
        s0 += term(ka, a.x) + term(ka + 1, a.y);
        s1 += term(ka + 2, a.z) + term(ka + 3, a.w);
        s0 += term(kb, b.x) + term(kb + 1, b.y);
        s1 += term(kb + 2, b.z) + term(kb + 3, b.w);
    }
    if (v < nvec) {
        const uint4 a = vec[v];
        const uint64_t ka = base + 4 * (uint64_t)v;
        s0 += term(ka, a.x) + term(ka + 1, a.y);
        s1 += term(ka + 2, a.z) + term(ka + 3, a.w);
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) s0 += term(seed + threadIdx.x, words[threadIdx.x]);
        if (threadIdx.x < tail) {
            const uint64_t i = (uint64_t)head + 4 * (uint64_t)nvec + threadIdx.x;
            s1 += term(seed + i, words[i]);
        }
    }
    uint64_t s = s0 + s1;
    // wave sum (integer: any order), then one LDS slot per wave, then ONE 64-bit vector atomic per workgroup
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += shfl_xor_u64(s, m);
    __shared__ uint64_t part[kDigestThreads / CMDIAD_WAVE];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
#pragma unroll
        for (int w = 0; w < kDigestThreads / CMDIAD_WAVE; ++w) t += part[w];
        if (t) atomicAdd(acc, (unsigned long long)t);
    }
}

}  // namespace

extern "C" int cmdiad_digest64(const void* data, size_t bytes, uint64_t seed, uint64_t* acc, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(acc && ((uintptr_t)acc & 7) == 0, CMDIAD_ERR_ARG, "cmdiad_digest64: acc must be a non-null, 8-byte aligned device pointer");
    CMDIAD_REQUIRE(bytes % 4 == 0, CMDIAD_ERR_ARG, "cmdiad_digest64: bytes (%zu) must be a multiple of 4", bytes);
    if (bytes == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(data && ((uintptr_t)data & 3) == 0, CMDIAD_ERR_ARG, "cmdiad_digest64: data must be a non-null, 4-byte aligned device pointer");
    const size_t n = bytes / 4;
    const unsigned head = (unsigned)std::min<size_t>(n, ((16 - ((uintptr_t)data & 15)) & 15) / 4);
    const size_t nvec = (n - head) / 4;
    const unsigned tail = (unsigned)(n - head - 4 * nvec);
    // two uint4 per lane and trip; at most 8 workgroups per compute unit (256 lanes each: the whole chip's wave slots)
    const size_t want = (nvec + 2 * kDigestThreads - 1) / (2 * kDigestThreads);
    const unsigned blocks = (unsigned)std::max<size_t>(1, std::min<size_t>(want, (size_t)kPersistCUs * 8));
    hipLaunchKernelGGL(digest64_kernel, dim3(blocks), dim3(kDigestThreads), 0, (hipStream_t)stream, (const uint32_t*)data, head, nvec,
                       tail, seed, (unsigned long long*)acc);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
