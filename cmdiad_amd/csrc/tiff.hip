// Unpacking the xyz TIFFs on the device (cmdiad_amd/utils/tiff.py reads the file, inflates deflate chunks on the reader thread and
// uploads the bytes; docs/tiff.md).  The kernels below only MOVE bytes: raw file bytes with uncompressed chunks in, the image
// [B,H,W,C] of the file's own float type out.  A strip is a tile of full width (chunk_w == W); chunks are numbered row-major over the
// image, plane after plane for planar files; chunk_off [B, n_chunks] holds every chunk's byte offset into raw.
//
// Reads: chunk offsets of real files are only 2-byte aligned (and the tests make them odd), so a sample is never loaded through a
// misaligned vector access: the aligned dwords around it are loaded and combined with v_alignbyte_b32.  Every dword load is guarded
// -- a dword that does not lie inside [0, raw_bytes) reads as 0 -- so no table can make a kernel read outside the upload buffer
// (raw_bytes is a multiple of 4 and raw is dword aligned: checked by the entry point); ops.tiff_unpack checks the table on the host
// before the launch and refuses a bad one.  Writes go to samples of the image only: tile padding columns and rows and the missing
// rows of a short last strip are never read as samples and never written.
//
// predictor 1: one thread per output sample, coalesced stores.
// predictor 3 (libtiff's fpAcc): one workgroup per chunk row.  The row (chunk_w * Cc * bps bytes, Cc = C chunky / 1 planar, at most
//   64 KiB) is brought into LDS; the byte prefix sum mod 256 with stride Cc runs as per-thread segment sums (segments are multiples
//   of Cc bytes, so a byte's class is its position in the segment), one block scan of the 256 segment totals with the Cc classes packed
//   in the four bytes of a dword (byte-wise add without carries between the lanes), and a second walk that applies the running sums
//   in place; then byte k of sample i is gathered from plane k (plane 0 = most significant) and the sample is stored.
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxRowBytes = 64 * 1024;

struct TiffGeom {
    int W, H, C, chunk_w, chunk_h, across, per_plane, planar, bps, big_endian;
};

// the dword at byte index a (a multiple of 4) of raw, 0 when it does not lie inside the buffer
__device__ __forceinline__ uint32_t guarded_dword(const uint32_t* __restrict__ raw, int64_t raw_bytes, int64_t a)
{
    return (a >= 0 && a + 4 <= raw_bytes) ? raw[a >> 2] : 0u;
}

// the four bytes at ANY byte index src, little-endian
__device__ __forceinline__ uint32_t unaligned_dword(const uint32_t* __restrict__ raw, int64_t raw_bytes, int64_t src)
{
    const int64_t a = src & ~(int64_t)3;
    const uint32_t lo = guarded_dword(raw, raw_bytes, a), hi = guarded_dword(raw, raw_bytes, a + 4);
    return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(src & 3));
}

__global__ __launch_bounds__(kThreads) void tiff_copy_kernel(const uint32_t* __restrict__ raw, int64_t raw_bytes,
                                                             const int64_t* __restrict__ chunk_off, int n_chunks, TiffGeom g,
                                                             uint32_t* __restrict__ out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x, b = blockIdx.y;
    if (i >= g.H * g.W * g.C) return;
    const int pix = i / g.C, c = i - pix * g.C;
    const int y = pix / g.W, x = pix - y * g.W;
    const int cy = y / g.chunk_h, ry = y - cy * g.chunk_h, cx = x / g.chunk_w, rx = x - cx * g.chunk_w;
    int chunk = cy * g.across + cx, idx = ry * g.chunk_w + rx;
    if (g.planar) chunk += c * g.per_plane;
    else idx = idx * g.C + c;
    const int64_t src = chunk_off[(size_t)b * n_chunks + chunk] + (int64_t)idx * g.bps;
    const size_t o = (size_t)b * g.H * g.W * g.C + i;
    if (g.bps == 4) {
        const uint32_t v = unaligned_dword(raw, raw_bytes, src);
        out[o] = g.big_endian ? __builtin_bswap32(v) : v;
    } else {
        const int64_t a = src & ~(int64_t)3;
        const uint32_t sel = (uint32_t)(src & 3);
        const uint32_t d0 = guarded_dword(raw, raw_bytes, a), d1 = guarded_dword(raw, raw_bytes, a + 4),
                       d2 = guarded_dword(raw, raw_bytes, a + 8);
        const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, sel), hi = __builtin_amdgcn_alignbyte(d2, d1, sel);
        uint2 v = g.big_endian ? make_uint2(__builtin_bswap32(hi), __builtin_bswap32(lo)) : make_uint2(lo, hi);
        reinterpret_cast<uint2*>(out)[o] = v;
    }
}

// byte-wise a + b mod 256 in the four bytes of a dword, no carry from one byte into the next
__device__ __forceinline__ uint32_t add_bytes(uint32_t a, uint32_t b)
{
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}

// S = the stride of the byte sum = samples per pixel of a chunk (Cc).  Dynamic LDS: the row, rounded up to whole dwords, then
// kThreads dwords for the scan.
template <int S>
__global__ __launch_bounds__(kThreads) void tiff_fp_predictor_kernel(const uint32_t* __restrict__ raw, int64_t raw_bytes,
                                                                     const int64_t* __restrict__ chunk_off, int n_chunks, TiffGeom g,
                                                                     uint8_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int chunk = blockIdx.x / g.chunk_h, ry = blockIdx.x - chunk * g.chunk_h;
    const int plane = g.planar ? chunk / g.per_plane : 0, rest = chunk - plane * g.per_plane;
    const int cy = rest / g.across, cx = rest - cy * g.across;
    const int y = cy * g.chunk_h + ry;
    if (y >= g.H) return;                                   // padding rows of a tile, missing rows of a short last strip (block-uniform)
    const int wc = g.chunk_w * S, L = wc * g.bps, words = (L + 3) >> 2;      // (bps is 4 or 8: L is a whole number of dwords)
    uint8_t* row = reinterpret_cast<uint8_t*>(lds);
    uint32_t* scan = lds + words;

    const int64_t src = chunk_off[(size_t)b * n_chunks + chunk] + (int64_t)ry * L;
    for (int w = tid; w < words; w += kThreads) lds[w] = unaligned_dword(raw, raw_bytes, src + 4 * (int64_t)w);
    __syncthreads();

    // segments of seg bytes, seg a multiple of S: byte j of a segment belongs to class j % S
    const int seg = ((L + kThreads - 1) / kThreads + S - 1) / S * S;
    const int lo = min(tid * seg, L), hi = min(lo + seg, L);     // (L is a multiple of S)
    uint32_t acc[S];
#pragma unroll
    for (int c = 0; c < S; ++c) acc[c] = 0;
    for (int j = lo; j < hi; j += S) {
#pragma unroll
        for (int c = 0; c < S; ++c) acc[c] += row[j + c];
    }
    uint32_t packed = 0;
#pragma unroll
    for (int c = 0; c < S; ++c) packed |= (acc[c] & 0xffu) << (8 * c);
    // inclusive block scan of the packed totals (Hillis-Steele over kThreads dwords), then the exclusive value of this thread
    scan[tid] = packed;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kThreads; d <<= 1) {
        const uint32_t other = tid >= d ? scan[tid - d] : 0u;
        __syncthreads();
        scan[tid] = add_bytes(scan[tid], other);
        __syncthreads();
    }
    const uint32_t before = tid ? scan[tid - 1] : 0u;
#pragma unroll
    for (int c = 0; c < S; ++c) acc[c] = (before >> (8 * c)) & 0xffu;
    for (int j = lo; j < hi; j += S) {
#pragma unroll
        for (int c = 0; c < S; ++c) {
            acc[c] = (acc[c] + row[j + c]) & 0xffu;
            row[j + c] = (uint8_t)acc[c];
        }
    }
    __syncthreads();

    // sample i of the chunk row: byte k from plane k, most significant first; the value is stored in the device's byte order
    const int x0 = cx * g.chunk_w;
    for (int i = tid; i < wc; i += kThreads) {
        const int px = i / S, c = i - px * S, x = x0 + px;
        if (x >= g.W) continue;                              // padding columns of a tile
        const size_t o = (((size_t)b * g.H + y) * g.W + x) * g.C + (g.planar ? plane : c);
        if (g.bps == 4) {
            const uint32_t v = ((uint32_t)row[i] << 24) | ((uint32_t)row[wc + i] << 16) | ((uint32_t)row[2 * wc + i] << 8) | row[3 * wc + i];
            reinterpret_cast<uint32_t*>(out)[o] = v;
        } else {
            const uint32_t hi32 = ((uint32_t)row[i] << 24) | ((uint32_t)row[wc + i] << 16) | ((uint32_t)row[2 * wc + i] << 8) | row[3 * wc + i];
            const uint32_t lo32 = ((uint32_t)row[4 * wc + i] << 24) | ((uint32_t)row[5 * wc + i] << 16) | ((uint32_t)row[6 * wc + i] << 8) |
                                  row[7 * wc + i];
            reinterpret_cast<uint2*>(out)[o] = make_uint2(lo32, hi32);
        }
    }
}


}  // namespace

extern "C" int cmdiad_tiff_unpack(const uint8_t* raw, int64_t raw_bytes, const int64_t* chunk_off, int B, int n_chunks, int W, int H,
                                  int C, int chunk_w, int chunk_h, int planar, int bytes_per_sample, int big_endian, int predictor,
                                  void* out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(raw && chunk_off && out, CMDIAD_ERR_ARG, "cmdiad_tiff_unpack: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(W) && side_ok(H) && side_ok(chunk_w) && side_ok(chunk_h) && C >= 1 && C <= 4,
                   CMDIAD_ERR_ARG, "cmdiad_tiff_unpack: bad sizes B=%d (1..65535) W=%d H=%d chunk_w=%d chunk_h=%d (sides 1..%d) C=%d (1..4)",
                   B, W, H, chunk_w, chunk_h, kMaxSide, C);
    CMDIAD_REQUIRE((bytes_per_sample == 4 || bytes_per_sample == 8) && (planar == 0 || planar == 1) && (big_endian == 0 || big_endian == 1) &&
                       (predictor == 1 || predictor == 3),
                   CMDIAD_ERR_ARG, "cmdiad_tiff_unpack: bytes_per_sample=%d (4 | 8) planar=%d (0 | 1) big_endian=%d (0 | 1) predictor=%d (1 | 3)",
                   bytes_per_sample, planar, big_endian, predictor);
    CMDIAD_REQUIRE(raw_bytes >= 4 && raw_bytes % 4 == 0 && ((uintptr_t)raw & 3) == 0 && ((uintptr_t)out & 7) == 0, CMDIAD_ERR_ARG,
                   "cmdiad_tiff_unpack: raw must be dword aligned and raw_bytes=%lld a positive multiple of 4 (the upload buffer is padded), "
                   "out 8-byte aligned", (long long)raw_bytes);
    TiffGeom g;
    g.W = W, g.H = H, g.C = C, g.chunk_w = chunk_w, g.chunk_h = chunk_h, g.planar = planar, g.bps = bytes_per_sample, g.big_endian = big_endian;
    g.across = (W + chunk_w - 1) / chunk_w;
    g.per_plane = g.across * ((H + chunk_h - 1) / chunk_h);
    const int expect = g.per_plane * (planar ? C : 1);
    CMDIAD_REQUIRE(n_chunks == expect, CMDIAD_ERR_ARG, "cmdiad_tiff_unpack: n_chunks=%d, the geometry needs %d", n_chunks, expect);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t* raw32 = reinterpret_cast<const uint32_t*>(raw);
    if (predictor == 1) {
        const int samples = H * W * C;      // <= 2^30
        hipLaunchKernelGGL(tiff_copy_kernel, dim3((unsigned)((samples + kThreads - 1) / kThreads), (unsigned)B), dim3(kThreads), 0, s, raw32,
                           raw_bytes, chunk_off, n_chunks, g, reinterpret_cast<uint32_t*>(out));
        CMDIAD_CHECK_LAUNCH();
        return CMDIAD_OK;
    }
    const int stride = planar ? 1 : C;
    const int64_t row_bytes = (int64_t)chunk_w * stride * bytes_per_sample;
    CMDIAD_REQUIRE(row_bytes <= kMaxRowBytes, CMDIAD_ERR_ARG,
                   "cmdiad_tiff_unpack: a predictor-3 chunk row of %lld bytes exceeds %d (undo the predictor on the host)", (long long)row_bytes,
                   kMaxRowBytes);
    const size_t lds = (size_t)((row_bytes + 3) / 4 * 4) + kThreads * sizeof(uint32_t);
    const dim3 grid((unsigned)((int64_t)n_chunks * chunk_h), (unsigned)B), block(kThreads);
    uint8_t* o = reinterpret_cast<uint8_t*>(out);
    int rc = CMDIAD_OK;
    switch (stride) {
    case 1: rc = launch_lds<tiff_fp_predictor_kernel<1>>("cmdiad_tiff_unpack", grid, block, lds, s, raw32, raw_bytes, chunk_off, n_chunks, g, o); break;
    case 2: rc = launch_lds<tiff_fp_predictor_kernel<2>>("cmdiad_tiff_unpack", grid, block, lds, s, raw32, raw_bytes, chunk_off, n_chunks, g, o); break;
    case 3: rc = launch_lds<tiff_fp_predictor_kernel<3>>("cmdiad_tiff_unpack", grid, block, lds, s, raw32, raw_bytes, chunk_off, n_chunks, g, o); break;
    default: rc = launch_lds<tiff_fp_predictor_kernel<4>>("cmdiad_tiff_unpack", grid, block, lds, s, raw32, raw_bytes, chunk_off, n_chunks, g, o); break;
    }
    if (rc != CMDIAD_OK) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
