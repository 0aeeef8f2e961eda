// Undoing the row filters of the dataset's PNGs on the device (cmdiad_amd/utils/png.py parses the file, inflates its zlib stream on the
// reader thread and uploads the still-filtered scanlines; docs/png.md).  In: per image H scanlines of 1 + W * bpp bytes, the filter
// type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) in front of every row.  Out: [B,H,W,OC] uint8, converted at the store only.
//
// Byte x of row r needs byte x - bpp of row r (a), byte x of row r - 1 (b) and byte x - bpp of row r - 1 (c); Average and Paeth are
// not associative, so a row cannot be scanned.  The rows are SKEWED instead: a wave owns a band of 64 rows, lane k the row r0 + k;
// at step t lane k reconstructs pixel t - k, all five filter types through the same step.  b is what lane k - 1 produced one step
// earlier and arrives by __shfl_up; c is the previous step's b; a is the lane's own previous pixel.  A pixel (1..4 bytes) travels
// packed in one dword and is reconstructed byte by byte mod 256; the carried values are the file's own bytes.
//
// Between bands: lane 63 writes every pixel it finishes into its wave's ring in LDS, lane 0 of the next band reads its b there.
// One workgroup per image, NW waves, band j on wave j % NW.  Time is cut into supersteps of 64 steps with a workgroup barrier after
// each; band j runs its chunk c (steps 64c .. 64c + 63) in superstep LAG * j + c.
//   NW = 1 (the one-wave baseline): LAG = chunks per band, band after band; the ring is a whole carry row (W dwords rounded up to a
//     power of two, at most 64 KiB): lane 63 writes pixel p 63 steps after lane 0 has read it.
//   NW = 8 | 16: LAG = 2.  Lane 0 of band j + 1 reads pixels 64c .. 64c + 63 in its chunk c; lane 63 of band j wrote them in its chunks
//     c and c + 1, which ended one superstep (one barrier) earlier, and writes pixels 64c + 65 .. 64c + 128 meanwhile: a ring of 256
//     pixels never holds two live pixels in one slot.  A wave is free for band j + NW at superstep 2 (j + NW), so 2 NW >= chunks + 2
//     is required (the entry point picks NW from the width; wider images take NW = 1).
// Every wave executes every superstep's barrier whether it has a chunk or not: the loop bounds are uniform over the workgroup.
//
// Reads: scanlines are only 1-byte aligned (the filter byte), so pixels are read with byte loads, one group of 4 steps ahead of the
// arithmetic; any source byte outside [0, raw_bytes) reads as 0, so no offset makes the kernel read outside the upload buffer
// (ops.png_unfilter checks the offsets on the host before the launch and refuses a bad one).  A filter type above 4 acts as None
// (utils.png.read_raw refuses such a file).  Writes go to pixels of the image only.
//
// The encoder's direction, cmdiad_png_filter, is at the end of the file: filtering has none of these dependencies.
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kRing = 256;            // pixels of a wave's ring when NW > 1
constexpr int kGroup = 4;             // steps whose source bytes are loaded ahead together

enum { kTargetRgb = 0, kTargetL = 1, kTargetRaw = 2 };

// the BPP bytes at raw[at ..] packed into a dword, 0 for an inactive lane.  inside: the lane's whole scanline lies in [0, raw_bytes)
// (checked once per band); a scanline that does not is read byte by byte, every byte outside the buffer as 0.
template <int BPP>
__device__ __forceinline__ uint32_t load_pixel(const uint8_t* __restrict__ raw, int64_t raw_bytes, int64_t at, bool active, bool inside)
{
    uint32_t v = 0;
    if (!active) return v;
    if (inside) {
        const uint8_t* __restrict__ p = raw + at;
#pragma unroll
        for (int i = 0; i < BPP; ++i) v |= (uint32_t)p[i] << (8 * i);
        return v;
    }
#pragma unroll
    for (int i = 0; i < BPP; ++i) {
        const int64_t a = at + i;
        const uint32_t byte = (a >= 0 && a < raw_bytes) ? raw[a] : 0u;
        v |= byte << (8 * i);
    }
    return v;
}

// the pixel of filtered bytes x with left a, above b, above-left c (PNG specification, 9.2 and 9.4), byte-wise mod 256
template <int BPP>
__device__ __forceinline__ uint32_t reconstruct(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < BPP; ++i) {
        const uint32_t xi = (x >> (8 * i)) & 0xff, ai = (a >> (8 * i)) & 0xff, bi = (b >> (8 * i)) & 0xff, ci = (c >> (8 * i)) & 0xff;
        // pa = |b - c|, pb = |a - c| (v_sad_u8 of single bytes), pc = |a + b - 2c|
        const uint32_t pa = __builtin_amdgcn_sad_u8(bi, ci, 0u), pb = __builtin_amdgcn_sad_u8(ai, ci, 0u);
        const uint32_t pc = (uint32_t)abs((int)(ai + bi) - (int)(2 * ci));
        const uint32_t paeth = (pa <= pb && pa <= pc) ? ai : (pb <= pc ? bi : ci);
        const uint32_t pred = ft == 1 ? ai : ft == 2 ? bi : ft == 3 ? (ai + bi) >> 1 : ft == 4 ? paeth : 0u;
        out |= ((xi + pred) & 0xff) << (8 * i);
    }
    return out;
}

// the reconstructed pixel v of a file with BPP channels -> the target's bytes at o (grey: BPP 1 | 2, colour: BPP 3 | 4; alpha is dropped)
template <int BPP>
__device__ __forceinline__ void store_pixel(uint8_t* __restrict__ out, int pixel, int target, uint32_t v)
{
    const uint32_t v0 = v & 0xff, v1 = (v >> 8) & 0xff, v2 = (v >> 16) & 0xff;
    if (target == kTargetRaw) {
#pragma unroll
        for (int i = 0; i < BPP; ++i) out[pixel * BPP + i] = (uint8_t)(v >> (8 * i));
    } else if (target == kTargetRgb) {
        out[pixel * 3 + 0] = (uint8_t)v0;
        out[pixel * 3 + 1] = (uint8_t)(BPP <= 2 ? v0 : v1);
        out[pixel * 3 + 2] = (uint8_t)(BPP <= 2 ? v0 : v2);
    } else {
        out[pixel] = (uint8_t)(BPP <= 2 ? v0 : (v0 * 19595u + v1 * 38470u + v2 * 7471u + 0x8000u) >> 16);
    }
}

// dynamic LDS: NW rings of ring_len dwords (ring_len a power of two: kRing, or >= W when NW == 1)
template <int BPP, int NW>
__global__ __launch_bounds__(NW * 64) void png_unfilter_kernel(const uint8_t* __restrict__ raw, int64_t raw_bytes,
                                                               const int64_t* __restrict__ offsets, int W, int H, int target, int ring_len,
                                                               uint8_t* __restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t rings[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, img = blockIdx.x;
    const int64_t base = offsets[img];
    const int64_t stride = 1 + (int64_t)W * BPP;
    const int n_bands = (H + 63) >> 6, n_chunks = (W + 63 + 63) >> 6;
    const int lag = NW == 1 ? n_chunks : 2;
    const int supersteps = (n_bands - 1) * lag + n_chunks;
    const uint32_t slot_mask = (uint32_t)ring_len - 1;
    uint32_t* mine = rings + (size_t)wave * ring_len;                        // written by lane 63 of this wave's band
    const uint32_t* above = rings + (size_t)((wave + NW - 1) % NW) * ring_len;   // written by the band above (NW == 1: the same row)

    int band = wave;                 // the band this wave works on next / now
    int row = 0;
    int64_t src = 0;                 // byte 0 of the lane's first pixel
    uint8_t* out_row = out;          // pixel 0 of the lane's row in out
    uint32_t ft = 0, a = 0, prev_b = 0, prev_out = 0;
    bool has_row = false, inside = false;
    for (int s = 0; s < supersteps; ++s) {
        const int chunk = s - band * lag;
        if (band < n_bands && chunk >= 0) {                                   // (wave-uniform)
            if (chunk == 0) {
                row = band * 64 + lane;
                has_row = row < H;
                const int64_t line = base + (int64_t)row * stride;
                ft = (has_row && line >= 0 && line < raw_bytes) ? raw[line] : 0u;
                src = line + 1;
                inside = line >= 0 && line + stride <= raw_bytes;
                const int oc = target == kTargetRgb ? 3 : target == kTargetL ? 1 : BPP;
                out_row = out + ((size_t)img * H + (has_row ? row : 0)) * W * oc;
                a = prev_b = prev_out = 0;
            }
            const int t0 = chunk * 64;
            uint32_t cur[kGroup], nxt[kGroup];
#pragma unroll
            for (int i = 0; i < kGroup; ++i) {
                const int x = t0 + i - lane;
                cur[i] = load_pixel<BPP>(raw, raw_bytes, src + (int64_t)x * BPP, has_row && x >= 0 && x < W, inside);
            }
            for (int g = 0; g < 64 / kGroup; ++g) {
                const int tg = t0 + g * kGroup;
#pragma unroll
                for (int i = 0; i < kGroup; ++i) {
                    const int x = tg + kGroup + i - lane;
                    nxt[i] = load_pixel<BPP>(raw, raw_bytes, src + (int64_t)x * BPP, g + 1 < 64 / kGroup && has_row && x >= 0 && x < W, inside);
                }
#pragma unroll
                for (int i = 0; i < kGroup; ++i) {
                    const int t = tg + i, x = t - lane;
                    const bool active = has_row && x >= 0 && x < W;
                    uint32_t b = __shfl_up(prev_out, 1);                       // every lane of the wave takes part
                    if (lane == 0) b = (band > 0 && t < W) ? above[(uint32_t)t & slot_mask] : 0u;
                    if (active) {
                        const uint32_t o = reconstruct<BPP>(ft, cur[i], a, b, prev_b);
                        a = o, prev_b = b, prev_out = o;
                        store_pixel<BPP>(out_row, x, target, o);
                        if (lane == 63) mine[(uint32_t)x & slot_mask] = o;
                    }
                }
#pragma unroll
                for (int i = 0; i < kGroup; ++i) cur[i] = nxt[i];
            }
            if (chunk == n_chunks - 1) band += NW;
        }
        __syncthreads();
    }
}

template <int BPP>
int launch_bpp(int waves, dim3 grid, size_t lds, hipStream_t s, const uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, int W, int H,
               int target, int ring_len, uint8_t* out)
{
    const char* who = "cmdiad_png_unfilter";
    switch (waves) {
    case 1: return launch_lds<png_unfilter_kernel<BPP, 1>>(who, grid, dim3(64), lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out);
    case 8: return launch_lds<png_unfilter_kernel<BPP, 8>>(who, grid, dim3(512), lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out);
    default: return launch_lds<png_unfilter_kernel<BPP, 16>>(who, grid, dim3(1024), lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out);
    }
}

}  // namespace

extern "C" int cmdiad_png_unfilter(const uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, int B, int W, int H, int bpp, int target,
                                   int waves, uint8_t* out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(raw && offsets && out, CMDIAD_ERR_ARG, "cmdiad_png_unfilter: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(W) && side_ok(H) && bpp >= 1 && bpp <= 4, CMDIAD_ERR_ARG,
                   "cmdiad_png_unfilter: bad sizes B=%d (1..65535) W=%d H=%d (sides 1..%d) bpp=%d (1..4)", B, W, H, kMaxSide, bpp);
    CMDIAD_REQUIRE(target == kTargetRgb || target == kTargetL || target == kTargetRaw, CMDIAD_ERR_ARG,
                   "cmdiad_png_unfilter: target=%d (0 rgb | 1 l | 2 raw)", target);
    CMDIAD_REQUIRE(raw_bytes >= 1, CMDIAD_ERR_ARG, "cmdiad_png_unfilter: raw_bytes=%lld must be positive", (long long)raw_bytes);
    const int n_chunks = (W + 63 + 63) >> 6;
    const int fit = 2 * 8 >= n_chunks + 2 ? 8 : 2 * 16 >= n_chunks + 2 ? 16 : 1;      // the fewest waves whose schedule holds the width
    CMDIAD_REQUIRE(waves == 0 || waves == 1 || ((waves == 8 || waves == 16) && 2 * waves >= n_chunks + 2), CMDIAD_ERR_ARG,
                   "cmdiad_png_unfilter: waves=%d (0 = chosen from the width | 1 | 8 | 16 with 2 * waves >= %d chunks + 2)", waves, n_chunks);
    if (waves == 0) waves = fit;
    int ring_len = kRing;
    if (waves == 1)
        for (ring_len = 64; ring_len < W; ring_len <<= 1) {}
    const size_t lds = (size_t)waves * ring_len * sizeof(uint32_t);
    const dim3 grid((unsigned)B);
    hipStream_t s = (hipStream_t)stream;
    int rc = CMDIAD_OK;
    switch (bpp) {
    case 1: rc = launch_bpp<1>(waves, grid, lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out); break;
    case 2: rc = launch_bpp<2>(waves, grid, lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out); break;
    case 3: rc = launch_bpp<3>(waves, grid, lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out); break;
    default: rc = launch_bpp<4>(waves, grid, lds, s, raw, raw_bytes, offsets, W, H, target, ring_len, out); break;
    }
    if (rc != CMDIAD_OK) return rc;
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

// ---------------------------------------------------------------------------------------------------------------- the writer's side
// Filtering for the encoder (utils/png.py: write_many): images [n,H,W,C] uint8 -> scanlines [n, H * (1 + W * C)], the filter byte in
// front of every row.  The sources are the UNFILTERED image, so no row or byte waits for another: one wave owns a row, lane l takes
// bytes l, l + 64, ...  Adaptive (mode 5): a first walk sums m(b) = b < 128 ? b : 256 - b of the five candidates per lane, an
// integer butterfly adds them over the wave (exact, order-free; a row is at most 64 KiB, so a sum stays below 2^23), the lowest
// type among the smallest sums wins; a second walk writes it.  A forced mode takes the second walk only.
namespace {

__device__ __forceinline__ uint32_t filt_byte(uint32_t ft, uint32_t x, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t pa = __builtin_amdgcn_sad_u8(b, c, 0u), pb = __builtin_amdgcn_sad_u8(a, c, 0u);
    const uint32_t pc = (uint32_t)abs((int)(a + b) - (int)(2 * c));
    const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    const uint32_t pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0u;
    return (x - pred) & 0xff;
}

__device__ __forceinline__ uint32_t filt_cost(uint32_t v) { return v < 128u ? v : 256u - v; }

// grid (ceil(n H / 4)), 4 waves: wave w of workgroup g takes row 4 g + w of the batch's n * H rows
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t* __restrict__ img, long long rows, int H, int rb, int C, int mode,
                                                         uint8_t* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                   // (wave-uniform; the kernel has no barrier)
    const int r = (int)(row % H);
    const uint8_t* __restrict__ cur = img + (size_t)row * rb;
    const uint8_t* __restrict__ up = cur - rb;                 // read only when r > 0
    const bool has_up = r > 0;
    uint32_t ft = (uint32_t)mode;
    if (mode == 5) {
        uint32_t cost[5] = {0u, 0u, 0u, 0u, 0u};
        for (int i = lane; i < rb; i += 64) {
            const uint32_t x = cur[i], a = i >= C ? cur[i - C] : 0u, b = has_up ? up[i] : 0u, c = (has_up && i >= C) ? up[i - C] : 0u;
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += filt_cost(filt_byte((uint32_t)t, x, a, b, c));
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
            for (int t = 0; t < 5; ++t) cost[t] += __shfl_xor(cost[t], m, 64);
        ft = 0;
        uint32_t best = cost[0];
#pragma unroll
        for (int t = 1; t < 5; ++t)
            if (cost[t] < best) best = cost[t], ft = (uint32_t)t;
    }
    uint8_t* __restrict__ o = out + (size_t)row * (1 + (size_t)rb);
    if (lane == 0) o[0] = (uint8_t)ft;
    for (int i = lane; i < rb; i += 64) {
        const uint32_t x = cur[i], a = i >= C ? cur[i - C] : 0u, b = has_up ? up[i] : 0u, c = (has_up && i >= C) ? up[i - C] : 0u;
        o[1 + i] = (uint8_t)filt_byte(ft, x, a, b, c);
    }
}

}  // namespace

extern "C" int cmdiad_png_filter(const uint8_t* images, int n, int H, int W, int C, int mode, uint8_t* scanlines, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxImages && side_ok(W) && side_ok(H) && C >= 1 && C <= 4, CMDIAD_ERR_ARG,
                   "cmdiad_png_filter: bad sizes n=%d (0..65535) W=%d H=%d (sides 1..%d) C=%d (1..4)", n, W, H, kMaxSide, C);
    CMDIAD_REQUIRE(mode >= 0 && mode <= 5, CMDIAD_ERR_ARG, "cmdiad_png_filter: mode=%d (0..4 force a filter type, 5 = adaptive)", mode);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(images && scanlines, CMDIAD_ERR_ARG, "cmdiad_png_filter: null pointer");
    const long long rows = (long long)n * H;
    hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, images, rows, H, W * C, C,
                       mode, scanlines);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
