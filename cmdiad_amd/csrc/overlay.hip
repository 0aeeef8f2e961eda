// Anomaly overlays on the device (docs/overlay.md): score maps [n,H,W] f64 -> canvas [n,Ho,Wo,3] uint8 in ONE launch -- the map
// resampled to the canvas, normalised between lo and hi (device memory), sent through a 256-entry colour and alpha table, blended over
// a background, the contour of `score > thr` (thr in device memory, cmdiad_threshold_mask's convention) and the boxes of
// cmdiad_region_table's tables drawn on top.  Every floating-point step is one float64 operation in the written order (the file is
// compiled with -ffp-contract=off); everything behind k = floor(t * 255 + 0.5) is integer arithmetic.
//
// grid (ceil(Ho Wo / 1024), n), 256 lanes, a lane takes canvas pixels 4t .. 4t + 3 of its image (raster order, so a group may wrap
// to the next row).  kVec: Ho * Wo is a multiple of 4 and the canvas (and the background) aligned, so the 12 bytes of the group are
// three dword stores (the background's: three dword loads, or one 16-byte load per plane); otherwise bytes, each guarded.
// The workgroup first puts the table (packed r | g << 8 | b << 16 | a << 24) and its image's boxes, converted to canvas pixels and
// clamped, into LDS.  The contour's four neighbours are sampled again from the map (L2), not staged.  Reads: a tap of weight 0 is
// not read; every tap index is clamped to the map; the tables are read below min(count, K) only.  Writes: canvas pixels below
// Ho * Wo of the image, and one atomic add per wave that met a NaN.
#include "frames.h"
#include "launch.h"
#include "overlay_color.h"   // steps 2 and 3, shared with mesh.hip

namespace {

constexpr int kMaxBoxes = 64;
constexpr int kMaxLine = 8;

struct OverlayArgs {
    const double* maps;
    const double* lohi;
    const double* thr;          // null: no contour
    const void* bg;
    const uint8_t* lut;
    const uint8_t* alpha;
    const int32_t* count;       // null: no boxes
    const int32_t* ints;
    uint8_t* canvas;
    int32_t* nan_count;
    double sx, sy;              // W / Wo, H / Ho: divided once, on the host (IEEE division, as the device's)
    double mean[3], stdv[3];
    int H, W, Ho, Wo;
    int lohi_per_image, thr_per_image, bg_kind, K, line_px;
    uint32_t contour_rgb, box_rgb;
};

struct Axis { int i0, i1; double f; };

// canvas coordinate c of an axis with `size` map pixels -> the two taps and the weight of the second
__device__ __forceinline__ Axis axis_of(int c, double scale, int size)
{
    double u = ((double)c + 0.5) * scale;
    u = u - 0.5;
    const double top = (double)(size - 1);
    u = u < 0.0 ? 0.0 : u;
    u = u > top ? top : u;
    const double fl = floor(u);
    Axis a;
    a.i0 = (int)fl;
    a.i1 = min(a.i0 + 1, size - 1);
    a.f = u - fl;
    return a;
}

__device__ __forceinline__ double row_of(const double* __restrict__ row, const Axis& ax)
{
    double v = row[ax.i0] * (1.0 - ax.f);
    if (ax.f != 0.0) v = v + row[ax.i1] * ax.f;
    return v;
}

__device__ __forceinline__ double score_at(const double* __restrict__ m, int x, int y, const OverlayArgs& A)
{
    const Axis ax = axis_of(x, A.sx, A.W), ay = axis_of(y, A.sy, A.H);
    double s = row_of(m + (size_t)ay.i0 * A.W, ax) * (1.0 - ay.f);
    if (ay.f != 0.0) s = s + row_of(m + (size_t)ay.i1 * A.W, ax) * ay.f;
    return s;
}

template <bool kVec>
__global__ __launch_bounds__(256) void overlay_render_kernel(OverlayArgs A)
{
    __shared__ uint32_t sh_lut[256];
    __shared__ int sh_box[kMaxBoxes * 4];
    __shared__ int sh_boxes;
    const int tid = threadIdx.x, img = blockIdx.y;
    const int HoWo = A.Ho * A.Wo;
    sh_lut[tid] = (uint32_t)A.lut[tid * 3] | (uint32_t)A.lut[tid * 3 + 1] << 8 | (uint32_t)A.lut[tid * 3 + 2] << 16 | (uint32_t)A.alpha[tid] << 24;
    int boxes = 0;
    if (A.count) {
        boxes = A.count[img];
        boxes = boxes < 0 ? 0 : boxes > A.K ? A.K : boxes;
        if (tid < boxes) {
            const int32_t* e = A.ints + ((size_t)img * A.K + tid) * 8;
            const long long x0 = e[2], y0 = e[3], x1 = e[4], y1 = e[5];
            long long X0 = x0 * A.Wo / A.W, X1 = ((x1 + 1) * A.Wo + A.W - 1) / A.W - 1;
            long long Y0 = y0 * A.Ho / A.H, Y1 = ((y1 + 1) * A.Ho + A.H - 1) / A.H - 1;
            X0 = X0 < 0 ? 0 : X0, Y0 = Y0 < 0 ? 0 : Y0;
            X1 = X1 > A.Wo - 1 ? A.Wo - 1 : X1, Y1 = Y1 > A.Ho - 1 ? A.Ho - 1 : Y1;
            X1 = X1 < -1 ? -1 : X1, Y1 = Y1 < -1 ? -1 : Y1;      // (an empty box stays empty; the values fit an int)
            X0 = X0 > A.Wo ? A.Wo : X0, Y0 = Y0 > A.Ho ? A.Ho : Y0;
            sh_box[tid * 4 + 0] = (int)X0, sh_box[tid * 4 + 1] = (int)Y0, sh_box[tid * 4 + 2] = (int)X1, sh_box[tid * 4 + 3] = (int)Y1;
        }
    }
    if (tid == 0) sh_boxes = boxes;
    __syncthreads();
    boxes = sh_boxes;

    const int p0 = (blockIdx.x * 256 + tid) * 4;
    const double* __restrict__ m = A.maps + (size_t)img * A.H * A.W;
    const double lo = A.lohi[A.lohi_per_image ? 2 * img : 0], hi = A.lohi[A.lohi_per_image ? 2 * img + 1 : 1];
    const double d = hi - lo;
    const bool contour = A.thr != nullptr;
    const double thr = contour ? A.thr[A.thr_per_image ? img : 0] : 0.0;
    const size_t cbase = (size_t)img * HoWo * 3;

    // the background's bytes of the four pixels, r | g << 8 | b << 16
    uint32_t bgc[4] = {0u, 0u, 0u, 0u};
    if (A.bg_kind == kBgU8) {
        const uint8_t* __restrict__ b = (const uint8_t*)A.bg + cbase + (size_t)p0 * 3;
        if (kVec) {
            if (p0 < HoWo) {
                const uint32_t* __restrict__ w = reinterpret_cast<const uint32_t*>(b);
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
                bgc[0] = w0 & 0xffffffu, bgc[1] = (w0 >> 24 | w1 << 8) & 0xffffffu, bgc[2] = (w1 >> 16 | w2 << 16) & 0xffffffu, bgc[3] = w2 >> 8;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (p0 + k < HoWo) bgc[k] = (uint32_t)b[k * 3] | (uint32_t)b[k * 3 + 1] << 8 | (uint32_t)b[k * 3 + 2] << 16;
        }
    } else if (A.bg_kind == kBgF32) {
        const float* __restrict__ b = (const float*)A.bg + (size_t)img * 3 * HoWo + p0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (kVec) {
                if (p0 < HoWo) {
                    const float4 q = *reinterpret_cast<const float4*>(b + (size_t)c * HoWo);
                    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p0 + k < HoWo) v[k] = b[(size_t)c * HoWo + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) bgc[k] |= bg_byte(v[k], A.mean[c], A.stdv[c]) << (8 * c);
        }
    }

    uint32_t px[4];
    int xs[4], ys[4];
    int bad = 0;
    int y = p0 / A.Wo, x = p0 - y * A.Wo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = 0u;
        if (p0 + k < HoWo) {
            const double s = score_at(m, x, y, A);
            bool nan;
            const int kk = overlay_index(s, lo, d, nan);
            bad += nan;
            const uint32_t e = sh_lut[kk & 255];
            uint32_t c = e & 0xffffffu;
            if (A.bg_kind != kBgNone) c = blend_rgb(e, bgc[k]);
            if (contour && s > thr) {
                // the four samples do not wait for each other: a neighbour outside the canvas is sampled at the clamped
                // coordinate (a read inside the map) and then left out
                const double sl = score_at(m, max(x - 1, 0), y, A), sr = score_at(m, min(x + 1, A.Wo - 1), y, A);
                const double su = score_at(m, x, max(y - 1, 0), A), sd = score_at(m, x, min(y + 1, A.Ho - 1), A);
                const bool edge = ((x > 0) & !(sl > thr)) | ((x + 1 < A.Wo) & !(sr > thr)) | ((y > 0) & !(su > thr)) | ((y + 1 < A.Ho) & !(sd > thr));
                if (edge) c = A.contour_rgb;
            }
            px[k] = c;
        }
        xs[k] = x, ys[k] = y;
        if (++x == A.Wo) x = 0, ++y;
    }
    // boxes over everything else: a box is read from LDS once for the lane's four pixels (pixels past the image are not stored)
    for (int j = 0; j < boxes; ++j) {
        const int X0 = sh_box[j * 4], Y0 = sh_box[j * 4 + 1], X1 = sh_box[j * 4 + 2], Y1 = sh_box[j * 4 + 3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = xs[k], qy = ys[k];
            if (qx >= X0 && qx <= X1 && qy >= Y0 && qy <= Y1 && min(min(qx - X0, X1 - qx), min(qy - Y0, Y1 - qy)) < A.line_px) px[k] = A.box_rgb;
        }
    }

    uint8_t* __restrict__ o = A.canvas + cbase + (size_t)p0 * 3;
    if (kVec) {
        if (p0 < HoWo) {
            uint32_t* __restrict__ w = reinterpret_cast<uint32_t*>(o);
            w[0] = px[0] | px[1] << 24;
            w[1] = px[1] >> 8 | px[2] << 16;
            w[2] = px[2] >> 16 | px[3] << 8;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < HoWo) o[k * 3] = (uint8_t)px[k], o[k * 3 + 1] = (uint8_t)(px[k] >> 8), o[k * 3 + 2] = (uint8_t)(px[k] >> 16);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) bad += __shfl_xor(bad, s, 64);
    if (A.nan_count && bad && (tid & 63) == 0) atomicAdd(A.nan_count, bad);
}

}  // namespace

extern "C" int cmdiad_overlay_render(const double* maps, int n, int H, int W, int Ho, int Wo, const double* lohi, int lohi_per_image,
                                     const double* thr, int thr_per_image, const void* bg, int bg_kind, double mean_r, double mean_g,
                                     double mean_b, double std_r, double std_g, double std_b, const uint8_t* lut, const uint8_t* alpha,
                                     const int32_t* count, const int32_t* ints, int K, int line_px, uint32_t contour_rgb, uint32_t box_rgb,
                                     uint8_t* canvas, int32_t* nan_count, cmdiad_stream_t stream)
{
    const bool sides = side_ok(H) && side_ok(W) && side_ok(Ho) && side_ok(Wo);
    CMDIAD_REQUIRE(sides && n >= 0 && n <= kMaxImages && (long long)n * H * W <= kMaxTotal && (long long)n * Ho * Wo <= kMaxTotal,
                   CMDIAD_ERR_ARG, "cmdiad_overlay_render: bad sizes n=%d (0..%d) H=%d W=%d Ho=%d Wo=%d (sides 1..%d, n*H*W and n*Ho*Wo <= %d)",
                   n, kMaxImages, H, W, Ho, Wo, kMaxSide, kMaxTotal);
    CMDIAD_REQUIRE((lohi_per_image == 0 || lohi_per_image == 1) && (thr_per_image == 0 || thr_per_image == 1), CMDIAD_ERR_ARG,
                   "cmdiad_overlay_render: lohi_per_image=%d thr_per_image=%d (0 | 1)", lohi_per_image, thr_per_image);
    CMDIAD_REQUIRE(bg_kind == kBgNone || bg_kind == kBgU8 || bg_kind == kBgF32, CMDIAD_ERR_ARG,
                   "cmdiad_overlay_render: background kind %d (0 none | 1 uint8 [n,Ho,Wo,3] | 2 float32 [n,3,Ho,Wo])", bg_kind);
    CMDIAD_REQUIRE(K >= 1 && K <= kMaxBoxes && line_px >= 1 && line_px <= kMaxLine, CMDIAD_ERR_ARG,
                   "cmdiad_overlay_render: K=%d (1..%d) line_px=%d (1..%d)", K, kMaxBoxes, line_px, kMaxLine);
    hipStream_t s = (hipStream_t)stream;
    if (nan_count) CMDIAD_CHECK_HIP("cmdiad_overlay_render", hipMemsetAsync(nan_count, 0, sizeof(int32_t), s));
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(maps && lohi && lut && alpha && canvas && (bg_kind == kBgNone || bg) && (count == nullptr) == (ints == nullptr),
                   CMDIAD_ERR_ARG, "cmdiad_overlay_render: null pointer (maps, lohi, lut, alpha, canvas; bg with a background kind; count and "
                   "ints come together)");
    OverlayArgs A;
    A.maps = maps, A.lohi = lohi, A.thr = thr, A.bg = bg, A.lut = lut, A.alpha = alpha, A.count = count, A.ints = ints;
    A.canvas = canvas, A.nan_count = nan_count;
    A.sx = (double)W / (double)Wo, A.sy = (double)H / (double)Ho;
    A.mean[0] = mean_r, A.mean[1] = mean_g, A.mean[2] = mean_b, A.stdv[0] = std_r, A.stdv[1] = std_g, A.stdv[2] = std_b;
    A.H = H, A.W = W, A.Ho = Ho, A.Wo = Wo;
    A.lohi_per_image = lohi_per_image, A.thr_per_image = thr_per_image, A.bg_kind = bg_kind, A.K = K, A.line_px = line_px;
    A.contour_rgb = contour_rgb & 0xffffffu, A.box_rgb = box_rgb & 0xffffffu;
    const int HoWo = Ho * Wo;
    const bool bg_ok = bg_kind == kBgNone || ((uintptr_t)bg & (bg_kind == kBgU8 ? 3 : 15)) == 0;
    const bool vec = HoWo % 4 == 0 && ((uintptr_t)canvas & 3) == 0 && bg_ok;
    const dim3 grid((unsigned)((HoWo + 1023) / 1024), (unsigned)n);
    if (vec) hipLaunchKernelGGL(overlay_render_kernel<true>, grid, dim3(256), 0, s, A);
    else hipLaunchKernelGGL(overlay_render_kernel<false>, grid, dim3(256), 0, s, A);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
