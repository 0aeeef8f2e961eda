// Sample preparation on the device (dataset.py:62-65, 103-113, 168-171, 225-244 of the reference: PIL + torchvision + numpy on
// DataLoader workers, one sample at a time).  Decoded arrays in, the tensors of the reference's __getitem__ out.  The contract --
// Pillow's 8-bit bicubic arithmetic, the two nearest rules -- is written down in docs/sample_prep.md; every table of indices and
// coefficients is computed on the HOST (cmdiad_amd/dataset.py, float64 as Pillow does) and the kernels below do integer arithmetic
// and table look-ups only, so nothing here depends on how a compiler rounds.
//
// cmdiad_resize_bicubic_u8: Image.resize((ow, oh), BICUBIC) of a batch of equal-sized uint8 [H,W,3] images, then ToTensor +
//   Normalize through a [3][256] float table.  Horizontal pass into an 8-BIT intermediate [B,H,ow,3] (rounded and clamped: that
//   rounding is part of Pillow's result), then the vertical pass; a pass whose size does not change is skipped, as in Pillow.
//   The intermediate is a global scratch image of the caller, not an LDS tile: a tile of r output rows needs r * scale + 2 * support
//   intermediate rows (800 -> 224: 72 rows of 672 bytes for r = 16, 47 KiB, so 3 workgroups per CU) and recomputes the 2 * support
//   halo rows of every tile (+25 % of the horizontal pass), to save 0.5 MB of write + read per sample that stay in the 4 MiB L2 of
//   the XCD anyway -- against 1.9 MB of image and 7.7 MB of point cloud that have to come from HBM whatever the kernel does.
// cmdiad_organized_pc_prep[_f64]: nearest-resized cloud [B,3,xs,xs] (rows / columns from host tables: torch's mode='nearest' rule), the
//   z channel three times [B,3,ds,ds], and the number of resized pixels with three non-zero coordinates (wave ballot + one vector
//   atomic per wave).
// cmdiad_gt_mask_prep: Pillow NEAREST through host tables, then (v / 255 > 0.5) == (v >= 128) -> 1.0 / 0.0.
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kPrecisionBits = 22;   // Pillow's PRECISION_BITS for 8-bit channels (32 - 8 - 2)

__device__ __forceinline__ uint8_t clip8(int acc)
{
    const int v = acc >> kPrecisionBits;   // arithmetic shift, as Pillow's clip8 (negative sums clamp to 0)
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One pass of ImagingResample on [B,sh,sw,3] -> [B,dh,dw,3]: kVert ? (dw == sw, window along y) : (dh == sh, window along x).
// coef [n_out, ksize] int32, bounds [n_out, 2] int32 = (first source index, number of taps).  A window is clamped to the source
// and to ksize: a wrong table gives wrong pixels, never a read outside the image.  dst_u8 / dst_f32 [B,3,dh,dw] may be NULL.
template <bool kVert>
__global__ __launch_bounds__(256) void resample_pass_kernel(const uint8_t* __restrict__ src, int sh, int sw, int dh, int dw,
                                                            const int32_t* __restrict__ coef, const int32_t* __restrict__ bounds,
                                                            int ksize, uint8_t* __restrict__ dst_u8, float* __restrict__ dst_f32,
                                                            const float* __restrict__ norm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= dh * dw) return;
    const int b = blockIdx.y, y = i / dw, x = i - y * dw;
    const int pos = kVert ? y : x, span = kVert ? sh : sw;
    int lo = bounds[2 * pos], n = bounds[2 * pos + 1];
    lo = min(max(lo, 0), span);
    n = min(min(n, ksize), span - lo);
    const int32_t* __restrict__ k = coef + (size_t)pos * ksize;
    const uint8_t* __restrict__ p = src + (((size_t)b * sh + (kVert ? lo : y)) * sw + (kVert ? x : lo)) * 3;
    const size_t step = kVert ? (size_t)sw * 3 : 3;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0;
    for (int t = 0; t < n; ++t, p += step) {
        const int w = k[t];
        a0 += (int)p[0] * w, a1 += (int)p[1] * w, a2 += (int)p[2] * w;
    }
    const uint8_t v0 = clip8(a0), v1 = clip8(a1), v2 = clip8(a2);
    if (dst_u8) {
        uint8_t* o = dst_u8 + ((size_t)b * dh * dw + i) * 3;
        o[0] = v0, o[1] = v1, o[2] = v2;
    }
    if (dst_f32) {
        float* o = dst_f32 + (size_t)b * 3 * dh * dw + i;
        o[0] = norm[v0], o[(size_t)dh * dw] = norm[256 + v1], o[2 * (size_t)dh * dw] = norm[512 + v2];
    }
}

// neither side changes: Pillow returns a copy; ToTensor + Normalize only
__global__ __launch_bounds__(256) void normalize_u8_kernel(const uint8_t* __restrict__ src, int hw, uint8_t* __restrict__ dst_u8,
                                                           float* __restrict__ dst_f32, const float* __restrict__ norm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= hw) return;
    const uint8_t* p = src + ((size_t)blockIdx.y * hw + i) * 3;
    const uint8_t v0 = p[0], v1 = p[1], v2 = p[2];
    if (dst_u8) {
        uint8_t* o = dst_u8 + ((size_t)blockIdx.y * hw + i) * 3;
        o[0] = v0, o[1] = v1, o[2] = v2;
    }
    if (dst_f32) {
        float* o = dst_f32 + (size_t)blockIdx.y * 3 * hw + i;
        o[0] = norm[v0], o[hw] = norm[256 + v1], o[2 * (size_t)hw] = norm[512 + v2];
    }
}

__device__ __forceinline__ int clamp_index(int v, int n) { return min(max(v, 0), n - 1); }

// T = float or double (cmdiad_organized_pc_prep_f64): a double is converted at the gather, round to nearest, as torch's .float()
template <class T>
__global__ __launch_bounds__(256) void cloud_resize_kernel(const T* __restrict__ pc, int H, int W, const int32_t* __restrict__ rows,
                                                           const int32_t* __restrict__ cols, int S, float* __restrict__ out,
                                                           int32_t* __restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    bool valid = false;
    if (i < S * S) {
        const int y = i / S, x = i - y * S;
        const T* p = pc + (((size_t)b * H + clamp_index(rows[y], H)) * W + clamp_index(cols[x], W)) * 3;
        const float px = (float)p[0], py = (float)p[1], pz = (float)p[2];
        float* o = out + (size_t)b * 3 * S * S + i;
        o[0] = px, o[(size_t)S * S] = py, o[2 * (size_t)S * S] = pz;
        valid = px != 0.0f && py != 0.0f && pz != 0.0f;   // numpy's all(p != 0): a NaN coordinate counts, -0.0 does not
    }
    const unsigned long long m = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&count[b], __popcll(m));
}

template <class T>
__global__ __launch_bounds__(256) void depth3_resize_kernel(const T* __restrict__ pc, int H, int W, const int32_t* __restrict__ rows,
                                                            const int32_t* __restrict__ cols, int S, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= S * S) return;
    const int y = i / S, x = i - y * S;
    const float z = (float)pc[(((size_t)b * H + clamp_index(rows[y], H)) * W + clamp_index(cols[x], W)) * 3 + 2];
    float* o = out + (size_t)b * 3 * S * S + i;
    o[0] = z, o[(size_t)S * S] = z, o[2 * (size_t)S * S] = z;
}

__global__ __launch_bounds__(256) void gt_mask_kernel(const uint8_t* __restrict__ gt, int H, int W, const int32_t* __restrict__ rows,
                                                      const int32_t* __restrict__ cols, int S, float* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= S * S) return;
    const int y = i / S, x = i - y * S;
    const uint8_t v = gt[((size_t)b * H + clamp_index(rows[y], H)) * W + clamp_index(cols[x], W)];
    out[(size_t)b * S * S + i] = v >= 128 ? 1.0f : 0.0f;   // float32 v / 255 > 0.5 exactly for v >= 128
}

}  // namespace

extern "C" int cmdiad_resize_bicubic_u8(const uint8_t* src, int B, int H, int W, int out_h, int out_w, const int32_t* hcoef,
                                        const int32_t* hbounds, int hksize, const int32_t* vcoef, const int32_t* vbounds, int vksize,
                                        uint8_t* tmp, const float* norm, uint8_t* out_u8, float* out_f32, cmdiad_stream_t stream)
{
    const bool horiz = W != out_w, vert = H != out_h;
    CMDIAD_REQUIRE(src && (out_u8 || out_f32) && (norm || !out_f32), CMDIAD_ERR_ARG, "cmdiad_resize_bicubic_u8: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(H) && side_ok(W) && side_ok(out_h) && side_ok(out_w), CMDIAD_ERR_ARG,
                   "cmdiad_resize_bicubic_u8: bad sizes B=%d (1..65535) %dx%d -> %dx%d (sides 1..%d)", B, H, W, out_h, out_w, kMaxSide);
    CMDIAD_REQUIRE((!horiz || (hcoef && hbounds)) && (!vert || (vcoef && vbounds)) && (!(horiz && vert) || tmp), CMDIAD_ERR_ARG,
                   "cmdiad_resize_bicubic_u8: null pointer (the tables of a pass that changes a side, tmp when both do)");
    CMDIAD_REQUIRE((!horiz || (hksize >= 1 && hksize <= 2 * kMaxSide)) && (!vert || (vksize >= 1 && vksize <= 2 * kMaxSide)),
                   CMDIAD_ERR_ARG, "cmdiad_resize_bicubic_u8: bad sizes hksize=%d vksize=%d", hksize, vksize);
    hipStream_t s = (hipStream_t)stream;
    if (!horiz && !vert) {
        hipLaunchKernelGGL(normalize_u8_kernel, pixel_grid(H * W, B), dim3(256), 0, s, src, H * W, out_u8, out_f32, norm);
        CMDIAD_CHECK_LAUNCH();
        return CMDIAD_OK;
    }
    const uint8_t* vsrc = src;
    if (horiz) {
        hipLaunchKernelGGL(resample_pass_kernel<false>, pixel_grid(H * out_w, B), dim3(256), 0, s, src, H, W, H, out_w, hcoef, hbounds,
                           hksize, vert ? tmp : out_u8, vert ? (float*)nullptr : out_f32, norm);
        CMDIAD_CHECK_LAUNCH();
        vsrc = tmp;
    }
    if (vert) {
        hipLaunchKernelGGL(resample_pass_kernel<true>, pixel_grid(out_h * out_w, B), dim3(256), 0, s, vsrc, H, out_w, out_h, out_w,
                           vcoef, vbounds, vksize, out_u8, out_f32, norm);
        CMDIAD_CHECK_LAUNCH();
    }
    return CMDIAD_OK;
}

namespace {

template <class T>
int organized_pc_prep(const char* who, const T* pc, int B, int H, int W, const int32_t* xyz_rows, const int32_t* xyz_cols, int xyz_size,
                      const int32_t* depth_rows, const int32_t* depth_cols, int depth_size, float* cloud_out, float* depth_out,
                      int32_t* count_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(pc && xyz_rows && xyz_cols && cloud_out && count_out && (!depth_out || (depth_rows && depth_cols)), CMDIAD_ERR_ARG,
                   "%s: null pointer", who);
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(H) && side_ok(W) && side_ok(xyz_size) && (!depth_out || side_ok(depth_size)),
                   CMDIAD_ERR_ARG, "%s: bad sizes B=%d (1..65535) H=%d W=%d xyz_size=%d depth_size=%d (1..%d)", who, B, H, W, xyz_size,
                   depth_size, kMaxSide);
    hipStream_t s = (hipStream_t)stream;
    CMDIAD_CHECK_HIP(who, hipMemsetAsync(count_out, 0, (size_t)B * sizeof(int32_t), s));
    hipLaunchKernelGGL(cloud_resize_kernel<T>, pixel_grid(xyz_size * xyz_size, B), dim3(256), 0, s, pc, H, W, xyz_rows, xyz_cols,
                       xyz_size, cloud_out, count_out);
    CMDIAD_CHECK_LAUNCH();
    if (depth_out) {
        hipLaunchKernelGGL(depth3_resize_kernel<T>, pixel_grid(depth_size * depth_size, B), dim3(256), 0, s, pc, H, W, depth_rows,
                           depth_cols, depth_size, depth_out);
        CMDIAD_CHECK_LAUNCH();
    }
    return CMDIAD_OK;
}

}  // namespace

extern "C" int cmdiad_organized_pc_prep(const float* pc, int B, int H, int W, const int32_t* xyz_rows, const int32_t* xyz_cols,
                                        int xyz_size, const int32_t* depth_rows, const int32_t* depth_cols, int depth_size,
                                        float* cloud_out, float* depth_out, int32_t* count_out, cmdiad_stream_t stream)
{
    return organized_pc_prep("cmdiad_organized_pc_prep", pc, B, H, W, xyz_rows, xyz_cols, xyz_size, depth_rows, depth_cols, depth_size,
                             cloud_out, depth_out, count_out, stream);
}

extern "C" int cmdiad_organized_pc_prep_f64(const double* pc, int B, int H, int W, const int32_t* xyz_rows, const int32_t* xyz_cols,
                                            int xyz_size, const int32_t* depth_rows, const int32_t* depth_cols, int depth_size,
                                            float* cloud_out, float* depth_out, int32_t* count_out, cmdiad_stream_t stream)
{
    return organized_pc_prep("cmdiad_organized_pc_prep_f64", pc, B, H, W, xyz_rows, xyz_cols, xyz_size, depth_rows, depth_cols,
                             depth_size, cloud_out, depth_out, count_out, stream);
}

extern "C" int cmdiad_gt_mask_prep(const uint8_t* gt, int B, int H, int W, const int32_t* rows, const int32_t* cols, int gt_size,
                                   float* out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(gt && rows && cols && out, CMDIAD_ERR_ARG, "cmdiad_gt_mask_prep: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(H) && side_ok(W) && side_ok(gt_size), CMDIAD_ERR_ARG,
                   "cmdiad_gt_mask_prep: bad sizes B=%d (1..65535) H=%d W=%d gt_size=%d (1..%d)", B, H, W, gt_size, kMaxSide);
    hipLaunchKernelGGL(gt_mask_kernel, pixel_grid(gt_size * gt_size, B), dim3(256), 0, (hipStream_t)stream, gt, H, W, rows, cols,
                       gt_size, out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
