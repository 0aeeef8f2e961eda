// Eyecandies depth maps to organised clouds on the device (utils/preprocessing_eyecandies.py:16-89 of the reference: two Python
// loops over every pixel, numpy + BLAS, one scan at a time).  The contract -- the float32 depth stage, the float64 unprojection,
// the background cut with its collapsed point, and the ORDER of every operation -- is written down in docs/eyecandies.md; this file
// is compiled with -ffp-contract=off (Makefile: EXACT) so that every written operation rounds once, and the tests compare it bit
// for bit with a numpy restatement of the same order.
//
// One kernel, one thread per pixel, three instantiations:
//   <unproject, cut>   cmdiad_eyecandies_cloud       uint16 codes -> the reference's final [H,W,3] float64 cloud (+ removed, depth)
//   <unproject, ->     cmdiad_eyecandies_unproject   uint16 codes -> depth_to_pointcloud's [H*W,3] float64 points (+ depth)
//   <-, cut>           cmdiad_eyecandies_background  [n,3] float64 points -> remove_point_cloud_background's [n,3]
// The cut needs the points at flat indices 256 and n - 256 (the reference's pc[256], pc[-256]).  Every thread derives the two
// itself: their codes and the parameter block are wave-uniform loads, the arithmetic is ~40 float64 operations, a division and a
// square root beside 27 bytes of traffic per pixel, and it keeps the whole scan in ONE launch with nothing between the stages.
// (The ISA of the three instantiations uses 36 / 16 / 26 VGPRs, no scratch and no LDS; the alternative -- a one-wave prologue writing
// the anchors to a parameter block -- adds a launch per batch and a dependency between two kernels to save those operations.)
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kMinPixels = 513;          // both anchors (256 and n - 256) exist and are distinct
constexpr int kMaxPoints = 1 << 28;      // points of a lone background cut (= kMaxSide squared)

struct P3 {
    double x, y, z;
};

// Point j of the scan: depth_to_pointcloud's row j (kUnproject), or row j of a given cloud.
template <bool kUnproject>
__device__ __forceinline__ P3 point_at(const uint16_t* __restrict__ code, const cmdiad_eyecandies_params* __restrict__ prm,
                                       const double* __restrict__ pts, int j, int W, float* d_out)
{
    if constexpr (!kUnproject) {
        const double* p = pts + (size_t)j * 3;
        return P3{p[0], p[1], p[2]};
    } else {
        // float32, three operations: / 65535, * range, + mind (load_and_convert_depth)
        const float d = (float)code[j] / 65535.0f * prm->range + prm->mind;
        if (d_out) *d_out = d;
        const double r = (double)(1.0f / d);      // a float32 quotient, widened
        const int v = j / W;
        const double uu = (double)(j - v * W), vv = (double)v, dd = (double)d;
        const double* __restrict__ m = prm->inv_p;
        const double hx = ((m[0] * uu + m[1] * vv) + m[2]) + m[3] * r;
        const double hy = ((m[4] * uu + m[5] * vv) + m[6]) + m[7] * r;
        const double hz = ((m[8] * uu + m[9] * vv) + m[10]) + m[11] * r;
        return P3{dd * hx, dd * hy, dd * hz};
    }
}

// grid (ceil(n / 256), B).  code [B,n] (kUnproject), prm [B] (kUnproject), pts [B,n,3] (!kUnproject); cloud [B,n,3],
// removed [B,n] (kCut; NULL allowed), depth [B,n] (kUnproject; NULL allowed).
template <bool kUnproject, bool kCut>
__global__ __launch_bounds__(256) void eyecandies_kernel(const uint16_t* __restrict__ code, const cmdiad_eyecandies_params* __restrict__ prm,
                                                         const double* __restrict__ pts, int n, int W, double* __restrict__ cloud,
                                                         uint8_t* __restrict__ removed, float* __restrict__ depth)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (i >= n) return;
    const size_t base = (size_t)b * n;
    if (kUnproject) code += base, prm += b;
    else pts += base * 3;
    const P3 p = point_at<kUnproject>(code, prm, pts, i, W, depth ? depth + base + i : nullptr);
    double* o = cloud ? cloud + (base + i) * 3 : nullptr;
    if constexpr (!kCut) {
        if (o) o[0] = p.x, o[1] = p.y, o[2] = p.z;
    } else {
        const P3 a = point_at<kUnproject>(code, prm, pts, 256, W, nullptr);
        const P3 e = point_at<kUnproject>(code, prm, pts, n - 256, W, nullptr);
        const double dz = a.y - e.y, dy = a.z - e.z;      // "the second dim is z"
        const double norm = sqrt(dz * dz + dy * dy);
        const double c = dy / norm, s = dz / norm, ns = -s;
        // R (pc - start), start = (0, e.y, e.z), R = [[1,0,0],[0,c,-s],[0,s,c]]
        const double t1 = p.y - e.y, t2 = p.z - e.z;
        double p0 = p.x, p1 = c * t1 + ns * t2, p2 = s * t1 + c * t2;
        const bool cut = p1 > -0.02 || p2 > 1.8 || p0 > 1.0 || p0 < -1.0;      // a NaN compares false: kept
        if (cut) p0 = -0.0, p1 = -e.y, p2 = -e.z;                              // -start, not zero
        // R^T p + start, for kept and removed points alike
        const double q0 = p0 + 0.0, q1 = (c * p1 + s * p2) + e.y, q2 = (ns * p1 + c * p2) + e.z;
        if (o) o[0] = q0 * 0.1, o[1] = q2 * -0.1, o[2] = q1 * 0.1;
        if (removed) removed[base + i] = cut ? 1 : 0;
    }
}


}  // namespace

extern "C" int cmdiad_eyecandies_cloud(const uint16_t* depth_u16, const cmdiad_eyecandies_params* params, int B, int H, int W,
                                       double* cloud_out, uint8_t* removed_out, float* depth_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(depth_u16 && params && cloud_out, CMDIAD_ERR_ARG, "cmdiad_eyecandies_cloud: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(H) && side_ok(W) && (long long)H * W >= kMinPixels, CMDIAD_ERR_ARG,
                   "cmdiad_eyecandies_cloud: bad sizes B=%d (1..65535) H=%d W=%d (sides 1..%d, H*W >= %d: the anchors are pixels 256 "
                   "and H*W-256)", B, H, W, kMaxSide, kMinPixels);
    hipLaunchKernelGGL((eyecandies_kernel<true, true>), pixel_grid(H * W, B), dim3(256), 0, (hipStream_t)stream, depth_u16, params,
                       (const double*)nullptr, H * W, W, cloud_out, removed_out, depth_out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_eyecandies_unproject(const uint16_t* depth_u16, const cmdiad_eyecandies_params* params, int B, int H, int W,
                                           double* points_out, float* depth_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(depth_u16 && params && (points_out || depth_out), CMDIAD_ERR_ARG, "cmdiad_eyecandies_unproject: null pointer");
    CMDIAD_REQUIRE(B >= 1 && B <= kMaxImages && side_ok(H) && side_ok(W), CMDIAD_ERR_ARG,
                   "cmdiad_eyecandies_unproject: bad sizes B=%d (1..65535) H=%d W=%d (sides 1..%d)", B, H, W, kMaxSide);
    hipLaunchKernelGGL((eyecandies_kernel<true, false>), pixel_grid(H * W, B), dim3(256), 0, (hipStream_t)stream, depth_u16, params,
                       (const double*)nullptr, H * W, W, points_out, (uint8_t*)nullptr, depth_out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_eyecandies_background(const double* points, int n, double* cloud_out, uint8_t* removed_out,
                                            cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(points && cloud_out, CMDIAD_ERR_ARG, "cmdiad_eyecandies_background: null pointer");
    CMDIAD_REQUIRE(n >= kMinPixels && n <= kMaxPoints, CMDIAD_ERR_ARG,
                   "cmdiad_eyecandies_background: bad sizes n=%d (%d..%d: the anchors are points 256 and n-256)", n, kMinPixels,
                   kMaxPoints);
    hipLaunchKernelGGL((eyecandies_kernel<false, true>), pixel_grid(n, 1), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)nullptr, (const cmdiad_eyecandies_params*)nullptr, points, n, 1, cloud_out, removed_out,
                       (float*)nullptr);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
