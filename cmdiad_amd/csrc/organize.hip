// Unordered point clouds into the pixel grid (docs/organize.md): the inverse of cmdiad_unorganize.  points [P,3] float32, the clouds
// of a batch back to back behind offsets [n+1] int64, one camera per cloud (cams [n,16] f64: a row-major 3 x 4 transform T, then
// a, b, c, d) -> per pixel of an H x W grid the nearest point that projects into it.
//   c_k = ((T[k][0] x + T[k][1] y) + T[k][2] z) + T[k][3]
//   orthographic (kind 0): u = (c0 - x0) sx, v = (c1 - y0) sy;  pinhole (kind 1): u = fx (c0 / c2) + cx, v = fy (c1 / c2) + cy, c2 > 0
//   uf = floor(u + 0.5), vf = floor(v + 0.5), inside iff 0 <= uf < W and 0 <= vf < H (as doubles) and (float)c2 is finite
//   key = f2ord((float)c2, -0.0 -> +0.0) << 32 | (i - lo_b)
// Every floating-point step is one float64 operation in the written order (the file is compiled with -ffp-contract=off).  The only
// atomics are a 64-bit integer minimum on the key map and 32-bit integer adds on the counts, one per workgroup: the result does not
// depend on scheduling.
//   bounds_init / bounds / bounds_final   cmdiad_cloud_bounds: per cloud the min and max of c_0..c_2 over the valid points, held as
//                       ordered 64-bit keys in the output itself between the launches, and their count
//   splat_init          keys = all ones, stats columns 0 and 1 = 0
//   splat               grid (ceil(max_len / 256), n), one point per lane: pixel_of_point, the atomic minimum, dropped / outside
//   resolve             grid (ceil(H W / 256), n), one pixel per lane: the direct hit or the minimum direct key of the fill window;
//                       index, xyz, rgb, mask, direct / filled
// Reads: offsets[0..n], cams below 16 n, points / colors / labels of i in [lo_b, hi_b) only -- both ends clamped to [0, P], and a
// key whose index does not lie in the cloud is an empty pixel.  Writes: pixel_of_point of those i; keys, index, xyz, rgb, mask below
// n H W; stats [n,4]; nothing else.
#include "block_scan.h"
#include "cloud.h"
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kBoundsPts = 2048;                  // points of a workgroup of bounds_kernel: 256 lanes x 8
constexpr unsigned long long kEmpty = ~0ull;

struct Range { long long lo, hi; };

// the cloud's points [lo, hi): whatever the table holds, 0 <= lo <= hi <= P
__device__ __forceinline__ Range cloud_range(const long long* __restrict__ offsets, int b, int P)
{
    long long lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > P ? P : lo);
    hi = hi < lo ? lo : (hi > P ? P : hi);
    return {lo, hi};
}

struct Cam { double t[12], a, b, c, d; };

__device__ __forceinline__ Cam load_cam(const double* __restrict__ cams, int b)
{
    Cam m;
    const double* __restrict__ r = cams + (size_t)b * 16;
#pragma unroll
    for (int k = 0; k < 12; ++k) m.t[k] = r[k];
    m.a = r[12], m.b = r[13], m.c = r[14], m.d = r[15];
    return m;
}

__device__ __forceinline__ double cam_coord(const Cam& m, int k, double x, double y, double z)
{
    return ((m.t[4 * k] * x + m.t[4 * k + 1] * y) + m.t[4 * k + 2] * z) + m.t[4 * k + 3];
}

// ---------------------------------------------------------------------------------------------------------------- bounds
__global__ __launch_bounds__(256) void bounds_init_kernel(unsigned long long* __restrict__ slots, int32_t* __restrict__ count, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n * 6) slots[j] = d2ord(j % 6 < 3 ? (double)INFINITY : -(double)INFINITY);
    if (j < n) count[j] = 0;
}

// grid (ceil(max_len / kBoundsPts), n).  A NaN c_k is in neither its minimum nor its maximum; a zero of either sign is +0.0.
__global__ __launch_bounds__(256) void bounds_kernel(const float* __restrict__ pts, const long long* __restrict__ offsets,
                                                     const double* __restrict__ cams, int P, int max_len,
                                                     unsigned long long* __restrict__ slots, int32_t* __restrict__ count)
{
    __shared__ double sh_lo[4][3], sh_hi[4][3];
    __shared__ int sh_n[4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Range r = cloud_range(offsets, b, P);
    const long long len = r.hi - r.lo < max_len ? r.hi - r.lo : max_len;
    const Cam m = load_cam(cams, b);
    double lo[3] = {(double)INFINITY, (double)INFINITY, (double)INFINITY}, hi[3] = {-(double)INFINITY, -(double)INFINITY, -(double)INFINITY};
    int cnt = 0;
    const long long first = (long long)blockIdx.x * kBoundsPts + tid;
#pragma unroll 2
    for (int j = 0; j < kBoundsPts / 256; ++j) {
        const long long local = first + j * 256;
        if (local < len) {
            const float* __restrict__ q = pts + (r.lo + local) * 3;
            const Pt p = {q[0], q[1], q[2]};
            if (valid_pt(p)) {
                ++cnt;
                const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    double c = cam_coord(m, k, x, y, z);
                    if (c == 0.0) c = 0.0;
                    if (c < lo[k]) lo[k] = c;
                    if (c > hi[k]) hi[k] = c;
                }
            }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double ol = __shfl_xor(lo[k], s, 64), oh = __shfl_xor(hi[k], s, 64);
            if (ol < lo[k]) lo[k] = ol;
            if (oh > hi[k]) hi[k] = oh;
        }
        cnt += __shfl_xor(cnt, s, 64);
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) sh_lo[tid >> 6][k] = lo[k], sh_hi[tid >> 6][k] = hi[k];
        sh_n[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid < 3) {
        double l = sh_lo[0][tid], h = sh_hi[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            if (sh_lo[w][tid] < l) l = sh_lo[w][tid];
            if (sh_hi[w][tid] > h) h = sh_hi[w][tid];
        }
        if (l <= h) {
            atomicMin(slots + (size_t)b * 6 + tid, d2ord(l));
            atomicMax(slots + (size_t)b * 6 + 3 + tid, d2ord(h));
        }
    }
    if (tid == 0) {
        const int t = (sh_n[0] + sh_n[1]) + (sh_n[2] + sh_n[3]);
        if (t) atomicAdd(count + b, t);
    }
}

// the ordered keys back to doubles, each slot in place
__global__ __launch_bounds__(256) void bounds_final_kernel(unsigned long long* __restrict__ slots, int n)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n * 6) reinterpret_cast<double*>(slots)[j] = ord2d(slots[j]);
}

// ---------------------------------------------------------------------------------------------------------------- splat
// stats [n,4]: columns col, col + 1 = 0
__global__ __launch_bounds__(256) void zero_stats_kernel(int32_t* __restrict__ stats, int n, int col)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) stats[(size_t)j * 4 + col] = 0, stats[(size_t)j * 4 + col + 1] = 0;
}

__global__ __launch_bounds__(256) void splat_init_kernel(unsigned long long* __restrict__ keys, long long total, int32_t* __restrict__ stats, int n)
{
    const long long j0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    for (long long j = j0; j < total; j += step) keys[j] = kEmpty;
    if (j0 < n) stats[j0 * 4] = 0, stats[j0 * 4 + 1] = 0;
}

// grid (ceil(max_len / 256), n)
template <int kKind>
__global__ __launch_bounds__(256) void splat_kernel(const float* __restrict__ pts, const long long* __restrict__ offsets,
                                                    const double* __restrict__ cams, int P, int max_len, int H, int W,
                                                    unsigned long long* __restrict__ keys, int32_t* __restrict__ pixel_of_point,
                                                    int32_t* __restrict__ stats)
{
    __shared__ int sh[2][4];
    const int tid = threadIdx.x, b = blockIdx.y;
    const Range r = cloud_range(offsets, b, P);
    const long long len = r.hi - r.lo < max_len ? r.hi - r.lo : max_len;
    const long long local = (long long)blockIdx.x * 256 + tid;
    int dropped = 0, outside = 0;
    if (local < len) {
        const long long i = r.lo + local;
        const float* __restrict__ q = pts + i * 3;
        const Pt p = {q[0], q[1], q[2]};
        int pix;
        if (!valid_pt(p)) {
            pix = -2, dropped = 1;
        } else {
            const Cam m = load_cam(cams, b);
            const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
            const double c0 = cam_coord(m, 0, x, y, z), c1 = cam_coord(m, 1, x, y, z), c2 = cam_coord(m, 2, x, y, z);
            double u, v;
            bool inside = true;
            if (kKind == 0) {
                u = (c0 - m.a) * m.c;
                v = (c1 - m.b) * m.d;
            } else {
                u = m.a * (c0 / c2) + m.c;
                v = m.b * (c1 / c2) + m.d;
                inside = c2 > 0.0;
            }
            const double uf = floor(u + 0.5), vf = floor(v + 0.5);
            float d32 = (float)c2;
            if (d32 == 0.f) d32 = 0.f;
            inside = inside && uf >= 0.0 && uf < (double)W && vf >= 0.0 && vf < (double)H && fabsf(d32) < INFINITY;
            if (!inside) {
                pix = -1, outside = 1;
            } else {
                pix = (int)vf * W + (int)uf;
                const unsigned long long key = ((unsigned long long)f2ord(d32) << 32) | (unsigned long long)(uint32_t)local;
                atomicMin(keys + (size_t)b * H * W + pix, key);
            }
        }
        pixel_of_point[i] = pix;
    }
    const int t0 = block_sum(dropped, sh[0]), t1 = block_sum(outside, sh[1]);
    if (tid == 0) {
        if (t0) atomicAdd(stats + (size_t)b * 4 + 0, t0);
        if (t1) atomicAdd(stats + (size_t)b * 4 + 1, t1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- resolve
// grid (ceil(H W / 256), n)
template <int kFill>
__global__ __launch_bounds__(256) void resolve_kernel(const float* __restrict__ pts, const long long* __restrict__ offsets,
                                                      const uint8_t* __restrict__ colors, const uint8_t* __restrict__ labels,
                                                      const unsigned long long* __restrict__ keys, int P, int H, int W,
                                                      int32_t* __restrict__ index, float* __restrict__ xyz, uint8_t* __restrict__ rgb,
                                                      uint8_t* __restrict__ mask, int32_t* __restrict__ stats)
{
    __shared__ int sh[2][4];
    const int tid = threadIdx.x, b = blockIdx.y, HW = H * W;
    const int q = blockIdx.x * 256 + tid;
    int direct = 0, filled = 0;
    if (q < HW) {
        const Range r = cloud_range(offsets, b, P);
        const unsigned long long* __restrict__ km = keys + (size_t)b * HW;
        unsigned long long key = km[q];
        const bool hit = key != kEmpty;
        if (kFill > 0 && !hit) {
            const int y = q / W, x = q - y * W;
            for (int dy = -kFill; dy <= kFill; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -kFill; dx <= kFill; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= W) continue;
                    const unsigned long long k = km[yy * W + xx];
                    key = k < key ? k : key;
                }
            }
        }
        const long long idx = (long long)(uint32_t)key;
        const bool won = key != kEmpty && r.lo + idx < r.hi;
        const size_t o = (size_t)b * HW + q;
        float px = 0.f, py = 0.f, pz = 0.f;
        uint8_t cr = 0, cg = 0, cb = 0, mk = 0;
        if (won) {
            const long long i = r.lo + idx;
            px = pts[i * 3], py = pts[i * 3 + 1], pz = pts[i * 3 + 2];
            if (colors) cr = colors[i * 3], cg = colors[i * 3 + 1], cb = colors[i * 3 + 2];
            if (labels) mk = labels[i] ? 255 : 0;
            direct = hit, filled = !hit;
        }
        index[o] = won ? (int32_t)idx : -1;
        xyz[o * 3] = px, xyz[o * 3 + 1] = py, xyz[o * 3 + 2] = pz;
        if (rgb) rgb[o * 3] = cr, rgb[o * 3 + 1] = cg, rgb[o * 3 + 2] = cb;
        if (mask) mask[o] = mk;
    }
    const int t0 = block_sum(direct, sh[0]), t1 = block_sum(filled, sh[1]);
    if (tid == 0) {
        if (t0) atomicAdd(stats + (size_t)b * 4 + 2, t0);
        if (t1) atomicAdd(stats + (size_t)b * 4 + 3, t1);
    }
}

bool points_ok(const char* who, int n, int P, int max_len)
{
    if (!(n >= 0 && n <= kMaxImages && P >= 0 && max_len >= 0)) {
        cmdiad_set_error("%s: bad sizes n=%d (0..%d) P=%d max_len=%d (0..2^31-1)", who, n, kMaxImages, P, max_len);
        return false;
    }
    return true;
}

bool grid_ok(const char* who, int n, int H, int W)
{
    if (!sizes_ok(n, H, W)) {   // n itself has passed points_ok
        cmdiad_set_error("%s: bad grid H=%d W=%d for n=%d (sides >= 1, H*W <= 2^24, n*H*W <= 2^30)", who, H, W, n);
        return false;
    }
    return true;
}

inline unsigned blocks_of(long long items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" int cmdiad_cloud_bounds(const float* points, const int64_t* offsets, const double* cams, int n, int P, int max_len,
                                   double* bounds, int32_t* count, cmdiad_stream_t stream)
{
    if (!points_ok("cmdiad_cloud_bounds", n, P, max_len)) return CMDIAD_ERR_ARG;
    if (n == 0) return CMDIAD_OK;
    const bool any = P > 0 && max_len > 0;
    CMDIAD_REQUIRE(offsets && cams && bounds && count && (points || !any), CMDIAD_ERR_ARG,
                   "cmdiad_cloud_bounds: null pointer (offsets, cams, bounds, count; points where P and max_len are above 0)");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* slots = reinterpret_cast<unsigned long long*>(bounds);
    hipLaunchKernelGGL(bounds_init_kernel, dim3(blocks_of((long long)n * 6, 256)), dim3(256), 0, s, slots, count, n);
    CMDIAD_CHECK_LAUNCH();
    if (any) {
        hipLaunchKernelGGL(bounds_kernel, dim3(blocks_of(max_len, kBoundsPts), (unsigned)n), dim3(256), 0, s, points,
                           (const long long*)offsets, cams, P, max_len, slots, count);
        CMDIAD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(bounds_final_kernel, dim3(blocks_of((long long)n * 6, 256)), dim3(256), 0, s, slots, n);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_organize_splat(const float* points, const int64_t* offsets, const double* cams, int n, int P, int max_len,
                                     int kind, int H, int W, uint64_t* keys, int32_t* pixel_of_point, int32_t* stats,
                                     cmdiad_stream_t stream)
{
    if (!points_ok("cmdiad_organize_splat", n, P, max_len) || !grid_ok("cmdiad_organize_splat", n, H, W)) return CMDIAD_ERR_ARG;
    CMDIAD_REQUIRE(kind == 0 || kind == 1, CMDIAD_ERR_ARG, "cmdiad_organize_splat: camera kind %d (0 orthographic | 1 pinhole)", kind);
    if (n == 0) return CMDIAD_OK;
    const bool any = P > 0 && max_len > 0;
    CMDIAD_REQUIRE(offsets && cams && keys && stats && ((points && pixel_of_point) || !any), CMDIAD_ERR_ARG,
                   "cmdiad_organize_splat: null pointer (offsets, cams, keys, stats; points and pixel_of_point where P and max_len are "
                   "above 0)");
    hipStream_t s = (hipStream_t)stream;
    const long long total = (long long)n * H * W;
    unsigned long long* km = reinterpret_cast<unsigned long long*>(keys);
    const unsigned init_blocks = blocks_of(total, 256) < 8192u ? blocks_of(total, 256) : 8192u;
    hipLaunchKernelGGL(splat_init_kernel, dim3(init_blocks), dim3(256), 0, s, km, total, stats, n);
    CMDIAD_CHECK_LAUNCH();
    if (!any) return CMDIAD_OK;
    const dim3 grid(blocks_of(max_len, 256), (unsigned)n);
    if (kind == 0)
        hipLaunchKernelGGL(splat_kernel<0>, grid, dim3(256), 0, s, points, (const long long*)offsets, cams, P, max_len, H, W, km,
                           pixel_of_point, stats);
    else
        hipLaunchKernelGGL(splat_kernel<1>, grid, dim3(256), 0, s, points, (const long long*)offsets, cams, P, max_len, H, W, km,
                           pixel_of_point, stats);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_organize_resolve(const float* points, const int64_t* offsets, const uint8_t* colors, const uint8_t* labels,
                                       const uint64_t* keys, int n, int P, int H, int W, int fill, int32_t* index, float* xyz,
                                       uint8_t* rgb, uint8_t* mask, int32_t* stats, cmdiad_stream_t stream)
{
    if (!points_ok("cmdiad_organize_resolve", n, P, 0) || !grid_ok("cmdiad_organize_resolve", n, H, W)) return CMDIAD_ERR_ARG;
    CMDIAD_REQUIRE(fill >= 0 && fill <= 2, CMDIAD_ERR_ARG, "cmdiad_organize_resolve: fill=%d (0..2)", fill);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(offsets && keys && index && xyz && stats && (points || P == 0), CMDIAD_ERR_ARG,
                   "cmdiad_organize_resolve: null pointer (offsets, keys, index, xyz, stats; points where P is above 0)");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(zero_stats_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, stats, n, 2);
    CMDIAD_CHECK_LAUNCH();
    const dim3 grid(blocks_of((long long)H * W, 256), (unsigned)n);
    const unsigned long long* km = reinterpret_cast<const unsigned long long*>(keys);
    const long long* off = (const long long*)offsets;
    if (fill == 0)
        hipLaunchKernelGGL(resolve_kernel<0>, grid, dim3(256), 0, s, points, off, colors, labels, km, P, H, W, index, xyz, rgb, mask, stats);
    else if (fill == 1)
        hipLaunchKernelGGL(resolve_kernel<1>, grid, dim3(256), 0, s, points, off, colors, labels, km, P, H, W, index, xyz, rgb, mask, stats);
    else
        hipLaunchKernelGGL(resolve_kernel<2>, grid, dim3(256), 0, s, points, off, colors, labels, km, P, H, W, index, xyz, rgb, mask, stats);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
