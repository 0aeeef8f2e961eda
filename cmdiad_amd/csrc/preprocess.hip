// Scan preprocessing on the device (utils/preprocessing.py of the reference: RANSAC plane removal + largest DBSCAN cluster; the
// reference calls open3d for both).  The contract of the two stages is this project's own -- docs/preprocessing.md -- and is
// restated in numpy / scipy in tests/preprocess_ref.py.  Built with -ffp-contract=off: every float64 operation below rounds once,
// in the order written, so the inlier sets, the neighbour sets and therefore the labels do not depend on the compiler.
//
// cmdiad_plane_ransac: `iterations` hypotheses, one workgroup each.  Wave 0 draws n distinct point indices from a counter-based
//   hash of (seed, hypothesis, draw counter) -- lane l keeps sample l, a ballot rejects a repeated index --, fits the least-squares
//   plane of the sample in float64 (centroid, centred scatter matrix, cyclic Jacobi on the 3 x 3, eigenvector of the smallest
//   eigenvalue), then all four waves stream the points and count |n.p + d| < threshold.  (count << 32) | ~h goes through one
//   atomicMax: most inliers, ties to the lowest h.  A second kernel (one workgroup) refits over the winner's inliers.
// cmdiad_plane_mask: zeroes the xyz and the rgb entry of every pixel closer to the plane than the threshold.
// cmdiad_dbscan: uniform grid with cell edge eps (1 + 1e-6) (doubled until the grid fits the workspace), counting sort of the
//   points by cell, core test over the 3 x 3 x 3 cells (9 contiguous runs of the sorted array) that stops at min_points, union-find
//   over core pairs (the parent of a node is always a smaller sorted position: hooking is a compare-and-swap on a root, paths are
//   shortened with atomicMin, so there are no cycles whatever the schedule), flattening + the lowest ORIGINAL index of every
//   component, an exclusive scan over "index is the lowest core point of a cluster" that numbers the clusters, and the label pass
//   (a non-core point takes the lowest cluster number among its core neighbours).  Connected components, minima and counts do not
//   depend on the order in which threads run or in which the sort places the points of one cell, so neither do the labels.
// cmdiad_label_histogram: hist[label + 1] counts (bin 0 = noise).
// cmdiad_scan_edges / cmdiad_scan_compact: one stable compaction over a virtual sequence of pixels (the reference's edge strips, or
//   all pixels in raster order): per-block counts of the valid points (a 64-bit ballot per wave), an exclusive scan of the block
//   counts (scan_exclusive_kernel), a scatter that ranks a lane by the popcount of the ballot below it.  No atomic decides a
//   position, so the output order is the sequence order whatever the schedule.
// cmdiad_keep_largest_cluster: the first maximum of hist[0 .. n_clusters] (one workgroup), then pc / rgb are zeroed at index[i]
//   wherever labels[i] is not the winner.
#include <float.h>
#include <limits.h>

#include "common.h"
#include "block_scan.h"
#include "frames.h"
#include "union_find.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ plane
constexpr int kPlaneThreads = 256;
constexpr uint32_t kPlaneMaxDraws = 65536;   // a hypothesis that has not found n distinct indices by then does not compete

__host__ __device__ __forceinline__ uint32_t mix32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum over a workgroup of 256 threads, the same value in every thread; fixed order
__device__ __forceinline__ double block_sum_f64(double v, double* sh)
{
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// one Jacobi rotation that annihilates a_pq of a symmetric 3 x 3 (r = the third index); v?p / v?q = columns p, q of V
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p,
                                           double& v0q, double& v1p, double& v1q, double& v2p, double& v2q)
{
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    double a = arp, b = arq;
    arp = c * a - s * b;
    arq = s * a + c * b;
    a = v0p, b = v0q;
    v0p = c * a - s * b;
    v0q = s * a + c * b;
    a = v1p, b = v1q;
    v1p = c * a - s * b;
    v1q = s * a + c * b;
    a = v2p, b = v2q;
    v2p = c * a - s * b;
    v2q = s * a + c * b;
}

// plane (a, b, c, d) of a centroid (mx, my, mz) and a centred scatter matrix: unit normal of the smallest eigenvalue, c >= 0
__device__ __forceinline__ void plane_of_scatter(double mx, double my, double mz, double a00, double a01, double a02, double a11,
                                                 double a12, double a22, double& pa, double& pb, double& pc, double& pd)
{
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < 12; ++sweep) {
        if (a01 == 0.0 && a02 == 0.0 && a12 == 0.0) break;
        jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (p, q, r) = (0, 1, 2)
        jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2, 1)
        jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2, 0)
    }
    // column of the smallest eigenvalue (ties: the lowest index), picked with exact 0 / 1 weights: a chain of selects over the nine
    // values makes the compiler keep V in scratch memory and index it
    const int k = a22 < fmin(a00, a11) ? 2 : (a11 < a00 ? 1 : 0);
    const double w0 = k == 0 ? 1.0 : 0.0, w1 = k == 1 ? 1.0 : 0.0, w2 = k == 2 ? 1.0 : 0.0;
    double nx = (w0 * v00 + w1 * v01) + w2 * v02, ny = (w0 * v10 + w1 * v11) + w2 * v12, nz = (w0 * v20 + w1 * v21) + w2 * v22;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    nx = nx / len, ny = ny / len, nz = nz / len;
    if (nz < 0.0) nx = -nx, ny = -ny, nz = -nz;
    pa = nx, pb = ny, pc = nz;
    pd = -((nx * mx + ny * my) + nz * mz);
}

__device__ __forceinline__ bool plane_near(const float* __restrict__ p, double a, double b, double c, double d, double thr)
{
    return fabs((((a * (double)p[0] + b * (double)p[1]) + c * (double)p[2]) + d)) < thr;
}

__global__ __launch_bounds__(kPlaneThreads) void plane_hypothesis_kernel(const float* __restrict__ pts, int E, int n, uint32_t seed,
                                                                         double thr, double* __restrict__ planes,
                                                                         unsigned long long* __restrict__ best)
{
    __shared__ double s_plane[4];
    __shared__ int s_valid;
    __shared__ int s_count[kPlaneThreads / 64];
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) {
        int mine = -1, cnt = 0;
        const uint32_t base = mix32(seed + 0x9E3779B9u * ((uint32_t)h + 1u));
        for (uint32_t c = 0; c < kPlaneMaxDraws && cnt < n; ++c) {
            const int idx = (int)(mix32(base + c) % (uint32_t)E);
            if (__ballot(lane < cnt && mine == idx) == 0ull) {
                if (lane == cnt) mine = idx;
                ++cnt;
            }
        }
        double x = 0.0, y = 0.0, z = 0.0;
        const bool on = lane < cnt;
        if (on) x = (double)pts[(size_t)mine * 3], y = (double)pts[(size_t)mine * 3 + 1], z = (double)pts[(size_t)mine * 3 + 2];
        const double mx = wave_sum_f64(x) / (double)n, my = wave_sum_f64(y) / (double)n, mz = wave_sum_f64(z) / (double)n;
        const double dx = on ? x - mx : 0.0, dy = on ? y - my : 0.0, dz = on ? z - mz : 0.0;
        const double a00 = wave_sum_f64(dx * dx), a01 = wave_sum_f64(dx * dy), a02 = wave_sum_f64(dx * dz);
        const double a11 = wave_sum_f64(dy * dy), a12 = wave_sum_f64(dy * dz), a22 = wave_sum_f64(dz * dz);
        double pa, pb, pc, pd;
        plane_of_scatter(mx, my, mz, a00, a01, a02, a11, a12, a22, pa, pb, pc, pd);
        if (lane == 0) {
            s_valid = cnt == n;
            s_plane[0] = pa, s_plane[1] = pb, s_plane[2] = pc, s_plane[3] = pd;
            planes[(size_t)h * 4] = pa, planes[(size_t)h * 4 + 1] = pb, planes[(size_t)h * 4 + 2] = pc, planes[(size_t)h * 4 + 3] = pd;
        }
    }
    __syncthreads();
    if (!s_valid) return;
    const double a = s_plane[0], b = s_plane[1], c = s_plane[2], d = s_plane[3];
    int count = 0;
    for (int i = tid; i < E; i += kPlaneThreads) count += plane_near(pts + (size_t)i * 3, a, b, c, d, thr) ? 1 : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) count += __shfl_xor(count, m, 64);
    if (lane == 0) s_count[tid >> 6] = count;
    __syncthreads();
    if (tid == 0) {
        count = 0;
        for (int w = 0; w < kPlaneThreads / 64; ++w) count += s_count[w];
        atomicMax(best, ((unsigned long long)(uint32_t)count << 32) | (unsigned long long)(~(uint32_t)h));
    }
}

// least-squares plane over the inliers of the winning hypothesis; info = {inliers, winner} ({0, -1}: no hypothesis competed)
__global__ __launch_bounds__(kPlaneThreads) void plane_refit_kernel(const float* __restrict__ pts, int E, double thr,
                                                                    const double* __restrict__ planes,
                                                                    const unsigned long long* __restrict__ best,
                                                                    double* __restrict__ plane_out, int32_t* __restrict__ info)
{
    __shared__ double sh[kPlaneThreads / 64];
    const unsigned long long key = *best;
    const int tid = threadIdx.x;
    if (key == 0ull) {
        if (tid < 4) plane_out[tid] = 0.0;
        if (tid == 0) info[0] = 0, info[1] = -1;
        return;
    }
    const int h = (int)(~(uint32_t)key), inl = (int)(key >> 32);
    const double a = planes[(size_t)h * 4], b = planes[(size_t)h * 4 + 1], c = planes[(size_t)h * 4 + 2], d = planes[(size_t)h * 4 + 3];
    if (inl < 3) {   // nothing to refit on: the hypothesis itself
        if (tid == 0) plane_out[0] = a, plane_out[1] = b, plane_out[2] = c, plane_out[3] = d, info[0] = inl, info[1] = h;
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int i = tid; i < E; i += kPlaneThreads) {
        const float* p = pts + (size_t)i * 3;
        if (plane_near(p, a, b, c, d, thr)) sx += (double)p[0], sy += (double)p[1], sz += (double)p[2];
    }
    const double mx = block_sum_f64(sx, sh) / (double)inl, my = block_sum_f64(sy, sh) / (double)inl, mz = block_sum_f64(sz, sh) / (double)inl;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int i = tid; i < E; i += kPlaneThreads) {
        const float* p = pts + (size_t)i * 3;
        if (plane_near(p, a, b, c, d, thr)) {
            const double dx = (double)p[0] - mx, dy = (double)p[1] - my, dz = (double)p[2] - mz;
            a00 += dx * dx, a01 += dx * dy, a02 += dx * dz, a11 += dy * dy, a12 += dy * dz, a22 += dz * dz;
        }
    }
    a00 = block_sum_f64(a00, sh), a01 = block_sum_f64(a01, sh), a02 = block_sum_f64(a02, sh);
    a11 = block_sum_f64(a11, sh), a12 = block_sum_f64(a12, sh), a22 = block_sum_f64(a22, sh);
    double pa, pb, pc, pd;
    plane_of_scatter(mx, my, mz, a00, a01, a02, a11, a12, a22, pa, pb, pc, pd);
    if (tid == 0) plane_out[0] = pa, plane_out[1] = pb, plane_out[2] = pc, plane_out[3] = pd, info[0] = inl, info[1] = h;
}

__global__ __launch_bounds__(256) void plane_mask_kernel(float* __restrict__ pc, uint8_t* __restrict__ rgb, size_t n, int rgb_bytes,
                                                         const double* __restrict__ plane, double thr)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float* p = pc + i * 3;
    if (!plane_near(p, plane[0], plane[1], plane[2], plane[3], thr)) return;
    p[0] = 0.0f, p[1] = 0.0f, p[2] = 0.0f;
    for (int k = 0; k < rgb_bytes; ++k) rgb[i * (size_t)rgb_bytes + k] = 0;
}

// ----------------------------------------------------------------------------------------------------------------- DBSCAN
constexpr int kMaxPoints = 1 << 24;

struct GridParams {
    double ox, oy, oz, inv;
    int nx, ny, nz, ncell;
};
struct __attribute__((aligned(16))) SortedPoint {
    float x, y, z;
    int i;   // index in the caller's array
};

inline int dbscan_max_cells(int N)
{
    const long long c = 2ll * (long long)N;
    return (int)(c < 4096 ? 4096 : (c > (1ll << 21) ? (1ll << 21) : c));
}

struct DbscanWs {
    int maxc;
    GridParams* gp;
    uint32_t* bbox;
    int *start, *count, *key;
    SortedPoint* sp;
    int *core, *parent, *comp, *minorig, *rank;
    size_t total;
};
inline DbscanWs dbscan_layout(void* base, int N)
{
    const int maxc = dbscan_max_cells(N);
    const size_t n = (size_t)(N > 0 ? N : 1);
    Carve c(base);   // every piece padded to 256 bytes
    return {maxc, c.take<GridParams>(1, 256), c.take<uint32_t>(6, 256), c.take<int>((size_t)maxc + 1, 256), c.take<int>(maxc, 256),
            c.take<int>(n, 256), c.take<SortedPoint>(n, 256), c.take<int>(n, 256), c.take<int>(n, 256), c.take<int>(n, 256),
            c.take<int>(n, 256), c.take<int>(n + 1, 256), c.total()};
}

__global__ __launch_bounds__(256) void dbscan_bbox_kernel(const float* __restrict__ pts, int N, uint32_t* __restrict__ bbox)
{
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = blockIdx.x * 256 + threadIdx.x; i < N; i += gridDim.x * 256) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = pts[(size_t)i * 3 + k];
            if (fabsf(v) <= FLT_MAX) lo[k] = fminf(lo[k], v), hi[k] = fmaxf(hi[k], v);   // a non-finite coordinate does not size the grid
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) lo[k] = fminf(lo[k], __shfl_xor(lo[k], m, 64)), hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m, 64));
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (lo[k] <= hi[k]) atomicMin(&bbox[k], f2ord(lo[k])), atomicMax(&bbox[3 + k], f2ord(hi[k]));
        }
    }
}

__global__ void dbscan_grid_kernel(const uint32_t* __restrict__ bbox, double eps, int maxc, GridParams* __restrict__ gp)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double lo[3], ext[3];
    for (int k = 0; k < 3; ++k) {
        const bool any = bbox[k] <= bbox[3 + k];   // untouched: min = 0xFFFFFFFF, max = 0
        lo[k] = any ? (double)ord2f(bbox[k]) : 0.0;
        ext[k] = any ? (double)ord2f(bbox[3 + k]) - lo[k] : 0.0;
    }
    double cell = eps * (1.0 + 1e-6);   // > eps: two points within eps are never two cells apart, rounding included
    double nx, ny, nz;
    for (;;) {
        nx = floor(ext[0] / cell) + 1.0, ny = floor(ext[1] / cell) + 1.0, nz = floor(ext[2] / cell) + 1.0;
        if (nx * ny * nz <= (double)maxc) break;
        cell = cell * 2.0;
    }
    gp->ox = lo[0], gp->oy = lo[1], gp->oz = lo[2], gp->inv = 1.0 / cell;
    gp->nx = (int)nx, gp->ny = (int)ny, gp->nz = (int)nz, gp->ncell = (int)(nx * ny * nz);
}

__device__ __forceinline__ int cell_coord(float v, double origin, double inv, int dim)
{
    const double f = floor(((double)v - origin) * inv);
    return (int)fmin(fmax(f, 0.0), (double)(dim - 1));   // NaN -> 0: always a cell of the grid
}

__global__ __launch_bounds__(256) void dbscan_key_kernel(const float* __restrict__ pts, int N, const GridParams* __restrict__ gp,
                                                         int* __restrict__ key, int* __restrict__ count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int cx = cell_coord(pts[(size_t)i * 3], gp->ox, gp->inv, gp->nx), cy = cell_coord(pts[(size_t)i * 3 + 1], gp->oy, gp->inv, gp->ny);
    const int cz = cell_coord(pts[(size_t)i * 3 + 2], gp->oz, gp->inv, gp->nz);
    const int id = (cz * gp->ny + cy) * gp->nx + cx;
    key[i] = id;
    atomicAdd(&count[id], 1);
}

// exclusive scan of in[0 .. n) into out[0 .. n], out[n] = total; one workgroup of 1024, thread t owns one contiguous piece
// (in == out is fine).  n = *n_dev when n_dev is given.
__global__ __launch_bounds__(1024) void scan_exclusive_kernel(const int* in, int* out, int n, const int* __restrict__ n_dev)
{
    __shared__ int sh[16];
    if (n_dev) n = *n_dev;
    const int t = threadIdx.x;
    const int piece = (n + 1023) / 1024;
    const int lo = min(t * piece, n), hi = min(lo + piece, n);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += in[i];
    int total;
    int run = block_excl_scan<16>(s, sh, total);
    for (int i = lo; i < hi; ++i) {
        const int v = in[i];
        out[i] = run;
        run += v;
    }
    if (t == 1023) out[n] = total;
}

__global__ __launch_bounds__(256) void dbscan_scatter_kernel(const float* __restrict__ pts, int N, const int* __restrict__ key,
                                                             const int* __restrict__ start, int* __restrict__ count,
                                                             SortedPoint* __restrict__ sp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int id = key[i];
    const int pos = start[id] + atomicSub(&count[id], 1) - 1;
    SortedPoint p;
    p.x = pts[(size_t)i * 3], p.y = pts[(size_t)i * 3 + 1], p.z = pts[(size_t)i * 3 + 2], p.i = i;
    sp[pos] = p;
}

__device__ __forceinline__ bool within(const SortedPoint& p, const SortedPoint& q, double eps2)
{
    const double dx = (double)p.x - (double)q.x, dy = (double)p.y - (double)q.y, dz = (double)p.z - (double)q.z;
    return (dx * dx + dy * dy) + dz * dz <= eps2;
}

// the sorted positions [lo, hi) of the cells (cx-1 .. cx+1, cy+oy, cz+oz): contiguous because x runs fastest in the cell id
__device__ __forceinline__ bool cell_run(const GridParams& g, const int* __restrict__ start, int cx, int cy, int cz, int oy, int oz,
                                         int& lo, int& hi)
{
    const int y = cy + oy, z = cz + oz;
    if (y < 0 || y >= g.ny || z < 0 || z >= g.nz) return false;
    const int row = (z * g.ny + y) * g.nx;
    lo = start[row + max(cx - 1, 0)];
    hi = start[row + min(cx + 1, g.nx - 1) + 1];
    return hi > lo;
}

__global__ __launch_bounds__(256) void dbscan_core_kernel(const SortedPoint* __restrict__ sp, int N, const GridParams* __restrict__ gp,
                                                          const int* __restrict__ start, double eps2, int min_points,
                                                          int* __restrict__ core, int* __restrict__ parent)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N) return;
    const GridParams g = *gp;
    const SortedPoint p = sp[s];
    const int cx = cell_coord(p.x, g.ox, g.inv, g.nx), cy = cell_coord(p.y, g.oy, g.inv, g.ny), cz = cell_coord(p.z, g.oz, g.inv, g.nz);
    int cnt = 0;
    for (int r = 0; r < 9 && cnt < min_points; ++r) {
        // the point's own row of cells first: a dense neighbourhood is decided there
        const int q = r == 0 ? 4 : (r <= 4 ? r - 1 : r);
        int lo, hi;
        if (!cell_run(g, start, cx, cy, cz, q % 3 - 1, q / 3 - 1, lo, hi)) continue;
        for (int j = lo; j < hi && cnt < min_points; ++j) cnt += within(p, sp[j], eps2) ? 1 : 0;
    }
    core[s] = cnt >= min_points ? 1 : 0;
    parent[s] = s;
}

// uf_load / uf_find / uf_union: union_find.h

__global__ __launch_bounds__(256) void dbscan_union_kernel(const SortedPoint* __restrict__ sp, int N, const GridParams* __restrict__ gp,
                                                           const int* __restrict__ start, double eps2, const int* __restrict__ core,
                                                           int* parent)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N || !core[s]) return;
    const GridParams g = *gp;
    const SortedPoint p = sp[s];
    const int cx = cell_coord(p.x, g.ox, g.inv, g.nx), cy = cell_coord(p.y, g.oy, g.inv, g.ny), cz = cell_coord(p.z, g.oz, g.inv, g.nz);
    int root = s;
    for (int r = 0; r < 9; ++r) {
        int lo, hi;
        if (!cell_run(g, start, cx, cy, cz, r % 3 - 1, r / 3 - 1, lo, hi)) continue;
        hi = min(hi, s);   // every pair once, from its larger sorted position
        for (int j = lo; j < hi; ++j) {
            if (!core[j]) continue;
            if (uf_load(parent + j) == root) continue;   // already one tree (once joined, always joined)
            if (within(p, sp[j], eps2)) root = uf_union(parent, s, j);
        }
    }
}

__global__ __launch_bounds__(256) void dbscan_flatten_kernel(const SortedPoint* __restrict__ sp, int N, const int* __restrict__ core,
                                                             int* parent, int* __restrict__ comp, int* __restrict__ minorig)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N || !core[s]) return;
    const int r = uf_find(parent, s);
    comp[s] = r;
    atomicMin(&minorig[r], sp[s].i);
}

// rank[i] = 1 where original index i is the lowest core point of a cluster
__global__ __launch_bounds__(256) void dbscan_mark_kernel(int N, const int* __restrict__ core, const int* __restrict__ comp,
                                                          const int* __restrict__ minorig, int* __restrict__ rank)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= N || !core[s] || comp[s] != s) return;
    rank[minorig[s]] = 1;
}

__global__ __launch_bounds__(256) void dbscan_label_kernel(const SortedPoint* __restrict__ sp, int N, const GridParams* __restrict__ gp,
                                                           const int* __restrict__ start, double eps2, const int* __restrict__ core,
                                                           const int* __restrict__ comp, const int* __restrict__ minorig,
                                                           const int* __restrict__ rank, int32_t* __restrict__ labels,
                                                           int32_t* __restrict__ n_clusters)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s == 0) *n_clusters = rank[N];
    if (s >= N) return;
    const SortedPoint p = sp[s];
    int label;
    if (core[s]) {
        label = rank[minorig[comp[s]]];
    } else {
        const GridParams g = *gp;
        const int cx = cell_coord(p.x, g.ox, g.inv, g.nx), cy = cell_coord(p.y, g.oy, g.inv, g.ny), cz = cell_coord(p.z, g.oz, g.inv, g.nz);
        label = INT_MAX;
        for (int r = 0; r < 9; ++r) {
            int lo, hi;
            if (!cell_run(g, start, cx, cy, cz, r % 3 - 1, r / 3 - 1, lo, hi)) continue;
            for (int j = lo; j < hi; ++j)
                if (core[j] && within(p, sp[j], eps2)) label = min(label, rank[minorig[comp[j]]]);
        }
        if (label == INT_MAX) label = -1;
    }
    labels[p.i] = label;
}

__global__ __launch_bounds__(256) void label_histogram_kernel(const int32_t* __restrict__ labels, int N, int32_t* __restrict__ hist,
                                                              int bins)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int b = labels[i] + 1;
    if (b >= 0 && b < bins) atomicAdd(&hist[b], 1);
}

// ------------------------------------------------------------------------------------------- compaction, largest cluster
constexpr int kEdge = 10;   // get_edges_of_pc: the first and last 10 rows, the first and last 10 columns

// element k of the virtual sequence -> pixel (r, c).  edges = 0: all pixels in raster order.  edges = 1: rows 0 .. rh - 1, rows
// max(H - 10, 0) .. H - 1, then for every row the columns 0 .. cw - 1, then for every row the columns max(W - 10, 0) .. W - 1
// (rh = min(10, H), cw = min(10, W); the corner blocks appear twice).
__device__ __forceinline__ void seq_pixel(int k, int H, int W, int edges, int& r, int& c)
{
    if (!edges) {
        r = k / W, c = k - r * W;
        return;
    }
    const int rh = min(kEdge, H), cw = min(kEdge, W);
    const int A = rh * W, B = H * cw;
    if (k < A) {
        r = k / W, c = k - r * W;
    } else if (k < 2 * A) {
        k -= A;
        r = k / W, c = k - r * W, r += max(H - kEdge, 0);
    } else if (k < 2 * A + B) {
        k -= 2 * A;
        r = k / cw, c = k - r * cw;
    } else {
        k -= 2 * A + B;
        r = k / cw, c = k - r * cw, c += max(W - kEdge, 0);
    }
}

inline long long seq_length(int H, int W, int edges)
{
    if (!edges) return (long long)H * W;
    const long long rh = H < kEdge ? H : kEdge, cw = W < kEdge ? W : kEdge;
    return 2 * rh * W + 2 * cw * H;
}

// numpy's all(p != 0): -0.0 is a zero, NaN is not
__device__ __forceinline__ bool seq_valid(const float* __restrict__ pc, size_t pitch, int k, int L, int H, int W, int edges,
                                          int& r, int& c)
{
    if (k >= L) return false;
    seq_pixel(k, H, W, edges, r, c);
    const float* p = pc + (size_t)r * pitch + (size_t)c * 3;
    return p[0] != 0.0f && p[1] != 0.0f && p[2] != 0.0f;
}

__global__ __launch_bounds__(256) void compact_count_kernel(const float* __restrict__ pc, size_t pitch, int H, int W, int edges, int L,
                                                            int* __restrict__ block_count)
{
    __shared__ int s_wave[4];
    int r, c, total;
    block_ballot_rank<4>(seq_valid(pc, pitch, blockIdx.x * 256 + threadIdx.x, L, H, W, edges, r, c), s_wave, total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// block_start = the exclusive scan of block_count over the n_blocks blocks, block_start[n_blocks] = all valid points
__global__ __launch_bounds__(256) void compact_scatter_kernel(const float* __restrict__ pc, size_t pitch, int H, int W, int edges, int L,
                                                              const int* __restrict__ block_start, int n_blocks, int cap,
                                                              float* __restrict__ points, int32_t* __restrict__ index,
                                                              int32_t* __restrict__ count)
{
    __shared__ int s_wave[4];
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = block_start[n_blocks];
    int r = 0, c = 0, total;
    const bool ok = seq_valid(pc, pitch, blockIdx.x * 256 + threadIdx.x, L, H, W, edges, r, c);
    const int pos = block_start[blockIdx.x] + block_ballot_rank<4>(ok, s_wave, total);
    if (!ok || pos >= cap) return;
    const float* p = pc + (size_t)r * pitch + (size_t)c * 3;
    float* q = points + (size_t)pos * 3;
    q[0] = p[0], q[1] = p[1], q[2] = p[2];
    if (index) index[pos] = r * W + c;
}

// winner = (the first maximum of hist[0 .. min(n_clusters, bins - 1)]) - 1: np.unique + argmax over the labels that occur
__global__ __launch_bounds__(256) void cluster_winner_kernel(const int32_t* __restrict__ hist, int bins, const int32_t* __restrict__ n_clusters,
                                                             int32_t* __restrict__ winner)
{
    __shared__ unsigned long long s_key[4];
    const int last = min(max(*n_clusters, 0), bins - 1);
    unsigned long long key = 0xFFFFFFFFull;   // (count << 32) | ~bin: the largest count, ties to the lowest bin; (0, bin 0) to start
    for (int b = threadIdx.x; b <= last; b += 256) {
        const unsigned long long k = ((unsigned long long)(uint32_t)max(hist[b], 0) << 32) | (unsigned long long)(~(uint32_t)b);
        key = k > key ? k : key;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = shfl_xor_u64(key, m);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) key = s_key[w] > key ? s_key[w] : key;
        *winner = (int32_t)(~(uint32_t)key) - 1;
    }
}

__global__ __launch_bounds__(256) void cluster_keep_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ index, int N,
                                                           const int32_t* __restrict__ winner, float* __restrict__ pc,
                                                           uint8_t* __restrict__ rgb, size_t n_pixels, int rgb_bytes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N || labels[i] == *winner) return;
    const int32_t at = index[i];
    if (at < 0 || (size_t)at >= n_pixels) return;
    float* p = pc + (size_t)at * 3;
    p[0] = 0.0f, p[1] = 0.0f, p[2] = 0.0f;
    for (int k = 0; k < rgb_bytes; ++k) rgb[(size_t)at * (size_t)rgb_bytes + k] = 0;
}

}  // namespace

// the winning hypothesis' key (in 256 bytes of its own) | a plane per hypothesis
struct RansacWs { unsigned long long* best; double* planes; size_t total; };
static RansacWs ransac_layout(void* base, int iterations)
{
    Carve c(base);
    return {c.take<unsigned long long>(1, 256), c.take<double>((size_t)iterations * 4), c.total()};
}

extern "C" size_t cmdiad_plane_ransac_workspace_bytes(int iterations) { return iterations > 0 ? ransac_layout(nullptr, iterations).total : 0; }

extern "C" int cmdiad_plane_ransac(const float* points, int E, int n, int iterations, double distance_threshold, uint32_t seed,
                                   double* plane_out, int32_t* info_out, void* workspace, size_t workspace_bytes,
                                   cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(points && plane_out && info_out && workspace, CMDIAD_ERR_ARG, "cmdiad_plane_ransac: null pointer");
    CMDIAD_REQUIRE(n >= 3 && n <= 64 && E >= n && iterations >= 1 && iterations <= (1 << 20) && distance_threshold > 0.0,
                   CMDIAD_ERR_ARG, "cmdiad_plane_ransac: bad sizes E=%d n=%d (3..64, <= E) iterations=%d threshold=%g", E, n,
                   iterations, distance_threshold);
    const RansacWs L = ransac_layout(workspace, iterations);
    if (const int rc = workspace_ok("cmdiad_plane_ransac", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t s = (hipStream_t)stream;
    CMDIAD_CHECK_HIP("cmdiad_plane_ransac", hipMemsetAsync(L.best, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(plane_hypothesis_kernel, dim3(iterations), dim3(kPlaneThreads), 0, s, points, E, n, seed, distance_threshold,
                       L.planes, L.best);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(plane_refit_kernel, dim3(1), dim3(kPlaneThreads), 0, s, points, E, distance_threshold, (const double*)L.planes,
                       (const unsigned long long*)L.best, plane_out, info_out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_plane_mask(float* pc, uint8_t* rgb, size_t n_points, int rgb_bytes, const double* plane,
                                 double distance_threshold, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(pc && plane && (rgb || rgb_bytes == 0), CMDIAD_ERR_ARG, "cmdiad_plane_mask: null pointer");
    CMDIAD_REQUIRE(rgb_bytes >= 0 && rgb_bytes <= 64 && n_points <= ((size_t)1 << 31) && distance_threshold > 0.0, CMDIAD_ERR_ARG,
                   "cmdiad_plane_mask: bad sizes n_points=%zu rgb_bytes=%d threshold=%g", n_points, rgb_bytes, distance_threshold);
    if (n_points == 0) return CMDIAD_OK;
    hipLaunchKernelGGL(plane_mask_kernel, dim3((unsigned)((n_points + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pc, rgb,
                       n_points, rgb_bytes, plane, distance_threshold);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" size_t cmdiad_dbscan_workspace_bytes(int N) { return N < 0 ? 0 : dbscan_layout(nullptr, N).total; }

extern "C" int cmdiad_dbscan(const float* points, int N, double eps, int min_points, int32_t* labels, int32_t* n_clusters,
                             void* workspace, size_t workspace_bytes, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(points && labels && n_clusters && workspace, CMDIAD_ERR_ARG, "cmdiad_dbscan: null pointer");
    CMDIAD_REQUIRE(N >= 0 && N <= kMaxPoints && eps > 0.0 && eps <= 1e30 && min_points >= 1, CMDIAD_ERR_ARG,
                   "cmdiad_dbscan: bad sizes N=%d (0..%d) eps=%g min_points=%d", N, kMaxPoints, eps, min_points);
    const DbscanWs L = dbscan_layout(workspace, N);
    if (const int rc = workspace_ok("cmdiad_dbscan", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(n_clusters, 0, sizeof(int32_t), s));
        return CMDIAD_OK;
    }
    const double eps2 = eps * eps;
    const unsigned blocks = (unsigned)((N + 255) / 256);
    CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(L.bbox, 0xFF, 3 * sizeof(uint32_t), s));
    CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(L.bbox + 3, 0, 3 * sizeof(uint32_t), s));
    CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(L.count, 0, (size_t)L.maxc * 4, s));
    CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(L.minorig, 0x7F, (size_t)N * 4, s));
    CMDIAD_CHECK_HIP("cmdiad_dbscan", hipMemsetAsync(L.rank, 0, ((size_t)N + 1) * 4, s));
    hipLaunchKernelGGL(dbscan_bbox_kernel, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, s, points, N, L.bbox);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_grid_kernel, dim3(1), dim3(64), 0, s, (const uint32_t*)L.bbox, eps, L.maxc, L.gp);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_key_kernel, dim3(blocks), dim3(256), 0, s, points, N, (const GridParams*)L.gp, L.key, L.count);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(1024), 0, s, (const int*)L.count, L.start, 0, (const int*)&L.gp->ncell);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_scatter_kernel, dim3(blocks), dim3(256), 0, s, points, N, (const int*)L.key, (const int*)L.start, L.count, L.sp);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_core_kernel, dim3(blocks), dim3(256), 0, s, (const SortedPoint*)L.sp, N, (const GridParams*)L.gp,
                       (const int*)L.start, eps2, min_points, L.core, L.parent);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_union_kernel, dim3(blocks), dim3(256), 0, s, (const SortedPoint*)L.sp, N, (const GridParams*)L.gp,
                       (const int*)L.start, eps2, (const int*)L.core, L.parent);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_flatten_kernel, dim3(blocks), dim3(256), 0, s, (const SortedPoint*)L.sp, N, (const int*)L.core, L.parent, L.comp,
                       L.minorig);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_mark_kernel, dim3(blocks), dim3(256), 0, s, N, (const int*)L.core, (const int*)L.comp, (const int*)L.minorig,
                       L.rank);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(1024), 0, s, (const int*)L.rank, L.rank, N, (const int*)nullptr);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(dbscan_label_kernel, dim3(blocks), dim3(256), 0, s, (const SortedPoint*)L.sp, N, (const GridParams*)L.gp,
                       (const int*)L.start, eps2, (const int*)L.core, (const int*)L.comp, (const int*)L.minorig, (const int*)L.rank, labels,
                       n_clusters);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_label_histogram(const int32_t* labels, int N, int32_t* hist, int bins, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(labels && hist, CMDIAD_ERR_ARG, "cmdiad_label_histogram: null pointer");
    CMDIAD_REQUIRE(N >= 0 && bins >= 1, CMDIAD_ERR_ARG, "cmdiad_label_histogram: bad sizes N=%d bins=%d", N, bins);
    CMDIAD_CHECK_HIP("cmdiad_label_histogram", hipMemsetAsync(hist, 0, (size_t)bins * 4, (hipStream_t)stream));
    if (N == 0) return CMDIAD_OK;
    hipLaunchKernelGGL(label_histogram_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, labels, N, hist, bins);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

// ---- compaction: workspace = the block counts and their scan
struct CompactWs { int* block_count; size_t total; };   // one count per block of 256 elements, and the total
static CompactWs compact_layout(void* base, int H, int W, int edges)
{
    Carve c(base);
    return {c.take<int>((size_t)((seq_length(H, W, edges) + 255) / 256) + 1), c.total()};
}
static size_t compact_workspace(int H, int W, int edges)
{
    return !side_ok(H) || !side_ok(W) ? 0 : compact_layout(nullptr, H, W, edges).total;
}

static int compact_launch(const char* name, const float* pc, size_t pitch, int H, int W, int edges, float* points, int32_t* index, int cap,
                          int32_t* count, void* workspace, size_t workspace_bytes, hipStream_t s)
{
    CMDIAD_REQUIRE(pc && points && count && workspace, CMDIAD_ERR_ARG, "%s: null pointer", name);
    CMDIAD_REQUIRE(side_ok(H) && side_ok(W) && (long long)H * W <= (1ll << 26) && pitch >= (size_t)W * 3 &&
                       pitch <= ((size_t)1 << 24) && cap >= 0,
                   CMDIAD_ERR_ARG, "%s: bad sizes H=%d W=%d (1..%d, H*W <= 2^26) pitch=%zu (>= 3 W floats) cap=%d", name, H, W, kMaxSide,
                   pitch, cap);
    const CompactWs ws = compact_layout(workspace, H, W, edges);
    if (const int rc = workspace_ok(name, workspace, workspace_bytes, ws.total)) return rc;
    int* const block_count = ws.block_count;
    const int L = (int)seq_length(H, W, edges);
    const int blocks = (L + 255) / 256;
    hipLaunchKernelGGL(compact_count_kernel, dim3(blocks), dim3(256), 0, s, pc, pitch, H, W, edges, L, block_count);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(1024), 0, s, (const int*)block_count, block_count, blocks, (const int*)nullptr);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(compact_scatter_kernel, dim3(blocks), dim3(256), 0, s, pc, pitch, H, W, edges, L, (const int*)block_count, blocks, cap,
                       points, index, count);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" size_t cmdiad_scan_edges_workspace_bytes(int H, int W) { return compact_workspace(H, W, 1); }

extern "C" int cmdiad_scan_edges(const float* pc, size_t pitch, int H, int W, float* points, int cap, int32_t* count, void* workspace,
                                 size_t workspace_bytes, cmdiad_stream_t stream)
{
    return compact_launch("cmdiad_scan_edges", pc, pitch, H, W, 1, points, nullptr, cap, count, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

extern "C" size_t cmdiad_scan_compact_workspace_bytes(int H, int W) { return compact_workspace(H, W, 0); }

extern "C" int cmdiad_scan_compact(const float* pc, size_t pitch, int H, int W, float* points, int32_t* index, int cap, int32_t* count,
                                   void* workspace, size_t workspace_bytes, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(index, CMDIAD_ERR_ARG, "cmdiad_scan_compact: null pointer");
    return compact_launch("cmdiad_scan_compact", pc, pitch, H, W, 0, points, index, cap, count, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

extern "C" int cmdiad_keep_largest_cluster(const int32_t* labels, const int32_t* index, int N, const int32_t* hist, int bins,
                                           const int32_t* n_clusters, float* pc, uint8_t* rgb, size_t n_pixels, int rgb_bytes,
                                           int32_t* winner_out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(labels && index && hist && n_clusters && pc && winner_out && (rgb || rgb_bytes == 0), CMDIAD_ERR_ARG,
                   "cmdiad_keep_largest_cluster: null pointer");
    CMDIAD_REQUIRE(N >= 0 && N <= kMaxPoints && bins >= 1 && rgb_bytes >= 0 && rgb_bytes <= 64 && n_pixels <= ((size_t)1 << 31),
                   CMDIAD_ERR_ARG, "cmdiad_keep_largest_cluster: bad sizes N=%d (0..%d) bins=%d n_pixels=%zu rgb_bytes=%d", N, kMaxPoints,
                   bins, n_pixels, rgb_bytes);
    if (N == 0) return CMDIAD_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cluster_winner_kernel, dim3(1), dim3(256), 0, s, hist, bins, n_clusters, winner_out);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(cluster_keep_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, labels, index, N, (const int32_t*)winner_out, pc,
                       rgb, n_pixels, rgb_bytes);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
