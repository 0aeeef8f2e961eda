// Defect regions of score maps on the device (docs/regions.md): threshold -> mask, cmdiad_ccl_label (metrics.hip, unchanged) ->
// labels, and here the per-component statistics and the selection of the strongest regions into a fixed-size table.
// Everything but score_sum is an integer or a stored double picked by integer work, so nothing depends on the order in which
// threads or atomics arrive: the peak is an integer atomicMax on the order-preserving 64-bit key of the score (the key transform of
// metrics.hip), its position an atomicMin of the pixel index among the pixels whose key equals it, the box atomicMin / atomicMax,
// the centroid two exact 64-bit integer sums and one float64 division each.  No float goes through an atomic.  score_sum is
// computed for the kept regions only, by the selecting workgroup: it walks the region's bounding box in raster order, thread t
// taking box pixels t, t + 256, ..., then a fixed butterfly inside each wave and ((w0 + w1) + (w2 + w3)) over the four waves --
// an order that depends on the component's pixels alone, not on the batch, the image's place in it, or the run.
//
// cmdiad_threshold_mask: mask = score > thr as a comparison of doubles (a NaN is background and counted), thr read from DEVICE
//   memory (one value or one per image) so that a captured graph follows a threshold that changes between replays.
// cmdiad_region_table: two pixel passes (statistics, then the peak's first pixel) over tables of the labelling's own capacity
//   n ceil(H/2) ceil(W/2) -- every index into them is checked against it -- and one workgroup per image that runs K rounds of
//   "largest (key(peak), lowest label) strictly after the previous pick" over the components with area >= min_area: the order is
//   total, so no table of taken components is needed and no rank is counted.  The launch geometry depends on n, H, W alone.
// cmdiad_region_measure: the kept regions in the units of the organised cloud -- valid points, per-axis extent, first and second
//   moments about the minimum corner, the area of the triangle mesh -- by one workgroup per (slot, image) in score_sum's order.
#include <limits.h>

#include "block_scan.h"
#include "cloud.h"
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kMaxRegions = 64;

// per global component id, each of `cap` entries
struct RegionTables {
    unsigned long long* key;    // max of the score keys (0 = below every real key)
    unsigned long long* sumx;   // exact sums of the columns / rows
    unsigned long long* sumy;
    int32_t* x1;
    int32_t* y1;
    int32_t* x0;                // the three "min" tables start at 0x7F7F7F7F
    int32_t* y0;
    int32_t* pidx;              // first pixel (raster order) whose key equals key[]
};

// the tables of `cap` components; entries per table = cap rounded up to 64, so every table starts 256-byte aligned
struct RegionWs { size_t stride; RegionTables T; size_t total; };
inline RegionWs region_layout(void* base, long long cap)
{
    const size_t stride = ((size_t)cap + 63) & ~(size_t)63;
    Carve c(base);
    return {stride, {c.take<unsigned long long>(stride), c.take<unsigned long long>(stride), c.take<unsigned long long>(stride),
                     c.take<int32_t>(stride), c.take<int32_t>(stride), c.take<int32_t>(stride), c.take<int32_t>(stride), c.take<int32_t>(stride)},
            c.total()};
}

inline long long most_components(int n, int H, int W) { return (long long)n * ((H + 1) / 2) * ((W + 1) / 2); }

// ---------------------------------------------------------------------------------------------------------------- threshold
// grid (ceil(HW / 512), n): a lane takes pixels 2t and 2t + 1 of its image.  kVec: HW is even and both buffers are aligned, so the
// pair is one 16-byte load and one 2-byte store.
template <bool kVec>
__global__ __launch_bounds__(256) void threshold_mask_kernel(const double* __restrict__ maps, const double* __restrict__ thr,
                                                             int thr_per_image, int HW, uint8_t* __restrict__ mask,
                                                             int32_t* __restrict__ nan_count)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t at = (size_t)blockIdx.y * HW + p;
    const double t = thr[thr_per_image ? blockIdx.y : 0];
    int bad = 0;
    if (kVec) {
        if (p < HW) {   // p + 1 < HW as well: both are even
            const double2 s = *reinterpret_cast<const double2*>(maps + at);
            bad = (s.x != s.x) + (s.y != s.y);
            const unsigned short m = (unsigned short)((s.x > t ? 1u : 0u) | (s.y > t ? 0x100u : 0u));
            *reinterpret_cast<unsigned short*>(mask + at) = m;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (p + k < HW) {
                const double s = maps[at + k];
                bad += s != s;
                mask[at + k] = s > t ? 1 : 0;
            }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if (nan_count && bad && lane_id() == 0) atomicAdd(nan_count, bad);
}

// ---------------------------------------------------------------------------------------------------------------- statistics
// The tables' start values, written by a kernel and not by memset calls: 32 bytes of zero and three 0x7F7F7F7F per slot.
__global__ __launch_bounds__(256) void region_init_kernel(RegionTables T, int stride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    T.key[i] = 0ull, T.sumx[i] = 0ull, T.sumy[i] = 0ull;
    T.x1[i] = 0, T.y1[i] = 0;
    T.x0[i] = 0x7F7F7F7F, T.y0[i] = 0x7F7F7F7F, T.pidx[i] = 0x7F7F7F7F;
}

template <bool kVec>
__device__ __forceinline__ void load_pair(const double* __restrict__ maps, const int32_t* __restrict__ labels, size_t at, int p, int HW,
                                          double s[2], int lab[2])
{
    s[0] = s[1] = 0.0;
    lab[0] = lab[1] = 0;
    if (kVec) {
        if (p < HW) {
            const double2 v = *reinterpret_cast<const double2*>(maps + at);
            const int2 l = *reinterpret_cast<const int2*>(labels + at);
            s[0] = v.x, s[1] = v.y, lab[0] = l.x, lab[1] = l.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (p + k < HW) s[k] = maps[at + k], lab[k] = labels[at + k];
    }
}

// One pixel per lane into the tables of component g; every lane of the wave calls it.  When all active lanes of the wave belong to
// one component (the inside of a blob) the wave reduces first and its leader issues the seven atomics.
__device__ __forceinline__ void stats_update(const RegionTables& T, int g, bool active, unsigned long long key, int x, int y)
{
    const unsigned long long todo = __ballot(active);
    if (!todo) return;   // wave-uniform
    const int leader = __ffsll((long long)todo) - 1;
    const int lg = __shfl(g, leader, 64);
    if (__ballot(active && g == lg) == todo) {
        unsigned long long k = active ? key : 0ull;
        int mnx = active ? x : INT_MAX, mny = active ? y : INT_MAX, mxx = active ? x : -1, mxy = active ? y : -1;
        unsigned sx = active ? (unsigned)x : 0u, sy = active ? (unsigned)y : 0u;   // 64 values below 2^24 each
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long ok = shfl_xor_u64(k, m);
            k = ok > k ? ok : k;
            mnx = min(mnx, __shfl_xor(mnx, m, 64));
            mny = min(mny, __shfl_xor(mny, m, 64));
            mxx = max(mxx, __shfl_xor(mxx, m, 64));
            mxy = max(mxy, __shfl_xor(mxy, m, 64));
            sx += __shfl_xor(sx, m, 64);
            sy += __shfl_xor(sy, m, 64);
        }
        if (lane_id() == leader) {
            atomicMax(T.key + lg, k);
            atomicMin(T.x0 + lg, mnx);
            atomicMin(T.y0 + lg, mny);
            atomicMax(T.x1 + lg, mxx);
            atomicMax(T.y1 + lg, mxy);
            atomicAdd(T.sumx + lg, (unsigned long long)sx);
            atomicAdd(T.sumy + lg, (unsigned long long)sy);
        }
    } else if (active) {
        atomicMax(T.key + g, key);
        atomicMin(T.x0 + g, x);
        atomicMin(T.y0 + g, y);
        atomicMax(T.x1 + g, x);
        atomicMax(T.y1 + g, y);
        atomicAdd(T.sumx + g, (unsigned long long)x);
        atomicAdd(T.sumy + g, (unsigned long long)y);
    }
}

// grid (ceil(HW / 512), n)
template <bool kVec>
__global__ __launch_bounds__(256) void region_stats_kernel(const double* __restrict__ maps, const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ comp_offset, int HW, int W, int cap, RegionTables T)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t at = (size_t)blockIdx.y * HW + p;
    double s[2];
    int lab[2];
    load_pair<kVec>(maps, labels, at, p, HW, s, lab);
    const long long off = comp_offset[blockIdx.y];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long long g = off + lab[k] - 1;
        const bool active = lab[k] > 0 && g >= 0 && g < cap;
        const int q = p + k, y = q / W;
        stats_update(T, (int)g, active, f64_key(s[k]), q - y * W, y);
    }
}

// grid (ceil(HW / 512), n), after region_stats_kernel has finished: the first pixel whose key is the component's largest
template <bool kVec>
__global__ __launch_bounds__(256) void region_peak_kernel(const double* __restrict__ maps, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ comp_offset, int HW, int cap, RegionTables T)
{
    const int p = (blockIdx.x * 256 + threadIdx.x) * 2;
    const size_t at = (size_t)blockIdx.y * HW + p;
    double s[2];
    int lab[2];
    load_pair<kVec>(maps, labels, at, p, HW, s, lab);
    const long long off = comp_offset[blockIdx.y];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long long g = off + lab[k] - 1;
        if (lab[k] > 0 && g >= 0 && g < cap && f64_key(s[k]) == T.key[g]) atomicMin(T.pidx + g, p + k);
    }
}

// ---------------------------------------------------------------------------------------------------------------- selection
// (key, label) a comes before b: larger peak first, then the lower label
__device__ __forceinline__ bool comes_before(unsigned long long ka, int la, unsigned long long kb, int lb)
{
    return ka > kb || (ka == kb && la < lb);
}

// grid (n), one workgroup per image
__global__ __launch_bounds__(256) void region_select_kernel(const double* __restrict__ maps, const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ n_comp, const int32_t* __restrict__ comp_offset,
                                                            const int32_t* __restrict__ comp_size, int H, int W, int cap, int min_area,
                                                            int K, RegionTables T, int32_t* __restrict__ count,
                                                            int32_t* __restrict__ ints, double* __restrict__ vals)
{
    __shared__ int sh_count;
    __shared__ unsigned long long sh_k[4];
    __shared__ int sh_l[4];
    __shared__ double sh_d[4];
    const int img = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int HW = H * W;
    const size_t base = (size_t)img * HW;
    long long off = comp_offset[img];
    long long nc = n_comp[img];
    if (off < 0 || off > cap) off = cap;          // a table the labelling did not write: nothing is read outside the capacity
    if (nc < 0) nc = 0;
    if (nc > cap - off) nc = cap - off;
    if (tid == 0) sh_count = 0;
    __syncthreads();
    int mine = 0;
    for (int c = tid; c < nc; c += 256) mine += comp_size[off + c] >= min_area;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mine += __shfl_xor(mine, m, 64);
    if (lane_id() == 0 && mine) atomicAdd(&sh_count, mine);
    __syncthreads();
    const int total = sh_count;
    const int nsel = total < K ? total : K;
    if (tid == 0) count[img] = total;
    int32_t* my_ints = ints + (size_t)img * K * 8;
    double* my_vals = vals + (size_t)img * K * 4;
    for (int i = nsel * 8 + tid; i < K * 8; i += 256) my_ints[i] = 0;
    for (int i = nsel * 4 + tid; i < K * 4; i += 256) my_vals[i] = 0.0;

    unsigned long long pk = ~0ull;   // the previous pick: above every real key, label 0 below every real label
    int pl = 0;
    for (int r = 0; r < nsel; ++r) {
        unsigned long long bk = 0ull;
        int bl = INT_MAX;
        for (int c = tid; c < nc; c += 256) {
            if (comp_size[off + c] < min_area) continue;
            const unsigned long long k = T.key[off + c];
            const int l = c + 1;
            if (comes_before(pk, pl, k, l) && comes_before(k, l, bk, bl)) bk = k, bl = l;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long ok = shfl_xor_u64(bk, m);
            const int ol = __shfl_xor(bl, m, 64);
            if (comes_before(ok, ol, bk, bl)) bk = ok, bl = ol;
        }
        __syncthreads();   // the previous round's readers of sh_k / sh_l / sh_d are done
        if (lane_id() == 0) sh_k[wave] = bk, sh_l[wave] = bl;
        __syncthreads();
        bk = sh_k[0], bl = sh_l[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (comes_before(sh_k[w], sh_l[w], bk, bl)) bk = sh_k[w], bl = sh_l[w];
        if (bl == INT_MAX) break;   // block-uniform; cannot happen while r < nsel
        pk = bk, pl = bl;
        const long long g = off + bl - 1;
        // the region's box, clamped to the image: the walk below reads nothing outside it
        int x0 = T.x0[g], y0 = T.y0[g], x1 = T.x1[g], y1 = T.y1[g];
        x0 = max(x0, 0), y0 = max(y0, 0), x1 = min(x1, W - 1), y1 = min(y1, H - 1);
        const int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
        double sum = 0.0;
        if (bw > 0 && bh > 0) {
            const int nb = bw * bh;
            for (int j = tid; j < nb; j += 256) {
                const int yy = j / bw;
                const size_t at = base + (size_t)(y0 + yy) * W + x0 + (j - yy * bw);
                if (labels[at] == bl) sum += maps[at];
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
        if (lane_id() == 0) sh_d[wave] = sum;
        __syncthreads();
        if (tid == 0) {
            int pi = T.pidx[g];
            if (pi < 0 || pi >= HW) pi = 0;
            const int area = comp_size[g];
            const int py = pi / W;
            int32_t* o = my_ints + r * 8;
            o[0] = bl, o[1] = area, o[2] = x0, o[3] = y0, o[4] = x1, o[5] = y1, o[6] = pi - py * W, o[7] = py;
            double* v = my_vals + r * 4;
            v[0] = maps[base + pi];
            v[1] = (sh_d[0] + sh_d[1]) + (sh_d[2] + sh_d[3]);
            v[2] = (double)T.sumx[g] / (double)area;
            v[3] = (double)T.sumy[g] / (double)area;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- measurement
// The regions in the units of the organised cloud (docs/regions.md, "Contract of a measurement table"); the cloud is addressed
// through cloud.h, so both layouts are one code path.
// 0.5 |(b - a) x (c - a)| from the widened floats, every step one float64 operation rounded once (no contraction)
__device__ __forceinline__ double tri_area(const Pt& a, const Pt& b, const Pt& c)
{
#pragma clang fp contract(off)
    const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
    const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
    const double cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// grid (ceil(HW / 256), n): points with a non-finite coordinate, over the whole frames
__global__ __launch_bounds__(256) void cloud_bad_kernel(Cloud c, int HW, int32_t* __restrict__ bad_count)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    int bad = 0;
    if (q < HW) bad = !finite3(cloud_at(c, (size_t)blockIdx.y * 3 * HW, q));
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) bad += __shfl_xor(bad, m, 64);
    if (bad && lane_id() == 0) atomicAdd(bad_count, bad);
}

// grid (K, n), one workgroup per (slot, image).  Two walks over the slot's box in the order of score_sum: thread t takes box
// positions t, t + 256, ... in raster order, then the fixed 64-lane butterfly and (w0 + w1) + (w2 + w3).  Walk 1: n_pts, lo, hi
// (minimum and maximum are exact whatever the order).  Walk 2: the sums about lo, the area, n_tri.  The table is an input that is
// not trusted: count is clamped to [0, K], the box and the peak to the image, a label below 1 matches no pixel.
__global__ __launch_bounds__(256) void region_measure_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ count,
                                                             const int32_t* __restrict__ ints, Cloud c, int H, int W, int K,
                                                             int32_t* __restrict__ m_ints, double* __restrict__ m_vals)
{
#pragma clang fp contract(off)
    __shared__ int sh_i[4];
    __shared__ float sh_f[4][6];
    __shared__ double sh_d[4][10];
    const int slot = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, wave = tid >> 6;
    const int HW = H * W;
    int32_t* oi = m_ints + ((size_t)img * K + slot) * 4;
    double* ov = m_vals + ((size_t)img * K + slot) * 20;
    int cnt = count[img];
    cnt = cnt < 0 ? 0 : (cnt > K ? K : cnt);
    const int32_t* row = ints + ((size_t)img * K + slot) * 8;
    const int L = slot < cnt ? row[0] : 0;
    int x0 = 0, y0 = 0, bw = 0, bh = 0;
    if (L >= 1) {
        x0 = max(row[2], 0), y0 = max(row[3], 0);
        bw = min(row[4], W - 1) - x0 + 1, bh = min(row[5], H - 1) - y0 + 1;
    }
    const int nb = bw > 0 && bh > 0 ? bw * bh : 0;   // block-uniform
    const size_t lbase = (size_t)img * HW, cbase = (size_t)img * 3 * HW;

    int npts = 0;
    float lox = INFINITY, loy = INFINITY, loz = INFINITY, hix = -INFINITY, hiy = -INFINITY, hiz = -INFINITY;
    for (int j = tid; j < nb; j += 256) {
        const int yy = j / bw;
        const int q = (y0 + yy) * W + x0 + (j - yy * bw);
        if (labels[lbase + q] != L) continue;
        const Pt p = cloud_at(c, cbase, q);
        if (!valid_pt(p)) continue;
        ++npts;
        lox = fminf(lox, p.x), loy = fminf(loy, p.y), loz = fminf(loz, p.z);
        hix = fmaxf(hix, p.x), hiy = fmaxf(hiy, p.y), hiz = fmaxf(hiz, p.z);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        npts += __shfl_xor(npts, m, 64);
        lox = fminf(lox, __shfl_xor(lox, m, 64)), loy = fminf(loy, __shfl_xor(loy, m, 64)), loz = fminf(loz, __shfl_xor(loz, m, 64));
        hix = fmaxf(hix, __shfl_xor(hix, m, 64)), hiy = fmaxf(hiy, __shfl_xor(hiy, m, 64)), hiz = fmaxf(hiz, __shfl_xor(hiz, m, 64));
    }
    if (lane_id() == 0) {
        sh_i[wave] = npts;
        sh_f[wave][0] = lox, sh_f[wave][1] = loy, sh_f[wave][2] = loz, sh_f[wave][3] = hix, sh_f[wave][4] = hiy, sh_f[wave][5] = hiz;
    }
    __syncthreads();
    npts = (sh_i[0] + sh_i[1]) + (sh_i[2] + sh_i[3]);
    if (npts == 0) {   // block-uniform: a dead slot, an empty box, or a region without a valid point -- every value is zero
        if (tid < 4) oi[tid] = 0;
        if (tid < 20) ov[tid] = 0.0;
        return;
    }
    lox = fminf(fminf(sh_f[0][0], sh_f[1][0]), fminf(sh_f[2][0], sh_f[3][0]));
    loy = fminf(fminf(sh_f[0][1], sh_f[1][1]), fminf(sh_f[2][1], sh_f[3][1]));
    loz = fminf(fminf(sh_f[0][2], sh_f[1][2]), fminf(sh_f[2][2], sh_f[3][2]));
    hix = fmaxf(fmaxf(sh_f[0][3], sh_f[1][3]), fmaxf(sh_f[2][3], sh_f[3][3]));
    hiy = fmaxf(fmaxf(sh_f[0][4], sh_f[1][4]), fmaxf(sh_f[2][4], sh_f[3][4]));
    hiz = fmaxf(fmaxf(sh_f[0][5], sh_f[1][5]), fmaxf(sh_f[2][5], sh_f[3][5]));
    __syncthreads();   // sh_i is written again below

    const double ox = (double)lox, oy = (double)loy, oz = (double)loz;
    double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0, area = 0.0;
    int ntri = 0;
    for (int j = tid; j < nb; j += 256) {
        const int yy = j / bw;
        const int y = y0 + yy, x = x0 + (j - yy * bw);
        const int q = y * W + x;
        if (labels[lbase + q] != L) continue;
        const Pt a = cloud_at(c, cbase, q);
        if (!valid_pt(a)) continue;
        const double dx = (double)a.x - ox, dy = (double)a.y - oy, dz = (double)a.z - oz;
        sx += dx, sy += dy, sz += dz;
        sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
        if (y + 1 >= H || x + 1 >= W) continue;
        // the cell below and right of (y, x): both triangles hold the diagonal a - d
        if (labels[lbase + q + W + 1] != L) continue;
        const Pt d = cloud_at(c, cbase, q + W + 1);
        if (!valid_pt(d)) continue;
        if (labels[lbase + q + 1] == L) {
            const Pt b = cloud_at(c, cbase, q + 1);
            if (valid_pt(b)) area += tri_area(a, b, d), ++ntri;
        }
        if (labels[lbase + q + W] == L) {
            const Pt e = cloud_at(c, cbase, q + W);
            if (valid_pt(e)) area += tri_area(a, d, e), ++ntri;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        ntri += __shfl_xor(ntri, m, 64);
        sx += __shfl_xor(sx, m, 64), sy += __shfl_xor(sy, m, 64), sz += __shfl_xor(sz, m, 64);
        sxx += __shfl_xor(sxx, m, 64), sxy += __shfl_xor(sxy, m, 64), sxz += __shfl_xor(sxz, m, 64);
        syy += __shfl_xor(syy, m, 64), syz += __shfl_xor(syz, m, 64), szz += __shfl_xor(szz, m, 64);
        area += __shfl_xor(area, m, 64);
    }
    if (lane_id() == 0) {
        sh_i[wave] = ntri;
        double* o = sh_d[wave];
        o[0] = sx, o[1] = sy, o[2] = sz, o[3] = sxx, o[4] = sxy, o[5] = sxz, o[6] = syy, o[7] = syz, o[8] = szz, o[9] = area;
    }
    __syncthreads();
    if (tid < 10) ov[9 + tid] = (sh_d[0][tid] + sh_d[1][tid]) + (sh_d[2][tid] + sh_d[3][tid]);
    if (tid == 10) ov[19] = 0.0;
    if (tid == 11) {
        // the point at the peak pixel, wherever the table puts it inside the image
        const int px = row[6], py = row[7];
        Pt p = {0.f, 0.f, 0.f};
        const bool inside = px >= 0 && px < W && py >= 0 && py < H;
        if (inside) p = cloud_at(c, cbase, py * W + px);
        const bool ok = inside && valid_pt(p);
        oi[0] = npts, oi[1] = (sh_i[0] + sh_i[1]) + (sh_i[2] + sh_i[3]), oi[2] = ok ? 1 : 0, oi[3] = 0;
        ov[0] = ox, ov[1] = oy, ov[2] = oz, ov[3] = (double)hix, ov[4] = (double)hiy, ov[5] = (double)hiz;
        ov[6] = ok ? (double)p.x : 0.0, ov[7] = ok ? (double)p.y : 0.0, ov[8] = ok ? (double)p.z : 0.0;
    }
}

}  // namespace

extern "C" int cmdiad_threshold_mask(const double* maps, const double* thr, int thr_per_image, int n, int H, int W, uint8_t* mask,
                                     int32_t* nan_count, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(sizes_ok(n, H, W) && (thr_per_image == 0 || thr_per_image == 1), CMDIAD_ERR_ARG,
                   "cmdiad_threshold_mask: bad sizes n=%d (0..%d) H=%d W=%d (>= 1, H*W <= %d, n*H*W <= %d) thr_per_image=%d", n, kMaxImages,
                   H, W, kMaxImagePixels, kMaxTotal, thr_per_image);
    hipStream_t s = (hipStream_t)stream;
    CMDIAD_REQUIRE(n == 0 || (maps && thr && mask), CMDIAD_ERR_ARG, "cmdiad_threshold_mask: null pointer");
    if (nan_count) CMDIAD_CHECK_HIP("cmdiad_threshold_mask", hipMemsetAsync(nan_count, 0, sizeof(int32_t), s));
    if (n == 0) return CMDIAD_OK;
    const int HW = H * W;
    const bool vec = HW % 2 == 0 && ((uintptr_t)maps & 15) == 0 && ((uintptr_t)mask & 1) == 0;
    const dim3 grid(blocks512(HW), (unsigned)n);
    if (vec) hipLaunchKernelGGL(threshold_mask_kernel<true>, grid, dim3(256), 0, s, maps, thr, thr_per_image, HW, mask, nan_count);
    else hipLaunchKernelGGL(threshold_mask_kernel<false>, grid, dim3(256), 0, s, maps, thr, thr_per_image, HW, mask, nan_count);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" size_t cmdiad_region_table_workspace_bytes(int n, int H, int W)
{
    return sizes_ok(n, H, W) && n > 0 ? region_layout(nullptr, most_components(n, H, W)).total : 0;
}

extern "C" int cmdiad_region_table(const double* maps, const int32_t* labels, const int32_t* n_comp, const int32_t* comp_offset,
                                   const int32_t* comp_size, int comp_cap, int n, int H, int W, int min_area, int max_regions,
                                   int32_t* count, int32_t* ints, double* vals, void* workspace, size_t workspace_bytes,
                                   cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(sizes_ok(n, H, W) && comp_cap >= 0 && min_area >= 1 && max_regions >= 1 && max_regions <= kMaxRegions, CMDIAD_ERR_ARG,
                   "cmdiad_region_table: bad sizes n=%d (0..%d) H=%d W=%d (>= 1, H*W <= %d, n*H*W <= %d) comp_cap=%d min_area=%d (>= 1) "
                   "max_regions=%d (1..%d)", n, kMaxImages, H, W, kMaxImagePixels, kMaxTotal, comp_cap, min_area, max_regions, kMaxRegions);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(maps && labels && n_comp && comp_offset && comp_size && count && ints && vals && workspace, CMDIAD_ERR_ARG,
                   "cmdiad_region_table: null pointer");
    const long long most = most_components(n, H, W);
    CMDIAD_REQUIRE(comp_cap >= most, CMDIAD_ERR_ARG,
                   "cmdiad_region_table: comp_size holds %d components, %lld are possible (n ceil(H/2) ceil(W/2))", comp_cap, most);
    const RegionWs L = region_layout(workspace, most);
    if (const int rc = workspace_ok("cmdiad_region_table", workspace, workspace_bytes, L.total)) return rc;
    CMDIAD_REQUIRE(((uintptr_t)workspace & 7) == 0, CMDIAD_ERR_ARG, "cmdiad_region_table: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const RegionTables& T = L.T;
    const int HW = H * W, cap = (int)most;   // the tables' capacity: ids at or above it are skipped by every kernel
    hipLaunchKernelGGL(region_init_kernel, dim3((unsigned)((L.stride + 255) / 256)), dim3(256), 0, s, T, (int)L.stride);
    CMDIAD_CHECK_LAUNCH();
    const bool vec = HW % 2 == 0 && ((uintptr_t)maps & 15) == 0 && ((uintptr_t)labels & 7) == 0;
    const dim3 grid(blocks512(HW), (unsigned)n);
    if (vec) hipLaunchKernelGGL(region_stats_kernel<true>, grid, dim3(256), 0, s, maps, labels, comp_offset, HW, W, cap, T);
    else hipLaunchKernelGGL(region_stats_kernel<false>, grid, dim3(256), 0, s, maps, labels, comp_offset, HW, W, cap, T);
    CMDIAD_CHECK_LAUNCH();
    if (vec) hipLaunchKernelGGL(region_peak_kernel<true>, grid, dim3(256), 0, s, maps, labels, comp_offset, HW, cap, T);
    else hipLaunchKernelGGL(region_peak_kernel<false>, grid, dim3(256), 0, s, maps, labels, comp_offset, HW, cap, T);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(region_select_kernel, dim3((unsigned)n), dim3(256), 0, s, maps, labels, n_comp, comp_offset, comp_size, H, W, cap,
                       min_area, max_regions, T, count, ints, vals);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_region_measure(const int32_t* labels, const int32_t* count, const int32_t* ints, const float* cloud,
                                     long long pix_stride, long long ch_stride, int n, int H, int W, int max_regions, int32_t* m_ints,
                                     double* m_vals, int32_t* bad_count, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(sizes_ok(n, H, W) && max_regions >= 1 && max_regions <= kMaxRegions, CMDIAD_ERR_ARG,
                   "cmdiad_region_measure: bad sizes n=%d (0..%d) H=%d W=%d (>= 1, H*W <= %d, n*H*W <= %d) max_regions=%d (1..%d)", n,
                   kMaxImages, H, W, kMaxImagePixels, kMaxTotal, max_regions, kMaxRegions);
    const long long HW = (long long)H * W;
    CMDIAD_REQUIRE(cloud_strides_ok(pix_stride, ch_stride, HW), CMDIAD_ERR_ARG,
                   "cmdiad_region_measure: bad strides pix_stride=%lld ch_stride=%lld (planar [n,3,H,W]: 1 and H*W = %lld; interleaved "
                   "[n,H,W,3]: 3 and 1)", pix_stride, ch_stride, HW);
    CMDIAD_REQUIRE(n == 0 || (labels && count && ints && cloud && m_ints && m_vals), CMDIAD_ERR_ARG,
                   "cmdiad_region_measure: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (bad_count) CMDIAD_CHECK_HIP("cmdiad_region_measure", hipMemsetAsync(bad_count, 0, sizeof(int32_t), s));
    if (n == 0) return CMDIAD_OK;
    const Cloud c = {cloud, pix_stride, ch_stride};
    if (bad_count) {
        hipLaunchKernelGGL(cloud_bad_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)n), dim3(256), 0, s, c, (int)HW, bad_count);
        CMDIAD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(region_measure_kernel, dim3((unsigned)max_regions, (unsigned)n), dim3(256), 0, s, labels, count, ints, c, H, W,
                       max_regions, m_ints, m_vals);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
