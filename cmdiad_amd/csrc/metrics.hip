// Pixel-level metrics on the device (feature_extractors/features.py:302-324 of the reference: sklearn's roc_auc_score over every
// test pixel and utils/au_pro_util.py twice, each labelling every mask with scipy.ndimage.label and sorting every defect-free score
// on the host).  Contracts, the key transform and the edge cases: docs/metrics.md.  Everything below produces INTEGERS or
// permutation-invariant sets -- labels, sorted keys, counts -- so the results do not depend on the order in which threads or atomics
// arrive; the float64 expressions that turn them into P-AUROC and the PRO curve stay on the host (cmdiad_amd/metrics.py).
//
// cmdiad_ccl_label: 8-connected components of n masks.  The label buffer itself is the union-find forest (union_find.h: parent =
//   pixel index inside the image, -1 = background); a pixel joins its N neighbour, or else W (NW is then joined through W's own N)
//   or NW, and NE -- the other pairs among {W, NW, N, NE} are joined by those pixels themselves.  After the unions the root of a
//   component is its smallest pixel index = its first pixel in raster order, so numbering the components as scipy.ndimage.label
//   does is a prefix count of the roots per image: roots per 2048-pixel tile (the same pass flattens the forest), a scan of the
//   tile counts per image and of the component counts over the images, the rank of every root, and the relabel pass that also counts
//   the pixels of every component (lanes of a wave with the same component share one atomic).
// cmdiad_f64_to_keys / cmdiad_keys_to_f64: order-preserving map float64 <-> uint64 (-0.0 becomes +0.0), counting non-finite inputs.
// cmdiad_sort_u64: LSD radix sort, 8 passes of 8 bits, keys only, ping-pong between the keys and the workspace.  A pass: every block
//   counts the digits of its contiguous tile of kSortTile keys into a bin-major table; one block per bin scans its row; the scatter
//   re-reads the tile, each WAVE owning a contiguous quarter of it, and walks its quarter in 64-key chunks in order: peers with the
//   same digit are found with eight 64-bit ballots, the rank inside the chunk is a population count below the lane, and a per-wave,
//   per-digit cursor in LDS carries on from chunk to chunk -- stable, as every pass but the last has to be.
// cmdiad_metrics_split: defect-free pixels -> keys, defect pixels -> (score, global component id), each appended through one
//   reservation per block from an integer counter (the order inside the lists is not defined and does not matter).
// cmdiad_auc_counts: S = sum over defect pixels of #(ok < s) + #(ok <= s): two binary searches per pixel on the sorted keys
//   (integer order of the keys == order of the doubles), summed in the wave, one 64-bit integer atomic per wave.
// cmdiad_pro_hist: hist[component][#thresholds strictly below the score], thresholds in LDS, integer atomics aggregated per wave.
#include "block_scan.h"
#include "frames.h"
#include "launch.h"
#include "union_find.h"

namespace {

constexpr int kCclTile = 2048;             // pixels per block of the root count / rank passes: 8 steps of 256
constexpr int kSortTile = 4096;            // keys per block of a radix pass: 4 waves x 16 chunks of 64
constexpr int kMaxThresholds = 1024;

__device__ __forceinline__ unsigned long long lanes_below() { return (1ull << lane_id()) - 1ull; }

__device__ __forceinline__ bool f64_nonfinite(double x)
{
    return ((unsigned long long)__double_as_longlong(x) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull;
}

// ---------------------------------------------------------------------------------------------------------------- labelling
// grid (ceil(HW / 256), n).  labels[img][p] = p for a foreground pixel (value != 0), -1 otherwise; *nonbinary counts values that are
// neither 0 nor 1 (a NaN is one).
template <typename T>
__global__ __launch_bounds__(256) void ccl_init_kernel(const T* __restrict__ mask, int HW, int32_t* __restrict__ labels,
                                                       int32_t* __restrict__ nonbinary)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const size_t at = (size_t)blockIdx.y * HW + p;
    bool bad = false;
    if (p < HW) {
        const T v = mask[at];
        labels[at] = v != (T)0 ? p : -1;
        bad = !(v == (T)0 || v == (T)1);
    }
    const int nbad = __popcll(__ballot(bad));
    if (nonbinary && nbad && lane_id() == 0) atomicAdd(nonbinary, nbad);
}

__global__ __launch_bounds__(256) void ccl_union_kernel(int32_t* __restrict__ labels, int HW, int W)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    int* par = labels + (size_t)blockIdx.y * HW;
    if (uf_load(par + p) < 0) return;
    const int y = p / W, x = p - y * W;
    const bool up = y > 0, left = x > 0, right = x + 1 < W;
    if (up && uf_load(par + p - W) >= 0) {
        uf_union(par, p, p - W);
        return;
    }
    if (left && uf_load(par + p - 1) >= 0) uf_union(par, p, p - 1);
    else if (up && left && uf_load(par + p - W - 1) >= 0) uf_union(par, p, p - W - 1);
    if (up && right && uf_load(par + p - W + 1) >= 0) uf_union(par, p, p - W + 1);
}

// grid (tiles, n).  Flattens the forest (labels[p] = root) and counts the roots of the tile.
__global__ __launch_bounds__(256) void ccl_count_kernel(int32_t* __restrict__ labels, int HW, int tiles, int32_t* __restrict__ tile_count)
{
    __shared__ int sh[4];
    int* par = labels + (size_t)blockIdx.y * HW;
    int cnt = 0;
    for (int step = 0; step < kCclTile / 256; ++step) {
        const int p = blockIdx.x * kCclTile + step * 256 + threadIdx.x;
        bool root = false;
        if (p < HW && uf_load(par + p) >= 0) {
            const int r = uf_find(par, p);
            if (r != p) atomicMin(par + p, r);
            root = r == p;
        }
        cnt += __popcll(__ballot(root));
    }
    if (lane_id() == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[(size_t)blockIdx.y * tiles + blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// grid (rows), one block per row: out[row][i] = exclusive sum of in[row][0..i), total[row] = the sum (in == out allowed)
__global__ __launch_bounds__(256) void row_excl_scan_kernel(const int32_t* in, int32_t* out, int len, int32_t* __restrict__ total)
{
    __shared__ int sh[4];
    const int32_t* src = in + (size_t)blockIdx.x * len;
    int32_t* dst = out + (size_t)blockIdx.x * len;
    int running = 0;
    for (int s = 0; s < len; s += 256) {
        const int i = s + threadIdx.x;
        const int v = i < len ? src[i] : 0;
        int tot;
        __syncthreads();   // sh may still be read from the previous chunk
        const int e = block_excl_scan<4>(v, sh, tot);
        if (i < len) dst[i] = running + e;
        running += tot;
    }
    if (total && threadIdx.x == 0) total[blockIdx.x] = running;
}

// grid (tiles, n).  rank[img][p] = 1-based raster-order number of the component whose root is p (written at roots only).
__global__ __launch_bounds__(256) void ccl_rank_kernel(const int32_t* __restrict__ labels, int HW, int tiles,
                                                       const int32_t* __restrict__ tile_off, int32_t* __restrict__ rank)
{
    __shared__ int cnt[kCclTile / 64];   // roots per (step, wave), in pixel order
    const size_t img = (size_t)blockIdx.y * HW;
    const int wave = threadIdx.x >> 6;
    unsigned long long mine[kCclTile / 256];
#pragma unroll
    for (int step = 0; step < kCclTile / 256; ++step) {
        const int p = blockIdx.x * kCclTile + step * 256 + threadIdx.x;
        const bool root = p < HW && labels[img + p] == p;
        mine[step] = __ballot(root);
        if (lane_id() == 0) cnt[step * 4 + wave] = __popcll(mine[step]);
    }
    __syncthreads();
    int before = tile_off[(size_t)blockIdx.y * tiles + blockIdx.x];
#pragma unroll
    for (int step = 0; step < kCclTile / 256; ++step) {
        const int p = blockIdx.x * kCclTile + step * 256 + threadIdx.x;
        int pre = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int c = cnt[step * 4 + w];
            pre += w < wave ? c : 0;
            all += c;
        }
        if ((mine[step] >> lane_id()) & 1) rank[img + p] = before + pre + __popcll(mine[step] & lanes_below()) + 1;
        before += all;
    }
}

// grid (ceil(HW / 256), n).  labels[p]: root -> the component's number (0 = background); comp_size[comp_offset[img] + number - 1] += 1
__global__ __launch_bounds__(256) void ccl_relabel_kernel(int32_t* __restrict__ labels, int HW, const int32_t* __restrict__ rank,
                                                          const int32_t* __restrict__ comp_offset, int32_t* __restrict__ comp_size,
                                                          int comp_cap)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const size_t img = (size_t)blockIdx.y * HW;
    int lab = 0;
    if (p < HW) {
        const int r = labels[img + p];
        lab = r >= 0 ? rank[img + r] : 0;
        labels[img + p] = lab;
    }
    const long long g = (long long)comp_offset[blockIdx.y] + lab - 1;
    wave_agg_inc(comp_size, g, lab > 0 && g < comp_cap);
}

// ---------------------------------------------------------------------------------------------------------------- keys and sort
__global__ __launch_bounds__(256) void f64_to_keys_kernel(const double* __restrict__ x, int n, unsigned long long* __restrict__ keys,
                                                          int32_t* __restrict__ nonfinite)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const double v = x[i];
        bad = f64_nonfinite(v);
        keys[i] = f64_key(v);
    }
    const int nbad = __popcll(__ballot(bad));
    if (nonfinite && nbad && lane_id() == 0) atomicAdd(nonfinite, nbad);
}

__global__ __launch_bounds__(256) void keys_to_f64_kernel(const unsigned long long* __restrict__ keys, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = key_f64(keys[i]);
}

// key index of (block, wave, chunk, lane): a wave owns a contiguous quarter of the block's tile
__device__ __forceinline__ size_t sort_index(int chunk)
{
    return (size_t)blockIdx.x * kSortTile + (threadIdx.x >> 6) * (kSortTile / 4) + chunk * 64 + lane_id();
}

// grid (nb).  table[digit][block] = keys of the block's tile with that digit
__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned long long* __restrict__ keys, int n, int shift, int nb,
                                                        uint32_t* __restrict__ table)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < kSortTile / 256; ++c) {
        const size_t i = sort_index(c);
        if (i < (size_t)n) atomicAdd(&h[(keys[i] >> shift) & 255], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// grid (nb).  Stable scatter of the block's tile by the digit at `shift`.  table: the row-wise exclusive scan of sort_hist_kernel's
// counts, totals [256]: keys per digit.
__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                           int n, int shift, int nb, const uint32_t* __restrict__ table,
                                                           const int32_t* __restrict__ totals)
{
    constexpr int kChunks = kSortTile / 256;
    __shared__ uint32_t cursor[4][256];   // first the counts per (wave, digit), then where the wave's next key of that digit goes
    __shared__ int sh[4];
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int w = 0; w < 4; ++w) cursor[w][threadIdx.x] = 0;
    __syncthreads();
    unsigned long long k[kChunks];
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const size_t i = sort_index(c);
        k[c] = i < (size_t)n ? in[i] : 0;
        if (i < (size_t)n) atomicAdd(&cursor[wave][(k[c] >> shift) & 255], 1u);
    }
    __syncthreads();
    {   // thread = digit: keys with smaller digits + this digit's keys in earlier blocks + in earlier waves of this block
        int unused;
        uint32_t g = (uint32_t)block_excl_scan<4>(totals[threadIdx.x], sh, unused) + table[(size_t)threadIdx.x * nb + blockIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t c = cursor[w][threadIdx.x];
            cursor[w][threadIdx.x] = g;
            g += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < kChunks; ++c) {
        const bool valid = sort_index(c) < (size_t)n;
        const unsigned d = (unsigned)(k[c] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const int before = __popcll(peers & lanes_below());
        const uint32_t base = cursor[wave][d];
        __builtin_amdgcn_wave_barrier();   // every lane has read the cursor before the first peer moves it
        if (valid) {
            const uint32_t at = base + before;
            if (at < (uint32_t)n) out[at] = k[c];
            if (before == 0) cursor[wave][d] = base + __popcll(peers);
        }
        __builtin_amdgcn_wave_barrier();   // the wave's LDS accesses are issued in order: the next chunk reads the moved cursor
    }
}

// ---------------------------------------------------------------------------------------------------------------- split
// grid (ceil(HW / 256), n).  counts[0] / counts[1]: lengths of the two lists.
__global__ __launch_bounds__(256) void metrics_split_kernel(const double* __restrict__ preds, const int32_t* __restrict__ labels,
                                                            const int32_t* __restrict__ comp_offset, int HW,
                                                            unsigned long long* __restrict__ ok_keys, int ok_cap,
                                                            double* __restrict__ def_score, int32_t* __restrict__ def_comp, int def_cap,
                                                            unsigned long long* __restrict__ counts, int32_t* __restrict__ nonfinite)
{
    __shared__ int sh_ok[4], sh_def[4];
    __shared__ unsigned long long base[2];
    const int p = blockIdx.x * 256 + threadIdx.x, wave = threadIdx.x >> 6;
    const size_t at = (size_t)blockIdx.y * HW + p;
    const bool in = p < HW;
    const int lab = in ? labels[at] : 0;
    const double s = in ? preds[at] : 0.0;
    const bool ok = in && lab == 0, def = in && lab > 0;
    const unsigned long long m_ok = __ballot(ok), m_def = __ballot(def);
    const int nbad = __popcll(__ballot(in && f64_nonfinite(s)));
    if (nonfinite && nbad && lane_id() == 0) atomicAdd(nonfinite, nbad);
    if (lane_id() == 0) sh_ok[wave] = __popcll(m_ok), sh_def[wave] = __popcll(m_def);
    __syncthreads();
    if (threadIdx.x < 2) {
        const int* sh = threadIdx.x == 0 ? sh_ok : sh_def;
        const int tot = sh[0] + sh[1] + sh[2] + sh[3];
        base[threadIdx.x] = tot ? atomicAdd(&counts[threadIdx.x], (unsigned long long)tot) : 0;
    }
    __syncthreads();
    int pre_ok = 0, pre_def = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) pre_ok += w < wave ? sh_ok[w] : 0, pre_def += w < wave ? sh_def[w] : 0;
    if (ok) {
        const unsigned long long o = base[0] + pre_ok + __popcll(m_ok & lanes_below());
        if (o < (unsigned long long)ok_cap) ok_keys[o] = f64_key(s);
    }
    if (def) {
        const unsigned long long o = base[1] + pre_def + __popcll(m_def & lanes_below());
        if (o < (unsigned long long)def_cap) def_score[o] = s, def_comp[o] = comp_offset[blockIdx.y] + lab - 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------- counts
// number of keys[0..n) that are < k (kOrEqual: <= k)
template <bool kOrEqual>
__device__ __forceinline__ int count_below(const unsigned long long* __restrict__ keys, int n, unsigned long long k)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const unsigned long long v = keys[mid];
        if (kOrEqual ? v <= k : v < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void auc_counts_kernel(const unsigned long long* __restrict__ ok_sorted, int n_ok,
                                                         const double* __restrict__ def_score, int n_def,
                                                         unsigned long long* __restrict__ S)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    unsigned long long c = 0;
    if (i < n_def) {
        const unsigned long long k = f64_key(def_score[i]);
        c = (unsigned long long)count_below<false>(ok_sorted, n_ok, k) + (unsigned long long)count_below<true>(ok_sorted, n_ok, k);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += shfl_xor_u64(c, m);
    if (lane_id() == 0 && c) atomicAdd(S, c);
}

__global__ __launch_bounds__(256) void pro_hist_kernel(const double* __restrict__ thr, int T, const double* __restrict__ def_score,
                                                       const int32_t* __restrict__ def_comp, int n_def, int total_comp,
                                                       uint32_t* __restrict__ hist)
{
    __shared__ double t[kMaxThresholds];
    for (int j = threadIdx.x; j < T; j += 256) t[j] = thr[j];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    long long idx = 0;
    bool active = false;
    if (i < n_def) {
        const double s = def_score[i];
        const int c = def_comp[i];
        int lo = 0, hi = T;   // thresholds strictly below s
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (t[mid] < s) lo = mid + 1;
            else hi = mid;
        }
        active = c >= 0 && c < total_comp;
        idx = (long long)c * (T + 1) + lo;
    }
    wave_agg_inc(hist, idx, active);
}

// rank [n, HW] | roots per tile [n, tiles] | their exclusive scan per image
struct CclWs { int tiles; int32_t *rank, *tile_count, *tile_off; size_t total; };
inline CclWs ccl_layout(void* base, int n, int HW)
{
    const int tiles = (HW + kCclTile - 1) / kCclTile;
    Carve c(base);
    return {tiles, c.take<int32_t>((size_t)n * HW, 256), c.take<int32_t>((size_t)n * tiles, 256), c.take<int32_t>((size_t)n * tiles, 256), c.total()};
}

// the second copy of the keys | digit counts [256][nb] | the digit totals (not padded)
struct SortWs { int nb; unsigned long long* alt; uint32_t* table; int32_t* totals; size_t total; };
inline SortWs sort_layout(void* base, int n)
{
    const int nb = (n + kSortTile - 1) / kSortTile;
    Carve c(base);
    return {nb, c.take<unsigned long long>(n, 256), c.take<uint32_t>((size_t)nb * 256, 256), c.take<int32_t>(256), c.total()};
}

inline unsigned blocks256(int n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" size_t cmdiad_ccl_workspace_bytes(int n, int H, int W)
{
    return sizes_ok(n, H, W) && n > 0 ? ccl_layout(nullptr, n, H * W).total : 0;
}

extern "C" int cmdiad_ccl_label(const void* masks, int mask_is_u8, int n, int H, int W, int32_t* labels, int32_t* n_comp,
                                int32_t* comp_offset, int32_t* comp_size, int comp_cap, int32_t* nonbinary, void* workspace,
                                size_t workspace_bytes, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(sizes_ok(n, H, W) && comp_cap >= 0 && (mask_is_u8 == 0 || mask_is_u8 == 1), CMDIAD_ERR_ARG,
                   "cmdiad_ccl_label: bad sizes n=%d (0..%d) H=%d W=%d (>= 1, H*W <= %d, n*H*W <= %d) comp_cap=%d mask_is_u8=%d", n,
                   kMaxImages, H, W, kMaxImagePixels, kMaxTotal, comp_cap, mask_is_u8);
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        if (comp_offset) CMDIAD_CHECK_HIP("cmdiad_ccl_label", hipMemsetAsync(comp_offset, 0, sizeof(int32_t), s));
        return CMDIAD_OK;
    }
    CMDIAD_REQUIRE(masks && labels && n_comp && comp_offset && comp_size && workspace, CMDIAD_ERR_ARG, "cmdiad_ccl_label: null pointer");
    const int HW = H * W;
    const CclWs L = ccl_layout(workspace, n, HW);
    if (const int rc = workspace_ok("cmdiad_ccl_label", workspace, workspace_bytes, L.total)) return rc;
    // the pixels of a 2 x 2 cell touch one another, so a cell meets at most one component: at most ceil(H/2) ceil(W/2) per image
    const long long most = (long long)n * ((H + 1) / 2) * ((W + 1) / 2);
    CMDIAD_REQUIRE(comp_cap >= most, CMDIAD_ERR_ARG, "cmdiad_ccl_label: comp_size holds %d components, %lld are possible (n ceil(H/2) ceil(W/2))",
                   comp_cap, most);
    const dim3 px(blocks256(HW), (unsigned)n), tl((unsigned)L.tiles, (unsigned)n);
    CMDIAD_CHECK_HIP("cmdiad_ccl_label", hipMemsetAsync(comp_size, 0, (size_t)comp_cap * 4, s));
    if (nonbinary) CMDIAD_CHECK_HIP("cmdiad_ccl_label", hipMemsetAsync(nonbinary, 0, sizeof(int32_t), s));
    if (mask_is_u8) hipLaunchKernelGGL(ccl_init_kernel<uint8_t>, px, dim3(256), 0, s, (const uint8_t*)masks, HW, labels, nonbinary);
    else hipLaunchKernelGGL(ccl_init_kernel<float>, px, dim3(256), 0, s, (const float*)masks, HW, labels, nonbinary);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_union_kernel, px, dim3(256), 0, s, labels, HW, W);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_count_kernel, tl, dim3(256), 0, s, labels, HW, L.tiles, L.tile_count);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(row_excl_scan_kernel, dim3((unsigned)n), dim3(256), 0, s, (const int32_t*)L.tile_count, L.tile_off, L.tiles, n_comp);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(row_excl_scan_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)n_comp, comp_offset, n, comp_offset + n);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_rank_kernel, tl, dim3(256), 0, s, (const int32_t*)labels, HW, L.tiles, (const int32_t*)L.tile_off, L.rank);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(ccl_relabel_kernel, px, dim3(256), 0, s, labels, HW, (const int32_t*)L.rank, (const int32_t*)comp_offset, comp_size,
                       comp_cap);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_f64_to_keys(const double* x, int n, uint64_t* keys, int32_t* nonfinite, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxTotal, CMDIAD_ERR_ARG, "cmdiad_f64_to_keys: bad size n=%d (0..%d)", n, kMaxTotal);
    if (nonfinite) CMDIAD_CHECK_HIP("cmdiad_f64_to_keys", hipMemsetAsync(nonfinite, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(x && keys, CMDIAD_ERR_ARG, "cmdiad_f64_to_keys: null pointer");
    hipLaunchKernelGGL(f64_to_keys_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, x, n, (unsigned long long*)keys,
                       nonfinite);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_keys_to_f64(const uint64_t* keys, int n, double* out, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxTotal, CMDIAD_ERR_ARG, "cmdiad_keys_to_f64: bad size n=%d (0..%d)", n, kMaxTotal);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(keys && out, CMDIAD_ERR_ARG, "cmdiad_keys_to_f64: null pointer");
    hipLaunchKernelGGL(keys_to_f64_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)keys, n, out);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" size_t cmdiad_sort_u64_tile(void) { return kSortTile; }

extern "C" size_t cmdiad_sort_u64_workspace_bytes(int n) { return n > 0 && n <= kMaxTotal ? sort_layout(nullptr, n).total : 0; }

extern "C" int cmdiad_sort_u64(uint64_t* keys, int n, void* workspace, size_t workspace_bytes, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxTotal, CMDIAD_ERR_ARG, "cmdiad_sort_u64: bad size n=%d (0..%d)", n, kMaxTotal);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(keys && workspace, CMDIAD_ERR_ARG, "cmdiad_sort_u64: null pointer");
    const SortWs L = sort_layout(workspace, n);
    if (const int rc = workspace_ok("cmdiad_sort_u64", workspace, workspace_bytes, L.total)) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* a = (unsigned long long*)keys;
    unsigned long long* b = L.alt;
    for (int shift = 0; shift < 64; shift += 8) {   // eight passes: the result ends where it started
        hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)L.nb), dim3(256), 0, s, (const unsigned long long*)a, n, shift, L.nb, L.table);
        CMDIAD_CHECK_LAUNCH();
        hipLaunchKernelGGL(row_excl_scan_kernel, dim3(256), dim3(256), 0, s, (const int32_t*)L.table, (int32_t*)L.table, L.nb, L.totals);
        CMDIAD_CHECK_LAUNCH();
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)L.nb), dim3(256), 0, s, (const unsigned long long*)a, b, n, shift, L.nb,
                           (const uint32_t*)L.table, (const int32_t*)L.totals);
        CMDIAD_CHECK_LAUNCH();
        unsigned long long* t = a;
        a = b;
        b = t;
    }
    return CMDIAD_OK;
}

extern "C" int cmdiad_metrics_split(const double* preds, const int32_t* labels, const int32_t* comp_offset, int n, int HW,
                                    uint64_t* ok_keys, int ok_cap, double* def_score, int32_t* def_comp, int def_cap,
                                    uint64_t* counts, int32_t* nonfinite, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxImages && HW >= 0 && HW <= kMaxImagePixels && (long long)n * HW <= kMaxTotal && ok_cap >= 0 &&
                       def_cap >= 0, CMDIAD_ERR_ARG,
                   "cmdiad_metrics_split: bad sizes n=%d (0..%d) HW=%d (0..%d, n*HW <= %d) ok_cap=%d def_cap=%d", n, kMaxImages, HW,
                   kMaxImagePixels, kMaxTotal, ok_cap, def_cap);
    hipStream_t s = (hipStream_t)stream;
    if (counts) CMDIAD_CHECK_HIP("cmdiad_metrics_split", hipMemsetAsync(counts, 0, 2 * sizeof(uint64_t), s));
    if (nonfinite) CMDIAD_CHECK_HIP("cmdiad_metrics_split", hipMemsetAsync(nonfinite, 0, sizeof(int32_t), s));
    if (n == 0 || HW == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(preds && labels && comp_offset && counts && (ok_keys || ok_cap == 0) && ((def_score && def_comp) || def_cap == 0),
                   CMDIAD_ERR_ARG, "cmdiad_metrics_split: null pointer");
    hipLaunchKernelGGL(metrics_split_kernel, dim3(blocks256(HW), (unsigned)n), dim3(256), 0, s, preds, labels, comp_offset, HW,
                       (unsigned long long*)ok_keys, ok_cap, def_score, def_comp, def_cap, (unsigned long long*)counts, nonfinite);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_auc_counts(const uint64_t* ok_sorted_keys, int n_ok, const double* def_score, int n_def, uint64_t* S,
                                 cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n_ok >= 0 && n_ok <= kMaxTotal && n_def >= 0 && n_def <= kMaxTotal, CMDIAD_ERR_ARG,
                   "cmdiad_auc_counts: bad sizes n_ok=%d n_def=%d (0..%d)", n_ok, n_def, kMaxTotal);
    if (S) CMDIAD_CHECK_HIP("cmdiad_auc_counts", hipMemsetAsync(S, 0, sizeof(uint64_t), (hipStream_t)stream));
    if (n_def == 0 || n_ok == 0) return CMDIAD_OK;   // every count is 0
    CMDIAD_REQUIRE(ok_sorted_keys && def_score && S, CMDIAD_ERR_ARG, "cmdiad_auc_counts: null pointer");
    hipLaunchKernelGGL(auc_counts_kernel, dim3(blocks256(n_def)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)ok_sorted_keys, n_ok, def_score, n_def, (unsigned long long*)S);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_pro_hist(const double* thr, int T, const double* def_score, const int32_t* def_comp, int n_def, int total_comp,
                               uint32_t* hist, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(T >= 0 && T <= kMaxThresholds && n_def >= 0 && n_def <= kMaxTotal && total_comp >= 0 &&
                       (long long)total_comp * (T + 1) <= (1ll << 28), CMDIAD_ERR_ARG,
                   "cmdiad_pro_hist: bad sizes T=%d (0..%d) n_def=%d (0..%d) total_comp=%d (total_comp * (T + 1) <= 2^28 entries)", T,
                   kMaxThresholds, n_def, kMaxTotal, total_comp);
    if (n_def == 0 || total_comp == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(def_score && def_comp && hist && (thr || T == 0), CMDIAD_ERR_ARG, "cmdiad_pro_hist: null pointer");
    hipLaunchKernelGGL(pro_hist_kernel, dim3(blocks256(n_def)), dim3(256), 0, (hipStream_t)stream, thr, T, def_score, def_comp, n_def,
                       total_comp, hist);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
