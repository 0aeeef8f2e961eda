// Precision-recall numbers and defect detection counts on the device (docs/metrics.md, "Precision-recall and detection counts").
// As in metrics.hip, every result is an INTEGER or a stored key picked by integer work, so nothing depends on the order in which
// threads or atomics arrive; the float64 expressions that turn the run table into AP and F1 stay on the host
// (cmdiad_amd/metrics.py).  Integer atomics only; no cross-workgroup flag: a phase that needs another's result is another launch.
//
// cmdiad_pr_runs: the run table of the SORTED defect keys.  A run is a maximal group of equal keys, its head the first of them.
//   Heads are numbered the way the labelling numbers roots: heads per fixed tile of kPrTile keys, a scan of the tile counts, and a
//   compaction pass that ranks the heads of its tile in key order (block_scan.h) and writes, per head, the key, its index and
//   fp = n_ok - lower_bound(ok_sorted, key): the defect-free scores at or above the run's value, one binary search per head.
//   Rank = heads in front of it, so the runs come out in ascending key order whatever the launch geometry.
// cmdiad_pr_f1max: the run that maximises F1 = 2 tp / (tp + fp + n_def), tp = n_def - first.  Two fractions are compared exactly
//   by cross-multiplication in 64 bits (tp <= 2^30, denominator < 2^32), equal fractions by the run index (the larger = the higher
//   threshold wins): a total order, so the tree of the two-stage reduction does not matter.  The table is plain integers.
// cmdiad_region_overlap: per pixel that lies in a ground-truth component AND in a kept predicted component (size >= min_area),
//   covered[gt id] += 1 and hits[pred id] += 1; lanes of a wave with the same id share one atomic.  Every id is checked against
//   the capacity of the table it indexes.
// cmdiad_detection_counts: one workgroup per image folds the two tables into n_gt, n_detected, n_pred, n_false.
#include "block_scan.h"
#include "frames.h"
#include "launch.h"

namespace {

constexpr int kPrTile = 2048;               // keys per block of the head count / compaction passes: 8 steps of 256
constexpr int kF1Block = 256;               // runs per block-step of the first reduction stage
constexpr int kF1MaxBlocks = 1024;          // blocks of the first stage at most: the second stage is one block

// ---------------------------------------------------------------------------------------------------------------- run table
__device__ __forceinline__ bool run_head(const unsigned long long* __restrict__ keys, int i, int n)
{
    return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

// grid (tiles).  tile_count[tile] = run heads among the tile's keys
__global__ __launch_bounds__(256) void pr_count_kernel(const unsigned long long* __restrict__ keys, int n, int32_t* __restrict__ tile_count)
{
    __shared__ int sh[4];
    int cnt = 0;
    for (int step = 0; step < kPrTile / 256; ++step) {
        const int i = blockIdx.x * kPrTile + step * 256 + threadIdx.x;
        cnt += __popcll(__ballot(run_head(keys, i, n)));
    }
    if (lane_id() == 0) sh[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_count[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// one block: out[i] = exclusive sum of in[0..i), *total = the sum
__global__ __launch_bounds__(256) void pr_scan_kernel(const int32_t* __restrict__ in, int32_t* __restrict__ out, int len,
                                                      int32_t* __restrict__ total)
{
    __shared__ int sh[4];
    int running = 0;
    for (int s = 0; s < len; s += 256) {
        const int i = s + threadIdx.x;
        const int v = i < len ? in[i] : 0;
        int tot;
        __syncthreads();   // sh may still be read from the previous chunk
        const int e = block_excl_scan<4>(v, sh, tot);
        if (i < len) out[i] = running + e;
        running += tot;
    }
    if (threadIdx.x == 0) *total = running;
}

// number of keys[0..n) that are < k
__device__ __forceinline__ int lower_bound(const unsigned long long* __restrict__ keys, int n, unsigned long long k)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid (tiles).  The head of rank r < run_cap writes run_key[r], run_first[r], run_fp[r].
__global__ __launch_bounds__(256) void pr_compact_kernel(const unsigned long long* __restrict__ keys, int n,
                                                         const unsigned long long* __restrict__ ok_sorted, int n_ok,
                                                         const int32_t* __restrict__ tile_off, unsigned long long* __restrict__ run_key,
                                                         int32_t* __restrict__ run_first, int32_t* __restrict__ run_fp, int run_cap)
{
    __shared__ int sh[2][4];   // alternating rows: the barrier inside one call separates the reads of the call before from the next writes
    int before = tile_off[blockIdx.x];
    for (int step = 0; step < kPrTile / 256; ++step) {
        const int i = blockIdx.x * kPrTile + step * 256 + threadIdx.x;
        const bool head = run_head(keys, i, n);
        int all;
        const int r = before + block_ballot_rank<4>(head, sh[step & 1], all);
        if (head && r >= 0 && r < run_cap) {
            const unsigned long long k = keys[i];
            run_key[r] = k;
            run_first[r] = i;
            run_fp[r] = n_ok - lower_bound(ok_sorted, n_ok, k);
        }
        before += all;
    }
}

// ---------------------------------------------------------------------------------------------------------------- F1 maximum
// run a beats run b (indices into the table; -1 = none): the larger 2 tp / (tp + fp + n_def), then the larger index
__device__ __forceinline__ bool f1_better(int ra, int rb, const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_fp, int n_def)
{
    if (ra < 0) return false;
    if (rb < 0) return true;
    const unsigned long long tpa = (unsigned long long)(n_def - run_first[ra]), tpb = (unsigned long long)(n_def - run_first[rb]);
    const unsigned long long dena = tpa + (unsigned long long)run_fp[ra] + (unsigned long long)n_def;
    const unsigned long long denb = tpb + (unsigned long long)run_fp[rb] + (unsigned long long)n_def;
    const unsigned long long l = tpa * denb, r = tpb * dena;   // tp <= 2^30, den < 2^32: below 2^62
    return l > r || (l == r && ra > rb);
}

// a run the table's reader takes: 0 <= first < n_def (tp >= 1) and fp >= 0
__device__ __forceinline__ bool f1_valid(int r, const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_fp, int n_def)
{
    const int f = run_first[r];
    return f >= 0 && f < n_def && run_fp[r] >= 0;
}

// the block's best candidate, valid in thread 0
__device__ __forceinline__ int f1_block_best(int best, const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_fp, int n_def)
{
    __shared__ int sh[4];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(best, m, 64);
        if (f1_better(o, best, run_first, run_fp, n_def)) best = o;
    }
    if (lane_id() == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    best = sh[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (f1_better(sh[w], best, run_first, run_fp, n_def)) best = sh[w];
    return best;
}

// grid (nblk).  Block b takes the runs [256 j, 256 j + 256) for j = b, b + nblk, ...; partial[b] = its best run or -1
__global__ __launch_bounds__(256) void f1_partial_kernel(const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_fp,
                                                         const int32_t* __restrict__ n_runs, int run_cap, int n_def,
                                                         int32_t* __restrict__ partial)
{
    int R = *n_runs;
    R = R < 0 ? 0 : (R > run_cap ? run_cap : R);
    int best = -1;
    for (long long r = (long long)blockIdx.x * kF1Block + threadIdx.x; r < R; r += (long long)gridDim.x * kF1Block)
        if (f1_valid((int)r, run_first, run_fp, n_def) && f1_better((int)r, best, run_first, run_fp, n_def)) best = (int)r;
    best = f1_block_best(best, run_first, run_fp, n_def);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// one block over the partials
__global__ __launch_bounds__(256) void f1_final_kernel(const int32_t* __restrict__ run_first, const int32_t* __restrict__ run_fp, int n_def,
                                                       const int32_t* __restrict__ partial, int nblk, long long* __restrict__ best_out)
{
    int best = -1;
    for (int b = threadIdx.x; b < nblk; b += 256) {
        const int c = partial[b];
        if (f1_better(c, best, run_first, run_fp, n_def)) best = c;
    }
    best = f1_block_best(best, run_first, run_fp, n_def);
    if (threadIdx.x == 0) best_out[0] = best, best_out[1] = 0;
}

// ---------------------------------------------------------------------------------------------------------------- overlap
// grid (ceil(HW / 256), n)
__global__ __launch_bounds__(256) void region_overlap_kernel(const int32_t* __restrict__ gt_labels, const int32_t* __restrict__ gt_offset,
                                                             int gt_cap, const int32_t* __restrict__ pred_labels,
                                                             const int32_t* __restrict__ pred_offset, const int32_t* __restrict__ pred_size,
                                                             int pred_cap, int min_area, int HW, int32_t* __restrict__ covered,
                                                             int32_t* __restrict__ hits)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const size_t at = (size_t)blockIdx.y * HW + p;
    int gl = 0, pl = 0;
    if (p < HW) gl = gt_labels[at], pl = pred_labels[at];
    const long long g = (long long)gt_offset[blockIdx.y] + gl - 1, q = (long long)pred_offset[blockIdx.y] + pl - 1;
    const bool in_gt = gl > 0 && g >= 0 && g < gt_cap;
    const bool in_pred = pl > 0 && q >= 0 && q < pred_cap;
    const bool both = in_gt && in_pred && pred_size[in_pred ? q : 0] >= min_area;
    wave_agg_inc(covered, (int)g, both);
    wave_agg_inc(hits, (int)q, both);
}

// grid (n), one workgroup per image.  counts[img] = n_gt, n_detected, n_pred (kept), n_false (kept, no hit)
__global__ __launch_bounds__(256) void detection_counts_kernel(const int32_t* __restrict__ gt_offset, const int32_t* __restrict__ covered,
                                                               int gt_cap, const int32_t* __restrict__ pred_offset,
                                                               const int32_t* __restrict__ pred_size, const int32_t* __restrict__ hits,
                                                               int pred_cap, int min_area, int32_t* __restrict__ counts)
{
    __shared__ int sh[4][3];
    const int img = blockIdx.x, tid = threadIdx.x;
    // tables somebody else wrote: nothing is read outside the capacities
    long long g0 = gt_offset[img], g1 = gt_offset[img + 1], p0 = pred_offset[img], p1 = pred_offset[img + 1];
    g0 = g0 < 0 ? 0 : (g0 > gt_cap ? gt_cap : g0), g1 = g1 < g0 ? g0 : (g1 > gt_cap ? gt_cap : g1);
    p0 = p0 < 0 ? 0 : (p0 > pred_cap ? pred_cap : p0), p1 = p1 < p0 ? p0 : (p1 > pred_cap ? pred_cap : p1);
    int det = 0, kept = 0, wrong = 0;
    for (long long c = g0 + tid; c < g1; c += 256) det += covered[c] > 0;
    for (long long c = p0 + tid; c < p1; c += 256) {
        const bool k = pred_size[c] >= min_area;
        kept += k;
        wrong += k && hits[c] == 0;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        det += __shfl_xor(det, m, 64);
        kept += __shfl_xor(kept, m, 64);
        wrong += __shfl_xor(wrong, m, 64);
    }
    if (lane_id() == 0) sh[tid >> 6][0] = det, sh[tid >> 6][1] = kept, sh[tid >> 6][2] = wrong;
    __syncthreads();
    if (tid == 0) {
        int32_t* o = counts + (size_t)img * 4;
        o[0] = (int32_t)(g1 - g0);
        o[1] = sh[0][0] + sh[1][0] + sh[2][0] + sh[3][0];
        o[2] = sh[0][1] + sh[1][1] + sh[2][1] + sh[3][1];
        o[3] = sh[0][2] + sh[1][2] + sh[2][2] + sh[3][2];
    }
}

inline int pr_tiles(int n_def) { return (n_def + kPrTile - 1) / kPrTile; }
inline int f1_blocks(int run_cap)
{
    const int want = (run_cap + kF1Block - 1) / kF1Block;
    return want < kF1MaxBlocks ? want : kF1MaxBlocks;
}

inline bool cap_ok(int cap) { return cap >= 0 && cap <= kMaxTotal; }   // list lengths and capacities: every count fits an int

}  // namespace

extern "C" size_t cmdiad_pr_tile(void) { return kPrTile; }

extern "C" int cmdiad_pr_runs(const uint64_t* def_sorted_keys, int n_def, const uint64_t* ok_sorted_keys, int n_ok, uint64_t* run_key,
                              int32_t* run_first, int32_t* run_fp, int run_cap, int32_t* n_runs, int32_t* tile_heads, int tile_cap,
                              cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n_def >= 0 && n_def <= kMaxTotal && n_ok >= 0 && n_ok <= kMaxTotal && cap_ok(run_cap) && cap_ok(tile_cap), CMDIAD_ERR_ARG,
                   "cmdiad_pr_runs: bad sizes n_def=%d n_ok=%d run_cap=%d tile_cap=%d (0..%d)", n_def, n_ok, run_cap, tile_cap, kMaxTotal);
    CMDIAD_REQUIRE(n_def == 0 || (def_sorted_keys && n_runs && tile_heads && (ok_sorted_keys || n_ok == 0) &&
                                  ((run_key && run_first && run_fp) || run_cap == 0)),
                   CMDIAD_ERR_ARG, "cmdiad_pr_runs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (n_def == 0) {
        if (n_runs) CMDIAD_CHECK_HIP("cmdiad_pr_runs", hipMemsetAsync(n_runs, 0, sizeof(int32_t), s));
        return CMDIAD_OK;
    }
    const int tiles = pr_tiles(n_def);
    CMDIAD_REQUIRE(tile_cap >= 2 * tiles, CMDIAD_ERR_ARG, "cmdiad_pr_runs: tile_heads holds %d entries, %d are needed (2 ceil(n_def / %d))",
                   tile_cap, 2 * tiles, kPrTile);
    int32_t *tile_count = tile_heads, *tile_off = tile_heads + tiles;   // heads per tile | their exclusive scan
    const unsigned long long* keys = (const unsigned long long*)def_sorted_keys;
    hipLaunchKernelGGL(pr_count_kernel, dim3((unsigned)tiles), dim3(256), 0, s, keys, n_def, tile_count);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pr_scan_kernel, dim3(1), dim3(256), 0, s, (const int32_t*)tile_count, tile_off, tiles, n_runs);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(pr_compact_kernel, dim3((unsigned)tiles), dim3(256), 0, s, keys, n_def, (const unsigned long long*)ok_sorted_keys,
                       n_ok, (const int32_t*)tile_off, (unsigned long long*)run_key, run_first, run_fp, run_cap);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_pr_f1max(const int32_t* run_first, const int32_t* run_fp, const int32_t* n_runs, int run_cap, int n_def,
                               int64_t* best, int32_t* partial, int partial_cap, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(cap_ok(run_cap) && n_def >= 0 && n_def <= kMaxTotal && cap_ok(partial_cap), CMDIAD_ERR_ARG,
                   "cmdiad_pr_f1max: bad sizes run_cap=%d n_def=%d partial_cap=%d (0..%d)", run_cap, n_def, partial_cap, kMaxTotal);
    if (run_cap == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(run_first && run_fp && n_runs && best && partial, CMDIAD_ERR_ARG, "cmdiad_pr_f1max: null pointer");
    const int nblk = f1_blocks(run_cap);
    CMDIAD_REQUIRE(partial_cap >= nblk, CMDIAD_ERR_ARG, "cmdiad_pr_f1max: partial holds %d entries, %d are needed (min(ceil(run_cap / %d), %d))",
                   partial_cap, nblk, kF1Block, kF1MaxBlocks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(f1_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, s, run_first, run_fp, n_runs, run_cap, n_def, partial);
    CMDIAD_CHECK_LAUNCH();
    hipLaunchKernelGGL(f1_final_kernel, dim3(1), dim3(256), 0, s, run_first, run_fp, n_def, (const int32_t*)partial, nblk, (long long*)best);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_region_overlap(const int32_t* gt_labels, const int32_t* gt_comp_offset, int gt_comp_cap, const int32_t* pred_labels,
                                     const int32_t* pred_comp_offset, const int32_t* pred_comp_size, int pred_comp_cap, int n, int H, int W,
                                     int min_area, int32_t* covered, int32_t* hits, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(sizes_ok(n, H, W) && cap_ok(gt_comp_cap) && cap_ok(pred_comp_cap) && min_area >= 1, CMDIAD_ERR_ARG,
                   "cmdiad_region_overlap: bad sizes n=%d (0..%d) H=%d W=%d (>= 1, H*W <= %d, n*H*W <= %d) gt_comp_cap=%d pred_comp_cap=%d "
                   "(0..%d) min_area=%d (>= 1)", n, kMaxImages, H, W, kMaxImagePixels, kMaxTotal, gt_comp_cap, pred_comp_cap, kMaxTotal,
                   min_area);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(gt_labels && gt_comp_offset && pred_labels && pred_comp_offset && (covered || gt_comp_cap == 0) &&
                       ((pred_comp_size && hits) || pred_comp_cap == 0), CMDIAD_ERR_ARG, "cmdiad_region_overlap: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (gt_comp_cap) CMDIAD_CHECK_HIP("cmdiad_region_overlap", hipMemsetAsync(covered, 0, (size_t)gt_comp_cap * 4, s));
    if (pred_comp_cap) CMDIAD_CHECK_HIP("cmdiad_region_overlap", hipMemsetAsync(hits, 0, (size_t)pred_comp_cap * 4, s));
    if (gt_comp_cap == 0 || pred_comp_cap == 0) return CMDIAD_OK;   // no component on one side: nothing overlaps
    const int HW = H * W;
    hipLaunchKernelGGL(region_overlap_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)n), dim3(256), 0, s, gt_labels, gt_comp_offset,
                       gt_comp_cap, pred_labels, pred_comp_offset, pred_comp_size, pred_comp_cap, min_area, HW, covered, hits);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}

extern "C" int cmdiad_detection_counts(const int32_t* gt_comp_offset, const int32_t* covered, int gt_comp_cap,
                                       const int32_t* pred_comp_offset, const int32_t* pred_comp_size, const int32_t* hits,
                                       int pred_comp_cap, int n, int min_area, int32_t* counts, cmdiad_stream_t stream)
{
    CMDIAD_REQUIRE(n >= 0 && n <= kMaxImages && cap_ok(gt_comp_cap) && cap_ok(pred_comp_cap) && min_area >= 1, CMDIAD_ERR_ARG,
                   "cmdiad_detection_counts: bad sizes n=%d (0..%d) gt_comp_cap=%d pred_comp_cap=%d (0..%d) min_area=%d (>= 1)", n,
                   kMaxImages, gt_comp_cap, pred_comp_cap, kMaxTotal, min_area);
    if (n == 0) return CMDIAD_OK;
    CMDIAD_REQUIRE(gt_comp_offset && pred_comp_offset && counts && (covered || gt_comp_cap == 0) &&
                       ((pred_comp_size && hits) || pred_comp_cap == 0), CMDIAD_ERR_ARG, "cmdiad_detection_counts: null pointer");
    hipLaunchKernelGGL(detection_counts_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, gt_comp_offset, covered, gt_comp_cap,
                       pred_comp_offset, pred_comp_size, hits, pred_comp_cap, min_area, counts);
    CMDIAD_CHECK_LAUNCH();
    return CMDIAD_OK;
}
