// The 2-D cell grid of the two neighbourhood searches (kNN grouping: knn_group.hip, 64 x 64 cells over the points of a cloud;
// 3-NN interpolation: interp_pool.hip, 16 x 16 cells over its centres): the grid, its builder, the ring walk of a query and the
// workspace layout.  Everything but the builder is plain arithmetic that also compiles for the host, where
// tests/cell_grid_check.cpp walks it.
//
// The grid.  A depth-camera cloud is a 2.5-D sheet, so the elements are binned on the TWO axes of largest extent of their bounding
// box (A < B; ties: the lower axis) into SIDE x SIDE square cells of edge h = the larger extent / SIDE, and counting-sorted by cell
// (cells row-major, row = the coordinate on B: a run of cells of one grid row is one contiguous run of sorted elements,
// [cell_start[first], cell_start[last + 1])).  A cell coordinate is clamp((a - min) * inv_h, 0, SIDE - 1), so a query point
// outside the bounding box (or a NaN: 0) belongs to a border cell, and the coordinate is monotone in a.  A box of zero, infinite
// or NaN extent gives h = 0: every element in cell 0, and a query scans the whole grid.
//
// The ring rule.  A query at cell (ia, ib) scans the square of cells within m cells of it (Chebyshev), innermost rings first,
// the radius growing from round to round (ring_rows visits what the earlier rounds have not).  Every element NOT in a scanned
// cell differs from the query by more than m cells along a grid axis, i.e. it is farther than m * h: once the query's worst kept
// squared distance is below ((m - 0.01) h)^2 nothing outside the square can beat it.  The 0.01 cells of slack cover the roundings
// of the cell coordinate (SIDE * 2^-23 <= 8e-6 cells).  Radius SIDE is the whole grid.  The starting radius, the certificate and
// the next radius differ between the two searches and stay next to their distance formulas.
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#include "block_scan.h"
#define CMDIAD_GRID_HD __host__ __device__ __forceinline__
#else
#define CMDIAD_GRID_HD inline
#endif

namespace cellgrid {

CMDIAD_GRID_HD float pick3(float x, float y, float z, int axis) { return axis == 0 ? x : (axis == 1 ? y : z); }

// What a query needs of a built grid: 32 bytes in front of a cloud's slice of the workspace.
template <int SIDE>
struct CellGrid {
    float mnA, mnB, inv_h, h;   // bounding-box minimum on the two grid axes, 1 / h (0 when h = 0), cell edge
    int A, B;                   // the grid axes (0, 1, 2 = x, y, z), A < B
    float user, unused;         // the builder's extra reduced value

    CMDIAD_GRID_HD int coord(float a, float mn) const { return (int)fminf(fmaxf((a - mn) * inv_h, 0.0f), (float)(SIDE - 1)); }   // (NaN -> 0)
    CMDIAD_GRID_HD int ia(float x, float y, float z) const { return coord(pick3(x, y, z, A), mnA); }
    CMDIAD_GRID_HD int ib(float x, float y, float z) const { return coord(pick3(x, y, z, B), mnB); }
    CMDIAD_GRID_HD int cell(float x, float y, float z) const { return ib(x, y, z) * SIDE + ia(x, y, z); }
};

// The grid of the bounding box [mn, mx] (user left 0).
template <int SIDE>
CMDIAD_GRID_HD CellGrid<SIDE> choose_axes(const float mn[3], const float mx[3])
{
    const float e0 = mx[0] - mn[0], e1 = mx[1] - mn[1], e2 = mx[2] - mn[2];
    int A, B;
    if (e0 >= e1 && e0 >= e2) { A = 0; B = e1 >= e2 ? 1 : 2; }
    else if (e1 >= e2) { A = 1; B = e0 >= e2 ? 0 : 2; }
    else { A = 2; B = e0 >= e1 ? 0 : 1; }
    if (A > B) { const int t = A; A = B; B = t; }
    const float ext = fmaxf(pick3(e0, e1, e2, A), pick3(e0, e1, e2, B));
    const float h = ext > 0.0f && ext < INFINITY ? ext * (1.0f / SIDE) : 0.0f;
    return CellGrid<SIDE>{pick3(mn[0], mn[1], mn[2], A), pick3(mn[0], mn[1], mn[2], B), h > 0.0f ? 1.0f / h : 0.0f, h, A, B, 0.0f, 0.0f};
}

// One round of a query at cell (ia, ib): f(j, lo, hi) for every run of cells [lo, hi] of grid row j that lies within m cells of
// the query, inside the grid, and outside the square of radius m_done that the earlier rounds have scanned (m_done < m <= SIDE;
// -1: nothing yet).
template <int SIDE, class F>
CMDIAD_GRID_HD void ring_rows(int ia, int ib, int m, int m_done, F&& f)
{
    const int lo = ia - m > 0 ? ia - m : 0, hi = ia + m < SIDE - 1 ? ia + m : SIDE - 1;
    for (int dj = -m; dj <= m; ++dj) {
        const int j = ib + dj;
        if (j < 0 || j >= SIDE) continue;
        if (dj < -m_done || dj > m_done) {
            f(j, lo, hi);                                     // a row outside the scanned square: all of it
        } else {                                              // a row that crosses the scanned square: the two ends
            if (ia - m_done - 1 >= lo) f(j, lo, ia - m_done - 1);
            if (ia + m_done + 1 <= hi) f(j, ia + m_done + 1, hi);
        }
    }
}

// A cloud's slice of the workspace: CellGrid hdr | float4 elem[n] | int aux[n] (AUX only) | int cell_start[SIDE * SIDE + 1],
// padded to 16 bytes.  Everything behind the header is what a query kernel may copy to LDS in one piece.
template <int SIDE, bool AUX>
struct GridLayout {
    size_t elem, aux, cell_start, stride;   // byte offsets in the slice (the header at 0), bytes per cloud
    CMDIAD_GRID_HD explicit GridLayout(int n)
        : elem(sizeof(CellGrid<SIDE>)), aux(elem + (size_t)n * 16), cell_start(aux + (AUX ? (size_t)n * 4 : 0)),
          stride((cell_start + (size_t)(SIDE * SIDE + 1) * 4 + 15) / 16 * 16) {}
    CMDIAD_GRID_HD size_t bytes(int clouds) const { return (size_t)clouds * stride; }
    CMDIAD_GRID_HD size_t lds_bytes() const { return cell_start + (size_t)(SIDE * SIDE + 1) * 4 - elem; }
};
using KnnGridLayout = GridLayout<64, false>;      // elem = {x, y, z, original index}
using Interp3nnLayout = GridLayout<16, true>;     // elem = {x, y, z, |c|^2}, aux = original index

#if defined(__HIPCC__)
// The builder: one workgroup of THREADS bins the n elements of a cloud.  load(k, x, y, z) reads element k; extra(x, y, z) >= 0 is
// max-reduced over the elements into hdr->user; store(k, pos, x, y, z) writes element k at its sorted position.  Bounding box per
// thread, xor-butterfly, per-wave rows in LDS; cell counts by LDS atomics; their exclusive scan (SIDE * SIDE / THREADS cells per
// thread); the counts become write cursors; header; scatter.  (The order INSIDE a cell is that of the atomics: the searches do
// not depend on it, their keys carry the original index.)
template <int SIDE, int THREADS, class Load, class Extra, class Store>
__device__ __forceinline__ void build(int n, Load load, Extra extra, Store store, CellGrid<SIDE>* hdr, int* cell_start)
{
    constexpr int kCells = SIDE * SIDE, kWaves = THREADS / 64, kPer = kCells / THREADS;
    static_assert(kPer * THREADS == kCells && kWaves * 64 == THREADS, "whole cells per thread, whole waves");
    __shared__ int s_cnt[kCells];
    __shared__ float s_red[kWaves][7];
    __shared__ int s_wave[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY}, user = 0.0f;
    for (int k = tid; k < n; k += THREADS) {
        float p[3];
        load(k, p[0], p[1], p[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], p[a]); mx[a] = fmaxf(mx[a], p[a]); }
        user = fmaxf(user, extra(p[0], p[1], p[2]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = fminf(mn[a], __shfl_xor(mn[a], m, 64));
            mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], m, 64));
        }
        user = fmaxf(user, __shfl_xor(user, m, 64));
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_red[wave][a] = mn[a]; s_red[wave][3 + a] = mx[a]; }
        s_red[wave][6] = user;
    }
    for (int c = tid; c < kCells; c += THREADS) s_cnt[c] = 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = fminf(mn[a], s_red[w][a]); mx[a] = fmaxf(mx[a], s_red[w][3 + a]); }
        user = fmaxf(user, s_red[w][6]);
    }
    CellGrid<SIDE> g = choose_axes<SIDE>(mn, mx);
    g.user = user;
    for (int k = tid; k < n; k += THREADS) {
        float x, y, z;
        load(k, x, y, z);
        atomicAdd(&s_cnt[g.cell(x, y, z)], 1);
    }
    __syncthreads();
    int cnt[kPer], sum = 0, total;
#pragma unroll
    for (int i = 0; i < kPer; ++i) { cnt[i] = s_cnt[tid * kPer + i]; sum += cnt[i]; }
    int run = block_excl_scan<kWaves>(sum, s_wave, total);
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
        cell_start[tid * kPer + i] = run;
        s_cnt[tid * kPer + i] = run;     // now the cell's write cursor (a thread's own cells: no barrier since it read them)
        run += cnt[i];
    }
    if (tid == 0) { cell_start[kCells] = total; *hdr = g; }
    __syncthreads();
    for (int k = tid; k < n; k += THREADS) {
        float x, y, z;
        load(k, x, y, z);
        store(k, atomicAdd(&s_cnt[g.cell(x, y, z)], 1), x, y, z);
    }
}
#endif  // __HIPCC__

}  // namespace cellgrid
