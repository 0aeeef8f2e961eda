// Host-side walk of the cell grid of the two neighbourhood searches (cmdiad_amd/csrc/cell_grid.h: the code knn_grid_*_kernel and
// interp3nn_bin / _grid_kernel run on): the ring walk, the cell coordinate, the choice of the grid axes and the workspace layouts.
// The exactness of both searches rests on "after the round of radius m every cell within m cells of the query has been scanned,
// once": checked here on the code itself, for both grid sides and every query cell.
// Built and run by tests/test_host_cpu.py with the host compiler; exit code 0 = every check passed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../cmdiad_amd/csrc/cell_grid.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++failures <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                \
    } while (0)

float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
uint32_t to_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// bits lo .. hi of a grid row, clipped to the grid (empty when the clipped range is)
uint64_t range_mask(int lo, int hi, int side)
{
    lo = lo < 0 ? 0 : lo;
    hi = hi > side - 1 ? side - 1 : hi;
    if (lo > hi) return 0;
    const uint64_t upto_hi = hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull);
    return upto_hi & ~((1ull << lo) - 1ull);
}

// Every round a radius policy can ask for is a pair (m_done, m): m_done = -1 (nothing scanned; the first radius is 1 or 2, or
// SIDE on a degenerate grid) or the radius of the round before, m any larger radius up to SIDE (m + 1, 2 m, the radius the
// current best asks for: all of them, so every pair).  For every query cell and every pair the round must report exactly the
// cells of the clipped Chebyshev square of radius m that are not in the one of radius m_done, each once.  By induction over the
// rounds of a sequence every cell of the square of radius m is then reported exactly once, all cells of the grid at m = SIDE,
// and none outside.
template <int SIDE>
void check_rings()
{
    static uint64_t span[SIDE + 1][SIDE + 1];   // span[lo][n]: n cells from lo on
    for (int lo = 0; lo <= SIDE; ++lo)
        for (int n = 0; lo + n <= SIDE; ++n) span[lo][n] = range_mask(lo, lo + n - 1, SIDE);
    uint64_t got[SIDE] = {};
    for (int ib = 0; ib < SIDE; ++ib)
        for (int ia = 0; ia < SIDE; ++ia)
            for (int m_done = -1; m_done < SIDE; ++m_done) {
                const int dlo = ia - m_done > 0 ? ia - m_done : 0, dhi = ia + m_done < SIDE - 1 ? ia + m_done : SIDE - 1;
                const uint64_t done = m_done >= 0 ? span[dlo][dhi - dlo + 1] : 0;
                for (int m = m_done + 1 > 1 ? m_done + 1 : 1; m <= SIDE; ++m) {
                    const int j0 = ib - m > 0 ? ib - m : 0, j1 = ib + m < SIDE - 1 ? ib + m : SIDE - 1;
                    const int lo_m = ia - m > 0 ? ia - m : 0, hi_m = ia + m < SIDE - 1 ? ia + m : SIDE - 1;
                    bool ok = true;
                    cellgrid::ring_rows<SIDE>(ia, ib, m, m_done, [&](int j, int lo, int hi) {
                        if (!(j >= j0 && j <= j1 && lo >= 0 && lo <= hi && hi < SIDE)) { ok = false; return; }
                        const uint64_t run = span[lo][hi - lo + 1];
                        if (got[j] & run) ok = false;      // a cell reported twice
                        got[j] |= run;
                    });
                    CHECK(ok, "side %d query (%d, %d) round %d -> %d: a run outside the square, empty, or overlapping another", SIDE, ia, ib, m_done, m);
                    for (int j = j0; j <= j1; ++j) {       // (no other row was touched: checked in the callback)
                        const int dj = j > ib ? j - ib : ib - j;
                        const uint64_t want = span[lo_m][hi_m - lo_m + 1] & ~(dj <= m_done ? done : 0);
                        if (got[j] != want) {
                            CHECK(got[j] == want, "side %d query (%d, %d) round %d -> %d row %d: cells %016llx, expected %016llx", SIDE, ia, ib, m_done, m,
                                  j, (unsigned long long)got[j], (unsigned long long)want);
                            return;
                        }
                        got[j] = 0;
                    }
                }
            }
    // the same, literally, for whole sequences on a per-cell counter: start 1 or 2, then always m + 1 / always 2 m / alternating /
    // one jump to the whole grid -- from the corners, the middle and an edge
    const int at[5][2] = {{0, 0}, {SIDE - 1, SIDE - 1}, {0, SIDE - 1}, {SIDE / 2, SIDE / 2 - 1}, {SIDE / 3, 0}};
    for (const auto& q : at)
        for (int start = 1; start <= 2; ++start)
            for (int rule = 0; rule < 4; ++rule) {
                std::vector<int> seen(SIDE * SIDE, 0);
                int m_done = -1, m = start;
                for (int round = 0;; ++round) {
                    m = m < SIDE ? m : SIDE;
                    cellgrid::ring_rows<SIDE>(q[0], q[1], m, m_done, [&](int j, int lo, int hi) {
                        for (int i = lo; i <= hi; ++i) ++seen[j * SIDE + i];
                    });
                    for (int j = 0; j < SIDE; ++j)
                        for (int i = 0; i < SIDE; ++i) {
                            const int di = i > q[0] ? i - q[0] : q[0] - i, dj = j > q[1] ? j - q[1] : q[1] - j;
                            const int want = (di > dj ? di : dj) <= m ? 1 : 0;
                            if (seen[j * SIDE + i] != want) {
                                CHECK(seen[j * SIDE + i] == want, "side %d query (%d, %d) start %d rule %d after radius %d: cell (%d, %d) scanned %d times",
                                      SIDE, q[0], q[1], start, rule, m, i, j, seen[j * SIDE + i]);
                                return;
                            }
                        }
                    m_done = m;
                    if (m >= SIDE) break;
                    m = rule == 0 ? m + 1 : rule == 1 ? 2 * m : rule == 2 ? (round & 1 ? 2 * m : m + 1) : SIDE + 5;
                }
            }
}

struct Geometry {
    const char* name;
    uint32_t mn[3], mx[3];   // the bounding box, float bits
    int A, B;
    uint32_t h64, h16;       // h of the 64- and of the 16-cell grid, float bits
};
// _grid of tests/test_neighbourhood_model_cpu.py (numpy float32) on _geometries(RandomState(11)) of that file
const Geometry kGeometries[7] = {
    {"sheet", {0x39105D1Eu, 0x3A1FA123u, 0xBD4CA8F9u}, {0x3F7FC7FEu, 0x3F7FFE75u, 0x3D4C5836u}, 0, 1, 0x3C7FD68Du, 0x3D7FD68Du},
    {"wall", {0x39105D1Eu, 0xBD4CA8F9u, 0x3A1FA123u}, {0x3F7FC7FEu, 0x3D4C5836u, 0x3F7FFE75u}, 0, 2, 0x3C7FD68Du, 0x3D7FD68Du},
    {"blob", {0x3A04D9BBu, 0x393A9803u, 0x39F5A824u}, {0x3F7FFFB7u, 0x3F7FEB4Bu, 0x3F7FDF0Au}, 0, 1, 0x3C7FDFA1u, 0x3D7FDFA1u},
    {"two_clusters", {0xBD0AF039u, 0xBD083974u, 0xBD027612u}, {0x40A10BF4u, 0x40A10861u, 0x40A11E13u}, 0, 2, 0x3DA222FFu, 0x3EA222FFu},
    {"line", {0x00000000u, 0x00000000u, 0x00000000u}, {0x3F800000u, 0x00000000u, 0x00000000u}, 0, 1, 0x3C800000u, 0x3D800000u},
    {"identical", {0x3E99999Au, 0xBE4CCCCDu, 0x3F666666u}, {0x3E99999Au, 0xBE4CCCCDu, 0x3F666666u}, 0, 1, 0x00000000u, 0x00000000u},
    {"duplicates", {0x3B1A973Cu, 0x3AF10E50u, 0xBD4CA8F9u}, {0x3F7F3396u, 0x3F7F95A1u, 0x3D4C2B75u}, 0, 1, 0x3C7F1D1Au, 0x3D7F1D1Au},
};

template <int SIDE>
void check_axes_and_coord()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the two widest axes, ties to the lower axis: equal extents in every pairing
    const float tie[7][5] = {{1, 1, 1, 0, 1}, {1, 1, .5f, 0, 1}, {1, .5f, 1, 0, 2}, {.5f, 1, 1, 1, 2}, {1, .5f, .5f, 0, 1}, {.5f, 1, .5f, 0, 1}, {.5f, .5f, 1, 0, 2}};
    for (const auto& t : tie) {
        const float mn[3] = {-3.0f, 0.25f, 7.0f}, mx[3] = {mn[0] + t[0], mn[1] + t[1], mn[2] + t[2]};
        const auto g = cellgrid::choose_axes<SIDE>(mn, mx);
        CHECK(g.A == (int)t[3] && g.B == (int)t[4], "side %d extents (%g, %g, %g): axes (%d, %d)", SIDE, t[0], t[1], t[2], g.A, g.B);
        CHECK(g.h == 1.0f / SIDE && g.inv_h == (float)SIDE && g.mnA == mn[g.A] && g.mnB == mn[g.B], "side %d extents (%g, %g, %g): h %g", SIDE, t[0], t[1], t[2], g.h);
    }
    // degenerate boxes: zero, infinite and NaN extents, and the box of no points at all
    const float boxes[5][6] = {{1, 2, 3, 1, 2, 3}, {0, 0, 0, inf, 1, 1}, {-inf, 0, 0, 0, 1, 1}, {nan, nan, nan, nan, nan, nan}, {inf, inf, inf, -inf, -inf, -inf}};
    for (const auto& bx : boxes) {
        const auto g = cellgrid::choose_axes<SIDE>(bx, bx + 3);
        CHECK(g.h == 0.0f && g.inv_h == 0.0f && g.A >= 0 && g.A < g.B && g.B <= 2, "side %d box (%g %g %g)-(%g %g %g): h %g axes (%d, %d)", SIDE, bx[0], bx[1],
              bx[2], bx[3], bx[4], bx[5], g.h, g.A, g.B);
        CHECK(g.cell(0.5f, -7.0f, nan) == 0 && g.cell(bx[3], bx[4], bx[5]) == 0, "side %d degenerate grid: a point outside cell 0", SIDE);
    }
    for (const Geometry& geo : kGeometries) {
        float mn[3], mx[3];
        for (int a = 0; a < 3; ++a) { mn[a] = from_bits(geo.mn[a]); mx[a] = from_bits(geo.mx[a]); }
        const auto g = cellgrid::choose_axes<SIDE>(mn, mx);
        const uint32_t h = SIDE == 64 ? geo.h64 : geo.h16;
        CHECK(g.A == geo.A && g.B == geo.B && to_bits(g.h) == h, "side %d %s: axes (%d, %d) h %08x, the model has (%d, %d) %08x", SIDE, geo.name, g.A, g.B,
              to_bits(g.h), geo.A, geo.B, h);
        if (g.h == 0.0f) continue;
        // a point at the box maximum lands in the last cell of the wider axis; the minimum in cell 0; both ends clamp
        const bool a_wider = mx[g.A] - mn[g.A] >= mx[g.B] - mn[g.B];
        const float top = a_wider ? mx[g.A] : mx[g.B], low = a_wider ? g.mnA : g.mnB;
        CHECK(g.coord(top, low) == SIDE - 1 && g.coord(low, low) == 0, "side %d %s: box ends in cells %d and %d", SIDE, geo.name, g.coord(low, low), g.coord(top, low));
        CHECK(g.coord(low - 10.0f, low) == 0 && g.coord(-inf, low) == 0 && g.coord(top + 10.0f, low) == SIDE - 1 && g.coord(inf, low) == SIDE - 1 &&
                  g.coord(nan, low) == 0,
              "side %d %s: clamps below / above / NaN", SIDE, geo.name);
        CHECK(g.cell(mx[0], mx[1], mx[2]) == g.ib(mx[0], mx[1], mx[2]) * SIDE + g.ia(mx[0], mx[1], mx[2]), "side %d %s: cell is row-major in ib", SIDE, geo.name);
        // monotone in a: a fine sweep across the box and beyond, and every float around each cell border
        int prev = 0;
        for (int s = -100; s <= 4200; ++s) {
            const int c = g.coord(low + (top - low) * ((float)s / 4096.0f), low);
            CHECK(c >= prev && c >= 0 && c < SIDE, "side %d %s: coordinate %d after %d at step %d", SIDE, geo.name, c, prev, s);
            prev = c;
        }
        for (int cell = 1; cell < SIDE; ++cell) {
            float a = low + (float)cell * g.h;
            for (int s = 0; s < 8; ++s) a = std::nextafter(a, -inf);
            int before = g.coord(a, low);
            for (int s = 0; s < 16; ++s) {
                a = std::nextafter(a, inf);
                const int c = g.coord(a, low);
                CHECK(c >= before && c >= cell - 1 && c <= cell, "side %d %s: coordinate %d after %d next to the border of cell %d", SIDE, geo.name, c, before, cell);
                before = c;
            }
        }
    }
}

// offsets 16-byte aligned where a float4 (or the 32-byte header) lives, regions in order and disjoint, the slice holds them all
template <class Layout, int SIDE>
void check_layout(bool aux, int n_max)
{
    for (int n = 1; n <= n_max; n = n < 70 ? n + 1 : n * 2 + 1) {
        const Layout L(n);
        const size_t hdr_end = sizeof(cellgrid::CellGrid<SIDE>), elem_end = L.elem + (size_t)n * 16, aux_end = L.aux + (aux ? (size_t)n * 4 : 0);
        const size_t cs_end = L.cell_start + (size_t)(SIDE * SIDE + 1) * 4;
        CHECK(hdr_end == 32 && L.elem >= hdr_end && L.aux >= elem_end && L.cell_start >= aux_end && L.stride >= cs_end, "n %d: regions overlap", n);
        CHECK(L.elem % 16 == 0 && L.stride % 16 == 0 && L.aux % 4 == 0 && L.cell_start % 4 == 0, "n %d: alignment", n);
        CHECK(L.lds_bytes() == cs_end - L.elem && L.lds_bytes() % 4 == 0, "n %d: the LDS copy is not the slice behind the header", n);
        CHECK(L.bytes(1) == L.stride && L.bytes(7) == 7 * L.stride && L.bytes(7) >= 6 * L.stride + cs_end, "n %d: workspace bytes", n);
    }
}

}  // namespace

int main()
{
    check_rings<16>();
    check_rings<64>();
    check_axes_and_coord<16>();
    check_axes_and_coord<64>();
    check_layout<cellgrid::KnnGridLayout, 64>(false, 1 << 20);
    check_layout<cellgrid::Interp3nnLayout, 16>(true, 4096);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("cell grid ok\n");
    return 0;
}
