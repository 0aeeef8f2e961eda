// Host-side walk of the stream-K job list (cmdiad_amd/csrc/gemm_sk_jobs.h, the struct gemm_sk_kernel runs on): for every block
// of a launch, the jobs it executes in the order it executes them.  A wrong order or a wrong split cannot be tested small on the
// device (eligibility needs more than 256 tiles) and shows there as block b spinning on block b - 1: it is checked here.
// Built and run by tests/test_host_cpu.py with the host compiler; exit code 0 = every launch passed.
#include <cstdio>
#include <vector>

#include "../cmdiad_amd/csrc/gemm_sk_jobs.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++failures <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                \
    } while (0)

// nb blocks on an M x N x K product; one_tile_each: the residual-tiles form (grid = tiles, nothing parked or taken over)
void check_launch(int M, int N, int K, int nb, bool one_tile_each)
{
    const int MT = (M + 255) / 256, NT = N / 256, KT = K / 64, tiles = MT * NT;
    std::vector<int> covered((size_t)tiles * KT, 0);       // times each (tile, k-tile) unit is executed
    std::vector<int> sharers(tiles, 0);                    // blocks that execute a part of each tile
    std::vector<int> taker(tiles, -1), hander(tiles, -1);  // block that takes the tile over / hands it over
    long total = 0;
    for (int b = 0; b < nb; ++b) {
        gemm::SkJob job(MT, NT, KT, b, nb);
        if (job.total <= 0) continue;
        total += job.total;
        CHECK(job.total >= KT, "M=%d N=%d K=%d block %d: range of %d units is shorter than a tile (%d)", M, N, K, b, job.total, KT);
        int walked = 0;
        // the range, restated: units [u0, u1) of the tile-major list touch tiles first .. last
        const long all = (long)tiles * KT;
        const int first = (int)(all * b / nb) / KT, last = (int)(all * (b + 1) / nb - 1) / KT;
        const int nj = job.nj;
        CHECK(nj == last - first + 1, "block %d has %d jobs for tiles %d .. %d", b, nj, first, last);
        for (int j = 0; j < nj; ++j, job.next()) {
            const int t = job.tile(), k0 = job.k0(), kc = job.kc();
            CHECK(job.j == j, "block %d: cursor %d at job %d", b, job.j, j);
            CHECK(t >= 0 && t < tiles && k0 >= 0 && kc >= 1 && k0 + kc <= KT, "block %d job %d: tile %d k0 %d kc %d", b, j, t, k0, kc);
            if (!(t >= 0 && t < tiles && k0 >= 0 && kc >= 1 && k0 + kc <= KT)) return;
            CHECK(job.mt() == t / NT && job.nt() == t % NT, "block %d job %d: tile %d -> (%d, %d)", b, j, t, job.mt(), job.nt());
            CHECK(job.takes_over() == (k0 > 0) && job.hands_over() == (k0 + kc < KT), "block %d job %d: take / hand flags", b, j);
            for (int k = k0; k < k0 + kc; ++k) ++covered[(size_t)t * KT + k];
            ++sharers[t];
            walked += kc;
            // order: a piece that is handed over can only be the FIRST job, a piece that is taken over only the LAST one
            // (the predecessor parks its head piece at the very start of its own run, so nobody waits on a waiting block)
            if (job.hands_over()) {
                CHECK(j == 0, "block %d hands over tile %d in job %d of %d, not first", b, t, j, nj);
                CHECK(hander[t] < 0, "tile %d is handed over twice", t);
                hander[t] = b;
            }
            if (job.takes_over()) {
                CHECK(j == nj - 1, "block %d takes over tile %d in job %d of %d, not last", b, t, j, nj);
                CHECK(taker[t] < 0, "tile %d is taken over twice", t);
                taker[t] = b;
            }
            // head = the range's LAST tile, then the tiles between in ascending order, tail = the range's FIRST tile
            const int expect = nj == 1 ? first : (j == 0 ? last : (j == nj - 1 ? first : first + j));
            CHECK(t == expect, "block %d job %d of %d runs tile %d, expected %d", b, j, nj, t, expect);
            if (j > 0 && j < nj - 1) CHECK(k0 == 0 && kc == KT, "block %d: middle job %d is not a whole tile (k0 %d kc %d)", b, j, k0, kc);
            CHECK(!(job.hands_over() && job.takes_over()), "block %d both takes over and hands over tile %d", b, t);
        }
        CHECK(walked == job.total, "block %d: jobs cover %d units, range has %d", b, walked, job.total);
        if (one_tile_each) CHECK(nj == 1 && job.total == KT, "block %d of a one-tile-per-block launch: %d jobs, %d units", b, nj, job.total);
    }
    CHECK(total == (long)tiles * KT, "M=%d N=%d K=%d: blocks own %ld units of %ld", M, N, K, total, (long)tiles * KT);
    for (size_t u = 0; u < covered.size(); ++u)
        CHECK(covered[u] == 1, "M=%d N=%d K=%d: unit (tile %zu, k %zu) executed %d times", M, N, K, u / KT, u % KT, covered[u]);
    for (int t = 0; t < tiles; ++t) {
        CHECK(sharers[t] >= 1 && sharers[t] <= 2, "tile %d is shared by %d blocks", t, sharers[t]);
        // a shared tile is parked by block b and continued by block b + 1 (slot b, counter b: gemm_sk.hip); a whole one by neither
        if (sharers[t] == 2) CHECK(hander[t] >= 0 && taker[t] == hander[t] + 1, "tile %d: handed over by %d, taken over by %d", t, hander[t], taker[t]);
        else CHECK(hander[t] < 0 && taker[t] < 0, "unshared tile %d: handed over by %d, taken over by %d", t, hander[t], taker[t]);
        if (one_tile_each) CHECK(sharers[t] == 1, "tile %d of a one-tile-per-block launch has %d blocks", t, sharers[t]);
    }
}

}  // namespace

int main()
{
    // the eligible shapes of the stream-K device tests on the stream-K grid of 256 blocks: test_gemm_streamk_matches_128_tile_bit_for_bit ...
    const int shapes[8][3] = {{32 * 785, 768, 3072}, {32 * 785, 768, 768}, {100 * 256, 768, 1536}, {24000, 1024, 1024},
                              // the edges of the eligibility rule (test_gemm_streamk_at_the_edges_of_its_eligibility): 257 and 511 tiles of
                              // three K-tiles (a range is barely one tile long), 258 tiles of four, 511 whole tiles
                              {65537, 256, 192}, {130561, 256, 192}, {32924, 512, 256}, {130816, 256, 192}};
    for (const auto& s : shapes) check_launch(s[0], s[1], s[2], 256, false);
    // the residual-tiles form: one block per tile (test_gemm_residual_on_wide_tiles_matches_128_tile_bit_for_bit's shapes it is legal for)
    const int tiled[3][3] = {{32 * 785, 768, 768}, {9 * 256 + 17, 512, 1536}, {300, 256, 192}};
    for (const auto& s : tiled) check_launch(s[0], s[1], s[2], ((s[0] + 255) / 256) * (s[1] / 256), true);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("sk jobs ok\n");
    return 0;
}
