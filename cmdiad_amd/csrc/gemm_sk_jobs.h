// The job list of one stream-K block (gemm_sk.hip), as plain arithmetic: no HIP types, so the same struct compiles for the host
// and tests/sk_jobs_check.cpp walks it for every block of a launch.  The unit of work is a (tile, k-tile) pair; block b of nb
// owns units [units * b / nb, units * (b + 1) / nb) of the tile-major list.  Its jobs, IN EXECUTION ORDER:
//     [tile tB: k 0 .. kBe)   |   whole tiles tA + 1 .. tB - 1   |   [tile tA: k kA .. KT)
// -- the head piece it must HAND OVER first, the tail piece it must TAKE OVER last.  A wrong order here makes block b spin on
// block b - 1 for ever, which is why the order has a host-side check of its own.
#pragma once

#if defined(__HIPCC__)
#define CMDIAD_SK_HD __host__ __device__ __forceinline__
#else
#define CMDIAD_SK_HD inline
#endif

namespace gemm {

struct SkJob {
    int NT, KT;     // N tiles of the product, k-tiles of a tile
    int tA, kA;     // the range's first unit: tile, k-tile
    int tB, kBe;    // the range's last unit: tile, one past its k-tile
    int nj, j;      // jobs of the block, position in execution order
    int total;      // units of the block (<= 0: it has no work and every other member is meaningless)

    // the first job of block b of nb
    CMDIAD_SK_HD SkJob(int MT, int NT_, int KT_, int b, int nb) : NT(NT_), KT(KT_), j(0)
    {
        const long all = (long)MT * NT * KT;
        const int u0 = (int)(all * b / nb), u1 = (int)(all * (b + 1) / nb);
        tA = u0 / KT; kA = u0 - tA * KT;
        tB = (u1 - 1) / KT; kBe = (u1 - 1) - tB * KT + 1;
        nj = tB - tA + 1;
        total = u1 - u0;
    }
    CMDIAD_SK_HD int tile() const { return nj == 1 ? tA : (j == 0 ? tB : (j == nj - 1 ? tA : tA + j)); }
    CMDIAD_SK_HD int mt() const { return tile() / NT; }
    CMDIAD_SK_HD int nt() const { return tile() - mt() * NT; }
    CMDIAD_SK_HD int k0() const { return (nj == 1 || j == nj - 1) ? kA : 0; }
    CMDIAD_SK_HD int kc() const { return nj == 1 ? kBe - kA : (j == 0 ? kBe : (j == nj - 1 ? KT - kA : KT)); }
    CMDIAD_SK_HD bool takes_over() const { return k0() > 0; }           // continues a tile the previous block began
    CMDIAD_SK_HD bool hands_over() const { return k0() + kc() < KT; }   // stops before the tile's last k-tile
    CMDIAD_SK_HD void next() { ++j; }
};

}  // namespace gemm
