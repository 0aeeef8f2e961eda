// Which kernel of the GEMM family runs, on which grid, with which panel / group_m / splits / qgroup: plain host arithmetic on the
// arguments of a call and the environment switches (host only, no HIP headers, no kernel symbols).  The launchers (gemm.hip,
// gemm_sk.hip, l2min.hip, blocks.cpp) plan first and then only launch: they hold no selection rule, threshold or grid arithmetic
// of their own.  The rules read the environment switches themselves (plan::switches), through getenv in the library (launch.h) and
// through a table in tests/gemm_plan_check.cpp, which walks the rules on the host.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/cmdiad_hip.h"

namespace plan {

constexpr int kPersistCUs = 256;   // one persistent block per CU (MI355X)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// The LayerNorm-fold operands of a residual-row epilogue (gemm_core.h, ResRows): all null, or ln_xb and ln_part together, both
// 8-byte aligned; add2 only with them, 16-byte aligned; row pitches (elements) in multiples of 4.
inline bool ln_out_operands_ok(const void* ln_xb, int ld_xb, const void* ln_part, const void* add2, int ld_add2)
{
    if (!ln_xb && !ln_part && !add2) return true;
    return ln_xb && ln_part && ld_xb % 4 == 0 && aligned8(ln_xb) && aligned8(ln_part) && (!add2 || (aligned16(add2) && ld_add2 % 4 == 0));
}

// The selection switches ("Environment switches").  A switch is read where a rule consults it, so a call pays a
// getenv (a walk over the environment; cmdiad_gemm_bf16 runs some 600 times per image at B = 1) only for the switches that can
// act on it, and tests may change a switch between calls; every rule below asks for a switch at most once per call.  get = getenv
// in the library (launch.h), a table in tests/gemm_plan_check.cpp; none = the empty environment.
struct switches {
    const char* (*get)(const char* name) = nullptr;
    int l2_splits = 0, l2_qgroup = 0;   // CMDIAD_L2_SPLITS, CMDIAD_L2_QGROUP: fixed for the process, filled in by the caller

    int group_m() const { return num("CMDIAD_GEMM_GROUPM", 8); }
    long panel_min() const { return lnum("CMDIAD_GEMM_PANEL_MIN", 2048); }
    int pp3() const { return tri("CMDIAD_GEMM_PP3"); }
    bool res_wide() const { return is("CMDIAD_GEMM_RES_WIDE", '1'); }
    int wide() const { return num("CMDIAD_GEMM_WIDE", -1); }                       // acts in the A/B build only
    long pp3_grid() const { return lnum("CMDIAD_PP3_GRID", 0); }                    // A/B build only
    int l2_tile() const { return num("CMDIAD_L2_TILE", -1); }
    int l2_seg_splits() const { return num("CMDIAD_L2_SEG_SPLITS", 0); }
    int pmae_mlp() const { return tri("CMDIAD_PMAE_MLP"); }
    bool stage1_persist() const { return !is("CMDIAD_STAGE1_PERSIST", '0'); }      // A/B build only
    bool stage1_once() const { return !is("CMDIAD_STAGE1_ONCE", '0'); }            // A/B build only

    const char* text(const char* name) const { return get ? get(name) : nullptr; }
    int num(const char* name, int dflt) const { const char* e = text(name); return e ? atoi(e) : dflt; }
    long lnum(const char* name, long dflt) const { const char* e = text(name); return e ? atol(e) : dflt; }
    bool is(const char* name, char c) const { const char* e = text(name); return e && e[0] == c; }       // set, and starts with c
    int tri(const char* name) const { const char* e = text(name); return !e ? -1 : e[0] != '0'; }        // -1 unset, 0 "0...", else 1
};

// CMDIAD_OK, or the code and the text a launcher hands to cmdiad_set_error
struct status {
    int err = CMDIAD_OK;
    char text[200] = "";
    __attribute__((format(printf, 3, 4))) void fail(int code, const char* fmt, ...)
    {
        err = code;
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
    }
};
#define CMDIAD_PLAN_REQUIRE(pl, cond, ...)              \
    do {                                                \
        if (!(cond)) {                                  \
            (pl).fail(CMDIAD_ERR_ARG, __VA_ARGS__);     \
            return (pl);                                \
        }                                               \
    } while (0)

inline long ceil_div(long a, long b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------------------------------------
// Tile grids of the 128 x 128 kernels (cmdiad_gemm_bf16, cmdiad_gemm_qkv, cmdiad_gemm_groupmax, the generic encoder stage)
// ------------------------------------------------------------------------------------------------
// M tiles per L2 group of the block order (gemm.hip Coord); CMDIAD_GEMM_GROUPM=1 restores the row-major order (A/B runs)
inline int group_m_tiles(const switches& sw) { const int g = sw.group_m(); return g < 1 ? 1 : g; }

// N tiles per block.  Short-K, tall-M products (the Point-MAE encoder: M = 4.2 M rows, K <= 512) are bound by the
// HBM latency of each block's few K-steps, not by bandwidth or MFMA rate; walking the whole N panel in one block
// pays that latency once and re-reads A from L2.  CMDIAD_GEMM_PANEL_MIN = smallest M-tile count that switches
// it on (default 2048; 1 in the parity tests so small shapes cover the path; a huge value disables it).
inline int panel_tiles(long M, long N, long K, int split, const switches& sw)
{
    const long mt = ceil_div(M, 128), ntl = ceil_div(N, 128);
    if (split > 1 || ntl == 1 || K > 512 || mt < sw.panel_min()) return 1;
    return (int)(ntl < 8 ? ntl : 8);
}

// (Round 5 tried 160-row tiles -- Shape<160,128,4,2>, 5 x 4 MFMA tiles per wave, still two blocks per CU -- for the in-place residual
// products, whose 128-row tile count is a bad fit for 512 block slots at the ViT's batch-32 shape: 1 182 tiles = 2.31 rounds against
// 942 = 1.84.  Bit-identical, and measured on one box, interleaved: proj 54.9 -> 56.5 us, fc2 139.1 -> 143.9 us, the whole step
// 22.46 -> 22.72 ms: a partly filled last round is NOT a whole round -- its blocks have their CU to themselves and run ~1.5x faster,
// and in the pipeline the other streams' kernels take the idle CUs.  Removed; profiles/r5_notes.md section 2.)
inline unsigned grid128(long M, long N, int panel = 1) { return (unsigned)(ceil_div(M, 128) * ceil_div(ceil_div(N, 128), panel)); }

// 256 x 256 tiles of a product with whole 256-column tiles (the two-group kernels)
inline long tiles256(long M, long N) { return ceil_div(M, 256) * (N / 256); }

// grid of the two-group persistent kernel
inline unsigned persist_blocks(long M, long N, const switches& sw, bool ab_build)
{
    const long jobs = tiles256(M, N);
    const long forced = ab_build ? sw.pp3_grid() : 0;
    if (forced > 0) return (unsigned)(jobs < forced ? jobs : forced);
    // as many blocks as give every block the same number of tiles (+-1) at the same number of rounds: 1 188 tiles are five
    // rounds on 256 CUs and on 238; the smaller grid is 1-2 % faster (fewer CUs share the fabric in the last round;
    // tools/pp3_grid.py).  The vendor library picks its stream-K grids for these shapes the same way (198 blocks x 6 tiles).
    const long rounds = ceil_div(jobs, kPersistCUs);
    return (unsigned)(jobs < kPersistCUs ? jobs : ceil_div(jobs, rounds));
}

// Wide-shape choice for a product (A/B build): 0 = keep 128 x 128, 8 = 256 x 256, 4 = 256 x 128.  Measured on MI355X
// (profiles/r1_notes.md): the 4-wave shapes pay for issuing all LDS-DMA pieces from the MFMA-issuing wave; the only shape
// they win as a bare product (4.2M x 512 x 256: 2.34 vs 2.57 ms) they lose again inside the encoder, where that GEMM
// carries the group-bias + ReLU epilogue (encoder 8.6-8.9 vs 7.9 ms).  So no network GEMM selects them; the distance GEMM
// does (l2min.hip).  CMDIAD_GEMM_WIDE=4 / =8 force a shape (A/B runs and the parity tests).
inline int wide_choice(bool plain_epilogue, int split, const switches& sw, bool ab_build)
{
    if (!ab_build || !plain_epilogue || split > 1) return 0;
    const int wide = sw.wide();
    return wide == 4 || wide == 8 ? wide : 0;
}

struct tile_grid { unsigned x; int panel; };

// the 4-wave shapes (nj = 4: 256 x 128, nj = 8: 256 x 256); short K: the whole N panel in one block
inline tile_grid wide_grid(long M, long N, long K, int nj)
{
    const long ntl = ceil_div(N, 32 * nj);
    const int panel = (K <= 512 && ntl <= 8) ? (int)ntl : 1;
    return {(unsigned)(ceil_div(M, 256) * ceil_div(ntl, panel)), panel};
}

// cmdiad_gemm_groupmax: nj != 0 = a wide shape of the A/B build, else the 128 x 128 tile with its N panel
inline tile_grid groupmax_grid(long M, long N, long K, int nj, const switches& sw)
{
    if (nj) return wide_grid(M, N, K, nj);
    const int panel = panel_tiles(M, N, K, 1, sw);
    return {grid128(M, N, panel), panel};
}

// ------------------------------------------------------------------------------------------------
// cmdiad_gemm_bf16
// ------------------------------------------------------------------------------------------------
enum class gemm_kernel {
    general,        // gemm_std_kernel<S128, ACT, false>
    general_train,  // ... with the training terms (out_pre_bf16, dact_of)
    res_rows,       // the residual-row epilogue: out_f32 = acc + bias + residual, 8 rows x 128 bytes per store
    res_rows_ln,    // ... that also writes the LayerNorm-fold outputs (ln_xb, ln_part, add2)
    pp3,            // two-group persistent 256 x 256: out_bf16 = act(acc + bias)
    pp3_rscale,     // ... act(row_scale[m] * acc + bias)
    res_tiles,      // the residual form on 256 x 256 tiles, one per block (gemm_sk.hip)
    wide4, wide8,   // A/B build: the 4-wave 256 x 128 / 256 x 256 shapes
};

struct gemm_plan : status {
    gemm_kernel kernel = gemm_kernel::general;
    int act = CMDIAD_ACT_NONE;
    unsigned grid_x = 0, grid_y = 1;
    int panel = 1, group_m = 1;
    int first_empty_slab = -1;   // split-K: slabs from this one on hold no K-tile and are zeroed ahead of the launch; -1 = none
};

inline int split_of(const cmdiad_gemm_args& a) { return a.split_k > 1 ? a.split_k : 1; }
inline bool has_train_terms(const cmdiad_gemm_args& a) { return a.out_pre_bf16 || a.dact_of; }
inline bool has_ln_out(const cmdiad_gemm_args& a) { return a.ln_xb || a.ln_part || a.add2; }

// "the residual form only": out_f32 = A.W^T + bias + residual and nothing else (cmdiad_gemm_streamk_bf16 takes no other; the
// residual-tiles kernel is legal for no other)
inline bool residual_form_only(const cmdiad_gemm_args& a)
{
    return a.bias && a.residual && a.out_f32 && !a.out_bf16 && !a.group_bias && a.act == CMDIAD_ACT_NONE && !has_train_terms(a) &&
           a.split_k <= 1 && !a.m_count && !a.row_scale && !has_ln_out(a);
}
// residual products on the two-group 256 x 256 kernel, one tile per block (gemm_sk.hip): CMDIAD_GEMM_RES_WIDE=1 where it is legal
inline bool res_tiles_legal(const cmdiad_gemm_args& a) { return residual_form_only(a) && a.N % 256 == 0 && a.K >= 192; }

// two-group persistent kernel: whole 256-column tiles, bias, bf16-only output
inline bool pp3_legal(const cmdiad_gemm_args& a)
{
    return !has_train_terms(a) && !has_ln_out(a) && !a.group_bias && split_of(a) == 1 && a.N % 256 == 0 && a.K % 64 == 0 && a.K >= 192 &&
           a.bias && !a.residual && !a.out_f32 && a.out_bf16 && a.ldo16 % 8 == 0 && aligned16(a.out_bf16);
}
// ... chosen when every CU gets >= 2 tiles of a wide product.  CMDIAD_GEMM_PP3=1 / 0 forces it on / off wherever it is legal
// (A/B runs, parity tests)
inline bool pp3_wanted(const cmdiad_gemm_args& a, const switches& sw)
{
    const int forced = sw.pp3();
    return forced >= 0 ? forced != 0 : (a.N >= 1536 && tiles256(a.M, a.N) >= 2 * kPersistCUs);
}
// the 4-wave shapes of the A/B build know neither row_scale nor the LayerNorm outputs nor a live row count
inline bool wide_legal(const cmdiad_gemm_args& a)
{
    return !a.m_count && !has_train_terms(a) && !a.residual && !a.row_scale && !has_ln_out(a) && a.ldo16 % 4 == 0;
}
// fp32 residual stream in place (proj / fc2): out_f32 = acc + bias + residual through the row-contiguous epilogue of the 128 x 128
// kernel (its own instantiation: gemm.hip gemm_std_kernel, RES_ROWS), for a call of this form whose blocks own one N tile (panel 1)
inline bool res_rows_form(const cmdiad_gemm_args& a)
{
    return !has_train_terms(a) && a.act == CMDIAD_ACT_NONE && a.residual && a.out_f32 && !a.out_bf16 && !a.group_bias && a.bias &&
           split_of(a) == 1 && a.N % 64 == 0;
}

inline gemm_plan plan_gemm(const cmdiad_gemm_args& a, const switches& sw, bool ab_build)
{
    gemm_plan pl;
    CMDIAD_PLAN_REQUIRE(pl, a.A && a.W, "cmdiad_gemm_bf16: null operand");
    CMDIAD_PLAN_REQUIRE(pl, a.M > 0 && a.N > 0 && a.K > 0 && a.K % 64 == 0 && a.N % 4 == 0,
                        "cmdiad_gemm_bf16: need K%%64==0 and N%%4==0 (M=%d N=%d K=%d)", a.M, a.N, a.K);
    CMDIAD_PLAN_REQUIRE(pl, a.lda % 8 == 0 && a.ldw % 8 == 0 && aligned16(a.A) && aligned16(a.W),
                        "cmdiad_gemm_bf16: operands must be 16-byte aligned with ld%%8==0");
    CMDIAD_PLAN_REQUIRE(pl, a.out_f32 || a.out_bf16, "cmdiad_gemm_bf16: no output");
    CMDIAD_PLAN_REQUIRE(pl, (!a.out_f32 || (a.ldo32 % 4 == 0 && aligned16(a.out_f32))) && (!a.out_bf16 || (a.ldo16 % 4 == 0 && aligned8(a.out_bf16))) &&
                                (!a.residual || (a.ldr % 4 == 0 && aligned16(a.residual))) && (!a.bias || aligned16(a.bias)) &&
                                (!a.group_bias || (aligned16(a.group_bias) && a.group_rows > 0)),
                        "cmdiad_gemm_bf16: epilogue operand alignment");
    const int split = split_of(a);
    CMDIAD_PLAN_REQUIRE(pl, split == 1 || (a.out_f32 && !a.out_bf16 && !a.bias && !a.group_bias && !a.residual && a.act == CMDIAD_ACT_NONE && !has_train_terms(a)),
                        "cmdiad_gemm_bf16: split_k > 1 writes raw f32 slabs only");
    CMDIAD_PLAN_REQUIRE(pl, (!a.out_pre_bf16 || aligned8(a.out_pre_bf16)) && (!a.dact_of || aligned8(a.dact_of)), "cmdiad_gemm_bf16: out_pre_bf16 / dact_of alignment");
    CMDIAD_PLAN_REQUIRE(pl, ln_out_operands_ok(a.ln_xb, a.ld_xb, a.ln_part, a.add2, a.ld_add2),
                        "cmdiad_gemm_bf16: ln_xb and ln_part come together (8-byte aligned, ld_xb%%4==0); add2 only with them");
    CMDIAD_PLAN_REQUIRE(pl, !a.row_scale || (split == 1 && !has_train_terms(a) && !a.m_count), "cmdiad_gemm_bf16: row_scale with split_k / training terms / m_count");
    CMDIAD_PLAN_REQUIRE(pl, !a.m_count || split == 1, "cmdiad_gemm_bf16: m_count with split_k > 1");
    // These two ask whether the call has the residual-row form, which is that of a 128 x 128 block with one N tile.  Only such a call
    // needs the panel (and its switch) here, and no other kernel takes it: none knows LayerNorm outputs or a residual with a row_scale.
    const bool ln_out = has_ln_out(a), rr_form = res_rows_form(a);
    int panel = rr_form && (ln_out || a.row_scale) ? panel_tiles(a.M, a.N, a.K, split, sw) : 0;   // 0: not asked for yet
    CMDIAD_PLAN_REQUIRE(pl, !ln_out || (rr_form && panel == 1 && !a.row_scale && !a.m_count),
                        "cmdiad_gemm_bf16: ln_xb / ln_part need the in-place residual form (bias, residual, out_f32 only, N%%64==0)");
    CMDIAD_PLAN_REQUIRE(pl, !a.row_scale || !(rr_form && panel == 1), "cmdiad_gemm_bf16: row_scale with the residual-row form");

    pl.act = a.act;
    if (split > 1) {
        // a slab holds ceil(T / split) of the T K-tiles, so slabs ceil(T / per) .. split - 1 can be left without one (T = 33, split 8:
        // slab 7); their blocks return before any store (gemm_std_kernel), and the caller sums every slab: those are zeroed
        const int T = a.K / 64, per = (T + split - 1) / split, used = (T + per - 1) / per;
        if (used < split) pl.first_empty_slab = used;
    }
    if (const int wide = wide_legal(a) ? wide_choice(true, split, sw, ab_build) : 0) {
        const tile_grid g = wide_grid(a.M, a.N, a.K, wide);
        pl.kernel = wide == 8 ? gemm_kernel::wide8 : gemm_kernel::wide4;
        pl.grid_x = g.x;
        pl.panel = g.panel;
    } else if (res_tiles_legal(a) && sw.res_wide()) {
        pl.kernel = gemm_kernel::res_tiles;
        pl.grid_x = (unsigned)tiles256(a.M, a.N);
    } else if (pp3_legal(a) && pp3_wanted(a, sw)) {
        pl.kernel = a.row_scale ? gemm_kernel::pp3_rscale : gemm_kernel::pp3;
        pl.grid_x = persist_blocks(a.M, a.N, sw, ab_build);
    } else {
        // Every other network GEMM runs the 128 x 128 shape: the tile sweep on MI355X (profiles/r1_notes.md) had it ahead of
        // 256x128x3-stage and 256x256 on every ViT / Point-MAE shape
        if (!panel) panel = panel_tiles(a.M, a.N, a.K, split, sw);
        pl.kernel = rr_form && panel == 1 ? (ln_out ? gemm_kernel::res_rows_ln : gemm_kernel::res_rows)
                                          : (has_train_terms(a) ? gemm_kernel::general_train : gemm_kernel::general);
        pl.panel = panel;
        pl.group_m = panel == 1 && split == 1 ? group_m_tiles(sw) : 1;
        pl.grid_x = grid128(a.M, a.N, panel);
        pl.grid_y = (unsigned)split;
    }
    return pl;
}

// ------------------------------------------------------------------------------------------------
// Stream-K (gemm_sk.hip): every block's range must be at least one tile long (no block takes over and hands over the same
// tile), and the split must be worth it: more than one tile and less than two per CU
// ------------------------------------------------------------------------------------------------
inline bool streamk_eligible(int M, int N, int K)
{
    if (M <= 0 || N <= 0 || K <= 0 || N % 256 != 0 || K % 64 != 0 || K < 192) return false;
    const long tiles = tiles256(M, N), KT = K / 64;
    return tiles * KT / kPersistCUs >= KT && tiles > kPersistCUs && tiles < 2 * kPersistCUs;
}

// ------------------------------------------------------------------------------------------------
// Point-MAE block (blocks.cpp): fc1 + GELU + fc2 as one kernel (mlp_fused.hip), or the two launches it replaces.
// The fused MLP keeps a 128-row tile per CU (one block of 8 waves, all 160 KiB of LDS); below ~3/4 of a chip's worth of
// tiles the two launches, which spread smaller tiles over every CU, are at least as fast (B = 1: 8 tiles; the drop-in's
// micro-batches of 16: 128).  CMDIAD_PMAE_MLP=1 / 0 forces it on / off wherever it is legal (A/B runs, parity tests).
// ------------------------------------------------------------------------------------------------
inline bool pmae_mlp_fused_legal(bool folded, int C, int hidden) { return folded && C == 384 && hidden == 1536; }
inline bool pmae_mlp_fused_wanted(bool folded, int M, int C, int hidden, const switches& sw)
{
    if (!pmae_mlp_fused_legal(folded, C, hidden)) return false;
    const int forced = sw.pmae_mlp();
    return forced >= 0 ? forced != 0 : M >= 192 * 128;
}

// ------------------------------------------------------------------------------------------------
// Encoder first stage (cmdiad_encoder_stage1): persistent for M % 128 == 0; the once-per-block kernel keeps the ragged case
// (Mg = 32 / 64 with an odd group count).  A/B build: CMDIAD_STAGE1_PERSIST=0 selects the once-per-block kernel,
// CMDIAD_STAGE1_ONCE=0 the generic pipeline (conv1 re-staged per step).
// ------------------------------------------------------------------------------------------------
enum class stage1_kernel { persist, once, generic };
struct stage1_plan {
    stage1_kernel kernel;
    unsigned grid_x;
    int panel, n_tiles;
    bool g64;   // persistent form: Mg is 64 or 128, a wave's 64 rows are one group (encoder_stage1_persist_kernel<G64>)
};

inline stage1_plan plan_stage1(int M, int Mg, const switches& sw, bool ab_build)
{
    if (ab_build && !sw.stage1_once()) {
        const tile_grid g = groupmax_grid(M, 256, 128, 0, sw);
        return {stage1_kernel::generic, g.x, g.panel, 0, false};
    }
    if (M % 128 == 0 && !(ab_build && !sw.stage1_persist())) {
        const int n_tiles = M / 128;
        return {stage1_kernel::persist, (unsigned)(n_tiles < kPersistCUs ? n_tiles : kPersistCUs), 1, n_tiles, Mg >= 64};
    }
    return {stage1_kernel::once, (unsigned)ceil_div(M, 128), 1, 0, false};
}

// ------------------------------------------------------------------------------------------------
// Distance GEMM (l2min.hip): cmdiad_l2_min_keys / _counted / _segments
// ------------------------------------------------------------------------------------------------
enum class l2_tile { t128, two_group256, lockstep256 };   // l2_min_kernel<S128> | l2_min_pp3_kernel | l2_min_kernel<S2x2> (A/B build)

struct l2_call {
    const void *q, *q_sqnorm, *bank, *bank_sqnorm, *keys, *keys2;
    int Q, Nb, D;               // Q: the rows the launch is sized for (the caller's Q, Q_max, or n_seg * seg_stride)
    int n_seg, seg_stride;      // segments launch, or n_seg = 0
    uint32_t row_offset;
    int dtype;
};
struct l2_launch {
    l2_tile tile;
    int row0, rows;             // library rows [row0, row0 + rows) of the call's library
    int nq, nbt, splits, qgroup;
    unsigned grid_x;
};
struct l2_plan : status {
    int n = 0;                  // launches: 0 = nothing to search
    l2_launch launch[2];
};

// Library ranges per query tile of the segments launch (the W-way row-sharded search: W x the query tiles of one rank against
// 1/W of the library).  Measured on the bagel library at W = 1 / 2 / 4 / 8 (299 / 150 / 74 / 38 library tiles, 213 live query
// tiles per segment; tools/l2_segments_sweep.sh, profiles/r4_notes.md): ranges of ~15 tiles as in the single-library launch, but
// never fewer than 8 ranges -- a group of 4 query tiles x 8 ranges is what one XCD's 32 CUs hold at a time, with fewer ranges its
// L2 has to keep more query tiles than it can (W = 8: 1 range 6.35 ms, 8 ranges 5.96 ms) -- and ranges of at least 4 tiles.
inline int segment_splits(int nbt)
{
    int sp = nbt / 15;
    sp = sp < 8 ? 8 : (sp > 20 ? 20 : sp);
    const int most = nbt / 4 < 1 ? 1 : nbt / 4;
    return sp > most ? most : sp;
}

// one launch on `rows` library rows from row0: query tiles, library tiles, library ranges per query tile, query tiles per XCD group
inline l2_launch l2_geometry(l2_tile tile, const l2_call& c, int row0, int rows, const switches& sw)
{
    const int b = tile == l2_tile::t128 ? 128 : 256;   // BM = BN
    // segments: the launch is sized for every segment's cap (seg_stride rows); Q = n_seg * seg_stride
    const int nq = c.n_seg ? c.n_seg * (int)ceil_div(c.seg_stride, b) : (int)ceil_div(c.Q, b);
    const int nbt = (int)ceil_div(rows, b);
    // enough blocks to fill the chip a few times over, but long bank ranges per block so the running
    // min stays in registers and the per-block atomics stay negligible
    // measured on the bagel xyz library (profiles/r1_notes.md): 8 bank ranges for the 8-wave shapes; the 4-wave wide
    // shape gains another 5 % from 16-32 (shorter ranges, better tail balance), as long as a range keeps >= 4 tiles.
    // Round 3 (profiles/r3_notes.md, the two-group kernel on the de-duplicated 54 401 rows): 20 ranges of 15 tiles 5.40 ms against
    // 5.55 ms for 30 ranges of 10 -- a block's pipeline fill and drain are paid per range, and 213 live query tiles leave no
    // tail to balance; all 100 352 rows: within 1 % from 15 to 50 ranges.
    int splits = sw.l2_splits > 0 ? sw.l2_splits : 8;
    if (sw.l2_splits <= 0 && tile == l2_tile::two_group256) splits = nbt / 4 < 1 ? 1 : (nbt / 4 > 20 ? 20 : nbt / 4);
    const int seg_splits = c.n_seg && b == 256 ? sw.l2_seg_splits() : 0;
    if (c.n_seg && b == 256) splits = seg_splits > 0 ? seg_splits : segment_splits(nbt);   // tools/l2_segments.py sweeps it
    splits = splits > nbt ? nbt : splits;
    if (ceil_div(nbt, splits) > 4096) splits = (int)ceil_div(nbt, 4096);   // RowMin keeps a tile's place in 12 bits
    int qgroup = sw.l2_qgroup > 0 ? sw.l2_qgroup : 4;
    qgroup = qgroup > nq ? nq : qgroup;
    return {tile, row0, rows, nq, nbt, splits, qgroup, (unsigned)(ceil_div(nq, qgroup) * qgroup * splits)};
}

inline l2_plan plan_l2(const l2_call& c, const switches& sw, bool ab_build)
{
    l2_plan pl;
    CMDIAD_PLAN_REQUIRE(pl, c.Q >= 0 && c.Nb >= 0 && c.D > 0 && c.D % 64 == 0, "cmdiad_l2_min_keys: need D%%64==0 (D=%d)", c.D);
    CMDIAD_PLAN_REQUIRE(pl, c.dtype == CMDIAD_DT_BF16 || c.dtype == CMDIAD_DT_F16, "cmdiad_l2_min_keys: dtype");
    // nothing to search (an empty row shard: engine.Bank on a rank beyond the library's last row; a 0-row tensor has no address):
    // the keys stay what the caller put there
    if (c.Q == 0 || c.Nb == 0) return pl;
    CMDIAD_PLAN_REQUIRE(pl, c.q && c.q_sqnorm && c.bank && c.bank_sqnorm && c.keys, "cmdiad_l2_min_keys: null pointer");
    CMDIAD_PLAN_REQUIRE(pl, aligned16(c.q) && aligned16(c.bank), "cmdiad_l2_min_keys: 16-byte alignment");
    // the runner-up is defined on groups of 16 library rows (row >> 6, (row >> 2) & 3): launches whose keys are merged must agree on them
    CMDIAD_PLAN_REQUIRE(pl, !c.keys2 || c.row_offset % 64 == 0, "cmdiad_l2_min_keys: keys2 needs row_offset %% 64 == 0 (row_offset=%u)", c.row_offset);
    // production: the two-group 256 x 256 pipeline (l2_min_pp3_kernel) from Q >= 512, the 128 x 128 kernel below that, for the
    // last Nb % 256 library rows and for D < 192 (the two-group schedule assumes >= 3 K-tiles per library tile).
    // CMDIAD_L2_TILE (the parity tests force each shape on small inputs) = 0 / 5 for those two; the test-only
    // build (make ab) also knows 2 = the lock-step 256 x 256 shape of gemm::run.
    int tile = sw.l2_tile();
    if (tile < 0) tile = c.Q >= 512 ? 5 : 0;
    if (c.n_seg && tile != 0) tile = 5;    // segments exist for the production shapes only
    CMDIAD_PLAN_REQUIRE(pl, ab_build || tile != 2, "cmdiad_l2_min_keys: CMDIAD_L2_TILE=2 names an A/B variant that only the test build (make ab) contains");
    CMDIAD_PLAN_REQUIRE(pl, tile == 0 || tile == 2 || tile == 5, "cmdiad_l2_min_keys: CMDIAD_L2_TILE=%d is not a distance-GEMM shape (0, 5; test build: 2)", tile);
    if (tile == 5 && c.D < 192) tile = 0;
    if (tile == 5) {
        const int full = c.Nb / 256 * 256;
        if (full > 0) pl.launch[pl.n++] = l2_geometry(l2_tile::two_group256, c, 0, full, sw);
        if (c.Nb > full) pl.launch[pl.n++] = l2_geometry(l2_tile::t128, c, full, c.Nb - full, sw);
    } else pl.launch[pl.n++] = l2_geometry(tile == 2 ? l2_tile::lockstep256 : l2_tile::t128, c, 0, c.Nb, sw);
    return pl;
}

#undef CMDIAD_PLAN_REQUIRE

}  // namespace plan
