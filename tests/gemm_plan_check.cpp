// Host-side check of cmdiad_amd/csrc/gemm_plan.h, the header that decides which kernel of the GEMM family runs and on which grid
// (cmdiad_gemm_bf16, stream-K eligibility, the fused Point-MAE MLP, the encoder's first stage, the distance GEMM).  Without
// arguments: the launches of the workload, the switches, the argument errors and the smaller rules, against values derived by
// hand from the launchers the header replaced; prints "gemm plan ok".  With --lines: one case per line on stdin, one line out per
// case (per launch for the distance GEMM), so that tests/test_host_cpu.py can put the case tables of tests/gemm_ref.py through
// the plan.  Built and run by tests/test_host_cpu.py with the host compiler and the address + undefined sanitizers.
//
//   gemm key=value ...   keys: ab M N K bias gb (group_rows) act res rscale split out (f32 | bf16 | both) ln add2 pre dact mcount
//                              lda ldw ldr ldo32 ldo16, and any CMDIAD_* switch
//        -> <case> <kernel> <act> <grid.x> <grid.y> <panel> <group_m> <first empty slab or -1> <reads of the environment>
//           |   <case> error <code> <text>
//   l2 key=value ...     keys: ab Q Nb D nseg stride keys2 rowoff dtype, and any CMDIAD_* switch
//        -> <case> <tile> <first row> <rows> <nq> <nbt> <splits> <qgroup> <grid.x> <empty ranges> per launch   |   <case> nothing   |   <case> error ...
//   streamk M= N= K=     -> <case> eligible | <case> not
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>

#include "../cmdiad_amd/csrc/gemm_plan.h"

namespace {

using plan::gemm_kernel;
using plan::l2_tile;
typedef std::map<std::string, std::string> Case;

int failures = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            if (++failures <= 20) { std::printf("FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                \
    } while (0)

Case parse(const std::string& text)
{
    Case c;
    std::istringstream in(text);
    for (std::string tok; in >> tok;) {
        const size_t eq = tok.find('=');
        c[tok.substr(0, eq)] = eq == std::string::npos ? "1" : tok.substr(eq + 1);
    }
    return c;
}
long num(const Case& c, const char* key, long dflt = 0) { const auto it = c.find(key); return it == c.end() ? dflt : atol(it->second.c_str()); }

// The environment of a case: its CMDIAD_* words.  The plan reads it through this getenv, as the library does through the real one
// (csrc/launch.h env_switches), so the reads of a call can be counted.
const Case* fake_env = nullptr;
int reads = 0;
const char* fake_getenv(const char* name)
{
    ++reads;
    const auto it = fake_env->find(name);
    return it == fake_env->end() ? nullptr : it->second.c_str();
}
plan::switches switches_of(const Case& c)
{
    static const char* const known[] = {"CMDIAD_GEMM_GROUPM", "CMDIAD_GEMM_PANEL_MIN", "CMDIAD_GEMM_PP3", "CMDIAD_GEMM_RES_WIDE", "CMDIAD_GEMM_WIDE",
                                        "CMDIAD_PP3_GRID", "CMDIAD_L2_TILE", "CMDIAD_L2_SPLITS", "CMDIAD_L2_QGROUP", "CMDIAD_L2_SEG_SPLITS",
                                        "CMDIAD_PMAE_MLP", "CMDIAD_STAGE1_PERSIST", "CMDIAD_STAGE1_ONCE"};
    for (const auto& kv : c) {
        bool ok = kv.first.rfind("CMDIAD_", 0) != 0;
        for (const char* k : known) ok = ok || kv.first == k;
        if (!ok) { std::printf("unknown switch %s\n", kv.first.c_str()); exit(2); }
    }
    fake_env = &c;   // the caller keeps the case alive while it plans
    reads = 0;
    // the two that the library reads once per process (csrc/launch.h l2_switches)
    return {fake_getenv, (int)num(c, "CMDIAD_L2_SPLITS", 0), (int)num(c, "CMDIAD_L2_QGROUP", 0)};
}

// operands are addresses only: distinct, 256-byte aligned, never dereferenced
template <class T> T* addr(int i) { return reinterpret_cast<T*>((uintptr_t)0x100000 * (uintptr_t)(i + 1)); }

cmdiad_gemm_args gemm_args(const Case& c)
{
    cmdiad_gemm_args a{};
    a.M = (int)num(c, "M"); a.N = (int)num(c, "N"); a.K = (int)num(c, "K");
    a.A = addr<const uint16_t>(0); a.lda = (int)num(c, "lda", a.K);
    a.W = addr<const uint16_t>(1); a.ldw = (int)num(c, "ldw", a.K);
    if (num(c, "bias")) a.bias = addr<const float>(2);
    a.group_rows = (int)num(c, "gb", 0);
    if (a.group_rows) a.group_bias = addr<const float>(3);
    else a.group_rows = 1;
    a.act = (int)num(c, "act");
    if (num(c, "res")) { a.residual = addr<const float>(4); a.ldr = (int)num(c, "ldr", a.N); }
    const std::string out = c.count("out") ? c.at("out") : "";
    if (out == "f32" || out == "both") { a.out_f32 = addr<float>(5); a.ldo32 = (int)num(c, "ldo32", a.N); }
    if (out == "bf16" || out == "both") { a.out_bf16 = addr<uint16_t>(6); a.ldo16 = (int)num(c, "ldo16", a.N); }
    if (num(c, "pre")) a.out_pre_bf16 = addr<uint16_t>(7);
    if (num(c, "dact")) a.dact_of = addr<const uint16_t>(8);
    a.split_k = (int)num(c, "split", 1);
    if (num(c, "mcount")) a.m_count = addr<const int>(9);
    if (num(c, "rscale")) a.row_scale = addr<const float>(10);
    if (num(c, "ln")) { a.ln_xb = addr<uint16_t>(11); a.ld_xb = (int)num(c, "ld_xb", a.N); a.ln_part = addr<float>(12); }
    if (c.count("lnpart")) a.ln_part = addr<float>(12);   // ln_part without ln_xb
    if (num(c, "add2")) { a.add2 = addr<const float>(13); a.ld_add2 = (int)num(c, "ld_add2", a.N); }
    return a;
}
plan::gemm_plan plan_gemm_case(const Case& c) { return plan::plan_gemm(gemm_args(c), switches_of(c), num(c, "ab") != 0); }
plan::gemm_plan G(const char* text) { const Case c = parse(text); return plan_gemm_case(c); }

plan::l2_plan plan_l2_case(const Case& c)
{
    plan::l2_call q{addr<void>(0), addr<void>(1), addr<void>(2), addr<void>(3), addr<void>(4), num(c, "keys2") ? addr<void>(5) : nullptr,
                    (int)num(c, "Q"), (int)num(c, "Nb"), (int)num(c, "D"), (int)num(c, "nseg"), (int)num(c, "stride"),
                    (uint32_t)num(c, "rowoff"), (int)num(c, "dtype", CMDIAD_DT_BF16)};
    if (q.n_seg) q.Q = q.n_seg * q.seg_stride;
    return plan::plan_l2(q, switches_of(c), num(c, "ab") != 0);
}
plan::l2_plan L(const char* text) { const Case c = parse(text); return plan_l2_case(c); }

const char* name_of(gemm_kernel k)
{
    switch (k) {
    case gemm_kernel::general: return "general";
    case gemm_kernel::general_train: return "general_train";
    case gemm_kernel::res_rows: return "res_rows";
    case gemm_kernel::res_rows_ln: return "res_rows_ln";
    case gemm_kernel::pp3: return "pp3";
    case gemm_kernel::pp3_rscale: return "pp3_rscale";
    case gemm_kernel::res_tiles: return "res_tiles";
    case gemm_kernel::wide4: return "wide4";
    case gemm_kernel::wide8: return "wide8";
    }
    return "?";
}
const char* name_of(l2_tile t) { return t == l2_tile::t128 ? "t128" : (t == l2_tile::two_group256 ? "two_group256" : "lockstep256"); }

int lines()
{
    char buf[1024];
    for (int n = 0; std::fgets(buf, sizeof buf, stdin); ++n) {
        const Case c = parse(buf);
        if (c.count("gemm")) {
            const plan::gemm_plan p = plan_gemm_case(c);
            if (p.err) std::printf("%d error %d %s\n", n, p.err, p.text);
            else std::printf("%d %s %d %u %u %d %d %d %d\n", n, name_of(p.kernel), p.act, p.grid_x, p.grid_y, p.panel, p.group_m, p.first_empty_slab, reads);
        } else if (c.count("l2")) {
            const plan::l2_plan p = plan_l2_case(c);
            if (p.err) std::printf("%d error %d %s\n", n, p.err, p.text);
            else if (!p.n) std::printf("%d nothing\n", n);
            for (int i = 0; !p.err && i < p.n; ++i) {
                const plan::l2_launch& l = p.launch[i];
                // the kernels cut the nbt library tiles into `splits` ranges of per = ceil(nbt / splits) tiles (csrc/l2min.hip: nt0 =
                // split * per, ntc = min(per, nbt - nt0)): the ranges from ceil(nbt / per) on hold no tile and their blocks leave
                const int per = (l.nbt + l.splits - 1) / l.splits;
                std::printf("%d %s %d %d %d %d %d %d %u %d\n", n, name_of(l.tile), l.row0, l.rows, l.nq, l.nbt, l.splits, l.qgroup, l.grid_x,
                            l.splits - (l.nbt + per - 1) / per);
            }
        } else if (c.count("streamk")) {
            std::printf("%d %s\n", n, plan::streamk_eligible((int)num(c, "M"), (int)num(c, "N"), (int)num(c, "K")) ? "eligible" : "not");
        } else { std::printf("%d unknown case\n", n); return 2; }
    }
    return 0;
}

#define EXPECT_GEMM(spec, k, gx, gy, pn, gm)                                                                                   \
    do {                                                                                                                       \
        const plan::gemm_plan p_ = G(spec);                                                                                    \
        CHECK(!p_.err && p_.kernel == (k) && p_.grid_x == (unsigned)(gx) && p_.grid_y == (unsigned)(gy) && p_.panel == (pn) && p_.group_m == (gm), \
              "%s -> err %d %s, %s grid %u x %u panel %d group_m %d", spec, p_.err, p_.err ? p_.text : "", name_of(p_.kernel), p_.grid_x, p_.grid_y, p_.panel, p_.group_m); \
    } while (0)
#define EXPECT_ERROR(pl, want)                                                                                                 \
    do {                                                                                                                       \
        const auto p_ = (pl);                                                                                                  \
        CHECK(p_.err == CMDIAD_ERR_ARG && std::strcmp(p_.text, want) == 0, "err %d, text \"%s\"", p_.err, p_.err ? p_.text : ""); \
    } while (0)

// reads of the environment by the last plan: no more than the launcher that the plan replaced made for such a call
#define EXPECT_READS(spec, n) do { G(spec); CHECK(reads == (n), "%s: %d reads of the environment", spec, reads); } while (0)

void check_gemm()
{
    // the workload's launches, default switches, product build
    const char* fc1 = "M=25120 N=3072 K=768 bias act=1 out=bf16";                       // ViT fc1, batch 32: 1 188 tiles, five rounds
    const char* proj = "M=25120 N=768 K=768 bias res out=f32";                          // ViT proj, in place
    EXPECT_GEMM(fc1, gemm_kernel::pp3, 238, 1, 1, 1);
    CHECK(G(fc1).act == CMDIAD_ACT_GELU, "fc1's activation");
    EXPECT_GEMM(proj, gemm_kernel::res_rows, 1182, 1, 1, 8);
    EXPECT_GEMM("M=32768 N=384 K=384 bias res out=f32 ln add2", gemm_kernel::res_rows_ln, 768, 1, 1, 8);
    EXPECT_GEMM("M=32768 N=1536 K=384 bias rscale act=1 out=bf16", gemm_kernel::pp3_rscale, 256, 1, 1, 1);
    EXPECT_GEMM("M=4194304 N=512 K=256 gb=128 act=2 out=bf16", gemm_kernel::general, 32768, 1, 4, 1);
    CHECK(G("M=4194304 N=512 K=256 gb=128 act=2 out=bf16").act == CMDIAD_ACT_RELU, "the encoder product's activation");
    EXPECT_GEMM("M=256 N=256 K=2112 split=8 out=f32", gemm_kernel::general, 4, 8, 1, 1);
    CHECK(G("M=256 N=256 K=2112 split=8 out=f32").first_empty_slab == 7, "33 K-tiles in 8 slabs of 5: slab 7 is empty");
    CHECK(G("M=256 N=256 K=2048 split=8 out=f32").first_empty_slab == -1 && G(fc1).first_empty_slab == -1, "no empty slab");
    EXPECT_GEMM("M=25120 N=3072 K=768 bias act=1 out=bf16 dact", gemm_kernel::general_train, 4728, 1, 1, 8);
    // switches
    EXPECT_GEMM("M=25120 N=3072 K=768 bias act=1 out=bf16 CMDIAD_GEMM_PP3=0", gemm_kernel::general, 4728, 1, 1, 8);
    EXPECT_GEMM("M=25120 N=768 K=768 bias res out=f32 CMDIAD_GEMM_RES_WIDE=1", gemm_kernel::res_tiles, 297, 1, 1, 1);
    EXPECT_GEMM("M=25120 N=768 K=768 bias res out=f32 CMDIAD_GEMM_GROUPM=1", gemm_kernel::res_rows, 1182, 1, 1, 1);
    EXPECT_GEMM("M=25120 N=768 K=768 bias res out=f32 CMDIAD_GEMM_GROUPM=0", gemm_kernel::res_rows, 1182, 1, 1, 1);
    EXPECT_GEMM("M=300 N=256 K=192 bias out=bf16 CMDIAD_GEMM_PP3=1", gemm_kernel::pp3, 2, 1, 1, 1);
    EXPECT_GEMM("M=300 N=256 K=192 bias out=bf16 CMDIAD_GEMM_PP3=1 CMDIAD_PP3_GRID=1", gemm_kernel::pp3, 2, 1, 1, 1);   // acts in the A/B build only
    EXPECT_GEMM("ab M=300 N=256 K=192 bias out=bf16 CMDIAD_GEMM_PP3=1 CMDIAD_PP3_GRID=1", gemm_kernel::pp3, 1, 1, 1, 1);
    EXPECT_GEMM("M=300 N=256 K=128 bias out=bf16 CMDIAD_GEMM_PP3=1", gemm_kernel::general, 6, 1, 1, 8);                  // K < 192: not legal
    EXPECT_GEMM("M=300 N=1156 K=512 bias act=2 out=bf16 CMDIAD_GEMM_PANEL_MIN=1", gemm_kernel::general, 6, 1, 8, 1);     // 10 N tiles in panels of 8
    EXPECT_GEMM("M=300 N=1156 K=512 bias act=2 out=both CMDIAD_GEMM_WIDE=8", gemm_kernel::general, 30, 1, 1, 8);
    EXPECT_GEMM("ab M=300 N=1156 K=512 bias act=2 out=both CMDIAD_GEMM_WIDE=8", gemm_kernel::wide8, 2, 1, 5, 1);
    EXPECT_GEMM("ab M=300 N=1156 K=576 bias act=2 out=both CMDIAD_GEMM_WIDE=4", gemm_kernel::wide4, 20, 1, 1, 1);
    EXPECT_GEMM("ab M=300 N=1156 K=512 bias res out=both CMDIAD_GEMM_WIDE=8", gemm_kernel::general, 30, 1, 1, 8);        // the wide shapes take no residual
    // A switch is read only where a rule consults it (cmdiad_gemm_bf16 runs some 600 times per image).  Product build, the old
    // launcher's reads in brackets: fc1 CMDIAD_GEMM_PP3 [1]; proj _RES_WIDE and _GROUPM (K > 512: no panel) [4]; the LayerNorm form
    // _PANEL_MIN and _GROUPM [3]; legal for the persistent kernel but not chosen _PP3, _PANEL_MIN, _GROUPM [3]; the encoder's panel
    // _PANEL_MIN [2]; split-K none [2].  A/B build: _GEMM_WIDE where the wide shapes are legal, _PP3_GRID on the persistent kernel.
    EXPECT_READS(fc1, 1);
    EXPECT_READS(proj, 2);
    EXPECT_READS("M=32768 N=384 K=384 bias res out=f32 ln add2", 2);
    EXPECT_READS("M=300 N=512 K=256 bias act=1 out=bf16", 3);
    EXPECT_READS("M=4194304 N=512 K=256 gb=128 act=2 out=bf16", 1);
    EXPECT_READS("M=256 N=256 K=2112 split=8 out=f32", 0);
    EXPECT_READS("M=25120 N=768 K=768 bias res out=f32 CMDIAD_GEMM_RES_WIDE=1", 1);
    EXPECT_READS("ab M=25120 N=3072 K=768 bias act=1 out=bf16", 3);
    EXPECT_READS("ab M=300 N=1156 K=512 bias act=2 out=both CMDIAD_GEMM_WIDE=8", 1);
    EXPECT_READS("M=128 N=128 K=96 out=f32", 0);
    // argument errors, each with the launcher's text
    EXPECT_ERROR(G("M=128 N=128 K=96 out=f32"), "cmdiad_gemm_bf16: need K%64==0 and N%4==0 (M=128 N=128 K=96)");
    EXPECT_ERROR(G("M=128 N=128 K=64"), "cmdiad_gemm_bf16: no output");
    EXPECT_ERROR(G("M=128 N=128 K=128 split=2 bias out=f32"), "cmdiad_gemm_bf16: split_k > 1 writes raw f32 slabs only");
    EXPECT_ERROR(G("M=128 N=128 K=64 bias res out=f32 lnpart"),
                 "cmdiad_gemm_bf16: ln_xb and ln_part come together (8-byte aligned, ld_xb%4==0); add2 only with them");
    EXPECT_ERROR(G("M=128 N=128 K=64 bias res out=f32 ln act=1"),
                 "cmdiad_gemm_bf16: ln_xb / ln_part need the in-place residual form (bias, residual, out_f32 only, N%64==0)");
    EXPECT_ERROR(G("M=128 N=128 K=64 bias res out=f32 rscale"), "cmdiad_gemm_bf16: row_scale with the residual-row form");
    EXPECT_ERROR(G("M=128 N=128 K=64 bias out=bf16 rscale mcount"), "cmdiad_gemm_bf16: row_scale with split_k / training terms / m_count");
    EXPECT_ERROR(G("M=128 N=128 K=64 out=f32 lda=68"), "cmdiad_gemm_bf16: operands must be 16-byte aligned with ld%8==0");
    EXPECT_ERROR(G("M=128 N=128 K=64 out=bf16 ldo16=130"), "cmdiad_gemm_bf16: epilogue operand alignment");
    EXPECT_ERROR(G("M=128 N=128 K=128 split=2 out=f32 mcount"), "cmdiad_gemm_bf16: m_count with split_k > 1");
    // the two late errors of the old launcher come before anything is decided: here a split-K call that would also zero a slab
    // cannot carry LayerNorm outputs (it fails the raw-slab check first), and a panelled product is not the residual-row form
    EXPECT_ERROR(G("M=300 N=1152 K=512 bias res out=f32 ln CMDIAD_GEMM_PANEL_MIN=1"),
                 "cmdiad_gemm_bf16: ln_xb / ln_part need the in-place residual form (bias, residual, out_f32 only, N%64==0)");
    cmdiad_gemm_args a = gemm_args(parse("M=128 N=128 K=64 out=f32"));
    a.A = nullptr;
    EXPECT_ERROR(plan::plan_gemm(a, plan::switches(), false), "cmdiad_gemm_bf16: null operand");   // no getenv: the empty environment
    a = gemm_args(parse("M=128 N=128 K=64 out=f32"));
    a.W = reinterpret_cast<const uint16_t*>((uintptr_t)a.W + 8);
    EXPECT_ERROR(plan::plan_gemm(a, plan::switches(), false), "cmdiad_gemm_bf16: operands must be 16-byte aligned with ld%8==0");
}

void check_l2()
{
    plan::l2_plan p = L("Q=100352 Nb=76544 D=768");
    CHECK(!p.err && p.n == 1, "err %d n %d", p.err, p.n);
    const plan::l2_launch& a = p.launch[0];
    CHECK(a.tile == l2_tile::two_group256 && a.row0 == 0 && a.rows == 76544 && a.nq == 392 && a.nbt == 299 && a.splits == 20 && a.qgroup == 4 && a.grid_x == 7840,
          "%s rows %d nq %d nbt %d splits %d qgroup %d grid %u", name_of(a.tile), a.rows, a.nq, a.nbt, a.splits, a.qgroup, a.grid_x);
    CHECK(reads == 1, "one launch reads CMDIAD_L2_TILE: %d reads", reads);   // the old launcher: 2
    p = L("Q=100352 Nb=76644 D=768");
    CHECK(reads == 1, "two launches read CMDIAD_L2_TILE once: %d reads", reads);   // the old launcher: 3
    CHECK(!p.err && p.n == 2, "err %d n %d", p.err, p.n);
    const plan::l2_launch &b = p.launch[0], &r = p.launch[1];
    CHECK(b.tile == l2_tile::two_group256 && b.rows == 76544 && b.nq == 392 && b.nbt == 299 && b.splits == 20 && b.qgroup == 4 && b.grid_x == 7840, "the whole tiles");
    CHECK(r.tile == l2_tile::t128 && r.row0 == 76544 && r.rows == 100 && r.nq == 784 && r.nbt == 1 && r.splits == 1 && r.qgroup == 4 && r.grid_x == 784,
          "remainder: %s row0 %d rows %d nq %d nbt %d splits %d grid %u", name_of(r.tile), r.row0, r.rows, r.nq, r.nbt, r.splits, r.grid_x);
    p = L("nseg=8 stride=54528 Nb=9728 D=768");                      // 38 library tiles per rank of an 8-way sharded search
    CHECK(!p.err && p.n == 1 && p.launch[0].tile == l2_tile::two_group256 && p.launch[0].nbt == 38 && p.launch[0].splits == 8 && p.launch[0].nq == 8 * 213,
          "segments: n %d nbt %d splits %d nq %d", p.n, p.launch[0].nbt, p.launch[0].splits, p.launch[0].nq);
    CHECK(reads == 2, "segments read CMDIAD_L2_TILE and CMDIAD_L2_SEG_SPLITS: %d reads", reads);   // the old launcher: 2
    p = L("nseg=8 stride=54528 Nb=9728 D=768 CMDIAD_L2_SEG_SPLITS=3");
    CHECK(p.launch[0].splits == 3, "forced segment splits: %d", p.launch[0].splits);
    p = L("ab nseg=2 stride=100 Nb=9728 D=768 CMDIAD_L2_TILE=2");    // segments know the production shapes only: any other becomes 5 ...
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::two_group256 && p.launch[0].nq == 2 && p.launch[0].splits == 8, "segments, tile 2 asked for: %s", name_of(p.launch[0].tile));
    p = L("nseg=8 stride=54528 Nb=9728 D=768 CMDIAD_L2_TILE=0");     // ... unless it is tile 0, asked for or chosen (fewer than 512 rows)
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128 && p.launch[0].nq == 8 * 426 && p.launch[0].splits == 8, "segments on tile 0: %s splits %d", name_of(p.launch[0].tile), p.launch[0].splits);
    p = L("nseg=2 stride=100 Nb=9728 D=768");
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128 && p.launch[0].nq == 2, "small segments: %s", name_of(p.launch[0].tile));
    p = L("Q=100 Nb=3000 D=768");
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128 && p.launch[0].nbt == 24 && p.launch[0].splits == 8 && p.launch[0].nq == 1 && p.launch[0].qgroup == 1 && p.launch[0].grid_x == 8, "Q = 100");
    p = L("Q=100 Nb=500 D=768");
    CHECK(p.n == 1 && p.launch[0].nbt == 4 && p.launch[0].splits == 4, "Q = 100 on four library tiles: splits %d", p.launch[0].splits);
    p = L("Q=1000 Nb=3000 D=128");
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128, "D < 192: %s", name_of(p.launch[0].tile));
    p = L("Q=511 Nb=3000 D=768");
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128, "Q = 511");
    p = L("Q=512 Nb=3000 D=768");
    CHECK(p.n == 2 && p.launch[0].tile == l2_tile::two_group256 && p.launch[0].rows == 2816 && p.launch[0].splits == 2 && p.launch[1].rows == 184, "Q = 512");
    p = L("Q=512 Nb=200 D=768");
    CHECK(p.n == 1 && p.launch[0].tile == l2_tile::t128 && p.launch[0].row0 == 0 && p.launch[0].rows == 200, "a library below one 256-row tile");
    CHECK(!L("Q=0 Nb=3000 D=768").err && L("Q=0 Nb=3000 D=768").n == 0 && L("Q=100 Nb=0 D=768").n == 0, "nothing to launch");
    EXPECT_ERROR(L("Q=100 Nb=3000 D=768 keys2 rowoff=32"), "cmdiad_l2_min_keys: keys2 needs row_offset % 64 == 0 (row_offset=32)");
    CHECK(!L("Q=100 Nb=3000 D=768 rowoff=32").err && !L("Q=100 Nb=3000 D=768 keys2 rowoff=64").err, "row_offset without keys2, or a multiple of 64");
    EXPECT_ERROR(L("Q=100 Nb=3000 D=768 CMDIAD_L2_TILE=2"), "cmdiad_l2_min_keys: CMDIAD_L2_TILE=2 names an A/B variant that only the test build (make ab) contains");
    p = L("ab Q=100 Nb=3000 D=768 CMDIAD_L2_TILE=2");
    CHECK(!p.err && p.n == 1 && p.launch[0].tile == l2_tile::lockstep256 && p.launch[0].nbt == 12 && p.launch[0].splits == 8, "the lock-step shape in the A/B build");
    EXPECT_ERROR(L("Q=100 Nb=3000 D=768 CMDIAD_L2_TILE=3"), "cmdiad_l2_min_keys: CMDIAD_L2_TILE=3 is not a distance-GEMM shape (0, 5; test build: 2)");
    EXPECT_ERROR(L("Q=100 Nb=3000 D=100"), "cmdiad_l2_min_keys: need D%64==0 (D=100)");
    EXPECT_ERROR(L("Q=100 Nb=3000 D=768 dtype=7"), "cmdiad_l2_min_keys: dtype");
    p = L("Q=100 Nb=12800000 D=64 CMDIAD_L2_SPLITS=8");              // 100 000 library tiles: 12 500 per range do not fit RowMin's 12 bits
    CHECK(p.n == 1 && p.launch[0].nbt == 100000 && p.launch[0].splits == 25, "the 12-bit cap: nbt %d splits %d", p.launch[0].nbt, p.launch[0].splits);
    p = L("Q=100352 Nb=76544 D=768 CMDIAD_L2_QGROUP=8 CMDIAD_L2_SPLITS=30");
    CHECK(p.launch[0].splits == 30 && p.launch[0].qgroup == 8 && p.launch[0].grid_x == 392u * 30u, "forced splits and qgroup");
}

void check_rules()
{
    // (tests/gemm_ref.py STREAMK_SHAPES come through the line mode)
    CHECK(plan::streamk_eligible(65537, 256, 192), "257 tiles of three K-tiles");
    CHECK(!plan::streamk_eligible(65536, 256, 192), "256 tiles: not more than the CUs");
    CHECK(!plan::streamk_eligible(131073, 256, 192), "513 tiles");
    CHECK(!plan::streamk_eligible(65537, 256, 128), "K = 128");
    CHECK(!plan::streamk_eligible(65537, 260, 192) && !plan::streamk_eligible(0, 256, 192), "N not a multiple of 256, M = 0");
    CHECK(plan::residual_form_only(gemm_args(parse("M=65537 N=256 K=192 bias res out=f32"))), "the residual form");
    for (const char* more : {"out=both", "act=1", "gb=1", "split=2", "mcount", "rscale", "ln", "pre", "dact"}) {
        Case c = parse("M=65537 N=256 K=192 bias res out=f32");
        const Case extra = parse(more);
        for (const auto& kv : extra) c[kv.first] = kv.second;
        CHECK(!plan::residual_form_only(gemm_args(c)), "the residual form with %s", more);
    }
    const plan::switches sw;   // the empty environment
    const Case on_env = parse("CMDIAD_PMAE_MLP=1"), off_env = parse("CMDIAD_PMAE_MLP=0");
    const auto on = [&] { return switches_of(on_env); };   // one fake environment at a time: the last switches_of
    CHECK(plan::pmae_mlp_fused_wanted(true, 24576, 384, 1536, sw) && !plan::pmae_mlp_fused_wanted(true, 24448, 384, 1536, sw), "192 tiles of 128 rows");
    CHECK(!plan::pmae_mlp_fused_wanted(true, 24576, 768, 1536, sw) && !plan::pmae_mlp_fused_wanted(true, 24576, 384, 3072, sw), "C, hidden");
    CHECK(plan::pmae_mlp_fused_wanted(true, 128, 384, 1536, on()) && !plan::pmae_mlp_fused_wanted(true, 32768, 384, 1536, switches_of(off_env)), "forced on / off");
    CHECK(!plan::pmae_mlp_fused_wanted(false, 32768, 384, 1536, on()) && reads == 0 && !plan::pmae_mlp_fused_wanted(true, 32768, 768, 3072, on()), "never where it is not legal");
    CHECK(reads == 0, "the fused-MLP switch is read only where it can act: %d reads", reads);
    for (int ab = 0; ab < 2; ++ab) {
        plan::stage1_plan s = plan::plan_stage1(128, 128, sw, ab);
        CHECK(s.kernel == plan::stage1_kernel::persist && s.grid_x == 1 && s.n_tiles == 1 && s.panel == 1 && s.g64, "stage 1, M = 128");
        s = plan::plan_stage1(4096, 32, sw, ab);
        CHECK(s.kernel == plan::stage1_kernel::persist && s.grid_x == 32 && s.n_tiles == 32 && !s.g64, "stage 1, M = 4096 in groups of 32");
        s = plan::plan_stage1(4194304, 64, sw, ab);
        CHECK(s.kernel == plan::stage1_kernel::persist && s.grid_x == 256 && s.n_tiles == 32768 && s.g64, "stage 1, one block per CU");
        s = plan::plan_stage1(3 * 32, 32, sw, ab);
        CHECK(s.kernel == plan::stage1_kernel::once && s.grid_x == 1 && s.panel == 1, "stage 1, three groups of 32");
    }
    const Case stage1_env = parse("CMDIAD_STAGE1_PERSIST=0"), once_env = parse("CMDIAD_STAGE1_ONCE=0");
    const auto no_persist = [&] { return switches_of(stage1_env); };
    const auto no_once = [&] { return switches_of(once_env); };
    CHECK(plan::plan_stage1(4096, 128, no_persist(), false).kernel == plan::stage1_kernel::persist && plan::plan_stage1(4096, 128, no_once(), false).kernel == plan::stage1_kernel::persist,
          "the stage-1 switches act in the A/B build only");
    CHECK(plan::plan_stage1(4096, 128, no_persist(), true).kernel == plan::stage1_kernel::once && plan::plan_stage1(4096, 128, no_persist(), true).grid_x == 32, "CMDIAD_STAGE1_PERSIST=0");
    CHECK(plan::plan_stage1(4096, 128, no_once(), true).kernel == plan::stage1_kernel::generic && plan::plan_stage1(4096, 128, no_once(), true).grid_x == 64, "CMDIAD_STAGE1_ONCE=0");
    // group-max and QKV grids
    plan::tile_grid g = plan::groupmax_grid(4194304, 512, 256, 0, sw);
    CHECK(g.x == 32768 && g.panel == 4, "group-max, the encoder's shape: grid %u panel %d", g.x, g.panel);
    g = plan::groupmax_grid(4096, 384, 128, 0, sw);
    CHECK(g.x == 96 && g.panel == 1, "group-max, small: grid %u panel %d", g.x, g.panel);
    g = plan::groupmax_grid(4096, 384, 128, 8, sw);
    CHECK(g.x == 16 && g.panel == 2, "group-max on the 256 x 256 shape: grid %u panel %d", g.x, g.panel);
    CHECK(plan::grid128(25120, 3 * 768) == 197u * 18u, "QKV grid");
    CHECK(plan::persist_blocks(25120, 3072, sw, false) == 238 && plan::persist_blocks(300, 256, sw, false) == 2, "persistent grids");
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--lines") == 0) return lines();
    check_gemm();
    check_l2();
    check_rules();
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("gemm plan ok\n");
    return 0;
}
