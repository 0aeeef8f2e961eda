// Host check of csrc/workspace.h, the carver every workspace layout of the library is cut with: for sequences of takes that mix
// element sizes, counts (zero included) and paddings, a sizing pass (null base) and a real pass agree on the total, every piece
// lies inside [base, base + total), the pieces are pairwise disjoint and start where the padding of the pieces before them
// ends -- pad rounds a piece's SIZE, so a piece starts aligned to its own pad exactly when the pads before it are multiples of
// it (every layout of the library but the 16-byte pieces of the dedup plan, which follow a 4-byte one) --, and the sizing pass
// never forms a pointer.  workspace_ok answers as the launchers rely on.  Compiled for the host with address +
// undefined sanitizers (a null base plus an offset is what the latter would report): tests/test_host_cpu.py.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../cmdiad_amd/csrc/workspace.h"

static char g_error[256];
void cmdiad_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

static int g_failures = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            ++g_failures;                    \
            printf("FAIL %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);             \
            printf("\n");                    \
        }                                    \
    } while (0)

struct Take {
    int elem;   // 1, 2, 4, 8 or 16 bytes
    size_t count, pad;
};
struct Piece {
    char* at;
    size_t bytes, pad;
};
struct alignas(16) Elem16 {
    char b[16];
};

static char* take(Carve& c, const Take& t)
{
    switch (t.elem) {
    case 1: return (char*)c.take<unsigned char>(t.count, t.pad);
    case 2: return (char*)c.take<uint16_t>(t.count, t.pad);
    case 4: return (char*)c.take<float>(t.count, t.pad);
    case 8: return (char*)c.take<unsigned long long>(t.count, t.pad);
    default: return (char*)c.take<Elem16>(t.count, t.pad);
    }
}

static void check_sequence(const std::vector<Take>& seq, const char* name)
{
    Carve sizing(nullptr);
    for (const Take& t : seq) CHECK(take(sizing, t) == nullptr, "%s: the sizing pass formed a pointer", name);
    const size_t total = sizing.total();

    std::vector<char> storage(total + 512);
    char* base = storage.data() + (256 - (uintptr_t)storage.data() % 256) % 256;   // 256-byte aligned, total bytes behind it
    Carve real(base);
    std::vector<Piece> pieces;
    size_t expect = 0;
    for (const Take& t : seq) {
        char* p = take(real, t);
        const size_t bytes = t.count * (size_t)t.elem;
        CHECK(p == base + expect, "%s: piece %zu starts at %td, %zu expected", name, pieces.size(), p - base, expect);
        expect += (bytes + t.pad - 1) / t.pad * t.pad;
        CHECK(real.total() == expect, "%s: total %zu after piece %zu, %zu expected", name, real.total(), pieces.size(), expect);
        pieces.push_back(Piece{p, bytes, t.pad});
    }
    CHECK(real.total() == total, "%s: real pass %zu bytes, sizing pass %zu", name, real.total(), total);
    for (size_t i = 0; i < pieces.size(); ++i) {
        const Piece& a = pieces[i];
        CHECK(a.at >= base && a.at + a.bytes <= base + total, "%s: piece %zu leaves the workspace", name, i);
        bool pads_nest = true;   // every earlier pad is a multiple of this one's: then this piece starts pad-aligned
        for (size_t k = 0; k < i; ++k) pads_nest = pads_nest && seq[k].pad % a.pad == 0;
        if (pads_nest) CHECK((uintptr_t)a.at % a.pad == 0, "%s: piece %zu is not aligned to its pad %zu", name, i, a.pad);
        for (size_t k = i + 1; k < pieces.size(); ++k) {
            const Piece& b = pieces[k];
            CHECK(a.at + a.bytes <= b.at, "%s: pieces %zu and %zu overlap", name, i, k);
        }
    }
    for (const Piece& p : pieces) memset(p.at, 0xA5, p.bytes);   // (the address sanitizer watches the storage's ends)
}

int main()
{
    // the shapes of the library's layouts: all padded to 256 (dbscan), the last piece unpadded (coreset, sort), pads 4 16 16 4
    // (dedup), nothing padded (transformer block, scan), one padded piece and a tail (plane RANSAC), empty pieces
    check_sequence({{8, 1, 256}, {4, 6, 256}, {4, 4097, 256}, {16, 500, 256}, {4, 501, 256}}, "all padded");
    check_sequence({{2, 70 * 32, 256}, {2, 72 * 32, 256}, {2, 72, 256}, {8, 8, 1}}, "last unpadded");
    check_sequence({{4, 1029, 4}, {4, 4, 16}, {1, 1029, 16}, {4, 2, 4}}, "dedup pads");
    check_sequence({{2, 65 * 128, 1}, {2, 65 * 128, 1}, {2, 65 * 512, 1}, {4, 2 * 65 * 2, 1}, {4, 256, 1}}, "unpadded");
    check_sequence({{8, 1, 256}, {8, 16 * 4, 1}}, "padded head");
    check_sequence({{4, 0, 256}, {1, 0, 1}, {8, 3, 256}, {4, 0, 16}, {1, 5, 1}}, "empty pieces");
    check_sequence({}, "no piece");
    // every combination of three takes
    const int elems[] = {1, 2, 4, 8, 16};
    const size_t counts[] = {0, 1, 3, 64, 257}, pads[] = {1, 4, 16, 256};
    std::vector<Take> all;
    for (int e : elems)
        for (size_t n : counts)
            for (size_t p : pads) all.push_back(Take{e, n, p});
    for (size_t i = 0; i < all.size(); i += 7)
        for (size_t j = 0; j < all.size(); j += 3)
            for (size_t k = 0; k < all.size(); k += 11) check_sequence({all[i], all[j], all[k]}, "triple");

    // Carve(nullptr): offsets only
    Carve c(nullptr);
    CHECK(c.take<float>(1000, 256) == nullptr && c.take<char>(0) == nullptr && c.take<double>(7) == nullptr, "null base: pointer formed");
    CHECK(c.total() == 4096 + 56, "null base: total %zu", c.total());

    // workspace_ok: enough bytes at a real address, or nothing needed
    char buf[64];
    CHECK(workspace_ok("f", buf, 64, 64) == CMDIAD_OK && workspace_ok("f", buf, 64, 0) == CMDIAD_OK, "workspace_ok: refuses a fit");
    CHECK(workspace_ok("f", nullptr, 0, 0) == CMDIAD_OK, "workspace_ok: nothing needed");
    g_error[0] = 0;
    CHECK(workspace_ok("cmdiad_f", buf, 63, 64) == CMDIAD_ERR_WORKSPACE, "workspace_ok: accepts 63 of 64");
    CHECK(strcmp(g_error, "cmdiad_f: workspace of 63 bytes, 64 needed") == 0, "workspace_ok: text '%s'", g_error);
    CHECK(workspace_ok("cmdiad_f", nullptr, 64, 64) == CMDIAD_ERR_WORKSPACE && strstr(g_error, "workspace"), "workspace_ok: accepts null");

    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("workspace ok\n");
    return 0;
}
