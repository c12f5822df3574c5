// Stand-alone check of csrc/ipa_plan.hpp (its own main; tests/test_ipa_plan_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process).  It asserts
//   - the three layouts as literal segment lists at the smallest shapes where an offset can be wrong, unit and strided;
//   - over a sweep of sizes and strides: the plain sides split G and H exactly, the deferred sides split their four quarters, the
//     counts add up, and a strided plan is the unit plan with every index i mapped to first + i * stride;
//   - the policy of each route, and the gather length.
// The last line of stdout is "ipa_plan selftest ok"; a failed check is reported on stderr and the exit status is 1.
#include <cstdio>
#include <vector>
#include "ipa_plan.hpp"

using namespace arkbp;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed++; fprintf(stderr, "ipa_plan selftest: %s failed (%s:%d): ", #cond, __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const int G = IPA_G, H = IPA_H;
struct WantSeg { int table; size_t first, count, stride; int half; };
static const WantSeg Q = {IPA_Q, 0, 1, 1, 0};
struct Want { const char* name; IpaShape sh; size_t terms; std::vector<WantSeg> L, R; };

// working element 0 at G[3] and H[7], unit stride; then rank 1 of an index-cyclic world of 2 (first = 1, stride = 2)
static const Want WANT[] = {
    {"plain n=1", {IPA_PLAIN, 1, 0, 0, 3, 7, 1}, 3, {{G, 4, 1, 1, 0}, {H, 7, 1, 1, 0}, Q}, {{G, 3, 1, 1, 0}, {H, 8, 1, 1, 0}, Q}},
    {"plain n=2", {IPA_PLAIN, 2, 0, 0, 3, 7, 1}, 5, {{G, 5, 2, 1, 0}, {H, 7, 2, 1, 0}, Q}, {{G, 3, 2, 1, 0}, {H, 9, 2, 1, 0}, Q}},
    {"deferred n=1", {IPA_DEFERRED, 1, 2, 0, 3, 7, 1}, 5,
     {{G, 6, 1, 1, 0}, {G, 4, 1, 1, 0}, {H, 9, 1, 1, 0}, {H, 7, 1, 1, 0}, Q}, {{G, 5, 1, 1, 0}, {G, 3, 1, 1, 0}, {H, 10, 1, 1, 0}, {H, 8, 1, 1, 0}, Q}},
    {"deferred n=2", {IPA_DEFERRED, 2, 4, 0, 3, 7, 1}, 9,
     {{G, 9, 2, 1, 0}, {G, 5, 2, 1, 0}, {H, 11, 2, 1, 0}, {H, 7, 2, 1, 0}, Q}, {{G, 7, 2, 1, 0}, {G, 3, 2, 1, 0}, {H, 13, 2, 1, 0}, {H, 9, 2, 1, 0}, Q}},
    {"frozen n0=2", {IPA_FROZEN, 1, 0, 2, 3, 7, 1}, 5, {{G, 3, 2, 1, 1}, {H, 7, 2, 1, 0}, Q}, {{G, 3, 2, 1, 0}, {H, 7, 2, 1, 1}, Q}},
    {"frozen n0=4", {IPA_FROZEN, 2, 0, 4, 3, 7, 1}, 9, {{G, 3, 4, 1, 1}, {H, 7, 4, 1, 0}, Q}, {{G, 3, 4, 1, 0}, {H, 7, 4, 1, 1}, Q}},
    {"frozen n0=4, last round", {IPA_FROZEN, 1, 0, 4, 3, 7, 1}, 9, {{G, 3, 4, 1, 1}, {H, 7, 4, 1, 0}, Q}, {{G, 3, 4, 1, 0}, {H, 7, 4, 1, 1}, Q}},
    {"plain n=1 strided", {IPA_PLAIN, 1, 0, 0, 1, 1, 2}, 3, {{G, 3, 1, 2, 0}, {H, 1, 1, 2, 0}, Q}, {{G, 1, 1, 2, 0}, {H, 3, 1, 2, 0}, Q}},
    {"plain n=2 strided", {IPA_PLAIN, 2, 0, 0, 1, 1, 2}, 5, {{G, 5, 2, 2, 0}, {H, 1, 2, 2, 0}, Q}, {{G, 1, 2, 2, 0}, {H, 5, 2, 2, 0}, Q}},
    {"deferred n=1 strided", {IPA_DEFERRED, 1, 2, 0, 1, 1, 2}, 5,
     {{G, 7, 1, 2, 0}, {G, 3, 1, 2, 0}, {H, 5, 1, 2, 0}, {H, 1, 1, 2, 0}, Q}, {{G, 5, 1, 2, 0}, {G, 1, 1, 2, 0}, {H, 7, 1, 2, 0}, {H, 3, 1, 2, 0}, Q}},
    {"deferred n=2 strided", {IPA_DEFERRED, 2, 4, 0, 1, 1, 2}, 9,
     {{G, 13, 2, 2, 0}, {G, 5, 2, 2, 0}, {H, 9, 2, 2, 0}, {H, 1, 2, 2, 0}, Q}, {{G, 9, 2, 2, 0}, {G, 1, 2, 2, 0}, {H, 13, 2, 2, 0}, {H, 5, 2, 2, 0}, Q}},
    {"frozen n0=2 strided", {IPA_FROZEN, 1, 0, 2, 1, 1, 2}, 5, {{G, 1, 2, 2, 1}, {H, 1, 2, 2, 0}, Q}, {{G, 1, 2, 2, 0}, {H, 1, 2, 2, 1}, Q}},
    {"frozen n0=4 strided", {IPA_FROZEN, 2, 0, 4, 1, 1, 2}, 9, {{G, 1, 4, 2, 1}, {H, 1, 4, 2, 0}, Q}, {{G, 1, 4, 2, 0}, {H, 1, 4, 2, 1}, Q}},
};

static void check_literal() {
    for (const Want& w : WANT) {
        const IpaPlan p = ipa_plan(w.sh);
        for (int o = 0; o < 2; o++) {
            const IpaSide& sd = p.side[o];
            const std::vector<WantSeg>& want = o ? w.R : w.L;
            CHECK(sd.nseg == (int)want.size(), "%s side %d: %d segments", w.name, o, sd.nseg);
            CHECK(sd.terms == w.terms && sd.ip_slot == w.terms - 1, "%s side %d: terms %zu, inner product in slot %zu", w.name, o, sd.terms, sd.ip_slot);
            for (int k = 0; k < sd.nseg && k < (int)want.size(); k++) {
                const IpaSeg& s = sd.seg[k];
                const WantSeg& e = want[k];
                CHECK(s.table == e.table && s.first == e.first && s.count == e.count && s.stride == e.stride && s.half == e.half,
                      "%s side %d segment %d: {%d, %zu, %zu, %zu, %d}, expected {%d, %zu, %zu, %zu, %d}", w.name, o, k, s.table, s.first, s.count, s.stride, s.half, e.table,
                      e.first, e.count, e.stride, e.half);
            }
        }
    }
}

// marks the WORKING indices (table index = first + i * stride) a side's segments of `table` cover; uses[i] counts them
static void cover(const IpaSide& sd, int table, size_t first, size_t stride, std::vector<int>& uses, const char* what) {
    for (int k = 0; k < sd.nseg; k++) {
        const IpaSeg& s = sd.seg[k];
        if (s.table != table) continue;
        CHECK(s.stride == stride && s.first >= first && (s.first - first) % stride == 0, "%s: segment %d starts at %zu with stride %zu", what, k, s.first, s.stride);
        const size_t i0 = (s.first - first) / stride;
        CHECK(i0 + s.count <= uses.size(), "%s: segment %d ends at working element %zu of %zu", what, k, i0 + s.count, uses.size());
        for (size_t i = i0; i < i0 + s.count && i < uses.size(); i++) uses[i]++;
    }
}
static void check_common(const IpaPlan& p, const IpaShape& sh, const char* what) {
    const IpaPlan unit = ipa_plan(sh.compact());
    for (int o = 0; o < 2; o++) {
        const IpaSide &sd = p.side[o], &un = unit.side[o];
        size_t sum = 0;
        for (int k = 0; k < sd.nseg; k++) sum += sd.seg[k].count;
        CHECK(sd.terms == sum && sd.ip_slot == sum - 1, "%s side %d: terms %zu, counts add up to %zu", what, o, sd.terms, sum);
        CHECK(sd.nseg >= 1 && sd.nseg <= IPA_MAXSEG && sd.seg[sd.nseg - 1].table == IPA_Q && sd.seg[sd.nseg - 1].count == 1, "%s side %d: Q is not the last term", what, o);
        CHECK(sd.nseg == un.nseg && sd.terms == un.terms, "%s side %d: strided and unit plan differ in shape", what, o);
        for (int k = 0; k < sd.nseg && k < un.nseg; k++) {
            const IpaSeg &s = sd.seg[k], &u = un.seg[k];
            if (s.table == IPA_Q) { CHECK(u.table == IPA_Q && s.first == 0 && s.stride == 1, "%s side %d: Q", what, o); continue; }
            const size_t first = s.table == IPA_G ? sh.g_first : sh.h_first;
            CHECK(s.table == u.table && s.count == u.count && s.half == u.half && s.stride == sh.stride && u.stride == 1 && s.first == first + u.first * sh.stride,
                  "%s side %d segment %d: first %zu, the unit plan's %zu", what, o, k, s.first, u.first);
        }
    }
}

static void check_sweep() {
    static const size_t STRIDES[] = {1, 2, 4, 8};
    for (int lg = 0; lg <= 12; lg++)
        for (size_t stride : STRIDES)
            for (size_t rank = 0; rank < stride; rank += (stride > 2 ? stride - 1 : 1)) {
                const size_t n = (size_t)1 << lg;
                char what[96];
                // plain: the G segments of L and of R are disjoint and together the 2n working elements; likewise H
                const IpaShape pl = {IPA_PLAIN, n, 0, 0, rank + 5 * (stride == 1), rank + 11 * (stride == 1), stride};
                snprintf(what, sizeof what, "plain n=%zu stride=%zu first=%zu", n, stride, pl.g_first);
                const IpaPlan pp = ipa_plan(pl);
                check_common(pp, pl, what);
                for (int table = 0; table < 2; table++) {
                    std::vector<int> uses(2 * n, 0), one(2 * n, 0);
                    for (int o = 0; o < 2; o++) {
                        cover(pp.side[o], table, table == IPA_G ? pl.g_first : pl.h_first, stride, uses, what);
                        if (o == 0) one = uses;
                    }
                    size_t bad = 0, left = 0;
                    for (size_t i = 0; i < 2 * n; i++) { bad += uses[i] != 1; left += one[i]; }
                    CHECK(bad == 0 && left == n, "%s table %d: %zu elements not used exactly once, L takes %zu", what, table, bad, left);
                }
                CHECK(pp.side[0].terms == 2 * n + 1 && pp.side[1].terms == 2 * n + 1, "%s: terms", what);
                // deferred: each side takes two whole quarters of G and two of H, in descending order; L and R together take every quarter once
                const IpaShape df = {IPA_DEFERRED, n, 2 * n, 0, pl.g_first, pl.h_first, stride};
                snprintf(what, sizeof what, "deferred n=%zu stride=%zu first=%zu", n, stride, df.g_first);
                const IpaPlan dp = ipa_plan(df);
                check_common(dp, df, what);
                for (int table = 0; table < 2; table++) {
                    std::vector<int> uses(4 * n, 0);
                    const size_t first = table == IPA_G ? df.g_first : df.h_first;
                    for (int o = 0; o < 2; o++) {
                        cover(dp.side[o], table, first, stride, uses, what);
                        size_t quarters = 0, last = 4;
                        for (int k = 0; k < dp.side[o].nseg; k++) {
                            const IpaSeg& s = dp.side[o].seg[k];
                            if (s.table != table) continue;
                            const size_t i0 = (s.first - first) / stride;
                            CHECK(s.count == n && i0 % n == 0 && i0 / n < last, "%s side %d segment %d: not a quarter in descending order", what, o, k);
                            last = i0 / n; quarters++;
                        }
                        CHECK(quarters == 2, "%s side %d table %d: %zu quarters", what, o, table, quarters);
                    }
                    size_t bad = 0;
                    for (size_t i = 0; i < 4 * n; i++) bad += uses[i] != 1;
                    CHECK(bad == 0, "%s table %d: %zu elements not used exactly once", what, table, bad);
                }
                CHECK(dp.side[0].terms == 4 * n + 1 && dp.side[1].terms == 4 * n + 1, "%s: terms", what);
                // frozen at n0 = 2n: both sides over all of G and H, opposite halves of the periods
                const IpaShape fz = {IPA_FROZEN, n, 0, 2 * n, pl.g_first, pl.h_first, stride};
                snprintf(what, sizeof what, "frozen n0=%zu stride=%zu first=%zu", 2 * n, stride, fz.g_first);
                const IpaPlan fp = ipa_plan(fz);
                check_common(fp, fz, what);
                for (int o = 0; o < 2; o++) {
                    const IpaSide& sd = fp.side[o];
                    CHECK(sd.nseg == 3 && sd.terms == 4 * n + 1 && sd.seg[0].table == IPA_G && sd.seg[1].table == IPA_H && sd.seg[0].count == 2 * n && sd.seg[1].count == 2 * n &&
                              sd.seg[0].first == fz.g_first && sd.seg[1].first == fz.h_first && sd.seg[0].half == 1 - o && sd.seg[1].half == o,
                          "%s side %d", what, o);
                }
            }
}

static bool is(const IpaPolicy& p, IpaRows rows, IpaFallback fb) { return p.rows == rows && p.fallback == fb; }
static void check_policy() {
    //                         frozen direct deferred first tables have_qw fb_rows mode stride
    CHECK(is(ipa_policy({true, true, false, true, false, true, true, -1, 1}), IPA_ROWS_NONE, IPA_FB_DIRECT), "direct");
    CHECK(is(ipa_policy({true, false, false, false, false, true, true, -1, 1}), IPA_ROWS_NONE, IPA_FB_PAIR), "frozen");
    CHECK(is(ipa_policy({true, false, false, false, false, false, false, 0, 1}), IPA_ROWS_NONE, IPA_FB_PAIR), "frozen, replicated tail");
    CHECK(is(ipa_policy({false, false, true, false, true, true, true, 2, 4}), IPA_ROWS_EACH, IPA_FB_SIDE), "deferred, index-cyclic");
    CHECK(is(ipa_policy({false, false, true, false, true, true, false, 2, 4}), IPA_ROWS_NONE, IPA_FB_SIDE), "deferred, index-cyclic, no rows");
    CHECK(is(ipa_policy({false, false, true, false, true, false, true, 2, 4}), IPA_ROWS_NONE, IPA_FB_SIDE), "deferred, index-cyclic, any Q");
    CHECK(is(ipa_policy({false, false, true, false, true, true, true, -1, 1}), IPA_ROWS_L_THEN_R, IPA_FB_TWO), "deferred, single rank");
    CHECK(is(ipa_policy({false, false, true, false, true, false, true, -1, 1}), IPA_ROWS_NONE, IPA_FB_TWO), "deferred, single rank, any Q");
    CHECK(is(ipa_policy({false, false, true, false, true, true, true, 0, 1}), IPA_ROWS_NONE, IPA_FB_TWO), "deferred, replicated");
    CHECK(is(ipa_policy({false, false, false, true, true, true, true, -1, 1}), IPA_ROWS_L_THEN_R, IPA_FB_PAIR), "round 1 over the resident tables");
    CHECK(is(ipa_policy({false, false, false, true, true, true, false, -1, 1}), IPA_ROWS_L_THEN_R, IPA_FB_PAIR), "round 1 over the resident tables: the rows decline themselves");
    CHECK(is(ipa_policy({false, false, false, true, true, false, true, -1, 1}), IPA_ROWS_NONE, IPA_FB_PAIR), "round 1 over the resident tables, any Q");
    CHECK(is(ipa_policy({false, false, false, true, true, true, true, 2, 4}), IPA_ROWS_EACH, IPA_FB_SIDE), "round 1, index-cyclic");
    CHECK(is(ipa_policy({false, false, false, false, false, true, true, 2, 4}), IPA_ROWS_NONE, IPA_FB_PAIR), "later rounds, index-cyclic");
    CHECK(is(ipa_policy({false, false, false, true, true, true, false, 2, 4}), IPA_ROWS_NONE, IPA_FB_PAIR), "round 1, index-cyclic, no rows");
    CHECK(is(ipa_policy({false, false, false, true, true, true, true, 2, 1}), IPA_ROWS_NONE, IPA_FB_PAIR), "round 1, a world of one");
    CHECK(is(ipa_policy({false, false, false, true, false, false, false, -1, 0}), IPA_ROWS_NONE, IPA_FB_PAIR), "the plain pair");
    CHECK(is(ipa_policy({false, false, false, false, false, true, true, -1, 1}), IPA_ROWS_NONE, IPA_FB_PAIR), "the plain pair, later rounds");
}

static void check_gather_len() {
    static const size_t FREEZE[] = {0, 1, 2, 3, 4, 5, 255, 256, 257, 1000, 8192, 8193, 16384, 100000};
    for (size_t fz : FREEZE)
        for (size_t world = 1; world <= 64; world++) {
            const size_t g = ipa_gather_len(fz, world), least = std::max<size_t>(std::max(fz, world), 2);
            CHECK(g && !(g & (g - 1)) && g >= least && g < 2 * least, "gather length %zu for freeze length %zu, world %zu", g, fz, world);
        }
}

int main() {
    check_literal();
    check_sweep();
    check_policy();
    check_gather_len();
    if (g_failed) { fprintf(stderr, "ipa_plan selftest: %d checks failed\n", g_failed); return 1; }
    puts("ipa_plan selftest ok");
    return 0;
}
