// Stand-alone check of csrc/vfy_dev_plan.hpp (its own main; tests/test_vfy_dev_plan_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process).  It asserts
//   - literal placements, worked out by hand from the formulas the device front end had inline before the header existed: one small
//     job, the shape of the verify benchmark (4096 like-instances, k = 14, m = 256), and a call of three jobs of different k, one on
//     the wire and one crossing a block, where every job's place is the totals of the jobs before it;
//   - over a sweep of shapes: the staging parts are 256-byte aligned, hold what is written to them, do not overlap and sum to b_in;
//     in calls of up to BP_VFY_MAX_CLASSES jobs no two jobs overlap in any buffer, the flag words lie between the inputs and the small
//     area, every h_small and vfe_small field lies inside its 4096 bytes, and the sizes reserved cover the last element of each job;
//   - every decline reason from the value just inside and the value just outside its rule, and vfy_dev_fits at both of its bounds.
// The last line of stdout is "vfy_dev_plan selftest ok"; a failed check is reported on stderr and the exit status is 1.
#include <cstdio>
#include <vector>
#include "vfy_dev_plan.hpp"

using namespace arkbp;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed++; fprintf(stderr, "vfy_dev_plan selftest: %s failed (%s:%d): ", #cond, __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const size_t PB = 832;   // words per parameter block as the caller passes them in (any value serves here)
static size_t plen_of(size_t k) { return 539 + 66 * k; }

static VfyDevShape shape(size_t count, size_t k, size_t m, bool absorb, bool wire, bool shared, size_t G = 0, size_t ncoef = 0) {
    VfyDevShape s;
    const VfyDevDecline d = vfy_dev_shape(s, plen_of(k), count, m, absorb, wire, shared);
    CHECK(d == VFY_DEV_OK, "count=%zu k=%zu m=%zu: decline %d", count, k, m, (int)d);
    CHECK(vfy_dev_set_N(s, (size_t)1 << k) == VFY_DEV_OK, "k=%zu", k);
    CHECK(vfy_dev_set_tables(s, G, ncoef) == VFY_DEV_OK, "G=%zu ncoef=%zu", G, ncoef);
    return s;
}
static bool same(const VfyDevPlace& a, const VfyDevPlace& b) {
    return a.in == b.in && a.msg == b.msg && a.chal == b.chal && a.ws == b.ws && a.inst == b.inst && a.tail == b.tail && a.blk == b.blk && a.cls == b.cls;
}
static VfyDevPlace mk(size_t in, size_t msg, size_t chal, size_t ws, size_t inst, size_t tail, size_t blk, size_t cls) {
    VfyDevPlace p; p.in = in; p.msg = msg; p.chal = chal; p.ws = ws; p.inst = inst; p.tail = tail; p.blk = blk; p.cls = cls; return p;
}
static bool totals_are(const VfyDevTotals& t, const VfyDevPlace& sum, size_t Nmax) {
    return t.b_in == sum.in && t.msg == sum.msg && t.chal == sum.chal && t.ws == sum.ws && t.inst == sum.inst && t.tail == sum.tail && t.blocks == sum.blk &&
           t.classes == sum.cls && t.Nmax == Nmax;
}

static void literals() {
    VfyDevPlace pl[3];
    VfyDevTotals tot;
    {   // count = 3, plen = 803 (k = 4), m = 2 affine commitments absorbed, a state per instance
        const VfyDevShape s = shape(3, 4, 2, true, false, false);
        CHECK(s.plen == 803 && s.k == 4 && s.tail == 21 && s.nV == 2 && s.vbytes == 64 && s.nitems == 24 && s.nblocks == 1, "k=%zu tail=%zu nitems=%zu", s.k, s.tail, s.nitems);
        CHECK(s.b_proofs == 2560 && s.b_V == 512 && s.b_st == 768 && s.b_in == 4096, "%zu %zu %zu %zu", s.b_proofs, s.b_V, s.b_st, s.b_in);
        CHECK(s.o_V() == 2560 && s.o_st() == 3072 && s.o_alpha() == 3840 && s.b_in - s.o_alpha() == 256, "offsets");
        vfy_dev_place(&s, 1, pl, tot);
        CHECK(same(pl[0], VfyDevPlace()), "the first job starts every buffer");
        CHECK(totals_are(tot, mk(4096, 648, 30, 102, 3, 63, 1, 1), 16), "msg=%zu chal=%zu ws=%zu tail=%zu", tot.msg, tot.chal, tot.ws, tot.tail);
        const VfyDevSizes z = vfy_dev_sizes(tot, PB);
        CHECK(z.stage == 4096 + 256 && z.in == 4096 && z.msg == 5184 && z.chal == 960 && z.ws == 3264 && z.small == 4096 && z.flags == 12, "sizes");
        CHECK(z.r_g == (2 + 32 + 63) * 32 && z.r_tail == 63 * 64 && z.r_small == 9 * 32 && z.alpha == 96 && z.params == 3 * PB * 4, "sizes");
        CHECK(z.z_rg == 34 * 32 && z.z_small == 256 && z.z_flags == 12, "zeroing");
    }
    {   // the verify benchmark: 4096 like-instances, k = 14, m = 256 affine commitments absorbed, one shared state
        const VfyDevShape s = shape(4096, 14, 256, true, false, true);
        CHECK(s.plen == 1463 && s.tail == 295 && s.nitems == 298 && s.nblocks == 8, "tail=%zu nitems=%zu", s.tail, s.nitems);
        CHECK(s.b_proofs == 5992448 && s.b_V == 67108864 && s.b_st == 256 && s.b_in == 73232640, "%zu %zu %zu %zu", s.b_proofs, s.b_V, s.b_st, s.b_in);
        vfy_dev_place(&s, 1, pl, tot);
        CHECK(totals_are(tot, mk(73232640, 10985472, 81920, 139264, 4096, 1208320, 8, 1), 16384), "msg=%zu chal=%zu tail=%zu", tot.msg, tot.chal, tot.tail);
        CHECK(vfy_rg_h(tot.Nmax) == 16386 && vfy_rg_tails(tot.Nmax) == 32770 && vfy_rg_len(tot.Nmax, tot.tail) == 1241090, "r_g");
    }
    {   // three jobs: 513 instances of k = 3 (two blocks), 5 of k = 0 on the wire with a shared state, 2 of k = 5 with 3 gadget challenges
        const VfyDevShape s[3] = {shape(513, 3, 1, true, false, false), shape(5, 0, 3, true, true, true), shape(2, 5, 0, false, false, false, 3, 7)};
        CHECK(s[0].nblocks == 2 && s[0].tail == 18 && s[0].nitems == 21 && s[0].b_proofs == 378112 && s[0].b_V == 33024 && s[0].b_st == 102656 && s[0].b_in == 530432, "job 0");
        CHECK(s[1].vbytes == 33 && s[1].tail == 14 && s[1].nitems == 17 && s[1].b_proofs == 2816 && s[1].b_V == 512 && s[1].b_st == 256 && s[1].b_in == 3840, "job 1");
        CHECK(s[2].nV == 0 && s[2].tail == 21 && s[2].nitems == 24 && s[2].b_proofs == 1792 && s[2].b_V == 0 && s[2].b_st == 512 && s[2].b_in == 2560, "job 2");
        CHECK(s[2].gch() == 6 && s[2].tab() == 14, "two-phase tables");
        vfy_dev_place(s, 3, pl, tot);
        CHECK(same(pl[0], VfyDevPlace()), "job 0");
        CHECK(same(pl[1], mk(530432, 96957, 4617, 17442, 513, 9234, 2, 1)), "job 1: in=%zu msg=%zu chal=%zu ws=%zu", pl[1].in, pl[1].msg, pl[1].chal, pl[1].ws);
        CHECK(same(pl[2], mk(534272, 97722, 4647, 17612, 518, 9304, 3, 2)), "job 2: in=%zu msg=%zu chal=%zu ws=%zu", pl[2].in, pl[2].msg, pl[2].chal, pl[2].ws);
        CHECK(totals_are(tot, mk(536832, 98154, 4675, 17680, 520, 9346, 4, 3), 32), "totals: in=%zu msg=%zu chal=%zu", tot.b_in, tot.msg, tot.chal);
        VfyDevTotals run;   // every job's place equals the totals of the jobs before it
        for (int c = 0; c < 3; c++) {
            CHECK(totals_are(run, pl[c], run.Nmax), "job %d", c);
            (void)vfy_dev_append(run, s[c]);
        }
    }
}

static void check_parts(const VfyDevShape& s) {
    const size_t part[4] = {s.b_proofs, s.b_V, s.b_st, s.b_in - s.o_alpha()}, at[4] = {0, s.o_V(), s.o_st(), s.o_alpha()};
    const size_t used[4] = {s.count * s.plen, s.count * s.m * s.vbytes, (s.shared_state ? 1 : s.count) * 200, s.count * 32};
    size_t end = 0;
    for (int i = 0; i < 4; i++) {
        CHECK(part[i] % 256 == 0 && at[i] % 256 == 0, "part %d of count=%zu k=%zu m=%zu", i, s.count, s.k, s.m);
        CHECK(at[i] == end && used[i] <= part[i] && part[i] < used[i] + 256, "part %d of count=%zu k=%zu m=%zu", i, s.count, s.k, s.m);   // disjoint, in order, no slack but the alignment's
        end = at[i] + part[i];
    }
    CHECK(end == s.b_in, "count=%zu k=%zu m=%zu", s.count, s.k, s.m);
}
// one call: jobs side by side in every buffer, inside what vfy_dev_sizes reserves
static void check_call(const VfyDevShape* s, size_t nj) {
    VfyDevPlace pl[BP_VFY_MAX_CLASSES];
    VfyDevTotals tot;
    vfy_dev_place(s, nj, pl, tot);
    const VfyDevSizes z = vfy_dev_sizes(tot, PB);
    VfyDevPlace end;   // where the job before ended: ranges are disjoint when each job starts at or after it
    for (size_t c = 0; c < nj; c++) {
        const VfyDevPlace e = vfy_dev_extent(s[c]), &p = pl[c];
        CHECK(p.in >= end.in && p.msg >= end.msg && p.chal >= end.chal && p.ws >= end.ws && p.inst >= end.inst && p.tail >= end.tail && p.blk >= end.blk && p.cls >= end.cls, "job %zu of %zu", c, nj);
        end = mk(p.in + e.in, p.msg + e.msg, p.chal + e.chal, p.ws + e.ws, p.inst + e.inst, p.tail + e.tail, p.blk + e.blk, p.cls + e.cls);
        CHECK(p.in % 256 == 0 && end.in <= z.in && end.in <= vfy_dev_flags_at(tot), "staging of job %zu", c);
        CHECK(end.msg * 8 <= z.msg && end.chal * 32 <= z.chal && end.ws * 32 <= z.ws, "msg / chal / ws of job %zu", c);
        CHECK(e.msg == s[c].nitems * vfe::ITEM_WORDS * s[c].count && e.chal == s[c].count * (6 + s[c].k + s[c].G) && e.ws >= s[c].count * 32, "extent of job %zu", c);
        CHECK(end.inst * 4 <= z.flags && end.inst * 32 <= z.alpha && end.inst * PB * 4 <= z.params, "per-instance arrays of job %zu", c);
        CHECK((vfy_rg_tails(tot.Nmax) + end.tail) * 32 <= z.r_g && end.tail * 64 <= z.r_tail && e.tail == s[c].count * s[c].tail, "tails of job %zu", c);
        CHECK(end.blk * 32 <= z.r_small && end.blk * 32 <= VFY_HS_SUMS, "block slots of job %zu", c);
        CHECK((VFY_DS_SUMS + VFY_DS_JOB * end.cls) * 4 <= z.small && VFY_HS_SUMS + 64 * end.cls <= VFY_HS_STATUS, "sums of job %zu", c);
        CHECK(s[c].N <= tot.Nmax && VFY_RG_G + s[c].N <= vfy_rg_h(tot.Nmax) && vfy_rg_h(tot.Nmax) + s[c].N <= vfy_rg_tails(tot.Nmax), "accumulators of job %zu", c);
    }
    // the flag words start at tot.b_in and end before the small area, which starts no earlier than z.stage
    CHECK(vfy_dev_flags_at(tot) == tot.b_in && vfy_dev_flags_at(tot) + tot.inst * 4 <= z.stage && z.stage % 256 == 0, "flags");
    CHECK(VFY_HS_STATUS + 4 <= VFY_SMALL_BYTES && VFY_HS_SUMS < VFY_HS_STATUS && z.small == VFY_SMALL_BYTES && z.z_small <= VFY_DS_SUMS * 4, "small areas");
    CHECK(z.z_rg == vfy_rg_tails(tot.Nmax) * 32 && z.z_rg <= z.r_g && z.z_flags <= z.flags && z.z_flags >= tot.inst * 4, "zeroing");
    // vfy_dev_fits weighs each job's own N against the tails before it, so the call's terms stay below twice the bound: far inside 32 bits
    CHECK(vfy_rg_len(tot.Nmax, tot.tail) < 2 * VFY_TAIL_BOUND && tot.blocks <= VFY_SLOTS && tot.classes == nj, "what vfy_dev_fits promised");
}
static void sweep() {
    static const size_t counts[] = {1, 2, 511, 512, 513, 65535}, ms[] = {0, 1, 255, 65535};
    std::vector<VfyDevShape> ok;
    size_t declined = 0;
    for (size_t count : counts) for (size_t k = 0; k < 32; k++) for (size_t m : ms) for (int form = 0; form < 3; form++) for (int shared = 0; shared < 2; shared++) for (size_t G : {0, 3}) {
        const bool wire = form == 2, absorb = form != 0;   // affine in the transcripts already, affine absorbed, wire absorbed
        VfyDevShape s;
        const VfyDevDecline d = vfy_dev_shape(s, plen_of(k), count, m, absorb, wire, shared != 0);
        // the largest shapes run into the 2^31 / 2^32 limits, and only they
        if (d) { CHECK((d == VFY_DEV_TAILS || d == VFY_DEV_ITEMS || d == VFY_DEV_SLOTS) && count == 65535, "count=%zu k=%zu m=%zu: %d", count, k, m, (int)d); declined++; continue; }
        CHECK(!vfy_dev_set_N(s, (size_t)1 << k) && !vfy_dev_set_tables(s, G, G ? 5 : 0), "count=%zu k=%zu", count, k);
        check_parts(s);
        ok.push_back(s);
    }
    CHECK(ok.size() > 4000 && declined > 0, "%zu admitted, %zu declined", ok.size(), declined);
    // calls of 1 .. BP_VFY_MAX_CLASSES jobs drawn from all over the sweep, each taken while vfy_dev_fits says so (as batch_verify_classes does)
    size_t calls = 0, widest = 0;
    for (size_t g = 0; g < ok.size(); g++) {
        VfyDevShape call[BP_VFY_MAX_CLASSES];
        VfyDevTotals fit;
        size_t nj = 0;
        for (size_t j = 0; j < 1 + g % BP_VFY_MAX_CLASSES; j++) {
            const VfyDevShape& s = ok[(g + j * 2654435761u) % ok.size()];
            if (!vfy_dev_fits(fit, s)) continue;
            (void)vfy_dev_append(fit, s);
            call[nj++] = s;
        }
        if (nj) { check_call(call, nj); calls++; widest = std::max(widest, nj); }
    }
    CHECK(calls > 4000 && widest == BP_VFY_MAX_CLASSES, "%zu calls, %zu jobs at most", calls, widest);
}

static VfyDevDecline decl(size_t plen, size_t count, size_t m, bool absorb, bool wire) { VfyDevShape s; return vfy_dev_shape(s, plen, count, m, absorb, wire, true); }
static void declines() {
    // framing: 539 + 66 k exactly
    CHECK(decl(538, 1, 0, false, false) == VFY_DEV_FRAMING && decl(539, 1, 0, false, false) == VFY_DEV_OK && decl(540, 1, 0, false, false) == VFY_DEV_FRAMING, "framing");
    CHECK(decl(604, 1, 0, false, false) == VFY_DEV_FRAMING && decl(605, 1, 0, false, false) == VFY_DEV_OK && decl(0, 1, 0, false, false) == VFY_DEV_FRAMING, "framing");
    CHECK(decl(plen_of(31), 1, 0, false, false) == VFY_DEV_OK && decl(plen_of(32), 1, 0, false, false) == VFY_DEV_ROUNDS, "k < 32");
    CHECK(decl(539, 1, 1, true, true) == VFY_DEV_OK && decl(539, 1, 1, false, true) == VFY_DEV_WIRE, "wire commitments are absorbed on the device");
    CHECK(decl(539, 1, 65535, false, false) == VFY_DEV_OK && decl(539, 1, 65536, false, false) == VFY_DEV_M, "m");
    CHECK(decl(539, 65535, 0, false, false) == VFY_DEV_SLOTS && decl(539, 65536, 0, false, false) == VFY_DEV_COUNT, "count");   // (inside: a later rule's)
    // count * tail < 2^31: 65535 * 32768 is below, 65535 * 32769 is not (tail = 11 + m at k = 0)
    CHECK(decl(539, 65535, 32757, false, false) == VFY_DEV_SLOTS && decl(539, 65535, 32758, false, false) == VFY_DEV_TAILS, "count * tail");   // (inside: the next rule's)
    CHECK(decl(539, 32768, 65535 - 11, false, false) == VFY_DEV_OK && decl(539, 32768, 65536 - 11, false, false) == VFY_DEV_TAILS, "count * tail");
    // nitems * ITEM_WORDS * count < 2^32 (nitems = m + 14 at k = 0 with the commitments absorbed)
    {
        const size_t count = 49152, lim = (((size_t)1 << 32) + vfe::ITEM_WORDS * count - 1) / (vfe::ITEM_WORDS * count);   // the first nitems that is too many
        CHECK(decl(539, count, lim - 1 - 14, true, false) == VFY_DEV_OK && decl(539, count, lim - 14, true, false) == VFY_DEV_ITEMS, "items: %zu", lim);
    }
    CHECK(decl(539, VFY_SLOTS * VFY_BLOCK, 0, false, false) == VFY_DEV_OK && decl(539, VFY_SLOTS * VFY_BLOCK + 1, 0, false, false) == VFY_DEV_SLOTS, "one slot per block");
    VfyDevShape s;
    CHECK(vfy_dev_shape(s, plen_of(3), 4096, 1, true, false, true) == VFY_DEV_OK, "k = 3");
    CHECK(vfy_dev_set_N(s, 8) == VFY_DEV_OK && vfy_dev_set_N(s, 4) == VFY_DEV_N && vfy_dev_set_N(s, 16) == VFY_DEV_N && vfy_dev_set_N(s, 0) == VFY_DEV_N, "N = 2^k");
    // 4096 * 2048 scalars are the budget exactly
    CHECK(VFY2_TABLE_BUDGET == (size_t)4096 * 2048 * 32, "the budget");
    CHECK(vfy_dev_set_tables(s, 48, 2000) == VFY_DEV_OK && vfy_dev_set_tables(s, 49, 2000) == VFY_DEV_TABLES && vfy_dev_set_tables(s, 0, 2049) == VFY_DEV_TABLES, "table budget");
    CHECK(s.G == 0 && s.ncoef == 2049 && s.gch() == 0 && s.tab() == (size_t)4096 * 2049, "the tables' sizes");
}
static void fits() {
    const VfyDevShape one = shape(512, 0, 0, false, false, true), two = shape(513, 0, 0, false, false, true);
    VfyDevTotals t;
    t.blocks = VFY_SLOTS - 1;
    CHECK(vfy_dev_fits(t, one) && !vfy_dev_fits(t, two), "VFY_SLOTS blocks exactly, and one more");
    t.blocks = VFY_SLOTS - 2;
    CHECK(vfy_dev_fits(t, two), "VFY_SLOTS blocks exactly");
    // the mega-check's terms: 2 heads, 2 N accumulators (N = 4), the tails so far and this job's 3 x 15
    const VfyDevShape s = shape(3, 2, 0, false, false, true);
    VfyDevTotals u;
    u.tail = VFY_TAIL_BOUND - 45 - 10 - 1;
    CHECK(s.tail == 15 && vfy_dev_fits(u, s), "one below the bound");
    u.tail++;
    CHECK(!vfy_dev_fits(u, s), "at the bound");
    VfyDevShape n0 = s;   // a job whose N is not known counts as N = 1
    n0.N = 0;
    u.tail = VFY_TAIL_BOUND - 45 - 4 - 1;
    CHECK(vfy_dev_fits(u, n0) && !vfy_dev_fits(u, s), "N = 0 counts as 1");
}

int main() {
    literals();
    sweep();
    declines();
    fits();
    if (g_failed) { fprintf(stderr, "vfy_dev_plan selftest: %d checks failed\n", g_failed); return 1; }
    puts("vfy_dev_plan selftest ok");
    return 0;
}
