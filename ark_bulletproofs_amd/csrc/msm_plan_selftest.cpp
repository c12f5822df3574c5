// Stand-alone check of csrc/msm_plan.hpp (its own main; tests/test_msm_plan_host.py builds it with the address and
// undefined-behaviour sanitizers and runs it as a child process).  For every case — route x scalar width x size x knob set — it
//   - prints the plan as one JSON record on stdout: the test compares them, field by field, with tests/golden/msm_plans.json, which
//     the planning code made before it moved into the header;
//   - asserts what the kernels rely on and no GPU test can see: LDS sizes, index widths, grid bounds, per-job strides.
// The last line of stdout is "msm_plan selftest ok"; a failed check is reported on stderr and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "msm_plan.hpp"

using namespace arkbp;

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_failed++; fprintf(stderr, "msm_plan selftest: %s failed (%s:%d): ", #cond, __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const size_t SIZES[] = {1, 255, 256, 257, 1000, 4095, 4096, 4097, 5000, 8192, 8193, (size_t)1 << 15, (size_t)1 << 16, ((size_t)1 << 16) + 1, ((size_t)1 << 17) + 1,
                               (size_t)1 << 20, ((size_t)1 << 20) + 1, 1245184, (size_t)3 << 19, ((size_t)3 << 19) + 1, (size_t)1 << 21, (size_t)1 << 22, ((size_t)1 << 22) + 1,
                               ((size_t)1 << 23) + 1, ((size_t)1 << 24) - 1, (size_t)1 << 24, ((size_t)1 << 27) - 1};
struct KnobSet { const char* name; bool quad; size_t chunk_cap, bin_min, glv_min; bool pair, glv; };   // pair / glv: also the J = 2 and the GLV records
static const KnobSet KNOBS[] = {
    {"defaults", false, 0, 64, 256, true, false},        {"latency", true, 0, 64, 256, true, true},          {"cap8", false, 8, 64, 256, false, false},
    {"latency_cap8", true, 8, 64, 256, false, true},     {"latency_cap64", true, 64, 64, 256, false, true},  {"binmin_2p30", false, 0, (size_t)1 << 30, 256, false, false},
    {"latency_binmin_2p30", true, 0, (size_t)1 << 30, 256, false, true},   {"latency_glvmin_2p40", true, 0, 64, (size_t)1 << 40, false, true},
};

// ---- the record format ----
static void put_list(std::string& s, const char* key, const std::vector<u64>& v) {
    s += ",\""; s += key; s += "\":[";
    for (size_t i = 0; i < v.size(); i++) { if (i) s += ","; s += std::to_string(v[i]); }
    s += "]";
}
static void put_num(std::string& s, const char* key, u64 v) { s += ",\""; s += key; s += "\":"; s += std::to_string(v); }
static void put_pl(std::string& s, const MsmPlan& pl) { put_list(s, "pl", {(u64)pl.c, (u64)pl.W, (u64)pl.NB, pl.B, pl.n, (u64)pl.w_lo, (u64)pl.w_hi}); }
static void put_bp(std::string& s, const BinPlan& bp) { put_list(s, "bp", {bp.LB, bp.NBIN, bp.cap, bp.wb, bp.tpt, bp.top_nb, bp.glv}); }
// glv_route < 0: not a GLV record.  A GLV record that does not fit holds the MsmPlan alone
static void print_fs(const char* route, const KnobSet& k, int bits, size_t n, int J, const FsShape& r, int glv_route) {
    std::string s = "{\"route\":\""; s += route; s += "\",\"knobs\":\""; s += k.name; s += "\"";
    put_num(s, "bits", (u64)bits); put_num(s, "n", n); put_num(s, "J", (u64)J); put_num(s, "fits", r.fits);
    if (glv_route >= 0) put_num(s, "glv_route", (u64)glv_route);
    put_pl(s, r.pl);
    if (r.pl.W <= MSM_MAXW && (glv_route < 0 || r.fits)) { put_num(s, "binned", r.binned); put_bp(s, r.bp); }
    if (r.fits) {
        std::vector<u64> b, c;
        for (int w = 0; w < r.pl.W; w++) { b.push_back(r.sp.base[w]); c.push_back(r.sp.cap[w]); }
        put_list(s, "sp_base", b); put_list(s, "sp_cap", c);
        put_list(s, "fp", {r.fp.nbins, r.fp.has_top, r.fp.top_bits, r.fp.max_chunks, r.fp.top_parts});
        put_num(s, "nslots", r.nslots); put_num(s, "maxch", r.maxch); put_num(s, "tc", r.tc); put_num(s, "tb", r.tb); put_num(s, "red_g", r.red_g); put_num(s, "chl_fs", r.chl_fs);
        put_list(s, "jb", {r.jb.canon, r.jb.hist, r.jb.bin_cur, r.jb.slots, r.jb.buckets, r.jb.binch, r.jb.part, r.jb.sums, r.jb.T, r.jb.over});
    }
    s += "}";
    puts(s.c_str());
}
static void print_fb(int bits, size_t n, const FbPlan& r) {
    std::string s = "{\"route\":\"fixed-base\",\"knobs\":\"defaults\"";
    put_num(s, "bits", (u64)bits); put_num(s, "n", n); put_num(s, "decline", (u64)r.decline);
    if (!r.decline) {
        put_pl(s, r.pl); put_bp(s, r.bp);
        put_num(s, "tbits", r.tbits); put_num(s, "wbits", r.wbits); put_num(s, "vbits", r.vbits); put_num(s, "nl", (u64)r.nl);
    }
    s += "}";
    puts(s.c_str());
}

// ---- what the kernels rely on ----
static const size_t LDS_BYTES = 64 * 1024;
// the two-level sort's plan, as k_msm_bin_partition and a bin sort with `sort_extra` words beside the counters and the region use it
static void check_bins(const MsmPlan& pl, const BinPlan& bp, size_t entries_per_window, u32 sort_extra, const char* what, size_t n) {
    CHECK(bp.NBIN >= 1 && ((size_t)bp.NBIN << bp.LB) == (size_t)pl.NB, "%s n=%zu: NBIN %u << LB %u is not NB %d", what, n, bp.NBIN, bp.LB, pl.NB);
    CHECK((((size_t)1 << bp.LB) + sort_extra + bp.cap) * 4 <= LDS_BYTES, "%s n=%zu: the bin sort's LDS", what, n);
    CHECK(bp.cap >= 1 && bp.cap <= entries_per_window, "%s n=%zu: cap %u", what, n, bp.cap);
    CHECK(bp.tpt >= 1 && bp.tpt <= 16, "%s n=%zu: tpt %u", what, n, bp.tpt);
    // k_msm_bin_partition counts (windows per launch) x NBIN bins, and the slot window's buckets in the first launch, in LDS
    const size_t wg = std::max<size_t>(1, 12288 / bp.NBIN);
    CHECK((std::min<size_t>(wg, bp.wb) * bp.NBIN + bp.top_nb) * 4 <= LDS_BYTES, "%s n=%zu: the partition's LDS counters", what, n);
}
static void check_fs(const FsShape& s, size_t n, int J, bool glv, const char* what) {
    const MsmPlan& pl = s.pl; const BinPlan& bp = s.bp; const FsPlan& fp = s.fp; const FsJobs& jb = s.jb;
    const size_t ne = glv ? 2 * n : n;
    CHECK(s.binned && pl.W >= 1 && pl.W <= MSM_MAXW && pl.B == (u32)pl.W * (u32)pl.NB && pl.n == n, "%s n=%zu: MsmPlan", what, n);
    CHECK(bp.glv == (glv ? 1u : 0u), "%s n=%zu: bp.glv", what, n);
    check_bins(pl, bp, ne, 8, what, n);   // (k_msm_bin_sort_fs: 8 words)
    // an entry word: term field | fine bucket (LB bits) | sign; the term field of a GLV plan is 2 * i + half
    CHECK((u64)ne << (bp.LB + 1) <= ((u64)1 << 32), "%s n=%zu: the entry word", what, n);
    CHECK(bp.wb >= 1 && (bp.wb == (u32)pl.W || bp.wb + 1 == (u32)pl.W), "%s n=%zu: wb %u of W %d", what, n, bp.wb, pl.W);
    CHECK(fp.has_top == (bp.wb < (u32)pl.W ? 1u : 0u) && fp.nbins == bp.wb * bp.NBIN + fp.has_top && fp.nbins <= MSM_FS_MAXBINS, "%s n=%zu: bins %u", what, n, fp.nbins);
    if (fp.has_top) {
        CHECK(bp.top_nb >= 1 && bp.top_nb + 1 <= MSM_FS_TOP_WORDS, "%s n=%zu: top_nb %u", what, n, bp.top_nb);
        CHECK(((u64)1 << fp.top_bits) > bp.top_nb && ((u64)1 << fp.top_bits) <= 2 * (u64)bp.top_nb, "%s n=%zu: top_bits %u for %u buckets", what, n, fp.top_bits, bp.top_nb);
        CHECK(s.sp.base[bp.wb] == (u64)bp.wb * bp.NBIN * bp.cap && s.sp.cap[bp.wb] >= 1, "%s n=%zu: the slot window starts behind the bin regions", what, n);
        CHECK(s.nslots == (size_t)s.sp.base[bp.wb] + (size_t)bp.top_nb * s.sp.cap[bp.wb], "%s n=%zu: nslots", what, n);
    } else {
        CHECK(fp.top_bits == 0 && s.nslots == (size_t)bp.wb * bp.NBIN * bp.cap, "%s n=%zu: no slot window", what, n);
    }
    CHECK(fp.top_parts >= 4 && fp.top_parts <= MSM_TOP_PARTS_MAX, "%s n=%zu: top_parts", what, n);
    CHECK(s.nslots < ((size_t)1 << 32) && s.maxch < ((size_t)1 << 31) && fp.max_chunks == s.maxch, "%s n=%zu: nslots %zu, maxch %zu", what, n, s.nslots, s.maxch);
    CHECK(s.chl_fs >= 8 && s.chl_fs <= 64, "%s n=%zu: chl_fs %u", what, n, s.chl_fs);
    // chunks: every bucket's entries in chunks of chl_fs -> at most entries / chl_fs + one per non-empty bucket
    const size_t nwin = (size_t)(pl.w_hi - pl.w_lo);
    CHECK(s.maxch >= ne * nwin / s.chl_fs + std::min<size_t>(ne * nwin, nwin * (size_t)pl.NB), "%s n=%zu: maxch", what, n);
    CHECK(s.red_g == 1 || s.red_g == 4, "%s n=%zu: red_g", what, n);
    CHECK(s.tc == (size_t)bp.wb * pl.c + (size_t)fp.top_bits * fp.top_parts && s.tb == s.tc * 96 + 64 && s.tb % 4 == 0, "%s n=%zu: tc, tb", what, n);
    // per-job strides (32-bit words) >= what one job touches
    CHECK(J >= 1 && J <= MSM_JOBS, "%s n=%zu: J", what, n);
    CHECK(jb.canon >= n * (glv ? (size_t)MSM_GLV_WORDS : 8), "%s n=%zu: jb.canon", what, n);
    CHECK(jb.hist >= pl.B && jb.buckets >= pl.B, "%s n=%zu: jb.hist, jb.buckets", what, n);
    CHECK(jb.bin_cur >= (size_t)pl.W * bp.NBIN, "%s n=%zu: jb.bin_cur", what, n);
    CHECK(jb.slots >= s.nslots, "%s n=%zu: jb.slots", what, n);
    CHECK(jb.binch >= (size_t)fp.nbins + 1, "%s n=%zu: jb.binch", what, n);
    CHECK(jb.part >= s.maxch * 24, "%s n=%zu: jb.part", what, n);
    CHECK(jb.sums >= (size_t)bp.wb * pl.NB * 24, "%s n=%zu: jb.sums", what, n);
    CHECK(jb.T * 4 >= s.tb, "%s n=%zu: jb.T", what, n);
    CHECK(jb.over >= 1 && jb.over * (u64)J <= (u64)MSM_JOBS, "%s n=%zu: jb.over", what, n);
}
static void check_fb(const FbPlan& f, size_t n, int bits) {
    const MsmPlan& pl = f.pl; const BinPlan& bp = f.bp;
    CHECK(pl.c % 4 == 0 && pl.W == bits / pl.c + 1 && pl.B == (u32)pl.NB && pl.n == n, "fixed-base n=%zu: MsmPlan", n);
    CHECK((u32)(pl.W - 1) * (u32)(pl.c / 4) < FB_ROWS, "fixed-base n=%zu: the rows of the top window", n);
    CHECK(((size_t)1 << f.tbits) >= n && (1 << f.wbits) >= pl.W && f.vbits == f.tbits + f.wbits, "fixed-base n=%zu: tbits %u, wbits %u", n, f.tbits, f.wbits);
    CHECK(f.vbits + bp.LB + 1 <= 32, "fixed-base n=%zu: the entry word holds %u + %u + 1 bits", n, f.vbits, bp.LB);
    check_bins(pl, bp, n * (size_t)pl.W, 4, "fixed-base", n);   // (k_msm_bin_sort: 4 words; all windows share the one bucket set)
    CHECK((size_t)bp.NBIN * 4 <= LDS_BYTES, "fixed-base n=%zu: k_msm_fb_partition's LDS counters", n);
    CHECK((size_t)bp.NBIN * bp.cap < ((size_t)1 << 31) && bp.wb == 1 && bp.top_nb == 0 && bp.glv == 0, "fixed-base n=%zu: BinPlan", n);
    CHECK(f.nl >= 4 && f.nl <= MSM_NLMAX, "fixed-base n=%zu: nl %d", n, f.nl);
}

static void run_curve(int bits, bool has_glv) {
    for (const KnobSet& k : KNOBS) {
        MsmKnobs kn; kn.quad = k.quad; kn.chunk_cap = k.chunk_cap; kn.bin_min = k.bin_min; kn.glv_min = k.glv_min;
        for (size_t n : SIZES) {
            for (int J = 1; J <= (k.pair ? 2 : 1); J++) {
                const FsShape s = msm_fs_shape(n, bits, J, false, kn);
                print_fs("fixed-shape", k, bits, n, J, s, -1);
                if (s.fits) check_fs(s, n, J, false, "fixed-shape");
                if (s.binned) check_bins(s.pl, s.bp, n, 4, "binned general path", n);   // (k_msm_bin_sort: 4 words)
            }
            if (has_glv && k.glv) {
                const FsShape s = msm_fs_shape(n, bits, 1, true, kn);
                print_fs("glv", k, bits, n, 1, s, msm_glv_sizes(kn, n) ? 1 : 0);
                if (s.fits) check_fs(s, n, 1, true, "glv");
                // tests/test_gpu_primitives.py rests on this: n equal scalars put 2n half-terms into ONE bin region of a window,
                // which therefore overflows
                if (n == ((size_t)1 << 15)) CHECK(s.fits && s.bp.cap < 2 * n && s.bp.NBIN > 1, "glv n=2^15: cap %u, NBIN %u", s.bp.cap, s.bp.NBIN);
            }
        }
    }
    const MsmKnobs kn;
    for (size_t n : SIZES) {
        const FbPlan f = fb_plan(n, bits, kn);
        print_fb(bits, n, f);
        if (!f.decline) check_fb(f, n, bits);
    }
}
int main() {
    run_curve(256, true);    // secq256k1 (the curve with the endomorphism)
    run_curve(255, false);   // the curve over the 255-bit field
    if (g_failed) { fprintf(stderr, "msm_plan selftest: %d checks failed\n", g_failed); return 1; }
    puts("msm_plan selftest ok");
    return 0;
}
