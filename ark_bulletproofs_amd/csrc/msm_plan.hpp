// The shapes of an MSM: the plain-data plans the MSM kernels take as arguments (msm.cuh) and the host functions that make them — pure
// functions of (terms, scalar bits, knobs).  No HIP, no ctx, no getenv: compiles with a plain C++17 compiler, and
// msm_plan_selftest.cpp checks on the CPU what the kernels rely on (LDS sizes, index widths, per-job strides) and that every plan
// equals the recorded one (tests/golden/msm_plans.json).  arkbp.hip fills MsmKnobs once per call and does the launching.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace arkbp {

typedef uint32_t u32;
typedef uint64_t u64;

#ifndef ARKBP_MSM_CH
#define ARKBP_MSM_CH 16
#endif
static constexpr int MSM_CH = ARKBP_MSM_CH;  // entries per level-1 lane / fan-in of the reduction tree on the skew-tolerant path
static constexpr int MSM_CHL = MSM_CH == 8 ? 3 : MSM_CH == 16 ? 4 : MSM_CH == 32 ? 5 : 6;
static_assert((1 << MSM_CHL) == MSM_CH, "ARKBP_MSM_CH must be 8, 16, 32 or 64");
static constexpr int MSM_CHL_BINNED = MSM_CHL;   // measured: whole-bucket lanes (64) lose more to divergence and a thin grid than the tree levels cost
static constexpr int MSM_MAXLVL = 8;   // 16^8 = 2^32 >= any bucket population
static constexpr int MSM_NLMAX = MSM_MAXLVL + 1;
static constexpr int MSM_GLV_WORDS = 12;   // words per split scalar (glv.cuh glv_split)

// Jobs of the fixed-shape pipeline (msm.cuh section 7): blockIdx.z of its five kernels is the job.  The jobs of one launch have the
// same term count, hence the same plans; each has its own scalars and bases and its own copy of every buffer the kernels read or
// write, FsJobs words further per job.  Nothing is shared between jobs, so a job computes exactly what it computes alone; a launch
// with gridDim.z == 1 needs no strides (FsJobs{}).
static constexpr int MSM_JOBS = 2;   // (L and R of an inner-product round)
struct FsJobs {   // per-job strides in 32-bit words
    u64 canon, hist, bin_cur, slots, buckets /* boff, bcnt, loff */, binch, part, sums, T /* the marginals with the info words behind */, over;
};

struct MsmPlan {
    int c, W, NB;        // window bits, windows, buckets per window (2^(c-1))
    u32 B;               // W * NB
    u32 n;
    int w_lo, w_hi;      // windows this call accumulates (multi-GPU window sharding); [0, W) = all
};

// One-pass sort: bucket (w, v) owns the fixed slot range [base[w] + v*cap[w], +cap[w]) so the histogram pass can place
// entries directly; cap[w] is ~2x the expected population (windows with few possible digit values get wider slots).  A bucket
// that outgrows its slots raises `overflow` and the exact two-pass path (k_msm_scatter) is used for that MSM instead.
static constexpr int MSM_MAXW = 88;
struct SlotPlan {
    u32 base[MSM_MAXW];
    u32 cap[MSM_MAXW];
};

// Two-level sort for large MSMs (msm.cuh 1b): bin regions of fixed capacity (mean + 8 sigma) for the full windows, the short top
// window keeps the slot scheme.
struct BinPlan {
    u32 LB;      // bucket bits resolved inside a bin
    u32 NBIN;    // bins per window = NB >> LB
    u32 cap;     // entries per bin region
    u32 wb;      // windows [0, wb) are binned; [wb, W) use SlotPlan
    u32 tpt;     // terms per lane in k_msm_bin_partition
    u32 top_nb;  // > 0: the slot window has this many possible buckets (<= 2048) and is counted per workgroup in LDS
    u32 glv;     // the scalars are split (glv_split): every term contributes two half-terms 2 * i, 2 * i + 1 of 128 bits
};

static constexpr u32 MSM_FS_MAXBINS = 4096;
static constexpr u32 MSM_FS_BUCKET_MAX = 256;   // entries of a binned bucket; with chcap >= 8 at most 32 partials reach k_msm_reduce_fs
static constexpr u32 MSM_TOP_PARTS_MAX = 32;   // (a bit of the slot window collects ~n/32 partials: 4 .. 32 workgroups share them)
static constexpr u32 MSM_FS_TOP_WORDS = 2052;  // LDS words in which k_msm_marginals_fs holds the top_nb + 1 prefix counts of the slot window
struct FsPlan {
    u32 nbins;      // wb * NBIN (+ 1 when the slot window exists: the last "bin" is that window)
    u32 has_top;    // the slot window (w = wb) exists
    u32 top_bits;   // bit length of its largest |digit|
    u32 max_chunks; // grid bound of k_msm_accum_fs
    u32 top_parts;  // workgroups per bit of the slot window in k_msm_marginals_fs
};

static constexpr u32 FB_ROWS = 65;   // rows of a fixed-base table at bit positions 0, 4, 8, .., 256: any window width c that is a multiple of 4 finds its rows (the last one serves the carry window)

// What the planners read of the ctx (its BP_TUNE_MSM_* knobs: the initial values here are the ctx's) and of the environment (the
// ARKBP_MSM_* experiment switches; arkbp.hip reads them, once).
struct MsmKnobs {
    size_t wsum_min = (size_t)1 << 18;    // BP_TUNE_MSM_WSUM_MIN: buckets from which running-sum window aggregation replaces the marginals
    size_t bin_min = 64;                  // BP_TUNE_MSM_BIN_MIN
    size_t glv_min = 256;                 // BP_TUNE_MSM_GLV_MIN: terms from which an MSM on a GLV curve splits its scalars
    size_t chunk_cap = 0;                 // BP_TUNE_MSM_CHUNK_CAP: entries per level-1 chunk of the fixed-shape pipeline (0 = fs_chunk_cap's choice)
    size_t fixed_min = (size_t)1 << 20;   // BP_TUNE_MSM_FIXED_MIN: terms from which MSMs over the generator tables use the fixed-base rows
    bool quad = false;                    // latency-first: the caller waits for this one result (the bp_msm* entry points, ARKBP_MSM_LATENCY)
    // experiments (0 / false = unset)
    int env_c = 0, env_fs_cap = 0, env_tpt = 0, env_fixed_c = 0;   // ARKBP_MSM_C, ARKBP_MSM_FS_CAP, ARKBP_MSM_TPT, ARKBP_MSM_FIXED_C
    bool env_nobin = false, env_nofs = false, env_marginals = false;   // ARKBP_MSM_NOBIN, ARKBP_MSM_NOFS, ARKBP_MSM_MARGINALS
};

static inline MsmPlan msm_plan(size_t n, int bits, const MsmKnobs& kn) {
    double best = 1e300; int bc = 4;
    for (int c = 3; c <= 16; c++) {
        double W = bits / c + 1, NBk = std::ldexp(1.0, c - 1), B = W * NBk;
        double cost = n * W + (n * W / MSM_CH + B) * 1.45 + B * (0.5 * c) * 1.45 + 256.0 * c * W * 0.05;
        if (cost < best) { best = cost; bc = c; }
    }
    if (kn.env_c >= 3 && kn.env_c <= 16 && n >= 4096) bc = kn.env_c;
    MsmPlan pl; pl.c = bc; pl.W = bits / bc + 1; pl.NB = 1 << (bc - 1); pl.B = (u32)pl.W * pl.NB; pl.n = (u32)n;
    pl.w_lo = 0; pl.w_hi = pl.W;
    return pl;
}
// the bit-marginal bucket aggregation (else running window sums)
static inline bool msm_use_marginals(const MsmKnobs& kn, const MsmPlan& pl) { return kn.env_marginals || pl.B < kn.wsum_min; }
// the size part of the GLV route (msm_glv_route): mid-size MSMs of a caller that waits for the one result
static inline bool msm_glv_sizes(const MsmKnobs& kn, size_t n) { return kn.quad && n >= std::max<size_t>(kn.bin_min, kn.glv_min) && n < ((size_t)1 << 27); }

// Two-level (binned) sort for large MSMs: the full windows go to bin regions, the short top window keeps its slots behind them.
// n scalars of `bits` bits; glv: the plan is over their 2n half-terms (bits = 128, pl made for 2n terms) — then false means that the
// GLV route does not apply, and what it does differently from the plain plan is marked "GLV:" below.
static inline bool msm_bin_plan(size_t n, int bits, const MsmPlan& pl, const MsmKnobs& kn, bool glv, BinPlan& bp) {
    memset(&bp, 0, sizeof bp);
    const size_t ne = glv ? 2 * n : n;   // entries per window
    const int bits_last = bits - pl.c * (pl.W - 1);
    const int wbn = bits_last < pl.c - 1 ? pl.W - 1 : pl.W;
    if (wbn <= 0) return false;
    // GLV: the route has its own size gate (msm_glv_sizes) and ignores ARKBP_MSM_NOBIN
    if (!glv && !(n >= kn.bin_min && !kn.env_nobin)) return false;
    u32 nbin = 1, lg = 0;
    while ((size_t)nbin * 8192 < ne && nbin < (u32)pl.NB) { nbin <<= 1; lg++; }
    // bins of up to 12 K entries (43 KB of LDS in the bin sort) where that keeps the MSM inside the fixed-shape pipeline's bin
    // limit: 2^20 < n <= 1.5 * 2^20, e.g. the 1.25 M-term MSM of a 4096-proof batch verification.  GLV: no such rule
    if (!glv && (size_t)wbn * nbin + 1 > MSM_FS_MAXBINS && nbin >= 2 && (size_t)(nbin / 2) * 12288 >= ne && (size_t)wbn * (nbin / 2) + 1 <= MSM_FS_MAXBINS) { nbin >>= 1; lg--; }
    int LB = pl.c - 1 - (int)lg;
    while (LB > 11) { nbin <<= 1; LB--; }
    const double mu = (double)ne / nbin;
    const size_t cap = std::min<size_t>(ne, (size_t)(mu + 8.0 * std::sqrt(mu) + 64.0));
    // GLV: sized by k_msm_bin_sort_fs (8 words beside the counters and the region; k_msm_bin_sort has 4), the only sort it goes through
    const size_t lds_sort = (((size_t)1 << LB) + (glv ? 8 : 4) + cap) * 4;
    // GLV: the term field of an entry word is 2 * i + half, one bit wider
    if (!(ne < ((size_t)1 << ((glv ? 30 : 31) - LB)) && lds_sort <= 64 * 1024 && (size_t)wbn * nbin * cap < ((size_t)1 << 31))) return false;
    bp.LB = (u32)LB; bp.NBIN = nbin; bp.cap = (u32)cap; bp.wb = (u32)wbn; bp.glv = glv ? 1u : 0u;
    // terms per lane of the partition kernel: by the SCALARS it reads.  GLV: ARKBP_MSM_TPT is not read
    bp.tpt = !glv && kn.env_tpt > 0 ? (u32)kn.env_tpt : (u32)std::min<size_t>(16, std::max<size_t>(1, n / (256 * 512)));
    if (wbn < pl.W) {   // same-address device atomics serialise (~170 ns each): count a narrow top window per workgroup
        const size_t nb_top = std::min<size_t>((size_t)pl.NB, ((size_t)1 << std::max(bits_last, 0)) + 1);
        // GLV: up to 2049 buckets (k_msm_marginals_fs holds top_nb + 1 prefix counts in MSM_FS_TOP_WORDS words), and a wider top
        // window ends the route; the plain plan stays binned without top_nb, for the general path
        if (glv && nb_top > 2049) return false;
        if (glv || nb_top <= 2048) bp.top_nb = (u32)nb_top;
    }
    return true;
}
// slot plan of the one-pass sort for the windows from w_first on, behind first_slot entries; returns the entries in all.  ne: entries
// per window (terms, or half-terms of a GLV plan)
static inline size_t msm_make_slots(const MsmPlan& pl, int bits, size_t ne, bool glv, SlotPlan& sp, int w_first, size_t first_slot) {
    memset(&sp, 0, sizeof sp);
    size_t nslots = first_slot;
    for (int w = w_first; w < pl.W; w++) {
        const int bits_left = bits - pl.c * w;  // scalar bits at or above this window's base
        size_t nb_eff = (size_t)pl.NB;
        if (bits_left < pl.c - 1) nb_eff = std::min<size_t>(nb_eff, ((size_t)1 << std::max(bits_left, 0)) + 1);
        // GLV: the halves are not uniform below 2^128 (|k2| reaches 1.27 * 2^127, |k1| 1.08 * 2^127), so the low buckets of the narrow
        // top window are fuller than a uniform spread: four times the mean instead of twice
        const size_t mean = (ne + nb_eff - 1) / nb_eff;
        size_t cap = std::min<size_t>(ne, glv ? 4 * mean + 64 : 2 * mean + 32);
        sp.base[w] = (u32)nslots; sp.cap[w] = (u32)cap;
        nslots += nb_eff * cap;
    }
    return nslots;
}
// the MSM goes through the fixed-shape pipeline (msm.cuh 7).  GLV: neither ARKBP_MSM_MARGINALS nor ARKBP_MSM_NOFS is read here (the
// route checks the latter)
static inline bool msm_fs_fits(const MsmKnobs& kn, const MsmPlan& pl, const BinPlan& bp, bool binned, bool fixed_c4) {
    const bool marginals = bp.glv ? pl.B < kn.wsum_min : msm_use_marginals(kn, pl) && !kn.env_nofs;
    return binned && marginals && (bp.wb == (u32)pl.W || bp.top_nb > 0) && (size_t)bp.wb * bp.NBIN + 1 <= MSM_FS_MAXBINS && !fixed_c4;
}

// Entries per level-1 chunk of the fixed-shape pipeline.  Throughput callers keep 16.  For a caller waiting on ONE mid-size MSM the
// accumulate is a single round of workgroups whose duration is (entries per lane) x (latency of a mixed addition at the fill of
// the lane's SIMD: 6.7 us alone, ~5.6 us per resident wave from two up — tools/ubench_coop.hip): 2^16 terms at 16 entries per chunk
// make ~100 K lanes = 1.5 waves per SIMD, i.e. every lane waits for the SIMDs that hold two.  The cap is chosen so that the lanes
// fill a whole number of waves per SIMD with as few entries per lane as that allows (measured at 2^16 terms, secq256k1, accumulate /
// wall: cap 11 0.200 / 0.520 ms, 12 0.157 / 0.468, 13 0.169 / 0.479, 14 0.181 / 0.487, 16 0.205 / 0.506: profiles/r03_msm_chunk_cap.txt).
// binned: entries / buckets of the binned windows (bucket populations ~ Poisson); top: the narrow top window (a few full buckets).
static inline u32 fs_chunk_cap(const MsmKnobs& kn, double binned_entries, double binned_buckets, double top_entries, double top_buckets) {
    if (kn.env_fs_cap >= 8 && kn.env_fs_cap <= 64) return (u32)kn.env_fs_cap;
    if (kn.chunk_cap) return (u32)kn.chunk_cap;
    if (!kn.quad || binned_buckets < 1.0) return 1u << MSM_CHL_BINNED;
    const double lanes_per_fill = 256.0 * 4 * 64;   // one wave on every SIMD of the chip
    const double mu = binned_entries / binned_buckets, sd = std::sqrt(std::max(mu, 1e-9));
    u32 best_cap = 1u << MSM_CHL_BINNED; double best_t = 1e300;
    for (u32 cap = 8; cap <= 32; cap++) {
        double e_chunks = 0, e_work = 0, wsum = 0;   // E ceil(X / cap) and E X / ceil(X / cap) for X ~ N(mu, mu)
        for (int q = -30; q <= 30; q++) {
            const double z = q / 10.0, x = std::max(1.0, mu + sd * z), w = std::exp(-0.5 * z * z), k = std::ceil(x / cap);
            e_chunks += w * k; e_work += w * x / k; wsum += w;
        }
        const double chunks = binned_buckets * e_chunks / wsum + top_entries / cap + 0.5 * top_buckets;
        const double fill = std::ceil(chunks / lanes_per_fill - 0.004);
        if (fill > 4.0) continue;   // throughput-bound anyway: the default
        const double t = (e_work / wsum) * (fill <= 1.0 ? 6.7 : 5.6 * fill) + 0.02 * (chunks / 1000.0);   // (+ the partials the next kernel has to add)
        if (t < best_t) { best_t = t; best_cap = cap; }
    }
    return best_cap;
}

// Everything the fixed-shape chain (arkbp.hip msm_fs_jobs) needs to know before it touches a buffer: J <= MSM_JOBS MSMs of n scalars
// each, plain (bits-wide scalars, windows [w_lo, w_hi) — w_hi < 0: all) or GLV (2n half-terms of 128 bits).  pl / binned / bp are
// also what the general path of a plain MSM runs on when the shape does not fit.
struct FsShape {
    bool fits;           // the chain can run; false: nothing behind `bp` is set
    bool binned;         // bp holds a plan
    MsmPlan pl; BinPlan bp; SlotPlan sp; FsPlan fp; FsJobs jb;
    size_t nslots;       // entries of one job's slot array: the bin regions, then the slot window
    size_t maxch;        // bound on the level-1 chunks of one job: grid of k_msm_accum_fs, partials in lvA
    size_t tc, tb;       // marginal points of one job (grid of k_msm_marginals_fs), bytes of its result block (the points, 64 bytes of info words)
    u32 red_g;           // lanes per bucket of k_msm_reduce_fs: groups while the lanes fit the chip at once, one lane per bucket beyond
    u32 chl_fs;          // entries per chunk (any value from 8)
};
static inline FsShape msm_fs_shape(size_t n, int bits, int J, bool glv, const MsmKnobs& kn, int w_lo = 0, int w_hi = -1, bool fixed_c4 = false) {
    FsShape s; memset(&s, 0, sizeof s);
    const size_t ne = glv ? 2 * n : n;
    if (glv) bits = 128;   // magnitudes of the halves (glv_split guarantees < 2^128 or flags the MSM)
    MsmPlan& pl = s.pl; BinPlan& bp = s.bp; FsPlan& fp = s.fp;
    pl = msm_plan(ne, bits, kn);
    pl.n = (u32)n;       // scalars the partition kernel reads
    if (w_hi >= 0) { pl.w_lo = std::max(0, w_lo); pl.w_hi = std::min(pl.W, w_hi); }
    if (pl.W > MSM_MAXW) return s;
    s.binned = msm_bin_plan(n, bits, pl, kn, glv, bp);
    if (!msm_fs_fits(kn, pl, bp, s.binned, fixed_c4)) return s;
    s.chl_fs = fs_chunk_cap(kn, (double)ne * bp.wb * (1.0 - std::ldexp(1.0, -pl.c)), (double)bp.wb * pl.NB, bp.wb < (u32)pl.W ? (double)ne : 0.0, (double)bp.top_nb);
    fp.has_top = bp.wb < (u32)pl.W ? 1u : 0u;
    fp.nbins = bp.wb * bp.NBIN + fp.has_top;
    if (fp.has_top) { u32 t = bp.top_nb; while (t) { fp.top_bits++; t >>= 1; } }
    const size_t nwin = (size_t)(pl.w_hi - pl.w_lo);
    s.red_g = (size_t)bp.wb * pl.NB > 49152 ? 1u : 4u;
    s.maxch = (ne * nwin) / s.chl_fs + std::min<size_t>(ne * nwin, nwin * (size_t)pl.NB) + 64;
    fp.max_chunks = (u32)s.maxch;
    s.nslots = msm_make_slots(pl, bits, ne, glv, s.sp, (int)bp.wb, (size_t)bp.wb * bp.NBIN * bp.cap);
    fp.top_parts = (u32)std::min<size_t>(MSM_TOP_PARTS_MAX, std::max<size_t>(4, ne >> 15));
    s.tc = (size_t)bp.wb * pl.c + (size_t)fp.top_bits * fp.top_parts;
    s.tb = s.tc * 96 + 64;
    if (J < 1 || J > MSM_JOBS || !(s.nslots < ((size_t)1 << 32) && s.maxch < ((size_t)1 << 31))) return s;
    FsJobs& jb = s.jb;
    jb.canon = n * (glv ? MSM_GLV_WORDS : 8); jb.hist = pl.B; jb.bin_cur = (size_t)pl.W * bp.NBIN; jb.slots = s.nslots; jb.buckets = pl.B; jb.binch = MSM_FS_MAXBINS + 1;
    jb.part = s.maxch * 24; jb.sums = (size_t)bp.wb * pl.NB * 24; jb.T = s.tb / 4; jb.over = 1;
    s.fits = true;
    return s;
}

// The fixed-base schedule (msm.cuh 1c) for n terms: window width, the entry word's fields, bins, reduction depth.  decline: 0, or
// the exit at which the schedule steps aside (the numbers of the ARKBP_FB_TRACE lines; 1, 3 and 7 are the caller's).
struct FbPlan {
    int decline;
    MsmPlan pl;          // (B = NB: one bucket set, the rows carry the windows' powers of two)
    BinPlan bp;
    u32 tbits, wbits, vbits;   // term index, window, both: the vterm field of an entry word, vterm | fine bucket (LB bits) | sign
    int nl;              // reduction levels that can be needed
};
static inline FbPlan fb_plan(size_t n, int bits, const MsmKnobs& kn) {
    FbPlan f; memset(&f, 0, sizeof f);
    // pays from ~2^20 terms (2^21: all kernels 5.6 -> 4.5 ms; at 2^19 and below the single latency-bound aggregation pass costs more
    // than the saved additions: tools/exp_msm_gens.py)
    if (n < std::max<size_t>(kn.fixed_min, 4096) || n >= ((size_t)1 << 24)) { f.decline = 2; return f; }
    // window width: a multiple of 4 (the table rows); cost = mixed adds (n * W) + bucket aggregation (~6 add-equivalents per bucket)
    int bc = 8; double best = 1e300;
    for (int c = 8; c <= 24; c += 4) {
        const double W = bits / c + 1, NBk = std::ldexp(1.0, c - 1);
        const double cost = n * W * 1.1 + NBk * 6.0;
        if (cost < best) { best = cost; bc = c; }
    }
    if (kn.env_fixed_c >= 8 && kn.env_fixed_c <= 24 && kn.env_fixed_c % 4 == 0) bc = kn.env_fixed_c;
    MsmPlan pl; pl.c = bc; pl.W = bits / bc + 1; pl.NB = 1 << (bc - 1); pl.B = (u32)pl.NB; pl.n = (u32)n; pl.w_lo = 0; pl.w_hi = pl.W;
    if ((u32)(pl.W - 1) * (u32)(bc / 4) >= FB_ROWS) { f.decline = 4; return f; }
    u32 tbits = 1; while (((size_t)1 << tbits) < n) tbits++;   // (term indices are < n: n itself need not fit)
    u32 wbits = 1; while ((1 << wbits) < pl.W) wbits++;
    const u32 vbits = tbits + wbits;
    // bins: ~6 K entries each; the entry word must hold vterm | fine bucket | sign
    const double entries = (double)n * (pl.W - 1) + (double)n * 0.5;
    u32 nbin = 1, lg = 0;
    while ((double)nbin * 6000.0 < entries && nbin < (u32)pl.NB) { nbin <<= 1; lg++; }
    int LB = bc - 1 - (int)lg;
    while (LB > 0 && (LB > 11 || vbits + (u32)LB + 1 > 32)) { nbin <<= 1; LB--; }
    if (vbits + (u32)LB + 1 > 32 || (size_t)nbin * 4 > 64 * 1024) { f.decline = 5; return f; }
    // expected load of the fullest bin: every full window spreads n(1 - 2^-c) digits uniformly; the top window (tb bits) only reaches
    // the lowest 2^(tb-1) buckets
    const int tb = bits - bc * (pl.W - 1);
    double mu = (double)n * (pl.W - 1) / nbin;
    if (tb > 0) { const double reach = std::max(1.0, std::ldexp(1.0, tb - 1) / (double)((u32)1 << LB)); mu += (double)n / std::min<double>(reach, nbin); }
    const size_t cap = (size_t)(mu + 8.0 * std::sqrt(mu) + 64.0);
    if ((((size_t)1 << LB) + 4 + cap) * 4 > 64 * 1024 || (size_t)nbin * cap >= ((size_t)1 << 31)) { f.decline = 6; return f; }
    f.pl = pl;
    f.bp.LB = (u32)LB; f.bp.NBIN = nbin; f.bp.cap = (u32)cap; f.bp.wb = 1; f.bp.tpt = (u32)std::min<size_t>(16, std::max<size_t>(1, n / (256 * 512)));
    f.tbits = tbits; f.wbits = wbits; f.vbits = vbits;
    f.nl = 2;
    { u64 capl = MSM_CH; while (capl < entries + 1 && f.nl < MSM_NLMAX) { capl *= MSM_CH; f.nl++; } }
    if (f.nl < 4) f.nl = 4;
    return f;
}

}  // namespace arkbp
