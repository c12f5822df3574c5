// Everything about a call of the verifier's device front end that is arithmetic: the shape rules of a job (one class of
// like-instances), where the jobs of a call live in the ctx's buffers, and the layout of every buffer they share.  No HIP, no ctx, no
// getenv: compiles with a plain C++17 compiler, and vfy_dev_plan_selftest.cpp checks it on the CPU.  verify_dev.inc admits, places and
// launches from these values; verify_steps.inc shares the r_g layout and the block size.
//
//   pinned staging (bytes)  [job 0: proofs | commitments | states | alphas, each part 256-aligned][job 1] .. | flags, a word per
//                           instance, at tot.b_in | .. | h_small, the last VFY_SMALL_BYTES of the allocation
//   h_small (bytes)         [block deltas, 32 each, VFY_SLOTS | B / B_blinding sums, 64 per job, at VFY_HS_SUMS | status word at VFY_HS_STATUS]
//   vfe_small (words)       [status | .. | sums at VFY_DS_SUMS, VFY_DS_JOB per job]
//   r_g (scalars)           [2 heads | g Nmax | h Nmax | tails, job after job]; r_tail holds the tails' points in the same order
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/arkbp.h"   // BP_VFY_MAX_CLASSES
#include "vfe_sched.hpp"           // vfe::ITEM_WORDS

namespace arkbp {

static constexpr size_t VFY_BLOCK = 512;                             // proofs per k_vfy_tables / k_vfy_batch launch
static constexpr size_t VFY_SLOTS = 96;                              // block result slots (r_small / h_small) of one call, all jobs together
static constexpr size_t VFY_SMALL_BYTES = 4096;                      // vfe_small, and h_small at the end of the pinned staging
static constexpr size_t VFY_HS_SUMS = VFY_SLOTS * 32;
static constexpr size_t VFY_HS_STATUS = VFY_HS_SUMS + BP_VFY_MAX_CLASSES * 64;
static constexpr size_t VFY_DS_SUMS = 64, VFY_DS_JOB = 16;           // (the words before the sums are zeroed per call: the status word)
static_assert(VFY_HS_STATUS + 4 <= VFY_SMALL_BYTES && (VFY_DS_SUMS + BP_VFY_MAX_CLASSES * VFY_DS_JOB) * 4 <= VFY_SMALL_BYTES, "the small result areas are 4096 bytes");
static constexpr size_t VFY2_TABLE_BUDGET = (size_t)256 << 20;       // bytes of per-proof gadget challenges + coefficient tables per batch
static constexpr size_t VFY_TAIL_BOUND = (size_t)1 << 30;            // terms of one call's mega-check MSM, heads and accumulators included

static inline size_t vfy_up256(size_t x) { return (x + 255) & ~(size_t)255; }

// r_g, in scalars (32 bytes)
static constexpr size_t VFY_RG_G = 2;
static inline size_t vfy_rg_h(size_t Nmax) { return 2 + Nmax; }
static inline size_t vfy_rg_tails(size_t Nmax) { return 2 + 2 * Nmax; }
static inline size_t vfy_rg_len(size_t Nmax, size_t tails) { return vfy_rg_tails(Nmax) + tails; }

// Why a job is not the device's, one value per rule; everything else about it is the host replay's to report.
enum VfyDevDecline {
    VFY_DEV_OK = 0,
    VFY_DEV_FRAMING, VFY_DEV_ROUNDS,   // plen != 539 + 66 k; k >= 32
    VFY_DEV_WIRE,                      // 33-byte commitments that the transcripts already hold
    VFY_DEV_COUNT, VFY_DEV_M,          // more than 65535 instances, commitments
    VFY_DEV_TAILS, VFY_DEV_ITEMS,      // count * tail >= 2^31; nitems * ITEM_WORDS * count >= 2^32
    VFY_DEV_SLOTS,                     // more blocks than result slots
    VFY_DEV_N,                         // the statement's padded size is not 2^k
    VFY_DEV_TABLES,                    // two-phase: challenges and coefficient tables beyond VFY2_TABLE_BUDGET (include/arkbp.h)
};

struct VfyDevShape {
    size_t plen = 0, count = 0, m = 0;
    bool absorb = false, wire = false, shared_state = false;
    size_t N = 0, G = 0, ncoef = 0;                                       // known after the template / the rehearsal (vfy_dev_set_*)
    size_t k = 0, tail = 0, nV = 0, vbytes = 0, nitems = 0, nblocks = 0;  // derived
    size_t b_proofs = 0, b_V = 0, b_st = 0, b_in = 0;                     // staging parts (the alphas are the rest of b_in)
    size_t o_V() const { return b_proofs; }
    size_t o_st() const { return b_proofs + b_V; }
    size_t o_alpha() const { return b_proofs + b_V + b_st; }
    size_t gch() const { return count * G; }                              // two-phase pinned / device tables, in scalars: [gch | tab]
    size_t tab() const { return count * ncoef; }
};
// absorb: the device appends the m commitments to the transcripts; wire: they are staged as 33-byte encodings
static inline VfyDevDecline vfy_dev_shape(VfyDevShape& s, size_t plen, size_t count, size_t m, bool absorb, bool wire, bool shared_state) {
    s = VfyDevShape();
    s.plen = plen; s.count = count; s.m = m; s.absorb = absorb; s.wire = wire; s.shared_state = shared_state;
    if (plen < 539 || (plen - 539) % 66) return VFY_DEV_FRAMING;
    s.k = (plen - 539) / 66;
    if (s.k >= 32) return VFY_DEV_ROUNDS;
    if (wire && !absorb) return VFY_DEV_WIRE;
    if (count > 65535) return VFY_DEV_COUNT;
    if (m > 65535) return VFY_DEV_M;
    s.tail = 6 + m + 5 + 2 * s.k;
    s.nV = absorb ? m : 0;
    s.vbytes = wire ? 33 : 64;
    s.nitems = s.nV + 11 + 2 * s.k + 3;
    if (count * s.tail >= ((size_t)1 << 31)) return VFY_DEV_TAILS;
    if (s.nitems * vfe::ITEM_WORDS * count >= ((size_t)1 << 32)) return VFY_DEV_ITEMS;
    s.nblocks = (count + VFY_BLOCK - 1) / VFY_BLOCK;
    if (s.nblocks > VFY_SLOTS) return VFY_DEV_SLOTS;
    s.b_proofs = vfy_up256(count * plen); s.b_V = vfy_up256(count * m * s.vbytes); s.b_st = vfy_up256((shared_state ? 1 : count) * 200);
    s.b_in = s.b_proofs + s.b_V + s.b_st + vfy_up256(count * 32);
    return VFY_DEV_OK;
}
static inline VfyDevDecline vfy_dev_set_N(VfyDevShape& s, size_t N) { s.N = N; return N == ((size_t)1 << s.k) ? VFY_DEV_OK : VFY_DEV_N; }
static inline VfyDevDecline vfy_dev_set_tables(VfyDevShape& s, size_t G, size_t ncoef) {
    s.G = G; s.ncoef = ncoef;
    return s.count * (G + ncoef) * 32 > VFY2_TABLE_BUDGET ? VFY_DEV_TABLES : VFY_DEV_OK;
}

// A job's offsets in the call's buffers, and (vfy_dev_extent) what it occupies from there, in the same units: bytes of staging (in),
// 64-bit words (msg), scalars (chal, ws), instances (inst: alphas, parameter blocks, flags), tail terms, block slots, jobs (cls)
struct VfyDevPlace { size_t in = 0, msg = 0, chal = 0, ws = 0, inst = 0, tail = 0, blk = 0, cls = 0; };
struct VfyDevTotals { size_t b_in = 0, msg = 0, chal = 0, ws = 0, inst = 0, tail = 0, blocks = 0, classes = 0, Nmax = 0; };
static inline VfyDevPlace vfy_dev_extent(const VfyDevShape& s) {
    VfyDevPlace e;
    e.in = s.b_in; e.msg = s.nitems * vfe::ITEM_WORDS * s.count; e.chal = s.count * (6 + s.k + s.G); e.ws = s.count * 34; e.inst = s.count;
    e.tail = s.count * s.tail; e.blk = s.nblocks; e.cls = 1;
    return e;
}
// one more job behind the ones in tot: its place is their totals
static inline VfyDevPlace vfy_dev_append(VfyDevTotals& t, const VfyDevShape& s) {
    VfyDevPlace p;
    p.in = t.b_in; p.msg = t.msg; p.chal = t.chal; p.ws = t.ws; p.inst = t.inst; p.tail = t.tail; p.blk = t.blocks; p.cls = t.classes;
    const VfyDevPlace e = vfy_dev_extent(s);
    t.b_in += e.in; t.msg += e.msg; t.chal += e.chal; t.ws += e.ws; t.inst += e.inst; t.tail += e.tail; t.blocks += e.blk; t.classes += e.cls;
    t.Nmax = std::max(t.Nmax, s.N);
    return p;
}
// where the jobs of one call live: one after the other, job order = launch order
static inline void vfy_dev_place(const VfyDevShape* shapes, size_t nj, VfyDevPlace* places, VfyDevTotals& tot) {
    tot = VfyDevTotals();
    for (size_t c = 0; c < nj; c++) places[c] = vfy_dev_append(tot, shapes[c]);
}
// whether a call that holds tot takes one more class: a result slot per block, the mega-check's terms below VFY_TAIL_BOUND
static inline bool vfy_dev_fits(const VfyDevTotals& tot, const VfyDevShape& s) {
    return tot.blocks + s.nblocks <= VFY_SLOTS && tot.tail + s.count * s.tail + vfy_rg_tails(std::max<size_t>(s.N, 1)) < VFY_TAIL_BOUND;
}

// pinned staging: the flag words behind the jobs' inputs; `stage` bytes before the small area
static inline size_t vfy_dev_flags_at(const VfyDevTotals& tot) { return tot.b_in; }
// What a call asks of each buffer, in bytes, and what it zeroes before the first launch (z_*).  pb_words: vfe::PB_WORDS.
struct VfyDevSizes { size_t stage, in, msg, chal, ws, small, flags, r_g, r_tail, r_small, alpha, params, z_rg, z_small, z_flags; };
static inline VfyDevSizes vfy_dev_sizes(const VfyDevTotals& t, size_t pb_words) {
    VfyDevSizes z;
    z.stage = t.b_in + vfy_up256(t.inst * 4);
    z.in = t.b_in; z.msg = t.msg * 8; z.chal = t.chal * 32; z.ws = t.ws * 32; z.small = VFY_SMALL_BYTES;
    z.flags = std::max<size_t>(t.inst, 1) * 4;
    z.r_g = vfy_rg_len(t.Nmax, t.tail) * 32; z.r_tail = std::max<size_t>(t.tail, 1) * 64; z.r_small = (t.blocks + 8) * 32;
    z.alpha = t.inst * 32; z.params = t.inst * pb_words * 4;
    z.z_rg = vfy_rg_tails(t.Nmax) * 32; z.z_small = VFY_DS_SUMS * 4; z.z_flags = z.flags;
    return z;
}

}  // namespace arkbp
