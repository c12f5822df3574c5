// The layout of one inner-product round's L and R as plain data: which slices of the generator vectors G and H (and Q) each side
// sums over, in the order of its scalars, and which runner computes the two sums.  No HIP, no ctx, no getenv: compiles with a plain
// C++17 compiler, and ipa_plan_selftest.cpp checks every layout on the CPU.  arkbp.hip launches the scalar kernels of a round, makes
// the plan and hands its sides to the MSM runners (ipa_round_lr); prove_batch.inc builds its direct-table jobs from the same plan.
#pragma once
#include <algorithm>
#include <cstddef>

namespace arkbp {

enum IpaKind { IPA_PLAIN, IPA_DEFERRED, IPA_FROZEN };
enum IpaTable { IPA_G = 0, IPA_H = 1, IPA_Q = 2 };   // (the table numbers of the fixed-base rows: 2 is the Pedersen table, whose row 0 is B)

// A round of half length n.  The working G and H of the round are (a slice of) two generator tables: working element i is table
// element first + i * stride (stride = the world size of an index-cyclic slice).  A compact copy is first = 0, stride = 1.
struct IpaShape {
    IpaKind kind;
    size_t n;                  // half length of the round: a and b have 2n elements
    size_t n1;                 // deferred: the half length of the round before, 2n (G and H still have 2 * n1 elements)
    size_t n0;                 // frozen: the length at which G and H froze
    size_t g_first, h_first;   // where working element 0 sits in the tables
    size_t stride;
    IpaShape compact() const { IpaShape c = *this; c.g_first = c.h_first = 0; c.stride = 1; return c; }
};

struct IpaSeg {
    int table;
    size_t first, count, stride;
    // frozen only: this side's scalars are zero outside the lower (0) / upper (1) half of every period of 2n elements; the direct
    // window tables visit only that half (DtSeg fold_n = n, fold_hi = half), every other runner sums over the whole segment
    int half;
};
static constexpr int IPA_MAXSEG = 5;
// One side: scalar slot k belongs to the k-th base of the segments in order, so Q's scalar (the inner product of the side) is in
// slot ip_slot = terms - 1.  Where Q = qw * B is read from the Pedersen table instead (fixed-base rows, direct window tables), the
// inner product scaled by qw is taken from the slot after it.
struct IpaSide {
    IpaSeg seg[IPA_MAXSEG];
    int nseg;
    size_t terms, ip_slot;
};
struct IpaPlan { IpaSide side[2]; };   // L, R

//   plain     L = G[n..2n) H[0..n) Q                              R = G[0..n) H[n..2n) Q                               2n + 1 terms
//   deferred  L = G[n1+n..) G[n..) H[n1..) H[0..), n each, Q      R = G[n1..) G[0..) H[n1+n..) H[n..), Q               4n + 1
//   frozen    L = R = G[0..n0) H[0..n0) Q (L: upper half-periods of G and lower ones of H carry scalars, R the others)    2n0 + 1
static inline IpaPlan ipa_plan(const IpaShape& sh) {
    IpaPlan p = IpaPlan();
    for (int o = 0; o < 2; o++) {
        IpaSide& sd = p.side[o];
        auto add = [&](int table, size_t off, size_t count, int half) {
            const size_t first = table == IPA_G ? sh.g_first : sh.h_first;
            sd.seg[sd.nseg++] = table == IPA_Q ? IpaSeg{IPA_Q, 0, 1, 1, 0} : IpaSeg{table, first + off * sh.stride, count, sh.stride, half};
            sd.terms += count;
        };
        const size_t g = o == 0 ? sh.n : 0, h = sh.n - g;   // the half of G, of H this side takes
        switch (sh.kind) {
        case IPA_PLAIN: add(IPA_G, g, sh.n, 0); add(IPA_H, h, sh.n, 0); break;
        case IPA_DEFERRED: add(IPA_G, sh.n1 + g, sh.n, 0); add(IPA_G, g, sh.n, 0); add(IPA_H, sh.n1 + h, sh.n, 0); add(IPA_H, h, sh.n, 0); break;
        case IPA_FROZEN: add(IPA_G, 0, sh.n0, o == 0 ? 1 : 0); add(IPA_H, 0, sh.n0, o == 0 ? 0 : 1); break;
        }
        add(IPA_Q, 0, 1, 0);
        sd.ip_slot = sd.terms - 1;
    }
    return p;
}

// Who computes the two sums.  Rows: the fixed-base rows of the resident tables, tried first, and they may decline a side.
// EACH: each side on its own (a rank's index-cyclic slice: shard mode 2); L_THEN_R: R only if L was done
enum IpaRows { IPA_ROWS_NONE, IPA_ROWS_EACH, IPA_ROWS_L_THEN_R };
// DIRECT: the direct window tables, two jobs in one launch; PAIR / TWO: unless the rows did both sides, both — as one pair / one MSM
// each; SIDE: a side the rows did not do, alone, before the other side is begun
enum IpaFallback { IPA_FB_DIRECT, IPA_FB_PAIR, IPA_FB_TWO, IPA_FB_SIDE };
struct IpaPolicy { IpaRows rows; IpaFallback fallback; };
struct IpaRoute {
    bool frozen, direct, deferred, first /* round 1 */, tables /* G and H are read from the resident generator tables */;
    bool have_qw /* Q = qw * B */, fb_rows /* the ctx has fixed-base rows */;
    int msm_mode;      // -1 = the ctx default, 2 = an index-cyclic slice, 0 = replicated
    size_t stride;
};
static inline IpaPolicy ipa_policy(const IpaRoute& r) {
    if (r.frozen) return {IPA_ROWS_NONE, r.direct ? IPA_FB_DIRECT : IPA_FB_PAIR};
    if (r.deferred) {
        if (r.msm_mode == 2) return {r.have_qw && r.fb_rows ? IPA_ROWS_EACH : IPA_ROWS_NONE, IPA_FB_SIDE};
        return {r.have_qw && r.msm_mode == -1 ? IPA_ROWS_L_THEN_R : IPA_ROWS_NONE, IPA_FB_TWO};
    }
    if (r.tables && r.have_qw && r.msm_mode == -1) return {IPA_ROWS_L_THEN_R, IPA_FB_PAIR};
    if (r.first && r.msm_mode == 2 && r.stride > 1 && r.have_qw && r.fb_rows) return {IPA_ROWS_EACH, IPA_FB_SIDE};
    return {IPA_ROWS_NONE, IPA_FB_PAIR};
}

// Global length at which the ranks of an index-cyclic argument gather what is left and finish replicated: the freeze length, but no
// less than the world or 2, rounded up to a power of two.  The test that partitions and the prover that gathers must agree on it.
static inline size_t ipa_gather_len(size_t freeze_len, size_t world) {
    const size_t least = std::max<size_t>(std::max(freeze_len, world), 2);
    size_t p = 1;
    while (p < least) p <<= 1;
    return p;
}

}  // namespace arkbp
