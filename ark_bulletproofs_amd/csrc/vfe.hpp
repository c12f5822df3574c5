// Verifier front end on the device, part 2: launch interface of vfe.hip (its own translation unit: the kernels need nothing from
// the engine but the field / curve headers).  Everything is enqueued on the caller's stream; nothing here waits for the GPU.
// Layouts are documented at the kernels (vfe.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace arkbp {
namespace vfe {

static constexpr uint32_t PB_WORDS = 832;   // words per proof parameter block: r1cs.cuh VFY_PB_WORDS (checked where both are visible)

struct Shape {
    uint32_t P;        // proofs in the batch
    uint32_t m;        // commitments per statement
    uint32_t nV;       // commitments the sponge absorbs itself (m, or 0 when the transcripts already hold them)
    uint32_t k;        // inner-product rounds: N = 2^k
    uint32_t plen;     // bytes per compressed proof: 539 + 66 k
    uint32_t tail;     // tail terms per proof in the mega-check: 6 + m + 5 + 2 k
    uint32_t nitems;   // ItemMap::count()
    uint32_t G = 0;    // gadget challenges per proof (two-phase statements): challenges per proof = 6 + k + G
    uint32_t vwire = 0;   // d_V holds P x m x 33 bytes (serialize_compressed) instead of ark words; k_vfe_points decodes them
};

// status bits raised by the kernels (any bit: the batch goes through the host replay instead, which reports the reference's error)
static constexpr uint32_t ST_FORMAT = 1;        // a point or scalar the reference's deserializer rejects (proof.rs:83-91)
static constexpr uint32_t ST_IDENTITY = 2;      // an identity point where validate_and_append_point rejects it (transcript.rs:81-93)
static constexpr uint32_t ST_FRAMING = 4;       // L_vec / R_vec length fields disagree with the proof's size

// k_vfe_points: decompression, validation and serialization of every point of the batch.
//   d_proofs   P x plen bytes (R1CSProof::to_bytes)
//   d_V        P x m x 16 words, ark layout; with sh.vwire P x m x 33 bytes, ark-serialize's compressed form (a rejected one raises
//              ST_FORMAT, the identity is taken as all-zero words are)
//   d_msg      nitems x 9 x P 64-bit words: word w of item `it` of proof p at [(it * 9 + w) * P + p]
//   d_tail_pts P x tail x 16 words, resident layout, the mega-check's per-proof bases in verification_scalars' order
//   d_status   one word, OR of ST_*
//   d_flags    P words (may be null): the same bits per proof — word p holds what proof p raised
int launch_points(int curve, hipStream_t st, const Shape& sh, const uint8_t* d_proofs, const uint32_t* d_V, uint64_t* d_msg, uint32_t* d_tail_pts, uint32_t* d_status,
                  uint32_t* d_flags);

// k_vfe_sponge: one lane per proof runs the schedule (vfe_sched.hpp) from its transcript state; d_state0: 25 words per proof
// (state_stride = 25) or one shared state (0).  d_chal: P x (6 + k + G) x 8 words, resident form, order y z u x w u_1..u_k r g_1..g_G.
// d_gch (two-phase, optional): P x G x 8 words, the gadget challenges once more as ark words (what the host's callbacks receive).
int launch_sponge(int curve, hipStream_t st, const Shape& sh, const uint32_t* d_sched, const uint64_t* d_state0, uint32_t state_stride, const uint64_t* d_msg, uint32_t* d_chal,
                  uint8_t* d_seeds_or_null, uint32_t* d_gch = nullptr);

// k_vfe_consts + k_vfe_wv + k_vfe_sum2: everything of verification_scalars that is not of length N (verifier.rs:462-541 minus the
// g / h scalars).  d_alpha: P x 8 resident.  d_pb: P parameter blocks (r1cs.cuh VFY_PB_WORDS, resident form).  d_tail_sc: P x tail x 8
// canonical integers (alpha-scaled).  d_voff / d_vq / d_vc: the statement's terms on committed variables by commitment (CSR; vc
// resident).  d_ws: P x 32 x 8 words scratch.  d_sums: 2 x 8 words (ark form): sum_p alpha_p sB_p, sum_p alpha_p sBb_p.
int launch_prepare(int curve, hipStream_t st, const Shape& sh, const uint8_t* d_proofs, const uint32_t* d_chal, const uint32_t* d_alpha, const uint32_t* d_voff,
                   const uint32_t* d_vq, const uint32_t* d_vc, uint32_t* d_pb, uint32_t* d_tail_sc, uint32_t* d_ws, uint32_t* d_sums);

// The two-phase split of launch_prepare: the coefficients of a randomized statement's phase-2 terms are known per proof only after
// the host ran its callbacks, so k_vfe_consts + k_vfe_sum2 go first (launch_consts) and the committed-variable sums per block of
// proofs after (launch_wv_tab).  d_vcid: the terms' coefficient ids (host_proto.hpp CID_ONE / CID_MONE flags, else an index into
// the proof's own table); d_coefs: the tables of proofs [p0, p0 + np), coef_stride words apart, resident form.
int launch_consts(int curve, hipStream_t st, const Shape& sh, const uint8_t* d_proofs, const uint32_t* d_chal, const uint32_t* d_alpha, uint32_t* d_pb, uint32_t* d_tail_sc,
                  uint32_t* d_ws, uint32_t* d_sums);
int launch_wv_tab(int curve, hipStream_t st, const Shape& sh, uint32_t p0, uint32_t np, const uint32_t* d_pb, const uint32_t* d_voff, const uint32_t* d_vq,
                  const uint32_t* d_vcid, const uint32_t* d_coefs, uint32_t coef_stride, uint32_t* d_tail_sc);

// bp_gens_digest (include/arkbp.h has the definition): k_gens_leaves over the resident pair d_pc (2 points), d_G[0..n) and d_H[0..n),
// k_gens_nodes level by level, k_gens_root.  d_ws: gens_digest_ws_bytes(n) bytes of scratch, 64-byte aligned.  d_out: 128 bytes, 32-byte
// aligned = root | pair root | G root | H root.  n >= 1.
size_t gens_digest_ws_bytes(size_t n);
int launch_gens_digest(int curve, hipStream_t st, const uint32_t* d_pc, const uint32_t* d_G, const uint32_t* d_H, uint32_t n, uint8_t* d_ws, uint8_t* d_out);

}  // namespace vfe
}  // namespace arkbp
