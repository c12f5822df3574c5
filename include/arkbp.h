/* arkbp.h — C ABI of libarkbp_hip.so: the MI355X (gfx950) engine behind the MSM / inner-product hot path of
 * FindoraNetwork/ark-bulletproofs.  Every entry point names the reference interface it replaces
 * (paths are into the reference repository).  A Rust shim binds these with `extern "C"`
 * (see INTEGRATION.md); the repo's own tests bind them with ctypes.
 *
 * Data conventions (identical to the reference's in-memory types, so a shim passes pointers):
 *   field element  4 x uint64_t little-endian limbs, Montgomery form with R = 2^256 — ark-ff's
 *                  Fp256<MontBackend<_,4>>.  "scalar" = element of G::ScalarField, coordinates are in
 *                  the curve's base field.
 *   affine point   8 x uint64_t = x || y.  ark's Affine{x,y,infinity} packs to this with the identity
 *                  encoded as all-zero (0,0 is on neither curve).
 *   curve          0 = secq256k1 (ark-secq256k1), 1 = zorro (src/curve/zorro/)
 * All functions return 0 on success or a negative BP_E_* code; nothing throws or aborts across the
 * boundary.  A bp_ctx owns one HIP stream and its workspaces: calls on one ctx are serialised, distinct
 * contexts are independent (one per device / host thread).
 */
#ifndef ARKBP_H
#define ARKBP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define BP_CURVE_SECQ256K1 0
#define BP_CURVE_ZORRO 1

#define BP_OK 0
#define BP_E_ARG (-1)          /* bad argument (null pointer, unknown curve, length mismatch) */
#define BP_E_HIP (-2)          /* HIP runtime error; bp_last_error() has the text */
#define BP_E_NO_DEVICE (-3)    /* no gfx950 device visible: the engine has no CPU fallback */
#define BP_E_VERIFICATION (-4) /* R1CSError::VerificationError / ProofError::VerificationError (src/errors.rs) */
#define BP_E_GENS_LENGTH (-5)  /* R1CSError::InvalidGeneratorsLength */
#define BP_E_FORMAT (-6)       /* R1CSError::FormatError */
#define BP_E_MISSING (-7)      /* R1CSError::MissingAssignment */
#define BP_E_UNSATISFIED (-8)  /* the witness violates a gate or a constraint; no proof was produced */

typedef struct bp_ctx bp_ctx;

const char* bp_last_error(void);
/* number of HIP devices visible (0 => every compute entry point returns BP_E_NO_DEVICE) */
int bp_device_count(void);
int bp_ctx_create(int curve, int device, bp_ctx** out);
void bp_ctx_destroy(bp_ctx* ctx);
int bp_ctx_sync(bp_ctx* ctx);

/* ---- device memory (HBM-resident vectors, so repeated calls do not re-cross PCIe) ---------------- */
int bp_dev_alloc(bp_ctx* ctx, size_t bytes, void** dptr);
int bp_dev_free(bp_ctx* ctx, void* dptr);
int bp_dev_upload(bp_ctx* ctx, void* dptr, const void* host, size_t bytes);
int bp_dev_download(bp_ctx* ctx, void* host, const void* dptr, size_t bytes);
/* affine points, ark layout -> the engine's resident layout (64 B/point, radix-2^29 Montgomery, packed),
 * device to device; in == out is allowed.  bp_points_export is the inverse. */
int bp_points_import(bp_ctx* ctx, const void* d_in_ark, void* d_out, size_t n);
int bp_points_export(bp_ctx* ctx, const void* d_in, void* d_out_ark, size_t n);

/* ---- VariableBaseMSM::msm -------------------------------------------------------------------------
 * Replaces `<G::Group as VariableBaseMSM>::msm(&bases, &scalars).unwrap().into_affine()`
 * (src/inner_product_proof.rs:104,124,187,202,375; src/r1cs/prover.rs:516,532,546,607,622,635;
 *  src/r1cs/verifier.rs:574,685 — the verifier only tests `is_zero()`, i.e. out == all-zero).
 * Host buffers: bases_xy n points (ark layout), scalars n field elements (Montgomery, or canonical
 * integers if scalars_canonical != 0 — what ark's msm_bigint takes).  out_xy = affine result. */
int bp_msm(bp_ctx* ctx, const uint64_t* bases_xy, const uint64_t* scalars, size_t n, int scalars_canonical, uint64_t out_xy[8]);
/* Same with operands already resident: d_bases in the engine's layout (bp_points_import), d_scalars n x
 * 32 B.  This is the call the timed region of bench.py makes. */
int bp_msm_dev(bp_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, int scalars_canonical, uint64_t out_xy[8]);
/* `count` independent VariableBaseMSM::msm calls in one: job j owns terms [offsets[j], offsets[j + 1]) of bases_xy / scalars (count + 1
 * offsets); out_xy[8 j ..] is exactly what bp_msm(ctx, bases_xy + 8 offsets[j], scalars + 4 offsets[j], n_j, scalars_canonical, ..)
 * returns, whatever the other jobs of the call are.  The identity is all-zero; a job without terms gives the identity.  With
 * scalars_canonical != 0 a scalar may be any 256-bit integer k (the term is k * P); Montgomery input is the ark form.
 * Refused before any work with BP_E_ARG: a null ctx, offsets or out_xy, decreasing offsets, 2^31 terms or more in all, null bases or
 * scalars with a non-zero total; then BP_E_NO_DEVICE on a host-only ctx.  count == 0 returns BP_OK at once (null pointers allowed).
 * Routes, by job length n_j (results never depend on the route):
 *   short     n_j <= BP_TUNE_MSM_BATCH_SHORT: one workgroup per job, bit-plane accumulators (k_ve_tail);
 *   bucketed  up to BP_TUNE_MSM_BATCH_MAX: the job is cut into slices of at most BP_TUNE_MSM_BATCH_SLICE terms, one workgroup per
 *             slice with 15 buckets per 4-bit window in LDS, then one workgroup per job combines the slices (k_msb_accum, k_msb_combine);
 *   single    longer jobs, a job no staging arena could hold, EVERY job of a window-sharded ctx (the shard callbacks keep their
 *             meaning) and EVERY job of a call with fewer than BP_TUNE_MSM_BATCH_MIN_JOBS short and bucketed jobs (a loop is the
 *             faster path there): one after the other inside the call, exactly as bp_msm / bp_msm_dev.
 * Consecutive short and bucketed jobs form a GROUP — what a 256 MB device arena holds; a single-route job in between also ends it —:
 * one staging copy, one sequence of launches on the ctx's stream, BP_MSM_BATCH_WAITS_PER_GROUP host wait, one shared inversion for the
 * affine results.
 * The environment variable ARKBP_MSM_BATCH_ARENA=<bytes> (read per call; values from 1 to 256 MB) narrows the arena budget: it exists so
 * that the cut into groups can be exercised with a few hundred terms; results never depend on it.
 * bp_ctx_msm_batch_stats: jobs per route, groups, and host waits made by the groups (not those of single-route jobs), since ctx creation. */
#define BP_MSM_BATCH_WAITS_PER_GROUP 1
int bp_msm_batch(bp_ctx* ctx, size_t count, const size_t* offsets, const uint64_t* bases_xy, const uint64_t* scalars, int scalars_canonical, uint64_t* out_xy);
/* operands resident: d_bases in the engine's layout (bp_points_import), d_scalars 32 B each; neither buffer is modified */
int bp_msm_batch_dev(bp_ctx* ctx, size_t count, const size_t* offsets, const void* d_bases, const void* d_scalars, int scalars_canonical, uint64_t* out_xy);
int bp_ctx_msm_batch_stats(bp_ctx* ctx, uint64_t* short_jobs, uint64_t* bucketed_jobs, uint64_t* single_jobs, uint64_t* groups, uint64_t* host_waits);
/* test hook, host only: the plan bp_msm_batch makes for `count` jobs under the given knob values (0 = default), csrc/msm_batch.cuh's own
 * functions: route[j] (0 short, 1 bucketed, 2 single: by the job's length alone, on a ctx that is not sharded and a call of enough
 * jobs) and nslices[j] = the slices job j has on the bucketed route, for every job (the default slice cap follows from these jobs); for
 * job `job`: slice_first[s] (a term index relative to offsets[0]) / slice_len[s] for s < nslices[job], and for its term t and window
 * w < 64 digits[64 t + w] = the digit the kernel files the term under (unsigned 4-bit digits, 0 .. 15: no sign, no carry window;
 * scalars_canonical: canonical words of ALL terms).  Every output may be null. */
int bp_debug_msm_batch_plan(size_t count, const size_t* offsets, uint64_t short_max, uint64_t slice_terms, uint64_t batch_max, const uint64_t* scalars_canonical,
                            size_t job, uint8_t* route, uint32_t* nslices, uint32_t* slice_first, uint32_t* slice_len, int8_t* digits);

/* Window-sharded MSM for one large MSM across the GPUs of a node (every GPU holds all bases and scalars): the call
 * accumulates only Pippenger windows [w_lo, w_hi) of the bp_msm_window_count(curve, n) windows and returns that partial
 * sum already weighted by 2^(c*w); the ranks' partials add up to the full MSM (all-gather of one 64-byte point per rank,
 * then bp_host_points_sum).  The window schedule depends only on (curve, n), so all ranks agree on it. */
int bp_msm_window_count(int curve, size_t n, int* windows, int* window_bits);
int bp_msm_dev_windows(bp_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, int scalars_canonical, int w_lo, int w_hi,
                       uint64_t out_xy[8]);

/* MSM over the RESIDENT generator tables (bp_gens_derive / bp_gens_upload), for the prover's and verifier's own msm call sites
 * (e.g. A_I = msm([B_blinding] ++ G[..n] ++ H[..n], ..), src/r1cs/prover.rs:516-559): bases = G[off..off+n) if use_G, then
 * H[off..off+n) if use_H, then n_extra caller points (ark layout); scalars in the same order, (use_G ? n : 0) + (use_H ? n : 0) +
 * n_extra of them (ark Montgomery words, or canonical integers when scalars_canonical).  Nothing but the scalars and the extra
 * points crosses PCIe.  BP_E_GENS_LENGTH when the range exceeds the installed tables. */
int bp_msm_gens(bp_ctx* ctx, int use_G, int use_H, size_t off, size_t n, const uint64_t* extra_bases_xy, size_t n_extra, const uint64_t* scalars,
                int scalars_canonical, uint64_t out_xy[8]);

/* Window-sharded mode for whole computations (north_star: "large proofs shard Pippenger windows across the GPUs of one node with
 * a final point-reduce"): after bp_ctx_set_window_shard(ctx, rank, world, cb, user) EVERY MSM this ctx runs (bp_msm*, the L/R
 * MSMs of bp_ipa_create, the commitment MSMs of the prover, the verifier's mega-check) accumulates only the windows of `rank`
 * and then calls cb(user, xy): the callback must replace the partial point in xy by the sum of all ranks' partials
 * (all-gather over RCCL + bp_host_points_sum) and return 0.  All ranks run the same call sequence on the same inputs and obtain
 * identical results (same proof bytes).  world = 1 switches the mode off.  Calls with an explicit window range
 * (bp_msm_dev_windows) are not affected. */
typedef int (*bp_point_reduce_cb)(void* user, uint64_t xy[8]);
int bp_ctx_set_window_shard(bp_ctx* ctx, int rank, int world, bp_point_reduce_cb cb, void* user);
/* Optional second collective of the sharded mode: cb(user, send, bytes, recv) must fill recv with the `world` ranks' `bytes`-long
 * blocks in rank order (an all-gather) and return 0.  With it (and a power-of-two world) the prover also partitions the
 * inner-product argument: rank r keeps the elements i = r + j*world of a, b, G, H (src/inner_product_proof.rs:139-156,216-225 fold
 * element i with i + n/2 — both on the same rank), a round's L and R are sums of per-rank partial MSMs through the point-reduce
 * callback, and when the vectors are down to the frozen-tail length (BP_TUNE_IPA_FREEZE_LEN) the ranks all-gather the rest once
 * and finish replicated.  Every fold launch then does 1/world of the single-GPU work; proofs stay byte-identical on every rank. */
typedef int (*bp_allgather_cb)(void* user, const void* send, size_t bytes, void* recv);
int bp_ctx_set_shard_allgather(bp_ctx* ctx, bp_allgather_cb cb, void* user);
/* Native collectives: RCCL over xGMI, inside the library (no host callback, no interpreter lock on the data path).
 * One rank calls bp_rccl_unique_id (ncclGetUniqueId) and hands the 128 bytes to the others through whatever bootstrap the host
 * has (a torch.distributed broadcast in bench.py; a Rust host would use its own); then EVERY rank calls bp_ctx_rccl_init on its
 * ctx (ncclCommInitRank: collective, blocks until all ranks arrive).  The ctx is then in the sharded mode of
 * bp_ctx_set_window_shard with BOTH exchanges served by ncclAllGather on the ctx's stream: the per-MSM point-reduce
 * (64-byte affine partials, summed on the host: group addition is not an RCCL reduce op) and the one vector gather of the
 * index-cyclic inner-product argument.  Ranks must issue the same calls in the same order.  The library binds RCCL at run time
 * (the copy already in the process, else the ROCm installation's); BP_E_HIP with a message when there is none.
 * bp_ctx_collective_stats: number of native collectives since init and the host wall time spent in them. */
int bp_rccl_unique_id(uint8_t out[128]);
int bp_ctx_rccl_init(bp_ctx* ctx, const uint8_t unique_id[128], int rank, int world);
int bp_ctx_rccl_shutdown(bp_ctx* ctx);
int bp_ctx_collective_stats(bp_ctx* ctx, uint64_t* count, double* seconds);
/* test hook: one native all-gather of `bytes` bytes per rank (recv: world x bytes) */
int bp_debug_rccl_allgather(bp_ctx* ctx, const uint8_t* send, size_t bytes, uint8_t* recv);

/* ---- InnerProductProof::create -------------------------------------------------------------------
 * Replaces `InnerProductProof::create(transcript, &Q, &G_factors, &H_factors, G_vec, H_vec, a_vec, b_vec)`
 * (src/inner_product_proof.rs:37-239).  Host buffers of length n (a power of two, as the reference
 * asserts at :58-66).  The Merlin transcript stays with the caller: once per halving round the engine
 * hands the callback the affine L, R it would append (`append_point(b"L"|b"R")`, :132-133) and the
 * callback returns u = `challenge_scalar(b"u")` (:135); u^-1 is derived by the engine.  A non-zero
 * return from the callback aborts the call.  Outputs: L_vec, R_vec (lg n points each), a, b. */
typedef int (*bp_challenge_cb)(void* user, const uint64_t L_xy[8], const uint64_t R_xy[8], uint64_t u_out[4]);
int bp_ipa_create(bp_ctx* ctx, const uint64_t Q_xy[8], const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t* G_xy,
                  const uint64_t* H_xy, const uint64_t* a, const uint64_t* b, size_t n, bp_challenge_cb cb, void* user, uint64_t* L_out_xy,
                  uint64_t* R_out_xy, uint64_t a_out[4], uint64_t b_out[4]);

/* The same computation cut at the Fiat-Shamir step, for hosts that keep the transcript on their side without a callback and
 * for the index-cyclic multi-GPU partition (each rank holds the elements i = rank mod world of every vector; a round's L and R
 * are then the sums of the ranks' partial points, see ark_bulletproofs_amd/parallel.py):
 *   bp_ipa_begin       copies the instance to the GPU (the arguments of `create`, :37-46; n a power of two)
 *   bp_ipa_round_LR    L, R of the current round (:78-131 / :166-213), affine ark layout; the host appends them (:132-133)
 *   bp_ipa_round_fold  folds a, b, G, H with the challenge u (:137-155 / :214-224); u^-1 is derived by the engine
 *   bp_ipa_finish      a[0], b[0] once the vectors have length 1 (:226-231)
 *   bp_ipa_export      the current vectors between rounds (n_cur elements each) with the scalars the engine still owes the
 *                      generator vectors: G_true[i] = gamma_G * G[i], H_true[i] = gamma_H * H[i] (uniform rounds fold
 *                      G_R + u^-2 G_L and carry the common factor u instead of multiplying every point by it)
 * One stepping instance per ctx; bp_ipa_begin restarts it. */
int bp_ipa_begin(bp_ctx* ctx, const uint64_t Q_xy[8], const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t* G_xy, const uint64_t* H_xy,
                 const uint64_t* a, const uint64_t* b, size_t n);
int bp_ipa_round_LR(bp_ctx* ctx, uint64_t L_xy[8], uint64_t R_xy[8]);
int bp_ipa_round_fold(bp_ctx* ctx, const uint64_t u[4]);
int bp_ipa_finish(bp_ctx* ctx, uint64_t a[4], uint64_t b[4]);
int bp_ipa_export(bp_ctx* ctx, uint64_t* a, uint64_t* b, uint64_t* G_xy, uint64_t* H_xy, uint64_t gamma_G[4], uint64_t gamma_H[4], size_t* n_cur);

/* ---- InnerProductProof::verify -------------------------------------------------------------------
 * Replaces `proof.verify(n, transcript, G_factors, H_factors, &P, &Q, &G, &H)` (src/inner_product_proof.rs:321-382).
 * The caller replays its transcript (`innerproduct_domain_sep`, `validate_and_append_point(L|R)`, `challenge_scalar(u)`,
 * :266-277) and passes the lg_n challenges in creation order; the engine derives u^2, u^-2, the s vector (:279-311), builds
 * the 1 + 2n + 2 lg_n scalars on the GPU, runs the MSM and compares with P.  Returns BP_OK or BP_E_VERIFICATION. */
int bp_ipa_verify(bp_ctx* ctx, size_t n, const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t P_xy[8], const uint64_t Q_xy[8],
                  const uint64_t* G_xy, const uint64_t* H_xy, const uint64_t* L_xy, const uint64_t* R_xy, size_t lg_n, const uint64_t* challenges,
                  const uint64_t a[4], const uint64_t b[4]);

/* ---- generators -----------------------------------------------------------------------------------
 * bp_gens_derive replaces `BulletproofGens::new(cap, 1)` + `PedersenGens::default()` (src/generators.rs:174-221,
 * 47-66): derives party 0's G/H tables on the host cores and installs them in HBM (resident for the life of
 * the ctx; the reference clones them into fresh Vecs per proof, src/r1cs/prover.rs:796-797).
 * bp_gens_upload installs tables the caller already holds (ark layout). */
int bp_gens_derive(bp_ctx* ctx, size_t gens_capacity);
int bp_gens_upload(bp_ctx* ctx, const uint64_t* G_xy, const uint64_t* H_xy, size_t gens_capacity);
int bp_gens_download(bp_ctx* ctx, uint64_t* G_xy, uint64_t* H_xy, size_t n);
/* Optional: fixed-base tables of G[0..count), H[0..count) for the FIRST fold round of the prover's inner-product argument
 * (src/inner_product_proof.rs:139-156: there the bases are the generator tables themselves, the same for every proof, and the
 * multiplier is one scalar for all elements) — e * 2^(w*j) * G[i] for all windows j and digits e, so that the round becomes
 * ~34 look-ups + mixed adds per point (w = 8) instead of a 130-step double-and-add ladder.  count = the left half of the largest
 * proof: N/2.  window_bits 2..8, or 0 = the widest whose tables fit in budget_bytes (0 = 3/4 of the free device memory); the
 * choice and the table size come back in *window_bits_out / *bytes_out (2^19 bases, w = 8: 146 GB for both vectors on secq256k1).
 * Built on the ctx that owns the generators; bp_gens_share hands them on.  count = 0 frees them.  Results never depend on it.
 * WHICH WIDTHS ARE USED: a table has nwin = 130 / w + 1 windows on secq256k1 (the GLV halves) and 256 / w + 1 on zorro, the last one
 * for the carry of the signed digits, and the fold kernels take a multiplier's digits only when nwin <= 44.  So w = 3 .. 8 serve on
 * secq256k1 and w = 6, 7, 8 on zorro; w = 2 there, and w = 2 .. 5 on zorro, are built (and pass bp_gens_tables_check) but every fold
 * goes through the ladder kernels as if there were no tables.
 * The tables are multiples of the resident generators: bp_gens_upload releases them, the MSM rows and the direct tables below (views of
 * another ctx's tables are let go); bp_gens_derive to the same or a larger capacity extends the same chain and keeps them. */
int bp_gens_fold_tables(bp_ctx* ctx, size_t count, int window_bits, size_t budget_bytes, int* window_bits_out, size_t* bytes_out);
/* The same for ONE RANK of a sharded prover (bp_ctx_set_shard, index-cyclic inner-product argument): only the generators
 * rank + i * world, i < count / world — 1/world of the memory (count = 3N/4 of a 2^22 proof on 8 GPUs at w = 8: 110 GB per rank instead of
 * 876), which is all that rank's slice ever looks up.  These tables belong to the ctx that builds them, whoever owns the generators
 * (bp_gens_share first, then this); bp_gens_tables_check and bp_gens_fold_tables(.., 0, ..) treat them like the whole ones.
 * count must be a multiple of world.  Results never depend on it. */
int bp_gens_fold_tables_slice(bp_ctx* ctx, size_t count, int window_bits, size_t budget_bytes, int rank, int world, int* window_bits_out, size_t* bytes_out);
/* Optional: fixed-base rows 2^(4r) * G[i], 2^(4r) * H[i] (r <= 64: 65 rows, the last one — 2^256 * P — for the carry out of the top
 * window; i < count) and the same for PedersenGens, 65 * 64 B = 4160 bytes per generator and vector (count = 2^20: 8.7 GB).  With them every MSM the prover runs over the generator tables themselves — the commitments A_I, A_O, S
 * (src/r1cs/prover.rs:516-559, 604-649) and the first round's L, R (src/inner_product_proof.rs:83-131), 7/9 of a proof's MSM
 * terms — sorts the digits of ALL Pippenger windows into ONE bucket set (the row supplies the power of two): the per-window costs
 * are paid once, the window is wider (c = 20 at 2^21 terms: 13 mixed adds per term instead of 17-18) and the result needs no
 * doublings.  Skewed scalars (0/1 witness vectors) fall back to the ordinary schedule.  Results never depend on it. */
int bp_gens_msm_tables(bp_ctx* ctx, size_t count, size_t* bytes_out);
/* Optional: build the DIRECT WINDOW TABLES of the small-statement path now (d * 16^w * base for B, B_blinding and the first `count`
 * generators of G and H, 60 KiB per base: count = 8192 is 1 GB) instead of inside the first small proof — e.g. before bp_gens_share,
 * which hands them on (a ctx that shares generators without them builds its own copy on first use).  count is rounded down to what
 * BP_TUNE_DIRECT_MAX and the installed generators allow; count = 0 frees them.  As with the other tables: rebuilding them (a larger
 * count, other generators) on a ctx whose tables are shared is the owner's responsibility.  Results never depend on it. */
int bp_gens_direct_tables(bp_ctx* ctx, size_t count, size_t* bytes_out);
/* Integrity check of both kinds of precomputed tables of the LARGE-statement path (the fold tables and the MSM rows; the direct window
 * tables, the commitment tables and the resident points themselves: bp_gens_direct_tables_check below): every entry is re-derived from its stored neighbours by the chain rule
 * (e * 2^(w*j) * P = (e-1) * 2^(w*j) * P + 2^(w*j) * P, next window = the doubled last entry; MSM rows: next row = 16 * row) with
 * mixed additions / doublings compared projectively, anchored at the resident generators; *bad_fold_entries / *bad_msm_rows (either
 * may be NULL) receive the number of entries that do not fit.  A proof touches only the few rows its challenges select, so a
 * corrupted entry (a bit flip in 150 GB of HBM, a bad build) cannot be found by proving; this finds it, in about the time of one
 * proof.  Tables that are not installed count as 0. */
int bp_gens_tables_check(bp_ctx* ctx, uint64_t* bad_fold_entries, uint64_t* bad_msm_rows);
/* Integrity check of the tables that every small-statement proof, every group of bp_prover_prove_batch, every verdict of
 * bp_verifier_verify_batch and every bp_pedersen_commit_batch read, and of the resident points they are multiples of.  Four kinds:
 *   BP_TABLES_DIRECT     table 4 of bp_debug_tables_ptr: entry E[b][w][d] (w < 64, 1 <= d <= 15) at index (b * 64 + w) * 15 + d - 1,
 *                        bases b = [B, B_blinding | G[0..cap) | H[0..cap)];
 *   BP_TABLES_PC_DIRECT  table 5: the same layout for B and B_blinding alone;
 *   BP_TABLES_PC_WIDE    table 6: entry T[b][w][d] (b < 2, w < 32, d < 256) at index (b * 32 + w) * 256 + d;
 *   BP_TABLES_RESIDENT   the resident points: index 0 = B, 1 = B_blinding, 2 + i = G[i], 2 + gens_capacity + i = H[i].
 * Each entry has ONE rule, evaluated from its STORED affine neighbours with a complete mixed addition and a projective comparison
 * (no inversion; the builders use doublings and ladders):
 *   tables 4, 5:  E[b][0][1] == resident base b;   E[b][w][1] == E[b][w-1][15] + E[b][w-1][1] for w >= 1;
 *                 E[b][w][d] == E[b][w][d-1] + E[b][w][1] for d >= 2;   and no entry is the identity (all-zero words fail);
 *   table 6:      T[b][w][0] is the identity (all-zero words);   T[b][0][1] == base b;
 *                 T[b][w][1] == T[b][w-1][255] + T[b][w-1][1] for w >= 1;   T[b][w][d] == T[b][w][d-1] + T[b][w][1] for d >= 2;
 *   resident:     the point satisfies the equation of the ctx's curve and is not the identity.
 * In all four an entry must also hold the canonical representatives of its coordinates (values below the modulus), as every kernel
 * stores them.  Every table entry is some other entry's neighbour except the last digit of a base's last window, so ONE wrong entry
 * usually counts several times: itself and the entries derived from it (a unit entry d = 1: the 14 other digits of its window and the
 * next window's unit).  Off-curve words, the identity and arbitrary bit patterns all come out as "bad" and nothing else.
 * bad[k]: the entries of kind k that fail their own rule; first_bad[k]: the smallest index of one, UINT64_MAX when there is none;
 * checked[k]: the entries examined — 0 for a table that is not built, so that "0 bad" and "nothing looked at" differ.  Each of the
 * three arrays may be NULL.  Nothing is built or rebuilt: the call reads what is there, on the ctx's stream, with one copy back and
 * one wait after the last launch.  A ctx that shares generators (bp_gens_share) checks the owner's points and direct tables through
 * its view (tables 5 and 6 are each ctx's own).
 * WHAT IT CANNOT SEE: BP_TABLES_RESIDENT knows a point only as a point of the curve — two on-curve generators swapped in the
 * resident table, or any other valid point in a generator's place, pass it; the anchors of table 4 then fail (for generators within
 * the tables' reach), and generators beyond the reach are not pinned by anything here.  B and B_blinding are pinned by three anchors.
 * The resident points themselves are pinned by bp_gens_check (derived generators, against the chain) and bp_gens_digest (any
 * generators, against the caller's own copy) below.
 * BP_E_ARG for a null ctx, BP_E_NO_DEVICE for a host-only ctx. */
#define BP_TABLES_DIRECT 0      /* bp_debug_tables_ptr which = 4 */
#define BP_TABLES_PC_DIRECT 1   /* which = 5 */
#define BP_TABLES_PC_WIDE 2     /* which = 6 */
#define BP_TABLES_RESIDENT 3    /* the resident points themselves: B, B_blinding, G[0..gens_cap), H[0..gens_cap) */
#define BP_TABLES_KINDS 4
int bp_gens_direct_tables_check(bp_ctx* ctx, uint64_t bad[BP_TABLES_KINDS], uint64_t first_bad[BP_TABLES_KINDS], uint64_t checked[BP_TABLES_KINDS]);
/* The anchors of both table checks — the resident generators G[0..gens_capacity), H[0..gens_capacity) and the resident pair B,
 * B_blinding — against what they should be, word for word (every kernel stores the canonical representatives, so equal points have
 * equal words).  Three kinds:
 *   BP_GENS_G, BP_GENS_H  on a ctx whose generators were DERIVED (bp_gens_derive, or bp_gens_share from such a ctx): party 0's
 *                         GeneratorsChain is walked again as bp_gens_derive walks it — the host draws the ChaCha20 word stream, the GPU
 *                         tests the attempts, the first successes are gathered in stream order — in chunks of at most 2^16 attempts, into
 *                         scratch (a few MB at any capacity), and each chunk is compared with the resident slice.  checked = gens_capacity.
 *                         Caller-installed generators (bp_gens_upload, or a view of such an owner) have no chain to be compared with:
 *                         checked = 0, bad = 0, first_bad = UINT64_MAX and BP_OK — "0 = nothing to compare with", as "0 = not built"
 *                         in the table checks; bp_gens_digest below pins those.
 *   BP_GENS_PEDERSEN      always: the resident pair (index 0 = B, 1 = B_blinding) against the pair the ctx holds on the host
 *                         (bp_ctx_pedersen_gens: PedersenGens::default() or the installed one).  checked = 2.
 * bad[k]: the entries whose resident words differ; first_bad[k]: the smallest such index, UINT64_MAX when there is none.  Two swapped
 * generators count 2; any other point, on the curve or not, in a generator's place counts 1.  The call reads and compares: it builds,
 * rebuilds and repairs nothing, and the resident table is never written.  A ctx that shares generators checks the owner's points
 * through its view.  The walk waits for the GPU once per chunk (the same copies of the attempts' verdicts deriving waits for); the
 * counters come back with one copy after the last launch.  It costs about what bp_gens_derive costs.
 * BP_E_ARG for a null ctx or report, BP_E_NO_DEVICE for a host-only ctx, BP_E_GENS_LENGTH when no generators are installed. */
#define BP_GENS_G 0
#define BP_GENS_H 1
#define BP_GENS_PEDERSEN 2
#define BP_GENS_KINDS 3
typedef struct bp_gens_report {
    uint64_t checked[BP_GENS_KINDS];   /* entries compared; 0 = nothing to compare with */
    uint64_t bad[BP_GENS_KINDS];       /* entries whose resident words differ */
    uint64_t first_bad[BP_GENS_KINDS]; /* smallest such index, UINT64_MAX when none */
} bp_gens_report;
int bp_gens_check(bp_ctx* ctx, bp_gens_report* out);
/* A digest of the resident pair and of G[0..n), H[0..n) that the caller can reproduce from its own copy of the points
 * (bp_host_gens_digest, or a dozen lines over any SHA3-256): it pins caller-installed generators, and lets the ranks of a multi-GPU
 * run, or an owner ctx and its views, assert that they hold the same points by comparing 32 bytes.
 *   H = SHA3-256 (FIPS 202).  P64 = a point's 64 bytes in the ark layout, x then y, each four little-endian u64 Montgomery words: the
 *   bytes bp_gens_download and bp_ctx_pedersen_gens return.  LE64 = 8 bytes, little-endian.
 *   leaf(tag, i, P)      = H("arkbp-gens-leaf-v1" || u8 tag || LE64(i) || P64)       tag 0 = the pair (B, B_blinding), 1 = G, 2 = H
 *   node(level, j, a, b) = H("arkbp-gens-node-v1" || u8 level || LE64(j) || a || b)
 *   a vector's root: level 0 is its leaves; level k+1 has ceil(m / 2) nodes, node j = node(k + 1, j, N[2j], N[2j+1]) when 2j + 1 < m,
 *   else N[2j] carried up unchanged; until one node remains (a vector of one point: its leaf).
 *   root = H("arkbp-gens-root-v1" || u8 curve || LE64(n) || pair root || G root || H root)
 * out = root | pair root | G root | H root, 32 bytes each.  On the device one lane hashes one leaf or one node (every message is one
 * Keccak-f block); one copy back of 128 bytes, one wait.  A ctx that shares generators digests the owner's points and pair.
 * bp_gens_digest: 1 <= n <= gens_capacity; n == 0 or a null pointer is BP_E_ARG, n > gens_capacity BP_E_GENS_LENGTH, a host-only ctx
 * BP_E_NO_DEVICE.
 * bp_host_gens_digest (host only): the same over the caller's points.  It validates nothing about them — it hashes bytes; BP_E_ARG
 * for a null pointer, n == 0 or an unknown curve. */
int bp_gens_digest(bp_ctx* ctx, size_t n, uint8_t out[128]);
int bp_host_gens_digest(int curve, const uint64_t* G_xy, const uint64_t* H_xy, size_t n, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8], uint8_t out[128]);
/* test hook: device address and size in bytes of a table; NULL / 0 when it is not built.  which:
 *   0 / 1  fold tables of G / H, layout [window][digit-1][i] x 64 B;
 *   2 / 3  MSM rows of G / H, layout [row][i] x 64 B;
 *   4      the direct window tables of the small-statement path (bp_gens_direct_tables; cap = bp_ctx_direct_stats' bases per vector):
 *          (2 + 2 cap) * 61440 bytes, bases [B, B_blinding | G[0..cap) | H[0..cap)], entry ((base * 64 + w) * 15 + d - 1) x 64 B
 *          = d * 16^w * base for w < 64, 1 <= d <= 15 (no entry is the identity).  A ctx that shares generators (bp_gens_share)
 *          reports the owner's address;
 *   5      the direct window tables of B, B_blinding alone that batches of up to 4096 commitments read: 2 bases, layout as 4;
 *   6      the 8-bit tables that larger commitment batches read: layout [b < 2][w < 32][d < 256] x 64 B = d * 256^w * base_b, b = 0
 *          for B, 1 for B_blinding; d = 0 is the identity.
 *   5 and 6 exist once the ctx has run its first bp_pedersen_commit_batch.
 *   7      the resident points B, B_blinding (128 bytes); 8 / 9: the resident generators G / H, gens_capacity x 64 B — what the tables
 *          are anchored at and BP_TABLES_RESIDENT of bp_gens_direct_tables_check examines (the owner's, on a ctx that shares them).
 * Every entry is an affine point in the RESIDENT layout: bp_points_export turns entries into ark words (the identity: all zero). */
int bp_debug_tables_ptr(bp_ctx* ctx, int which, void** dptr, size_t* nbytes);
/* test hook: `njobs` (1 .. 6) sums over the direct window tables through the prover's own msm_direct (k_dt_accum, k_dt_finish, the
 * host's sum of partial points), as commit_direct and the rounds of the inner-product argument launch them.
 * desc: BP_DEBUG_DT_DESC_WORDS words per job = nseg (0 .. 3), has_imm (0 / 1), imm_base, then (base0, count, format, fold_n, fold_hi)
 * for each of three segments (those past nseg are ignored).  Bases are indices into table 4 of bp_debug_tables_ptr: 0 = B,
 * 1 = B_blinding, 2 + i = G[i], 2 + cap + i = H[i].  Term j of a segment is element t = j when fold_n = 0, else
 * t = (j / fold_n) * 2 * fold_n + j % fold_n + (fold_hi ? fold_n : 0); it multiplies base base0 + t by scalar t of the segment's
 * array scalars[3 * job + seg] (4 words each, scalar_lens[3 * job + seg] of them: at least the last visited element + 1).
 * format 0: any 256-bit integers, used digit by digit as they are (an integer k >= r still gives (k mod r) * base);
 * format 1: ark Montgomery words, which the hook turns into the resident form first (k_scalars_import); format 2: ark Montgomery
 * words, read by the kernel as they are.  With has_imm the job's term 0 is imm[4 * job ..] (a 256-bit integer, as format 0) times
 * base imm_base.  out_xy: one affine point per job, ark layout, all-zero words for the identity.  *workgroups (may be
 * NULL): k_dt_accum's workgroups per job in this launch — 1: its points are the results; 2 .. 16: the host added the partial
 * points; more: k_dt_finish did.
 * BP_E_ARG — and nothing launched — when the tables are not built, a job has no terms, a used segment has count 0, a format is
 * unknown, a scalar array is too short, or any element a job would visit lies outside [0, 2 + 2 cap). */
#define BP_DEBUG_DT_DESC_WORDS 18
int bp_debug_msm_direct(bp_ctx* ctx, size_t njobs, const uint32_t* desc, const uint64_t* imm, const uint64_t* const* scalars, const size_t* scalar_lens,
                        uint64_t* out_xy, uint32_t* workgroups);
/* test hook: two variable-base MSMs of n terms each through the prover's own msm_run_pair, as the rounds of the inner-product argument
 * call it.  Job j (0, 1) reads its bases as up to BP_DEBUG_MSM_PAIR_RUNS runs: run r is base_counts[j * RUNS + r] points (resident layout,
 * bp_points_import) at device pointer base_ptrs[j * RUNS + r]; the first count of 0 ends the job's runs, and they must add up to n.
 * d_scalars[j]: n device scalars of 4 words (ark Montgomery words, or integers below r with canonical = 1).  latency_first = 0
 * runs exactly the schedule the prover gets; 1 sets what the bp_msm* entry points set for the duration of the call (the
 * latency-first schedule, which on secq256k1 takes mid-size MSMs through the GLV split and therefore declines the pairing).
 * out_xy: the two affine sums, 8 ark words each, all zero for the identity.  bp_ctx_msm_pair_stats tells whether the call paired. */
#define BP_DEBUG_MSM_PAIR_RUNS 6
int bp_debug_msm_pair(bp_ctx* ctx, const void* const* base_ptrs, const size_t* base_counts, const void* const* d_scalars, size_t n, int canonical, int latency_first,
                      uint64_t* out_xy);
/* test hook: ONE fold of the inner-product argument through the prover's own launchers (launch_uniform_fold, launch_tab_fold,
 * launch_tab_fold2 and the shared-inversion epilogue) with caller-chosen multipliers — the multipliers themselves (ark Montgomery
 * words), not the challenge u.  n outputs per vector.  route:
 *   BP_DEBUG_FOLD_LADDER      out[i] = V[n+i] + t_V * V[i] over the caller's points G_xy, H_xy (2n each, ark layout): the GLV ladder on
 *                             secq256k1, the NAF ladder on zorro; BP_TUNE_FOLD_QUAD_MAX and BP_TUNE_FOLD_BATCH_MIN apply as in the prover;
 *   BP_DEBUG_FOLD_LADDER_NAF  the same with the NAF ladder on secq256k1 as well (what a multiplier without a short GLV split takes);
 *   BP_DEBUG_FOLD_TAB         out[i] = Gen[n+i] + t_V * Gen[i] from the fold tables and the resident generators (G_xy, H_xy unused);
 *   BP_DEBUG_FOLD_TAB2        out[i] = Gen[3n+i] + tV * Gen[n+i] + t2V * Gen[2n+i] + tV*t2V * Gen[i]: two rounds from the tables.
 * Gen[j] is generator gens_first + j * gens_stride.  gens_first = 0, gens_stride = 1: the whole vectors, whose upper halves are read
 * in place; anything else: an index-cyclic slice, gathered into a compact copy first, as the sharded prover does.  t2G, t2H: TAB2 only.
 * G_out_xy, H_out_xy: n affine points each, ark layout, all-zero words for the identity.
 * *took: bit 0 a GLV ladder ran, 1 a NAF ladder, 2 in the quad form, 3 the shared-inversion epilogue (k_ipa_fold_finish), 4
 * k_ipa_fold_tab, 5 k_ipa_fold_tab2; 0: the launcher declined (a table width whose digits do not fit, see bp_gens_fold_tables; n < 64
 * for TAB) and nothing was written.
 * BP_E_ARG — and nothing launched — when a table route finds no tables, or an element would lie outside the tables' columns or the
 * installed generators. */
#define BP_DEBUG_FOLD_LADDER 0
#define BP_DEBUG_FOLD_LADDER_NAF 1
#define BP_DEBUG_FOLD_TAB 2
#define BP_DEBUG_FOLD_TAB2 3
int bp_debug_fold(bp_ctx* ctx, int route, size_t n, const uint64_t tG[4], const uint64_t tH[4], const uint64_t t2G[4], const uint64_t t2H[4], uint32_t gens_first,
                  uint32_t gens_stride, const uint64_t* G_xy, const uint64_t* H_xy, uint64_t* G_out_xy, uint64_t* H_out_xy, uint32_t* took);
/* PedersenGens::default() -> (B, B_blinding); host only */
int bp_pedersen_gens(int curve, uint64_t B_xy[8], uint64_t B_blinding_xy[8]);
/* `PedersenGens { pub B, pub B_blinding }` (src/generators.rs:27-36) of the caller's choice for everything this ctx does: the pc_gens
 * argument of `verifier.verify(&proof, &pc_gens, &bp_gens)` (verifier.rs:549-557) and `batch_verify(prng, instances, pc_gens, bp_gens)`
 * (:604-691), the bases of bp_pedersen_commit_batch, and the pair that provers committing or proving on this ctx must hold
 * (bp_prover_new_gens).  Both pointers NULL: back to PedersenGens::default().  A ctx that never installs holds the default pair.
 * The reference validates nothing here; the engine's affine tables cannot hold an identity entry, so BP_E_ARG — and nothing
 * changed — for exactly one null pointer, a point off the ctx's curve, a coordinate at or above p, or the identity (all-zero
 * words).  Any other pair is accepted, B == B_blinding included.  BP_E_NO_DEVICE on a host-only ctx; BP_E_ARG on a ctx that holds
 * another ctx's generators (bp_gens_share): the owner installs BEFORE it shares and the view receives the owner's pair.  An install
 * on an owner whose tables other ctxs already view is the owner's responsibility, as with the other tables: share again afterwards.
 * The pair survives bp_gens_derive (to any capacity) and bp_gens_upload.  Only what was computed from the pair is touched: bases 0
 * and 1 of the direct window tables and the Pedersen rows of bp_gens_msm_tables are rebuilt in place if built, the two commitment
 * tables (BP_TABLES_PC_DIRECT, BP_TABLES_PC_WIDE) are dropped and come back on next use; the fold tables, the G/H rows and the G/H
 * part of the direct tables are neither read nor written.  One host wait. */
int bp_pedersen_gens_install(bp_ctx* ctx, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8]);
/* what the ctx holds now; is_default = 1 when that is PedersenGens::default().  Any output may be NULL.  Host only. */
int bp_ctx_pedersen_gens(bp_ctx* ctx, uint64_t B_xy[8], uint64_t B_blinding_xy[8], int* is_default);
/* GeneratorsChain for label 'G'|'H' || LE32(party) (src/generators.rs:71-121), first `count` points; host only */
int bp_host_derive_generators(int curve, int which_H, uint32_t party, size_t count, uint64_t* out_xy);

/* ---- host transcript: merlin::Transcript + TranscriptProtocol (src/transcript.rs:45-102); host only ---- */
void* bp_transcript_new(const uint8_t* label, size_t n);
void bp_transcript_free(void* t);
void bp_transcript_append_message(void* t, const char* label, const uint8_t* msg, size_t n);
void bp_transcript_challenge_bytes(void* t, const char* label, uint8_t* out, size_t n);
int bp_transcript_append_point(int curve, void* t, const char* label, const uint64_t xy[8]);
int bp_transcript_challenge_scalar(int curve, void* t, const char* label, uint64_t out[4]);
int bp_host_sha3_512(const uint8_t* msg, size_t n, uint8_t out[64]);
/* test hook, host only: the prover's TranscriptRng (src/r1cs/prover.rs:483-494) then `count` Fr::rand draws; lanes = 1 scalar
 * path (one 32-byte seed), lanes = 8 the AVX-512 x8 stream (8 seeds; out = 8 x count scalars; BP_E_ARG if unavailable) */
int bp_debug_rng_draws(int curve, void* transcript, const uint64_t* witness, size_t nw, const uint8_t* seeds, int lanes, size_t count,
                       uint64_t* out);
/* Test hook of the lockstep transcript path of batch verification (host::StrobeX8; the eight verifier transcripts of a group take
 * their commitments through AVX-512 Keccak-f x8): appends `npts` points under `label` to each of the `lanes` (2..8) transcripts, which
 * must all be in the state of transcripts[0]; points_xy = [lane][npts][8].  The result must equal bp_transcript_append_point applied
 * lane by lane.  BP_E_ARG when the host has no AVX-512 (the product then takes the scalar path). */
int bp_debug_append_points_x8(int curve, void* const* transcripts, int lanes, const char* label, const uint64_t* points_xy, size_t npts);
/* Test hook of the rest of the lockstep replay (gather / same-message append / challenge / scatter of host::StrobeX8): the EIGHT
 * transcripts — any contents, but at the same STROBE position — take `msg` under `msg_label`, then give `nbytes` (1..64) challenge bytes
 * each under `chal_label`; out = [8][nbytes].  Must equal bp_transcript_append_message + bp_transcript_challenge_bytes lane by lane,
 * and leave the transcripts in the same states.  BP_E_ARG without AVX-512 or when the positions differ. */
int bp_debug_challenge_x8(void* const* transcripts, const char* msg_label, const uint8_t* msg, size_t msg_len, const char* chal_label, size_t nbytes,
                          uint8_t* out);
/* group sum of affine points on the host (the point-reduce after an all-gather of per-GPU partials) */
int bp_host_points_sum(int curve, const uint64_t* pts_xy, size_t count, uint64_t out_xy[8]);

/* ---- r1cs::Prover::prove -------------------------------------------------------------------------
 * Replaces `Prover::new` + commits + gadget + `prove(prng, bp_gens)` (src/r1cs/prover.rs:291-341, 444-831)
 * for the statement families the reference's tests and benches build ("scenarios": 0 k-shuffle
 * benches/r1cs_secq256k1.rs:34-112, 1 range proof tests/r1cs_secq256k1.rs:361-445, 2 example gadget
 * :216-267, 3 square chain and 4 multi-range: this build's synthetic large circuits).  params: 8 u64
 * (scenario-specific), seed: ChaCha20 seed of the external prng.  Outputs: compressed proof bytes
 * (`R1CSProof::to_bytes`, src/r1cs/proof.rs:74-81), the V commitments, scenario publics.
 * timing[8] (seconds): [0] inside prove(), [1] statement construction, [2] TranscriptRng draws, [3] uploads,
 * [4] commitment MSMs, [5] flattened_constraints, [6] polynomial kernels, [7] inner-product argument. */
int bp_r1cs_prove_scenario(bp_ctx* ctx, int scenario, const uint64_t* params, const uint8_t seed[32], uint8_t* proof_out, size_t* proof_len,
                           uint64_t* commit_xy, size_t m_cap, size_t* m_out, uint64_t* publics, size_t* npub, double* timing);

/* `PedersenGens::commit` (src/generators.rs:39-44) for m (value, blinding) pairs at once: out[i] = v[i]*B + blind[i]*B_blinding
 * with the ctx's bases (PedersenGens::default() unless bp_pedersen_gens_install put others there), by fixed-base window tables on the GPU.  v, blind: m x 4 words (ark layout);
 * out_xy: m x 8 words (affine, ark layout; the identity is all-zero). */
int bp_pedersen_commit_batch(bp_ctx* ctx, const uint64_t* v, const uint64_t* blind, size_t m, uint64_t* out_xy);

/* Statement handles: `Prover::new` + `commit`s + gadget (src/r1cs/prover.rs:291-341; host only, no GPU) separated from
 * `prove()` so that a service can keep several proofs in flight: the per-proof TranscriptRng chain (8 Keccak-f per
 * multiplier, strictly sequential inside one proof) of one statement overlaps the GPU work of the others.  Each in-flight
 * proof uses its own bp_ctx (stream + workspaces); bp_gens_share lets them all read one resident copy of the tables.
 * bp_stmt_prove consumes the statement (`prove(self, ..)`); timing as in bp_r1cs_prove_scenario ([1] = 0). */
typedef struct bp_stmt bp_stmt;
struct bp_cs;
/* a statement IS a prover handle (scenario code records through the same recorder as bp_cs_*): bp_stmt_prove / _precompute are
 * bp_prover_prove / _precompute on it */
struct bp_cs* bp_stmt_as_prover(bp_stmt* stmt);
int bp_stmt_prover_create(int curve, int scenario, const uint64_t* params, const uint8_t seed[32], bp_stmt** out);
/* same, with the statement's Pedersen commitments (`Prover::commit`, src/r1cs/prover.rs:327-341) computed on ctx's GPU in one
 * batch; the curve and the Pedersen pair are ctx's.  With the default pair: identical statement (same transcript, same commitments)
 * as the host-only constructor, which stays on PedersenGens::default(). */
int bp_stmt_prover_create_dev(bp_ctx* ctx, int scenario, const uint64_t* params, const uint8_t seed[32], bp_stmt** out);
void bp_stmt_free(bp_stmt* stmt);
int bp_stmt_info(bp_stmt* stmt, uint64_t* commit_xy, size_t m_cap, size_t* m_out, uint64_t* publics, size_t* npub, size_t* multipliers,
                 size_t* constraints);
/* Optional, host only (no ctx): runs the head of prove() — `m`, TranscriptRng construction and the phase-1 blinding draws
 * (src/r1cs/prover.rs:466-513) — so it can overlap other proofs' GPU work; bp_stmt_prove continues from that state. */
int bp_stmt_precompute(bp_stmt* stmt);
/* Batch form: statements of the same curve; every group of 8 with equal multiplier / commitment counts advances its eight
 * TranscriptRng chains in lockstep in AVX-512 lanes (Keccak-f x8), producing exactly the per-statement streams. */
int bp_stmt_precompute_batch(bp_stmt** stmts, size_t count);
int bp_stmt_prove(bp_ctx* ctx, bp_stmt* stmt, uint8_t* proof_out, size_t* proof_len, double* timing);
int bp_gens_share(bp_ctx* dst, bp_ctx* src);

/* ---- r1cs::ConstraintSystem / Prover / Verifier for the caller's OWN gadgets ------------------------------------------------
 * The reference's public surface for circuits is the trait API of src/r1cs/constraint_system.rs:19-135 (`multiply`, `allocate`,
 * `allocate_multiplier`, `constrain`, `specify_randomized_constraints`, `challenge_scalar`), recorded by `Prover` (src/r1cs/
 * prover.rs:96-268) and `Verifier` (src/r1cs/verifier.rs:69-224) and consumed by `prove` (prover.rs:444-831), `verify`
 * (verifier.rs:549-600) and `batch_verify` (verifier.rs:604-691).  A bp_cs is one such recorder; everything it records reaches the
 * same GPU path the scenario entry points use (they are callers of this API): the fused prover with GPU flattened constraints, the
 * TranscriptRng x8 pipeline, circuit templates and the block pipeline of batch verification — for single-phase and randomized
 * (two-phase) circuits alike.
 *
 *   Variable            bp_var {kind, index}: r1cs::Variable::{Committed(i), MultiplierLeft(i), MultiplierRight(i),
 *                       MultiplierOutput(i), One()} (src/r1cs/linear_combination.rs:12-24)
 *   LinearCombination   n terms as two parallel arrays: vars[n], coefs[4n] (ark Montgomery words)
 *   transcript          a bp_transcript_* handle, BORROWED for the life of the bp_cs like `T: BorrowMut<Transcript>`: the recorder
 *                       appends to it exactly what the reference appends, so afterwards it is in the state
 *                       `prove_and_return_transcript` / `verify_and_return_transcript` would return.  Hosts with their own merlin
 *                       move the 203-byte STROBE state across with bp_transcript_export_state / bp_transcript_import_state.
 *   external rng        `prove(prng, ..)` uses its rng for ONE thing: the 32 bytes of TranscriptRngBuilder::finalize (prover.rs:493);
 *                       the caller draws them (`prng.fill_bytes(&mut [0u8; 32])`) and passes them as rng_bytes.
 *   alphas              batch_verify's `G::ScalarField::rand(prng)` per instance (verifier.rs:649): drawn by the caller, in
 *                       instance order (ark Montgomery words); NULL = all ones (what Verifier::verify amounts to).
 * A bp_cs is not thread-safe; distinct handles are independent.  Errors are the reference's: BP_E_MISSING <-> MissingAssignment,
 * BP_E_VERIFICATION, BP_E_FORMAT, BP_E_GENS_LENGTH; a non-zero return of a randomized-constraint callback is passed through
 * (`R1CSError::GadgetError`). */
typedef struct bp_cs bp_cs;
#define BP_VAR_COMMITTED 0
#define BP_VAR_MULT_LEFT 1
#define BP_VAR_MULT_RIGHT 2
#define BP_VAR_MULT_OUT 3
#define BP_VAR_ONE 4
typedef struct bp_var { uint32_t kind; uint32_t index; } bp_var;

/* `Prover::new(&pc_gens, transcript)` (prover.rs:291-308) / `Verifier::new(transcript)` (verifier.rs:252-263): appends the r1cs
 * domain separator.  pc_gens is PedersenGens::default() (bp_pedersen_gens).  A verifier holds no pair: `Verifier::new` takes none,
 * and every verifying entry point uses the ctx's (bp_pedersen_gens_install). */
int bp_prover_new(int curve, void* transcript, bp_cs** out);
/* `Prover::new(&pc_gens, transcript)` (prover.rs:291-308) with the caller's pc_gens, validated as in bp_pedersen_gens_install
 * (BP_E_ARG for a null pointer, a point off the curve, a coordinate at or above p, the identity).  The handle keeps its pair:
 * bp_prover_commit without a ctx commits under it on the host; with a ctx — and in bp_prover_commit_batch, bp_prover_prove and
 * bp_prover_prove_batch — the ctx must hold the same pair, otherwise BP_E_ARG (the message names the instance), nothing is appended
 * to a transcript and no prover is consumed. */
int bp_prover_new_gens(int curve, void* transcript, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8], bp_cs** out);
int bp_verifier_new(int curve, void* transcript, bp_cs** out);
void bp_cs_free(bp_cs* cs);
/* `ConstraintSystem::transcript()` (constraint_system.rs:21): the recorder's transcript, for gadgets that bind extra data */
void* bp_cs_transcript(bp_cs* cs);
/* `Prover::commit(v, v_blinding) -> (V, Variable)` (prover.rs:327-341) for `count` values in order; with a ctx the Pedersen
 * commitments are one GPU batch (bp_pedersen_commit_batch), otherwise host arithmetic.  V_xy_out / vars_out may be NULL. */
int bp_prover_commit(bp_cs* prover, bp_ctx* ctx_or_null, const uint64_t* v, const uint64_t* v_blinding, size_t count, uint64_t* V_xy_out, bp_var* vars_out);
/* `Verifier::commit(V) -> Variable` (verifier.rs:279-287) for `count` commitments in order */
int bp_verifier_commit(bp_cs* verifier, const uint64_t* V_xy, size_t count, bp_var* vars_out);

/* ---- Commitments from the wire ----------------------------------------------------------------------------------------------
 * The 33-byte encoding is ark-serialize's `serialize_compressed` of a short-Weierstrass affine point: x as 32 little-endian bytes,
 * then a flag byte (0x80: y is the larger root, 0x40: the identity, then x = 0).  A decoder rejects: flag bits 0..5 set, both flags
 * set, x >= p, the identity flag with x != 0, x not on the curve.
 *
 * bp_points_decompress: n encodings -> affine ark words (x || y, 8 words per point), the square roots on the GPU in one launch; on
 * a host-only ctx (bp_debug_ctx_create_hostonly) on the host pool.  A rejected entry gives all-zero words and ok = 0; the identity
 * gives all-zero words and ok = 1.
 * bp_points_compress (host only): affine ark words -> encodings; all-zero words are the identity.  BP_E_ARG for a point off the curve. */
int bp_points_decompress(bp_ctx* ctx, const uint8_t* c33, size_t n, uint64_t* out_xy, uint8_t* ok);
int bp_points_compress(int curve, const uint64_t* xy, size_t n, uint8_t* c33_out);
/* `V = G::deserialize_compressed(bytes)?; verifier.commit(V)` for many verifiers in one call: verifier k receives the next
 * m_each[k] encodings of c33, in order.  vars_out (sum of m_each entries) and status (count entries) may be NULL.  BP_E_ARG, with
 * nothing changed: a handle that is not a live verifier of the ctx's curve, a handle given twice, c33 NULL with encodings to read.
 *
 * defer == 0: all encodings are decoded in one launch (one copy back), then every verifier commits its points in order on the
 * ctx's host pool: the state bp_verifier_commit leaves.  A verifier with a rejected encoding gets status[k] = BP_E_FORMAT and
 * receives none of its commitments from this call (handle and transcript untouched); the others proceed.  Returns the first
 * non-zero status in instance order.
 *
 * defer != 0: nothing is decoded, no transcript is touched.  The handle stores the bytes as PENDING wire commitments (vars_out
 * still receives Committed(i) in order) with a copy of its transcript's state.  While commitments are pending bp_verifier_commit
 * and the immediate form are BP_E_ARG; a further deferred call is allowed while the transcript is unchanged; recording calls
 * (bp_cs_multiply, bp_cs_constrain*, bp_cs_allocate*, bp_cs_specify_randomized_constraints) and bp_verifier_new_like (the new handle
 * starts with none) are allowed.  The transcript is borrowed: whoever appends to it while commitments are pending changes the order
 * the reference would see, so every use of pending commitments first compares the transcript with the stored state and a difference
 * is BP_E_ARG (the message names the instance).  A gadget that binds extra data through bp_cs_transcript calls
 * bp_verifier_materialize first.
 *
 * Every verifying entry point (bp_verifier_verify, bp_r1cs_batch_verify, bp_verifier_verify_batch, bp_r1cs_batch_verify_locate)
 * accepts handles with pending commitments: after its up-front checks it decodes the pending commitments of all instances in one
 * launch and commits them on the pool.  A rejected encoding is that instance's BP_E_FORMAT, reported before any error of the proof
 * bytes.  A batch of like-instances (bp_verifier_new_like) that the device front end takes, where every instance holds only pending
 * commitments and the same number of them, never decodes them on the host at all: k_vfe_points reads the encodings.
 *
 * bp_verifier_materialize: decodes and commits the handle's pending commitments now (GPU with a ctx, host roots with NULL or a
 * host-only ctx).  BP_E_FORMAT for a rejected encoding (the bytes stay pending); BP_OK when nothing is pending.
 * bp_ctx_commit_wire_stats: wire commitments decoded since ctx creation by k_vfe_points (the device front end) / by
 * k_points_decompress (the immediate form, materialize, the verify prologue) / by host square roots (host-only ctx, and the m
 * commitments of instance 0 a two-phase device batch rehearses). */
int bp_verifier_commit_compressed_batch(bp_ctx* ctx, size_t count, bp_cs* const* verifiers, const size_t* m_each, const uint8_t* c33, int defer, bp_var* vars_out,
                                        int* status);
int bp_verifier_materialize(bp_ctx* ctx_or_null, bp_cs* verifier);
int bp_ctx_commit_wire_stats(bp_ctx* ctx, uint64_t* by_front_end, uint64_t* by_prologue_gpu, uint64_t* on_host);
/* `multiply(left, right) -> (l, r, o)` (constraint_system.rs:30-41; prover.rs:103-133, verifier.rs:74-98) */
int bp_cs_multiply(bp_cs* cs, const bp_var* left_vars, const uint64_t* left_coefs, size_t n_left, const bp_var* right_vars, const uint64_t* right_coefs,
                   size_t n_right, bp_var out[3]);
/* `allocate(assignment)` (constraint_system.rs:43-54; prover.rs:135-157, verifier.rs:100-116); NULL = None (BP_E_MISSING for a prover) */
int bp_cs_allocate(bp_cs* cs, const uint64_t* assignment_or_null, bp_var* out);
/* `allocate_multiplier(input_assignments)` (constraint_system.rs:56-65; prover.rs:159-183, verifier.rs:118-138) */
int bp_cs_allocate_multiplier(bp_cs* cs, const uint64_t* left_or_null, const uint64_t* right_or_null, bp_var out[3]);
/* `constrain(lc)` (constraint_system.rs:70-75) */
int bp_cs_constrain(bp_cs* cs, const bp_var* vars, const uint64_t* coefs, size_t n);
/* bulk forms for large gadgets (one FFI call instead of one per gate): `count` allocate_multiplier calls (left / right: count x 4
 * words, NULL for a verifier; the multipliers get indices first_index .. first_index + count - 1), and `nconstraints` constrain
 * calls in CSR form (constraint q owns terms [offsets[q], offsets[q+1]) of vars / coefs) */
int bp_cs_allocate_multipliers(bp_cs* cs, const uint64_t* left, const uint64_t* right, size_t count, uint32_t* first_index);
int bp_cs_constrain_many(bp_cs* cs, const bp_var* vars, const uint64_t* coefs, const size_t* offsets, size_t nconstraints);
/* `specify_randomized_constraints(callback)` (constraint_system.rs:96-109; prover.rs:211-217, verifier.rs:172-178): cb runs in the
 * randomized phase of prove / verify (prover.rs:418-441, verifier.rs:353-376) with the recorder it belongs to; inside it
 * bp_cs_challenge_scalar is `RandomizedConstraintSystem::challenge_scalar(label)` (constraint_system.rs:127-134).  In batch
 * verification the callbacks of different instances run concurrently on the library's host threads. */
typedef int (*bp_randomize_cb)(void* user, bp_cs* cs);
int bp_cs_specify_randomized_constraints(bp_cs* cs, bp_randomize_cb cb, void* user);
int bp_cs_challenge_scalar(bp_cs* cs, const char* label, uint64_t out[4]);
int bp_cs_metrics(bp_cs* cs, size_t* multipliers, size_t* constraints, size_t* commitments);
/* `prover.prove(prng, &bp_gens)` (prover.rs:444-451): consumes the prover.  rng_bytes: see "external rng" above (may be NULL when
 * bp_prover_set_rng / bp_prover_precompute supplied them).  proof_out / *proof_len: `R1CSProof::to_bytes` (proof.rs:74-81).
 * timing (8 doubles, may be NULL) as in bp_r1cs_prove_scenario.  bp_gens are the ctx's resident tables.
 * bp_prover_precompute[_batch]: the host-only head of prove() (TranscriptRng chain), see bp_stmt_precompute. */
int bp_prover_set_rng(bp_cs* prover, const uint8_t rng_bytes[32]);
int bp_prover_precompute(bp_cs* prover, const uint8_t rng_bytes_or_null[32]);
int bp_prover_precompute_batch(bp_cs** provers, size_t count);
int bp_prover_prove(bp_ctx* ctx, bp_cs* prover, const uint8_t rng_bytes_or_null[32], uint8_t* proof_out, size_t* proof_len, double* timing);
/* How prove() obtains the blinding vectors s_L, s_R (prover.rs:510-513, 599-602), per prover handle.
 *   BP_BLINDING_TRANSCRIPT (the default): one `Fr::rand` per entry from the TranscriptRng, as the reference: the proof is the bytes the
 *     reference prover emits for the same external rng bytes.
 *   BP_BLINDING_EXPANDED: every draw from the TranscriptRng happens in the reference's order EXCEPT the 2c draws of a phase's s_L then
 *     s_R (c > 0 multipliers; phase 1: c = n1, first index 0; phase 2: c = n2, first index n1), which are replaced by ONE draw
 *     kappa = Fr::rand(rng); a phase with c = 0 draws no key.  With key = the 32 canonical little-endian bytes of kappa and the
 *     phase-local index j < c: s_L[first + j] = W(key, 2j), s_R[first + j] = W(key, 2j + 1), where W(key, t) is the ChaCha20 block of
 *     `key` at 64-bit block counter t, stream 0 (rand_chacha 0.3's layout), its 64 bytes read as one little-endian 512-bit integer and
 *     reduced mod r (no rejection; zero stays zero).  The vectors are computed on the GPU where they are used: the host chain of 8
 *     Keccak-f per multiplier and two of the five witness uploads of a phase disappear.  Such a proof is an ordinary R1CSProof that
 *     `Verifier::verify` accepts; it is NOT the bytes the reference prover emits (i_blinding1, o_blinding1, s_blinding1 are the same
 *     draws, so A_I1 and A_O1 — the first 66 bytes — are equal for equal rng bytes and S1 differs).  The bytes are the same on every
 *     proving route (bp_prover_prove on either path, after bp_prover_precompute[_batch], on a sharded ctx, bp_stmt_prove,
 *     bp_prover_prove_batch with or without front groups; a batch may hold provers of both modes).
 * bp_prover_set_blinding: BP_E_ARG for a null or verifier handle, an unknown mode, or once the head of prove() has run on the handle
 * (bp_prover_precompute*, a consumed prover).  A bp_stmt takes it through bp_stmt_as_prover.  bp_prover_blinding reads the mode back.
 * bp_host_blind_expand (host only): s_L / s_R (count x 4 ark words each) of the phase-local indices j0 .. j0 + count - 1 under kappa
 * (ark words of a reduced scalar; j0 + count <= 2^31) — the twin the device kernel is tested against.
 * bp_debug_blind_expand (test hook): the same values through the production kernel, exported back to ark words (count <= 2^24).
 * bp_ctx_blinding_stats: scalars the expansion kernels wrote / their launches, since ctx creation.  A single proof of n multipliers
 * adds 2n and one launch per non-empty phase; a front group of bp_prover_prove_batch makes ONE launch per stage for all its members,
 * and expands a member's phase-1 vectors once for that phase's commitments and again with the whole witness (as it stages them twice
 * in the default mode). */
#define BP_BLINDING_TRANSCRIPT 0
#define BP_BLINDING_EXPANDED 1
int bp_prover_set_blinding(bp_cs* prover, int mode);
int bp_prover_blinding(bp_cs* prover, int* mode_out);
int bp_host_blind_expand(int curve, const uint64_t kappa[4], uint64_t j0, size_t count, uint64_t* sL, uint64_t* sR);
int bp_debug_blind_expand(bp_ctx* ctx, const uint64_t kappa[4], uint64_t j0, size_t count, uint64_t* sL, uint64_t* sR);
int bp_ctx_blinding_stats(bp_ctx* ctx, uint64_t* expanded_scalars, uint64_t* launches);
/* Batch proving: `count` statements in one call, equivalent to bp_prover_prove(ctx, provers[k], rng_k, ..) for k = 0 .. count-1 in
 * order — the same proof bytes, the same transcript states afterwards, the same status per instance.
 *   rng_bytes: count x 32 bytes, or NULL when every prover has its rng already (bp_prover_set_rng / bp_prover_precompute).
 *   proofs_out: proof k at proofs_out + k * proof_stride, its length in proof_lens[k] (0 for a failed instance).
 *   status (count, may be NULL): instance k's own result.  timing (8 doubles, may be NULL): total, lockstep inner-product rounds,
 *   TranscriptRng, upload, commitments, flatten, t(x) and evaluations, inner-product arguments proved one at a time (seconds).
 * Up-front checks, before any work: every prover live, of the ctx's curve and given once; no two borrow one transcript; rng bytes
 * present (and equal to precomputed ones); proof_stride at least the length of a proof with lg(gens capacity) rounds.  A failed
 * check returns BP_E_ARG and consumes no prover.  Otherwise every prover is consumed; an instance fails on its own (a callback's
 * non-zero return, BP_E_MISSING inside a randomized phase, BP_E_GENS_LENGTH) without changing any other instance's bytes, and the
 * call returns the first non-zero status in instance order.  A host-only ctx returns BP_E_NO_DEVICE after the checks and consumes
 * nothing.  Randomized-phase callbacks of different instances may run in any order.
 * Grouping: an instance whose inner-product argument runs over the direct window tables (padded size 2 .. BP_TUNE_DIRECT_MAX, ctx
 * not sharded, enough generators) and whose constraints can be indexed runs EVERY stage of prove() in a group.  Instances are taken in
 * order of their phase-1 multiplier count; those of equal count form a FRONT GROUP (at most BP_TUNE_PROVE_BATCH of them): witness
 * upload, the A_I / A_O / S commitments, flatten, t(x), the T commitments and l(x) / r(x) are one launch per stage for all members, with
 * one host wait per Fiat-Shamir step of the group (BP_TUNE_PROVE_BATCH_FRONT).  Randomized phases run on the calling thread in
 * between; afterwards the surviving members are re-partitioned by padded size, and every part finishes the front stages and runs its
 * inner-product arguments in LOCKSTEP — one launch per stage and one host wait per round for the whole part.  Every other instance
 * proves as bp_prover_prove would, inside the same call (its argument still joins a lockstep group when it runs over the direct
 * tables).  The bytes are identical either way.  With front groups, timing[2..6] are totals over the groups' stages (the wall time a
 * stage took for all members of a group, not a sum over instances).  A batch leaves the ctx's single-proof path as it was: a
 * bp_prover_prove afterwards gives the bytes it gives on a fresh ctx.
 * bp_prover_commit_batch: `Prover::commit` for several provers, equal to bp_prover_commit(provers[k], ctx, v + .., v_blinding + ..,
 * m_each[k], ..) in order, with every commitment of the batch computed in one launch and normalised with one inversion.  v,
 * v_blinding, V_xy_out and vars_out hold the sum of m_each entries, prover after prover.
 * bp_ctx_prove_batch_stats: instances whose inner-product argument ran in a lockstep group / instances bp_prover_prove_batch proved
 * one at a time / lockstep groups, since ctx creation.
 * bp_ctx_prove_batch_front_stats: instances whose front stages ran group-wide / front groups (counted after the re-partition by padded
 * size) / host waits for the GPU made by those stages (the waits of the argument's rounds are not included), since ctx creation. */
int bp_prover_prove_batch(bp_ctx* ctx, size_t count, bp_cs* const* provers, const uint8_t* rng_bytes, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens,
                          int* status, double* timing);
int bp_prover_commit_batch(bp_ctx* ctx, size_t count, bp_cs* const* provers, const size_t* m_each, const uint64_t* v, const uint64_t* v_blinding, uint64_t* V_xy_out,
                           bp_var* vars_out);
int bp_ctx_prove_batch_stats(bp_ctx* ctx, uint64_t* lockstep_instances, uint64_t* single_instances, uint64_t* groups);
int bp_ctx_prove_batch_front_stats(bp_ctx* ctx, uint64_t* front_instances, uint64_t* front_groups, uint64_t* front_waits);
/* Witness check: does the recorded assignment satisfy the recorded constraint system?  (The reference has no such call: a prover
 * handed an unsatisfying witness runs the whole proof and returns bytes that no verifier accepts.)
 *   gate i (i < multipliers):  a_L[i] * a_R[i] == a_O[i]  (mod r)
 *   constraint k:              sum of coefficient * variable over its terms == 0  (mod r), with Committed(i) = v[i],
 *                              MultiplierLeft / Right / Output(i) = a_L / a_R / a_O[i] and One = 1.
 * Constraints are numbered in the order of the constrain calls, the two of every bp_cs_multiply included, the randomized phase
 * continuing where phase 1 stopped (the `constraints` of bp_cs_metrics count the same rows).
 * bp_witness_report: n and q examined; the number of violated gates and the smallest violated gate index (UINT64_MAX when none);
 * the same for constraints; deferred_callbacks = randomized-phase callbacks that have not run yet — their constraints do not exist
 * and are NOT covered, so a report with deferred_callbacks > 0 speaks about phase 1 only; first_bad_residual = the value of
 * first_bad_constraint's combination (ark words), re-evaluated on the host from the recorder (all zero when none).
 * With a device ctx the gates and the constraints are evaluated on the GPU (csrc/witness_check.cuh): one lane per gate, and the
 * constraints row by row, every row cut into pieces of at most bp_witness_check_piece() terms — one lane per piece, a second launch
 * summing the pieces of the rows that have several.  With a NULL or host-only ctx the host twin runs: plain loops over the recorder.
 * Both give the same report.
 * bp_prover_check: a diagnostic.  It uploads the witness itself, consumes nothing, touches no transcript and checks everything
 * recorded so far.  It returns BP_OK whatever the report says (the return value is about the call; the caller reads the counts);
 * BP_E_ARG for a null handle or report, a verifier handle, a consumed prover, or a ctx of another curve.
 * bp_prover_check_batch: the same for `count` provers (out[k] is prover k's report) with one launch sequence and one host wait for
 * all of them.  Up-front checks as in bp_prover_prove_batch: every prover live, of the ctx's curve, given once; BP_E_ARG otherwise,
 * and no report is written.  Nothing is consumed either way.  A host-only ctx runs the host twin per prover.
 * bp_prover_set_check(prover, 1): the GUARD.  Every proving route (bp_prover_prove over the direct tables or the folding path, after
 * bp_prover_precompute[_batch], bp_stmt_prove, bp_prover_prove_batch with and without front groups; both blinding modes) evaluates
 * the gates and ALL constraints once the whole witness is resident, after the randomized phase.  An instance with any violation
 * returns BP_E_UNSATISFIED, writes no proof bytes (proof_len 0 in a batch), and is consumed; its transcript is left unspecified.  In
 * a batch it is one more way for an instance to fail on its own: no other instance's bytes, status or transcript changes.  The guard
 * adds no host wait: the flags come back with a copy the route already waits for.  It changes no TranscriptRng draw, so a satisfied
 * statement proves to the same bytes with the guard on or off.  It may be set any time before the proof starts; the default is off,
 * and with it off nothing changes: not a byte, not a launch, not a wait.  BP_E_ARG for a null, verifier or consumed handle.
 * bp_prover_checking reads the flag back.
 * bp_ctx_last_unsatisfied: the reports of the instances the ctx's most recent proving call (bp_prover_prove, bp_stmt_prove,
 * bp_prover_prove_batch) refused with BP_E_UNSATISFIED, in instance order, with their instance indices (0 for a single proof).  *count
 * receives how many there are; at most `cap` are written (instance / reports may be NULL when cap is 0).  0 after a call that refused none.
 * bp_debug_prover_poke_witness (test hook): overwrites one recorded assignment — vec 0: a_L, 1: a_R, 2: a_O, 3: v; value: ark words
 * of a reduced scalar.  The only way to produce a violated gate (the recorder computes a_O itself), and the easy way to spoil a
 * satisfiable program.  Commitments already made are not recomputed.  BP_E_ARG for a bad handle, vector, index or value. */
typedef struct bp_witness_report {
    uint64_t gates_checked, constraints_checked;      /* n and q examined */
    uint64_t bad_gates, first_bad_gate;               /* UINT64_MAX when none */
    uint64_t bad_constraints, first_bad_constraint;   /* index = order of constrain calls, multiply's two included, phase 2 continuing */
    uint64_t deferred_callbacks;                      /* randomized-phase callbacks not yet run: their constraints are NOT covered */
    uint64_t first_bad_residual[4];                   /* value of first_bad_constraint's combination (ark words), re-evaluated on the host; zero when none */
} bp_witness_report;
size_t bp_witness_check_piece(void);
int bp_prover_check(bp_ctx* ctx_or_null, bp_cs* prover, bp_witness_report* out);
int bp_prover_check_batch(bp_ctx* ctx, size_t count, bp_cs* const* provers, bp_witness_report* out);
int bp_prover_set_check(bp_cs* prover, int on);
int bp_prover_checking(bp_cs* prover, int* on_out);
int bp_ctx_last_unsatisfied(bp_ctx* ctx, size_t cap, uint64_t* instance, bp_witness_report* reports, size_t* count);
int bp_debug_prover_poke_witness(bp_cs* prover, int vec /* 0 a_L, 1 a_R, 2 a_O, 3 v */, size_t index, const uint64_t value[4]);

/* ---- Many witnesses of one recorded gadget (an addition the reference lacks; the prover's counterpart of bp_verifier_new_like) ----
 * bp_prover_new_like: `of` must be a live prover that is not consumed, not inside prove, and on which the head of prove()
 * (bp_prover_precompute*) has not run; BP_E_ARG otherwise — also for a verifier handle or a null pointer — and nothing is frozen.
 * The call freezes `of`'s phase-1 constraints, its multiplier count and its randomized-constraint callbacks into ONE recording that
 * `of` and every like-prover share.  From then on they accept only commits and, inside their randomized phase, recording calls;
 * anything else is BP_E_ARG.  `of` keeps its witness and proves to the bytes it would have produced unfrozen.  The new handle
 * appends the r1cs domain separator to `transcript` (Prover::new), inherits `of`'s Pedersen pair and curve, and starts with no
 * commitments, no witness, the default blinding mode and the guard off.  bp_cs_metrics reports the shared counts.
 *
 * bp_prover_assign_multipliers: the witness of a like-prover, a_L = left, a_R = right, count x 4 ark Montgomery words each.  count
 * must be the recording's multiplier count; words at or above r, a second call, a handle that is no like-prover: BP_E_ARG, nothing
 * changed.  a_O is NOT passed: it is the product, taken by a kernel on the GPU when the witness goes up (a single-phase like-prover
 * on bp_prover_prove) and on the host, once, wherever the host reads it (randomized callbacks, the host witness check, the staging
 * of bp_prover_prove_batch's front groups, bp_prover_check's own upload, bp_debug_prover_poke_witness on a_O).  Proving,
 * precomputing or checking a like-prover without an assignment, or with fewer commitments than the shared constraints name, is
 * BP_E_ARG before anything is consumed (bp_prover_prove_batch: a failed up-front check, no prover consumed).
 *
 * A like-prover proves to the bytes of a prover that recorded the gadget itself with the same witness, commitments, transcript
 * state, rng bytes and blinding mode, on every route, and leaves its transcript in the same state.  The constraint index of a
 * single-phase recording is built once per recording and kept on the device per ctx (at most 8 recordings, least recently used
 * first out; an entry whose recording was freed is dropped at the next lookup): only the first proof of a recording on a ctx
 * uploads it.  Two-phase like-provers share the recording; their full index depends on the instance's challenges and is built per
 * proof.  On a sharded ctx nothing is kept resident.
 *
 * bp_ctx_prover_like_stats, since ctx creation: uploads of a recording's index / proofs that found it resident / bytes resident
 * now / multipliers whose product the GPU kernel took / multipliers whose product the host took.  Any pointer may be NULL. */
int bp_prover_new_like(bp_cs* of, void* transcript, bp_cs** out);
int bp_prover_assign_multipliers(bp_cs* prover, const uint64_t* left, const uint64_t* right, size_t count);
int bp_ctx_prover_like_stats(bp_ctx* ctx, uint64_t* index_uploads, uint64_t* index_hits, uint64_t* resident_bytes, uint64_t* gates_on_device, uint64_t* gates_on_host);

/* ---- A like-prover's witness from device memory (an addition the reference lacks; the prover's counterpart of bp_msm_dev) ----
 * bp_prover_assign_multipliers_dev: bp_prover_assign_multipliers with a_L = d_left and a_R = d_right in the memory of ctx's device
 * (bp_dev_alloc, or a host that links the same HIP runtime): count x 4 ark Montgomery words each, the public data convention, complete
 * before the call (the caller has synchronised its own producer).  The handle's rules are the host form's and are checked first,
 * before ctx is looked at: a live like-prover without an assignment, on which the head of prove() has not run, count = the
 * recording's multiplier count; anything else is BP_E_ARG and nothing changes.  Then: a null ctx, a ctx of the other curve, or a
 * null vector with count > 0: BP_E_ARG; a host-only ctx: BP_E_NO_DEVICE; nothing changes.  count == 0 with null vectors is allowed.
 *
 * The call takes a copy that the HANDLE owns: a plain allocation on that device, still ark words, from no ctx arena — it survives
 * bp_ctx_destroy of the assigning ctx.  One kernel copies both vectors and compares every word with r in the same pass; one copy
 * back, one host wait.  A word at or above r: BP_E_ARG, bp_last_error() names the vector and the smallest failing index (of both
 * vectors: the one with the smaller index, left on a tie), the copy is wiped and freed, and the handle is unchanged: a later valid
 * assignment by either entry point succeeds.  After return the caller's buffers are unread and may be reused.  The copy is wiped
 * (zeroes on the stream, then a wait) and freed when the prover is consumed, freed, or its witness is taken to the host.
 *
 * A prover with a device witness proves, checks and joins a batch only on a ctx of the same device: BP_E_ARG otherwise, before
 * anything is consumed (bp_prover_prove_batch: a failed up-front check, no prover consumed).  bp_prover_prove of a single-phase
 * like-prover on a ctx that is not sharded keeps the witness on the device: no staging and no H2D copy of a_L, a_R; one kernel
 * imports them from the handle's copy and forms a_O = a_L * a_R in the same pass.  Every other reader takes the witness to the host
 * once — a D2H copy of the ark words, then the products there — and from then on the handle is a host-assigned like-prover:
 * randomized callbacks of a two-phase like-prover, the host twin of the witness check, bp_prover_check's own upload, every route of
 * bp_prover_prove_batch (at its entry, after the up-front checks), a sharded ctx, bp_debug_prover_poke_witness, the residual of a
 * refused proof.  Proof bytes and the final transcript state are those of the same like-prover assigned through
 * bp_prover_assign_multipliers with the same words, on every route, with the guard on or off.
 *
 * bp_witness_range_bits_dev: a helper, not part of the prover's contract (any kernel that writes ark words serves equally well):
 * the witness of the reference's range gadget (tests/r1cs_secq256k1.rs:361-445) built on the GPU.  d_values: count 64-bit
 * integers; for value j and bit i < nbits, element j * nbits + i of d_left is 1 - bit and of d_right is the bit, as ark
 * Montgomery words: count * nbits x 32 bytes per vector.  nbits from 1 to 64 and count * nbits below 2^31, else BP_E_ARG (checked
 * before any device use); a host-only ctx: BP_E_NO_DEVICE.  Only the low nbits bits are decomposed: a value out of range is the
 * gadget's sum constraint's business (with the guard on: BP_E_UNSATISFIED).  One launch on the ctx's stream; returns after a wait.
 *
 * bp_ctx_witness_dev_stats, since ctx creation: device assignments accepted / multipliers the import kernel read from device
 * memory (they also count in gates_on_device of bp_ctx_prover_like_stats) / multipliers taken to the host instead.  Any pointer
 * may be NULL. */
int bp_prover_assign_multipliers_dev(bp_cs* prover, bp_ctx* ctx, const void* d_left, const void* d_right, size_t count);
int bp_witness_range_bits_dev(bp_ctx* ctx, const void* d_values, size_t count, unsigned nbits, void* d_left, void* d_right);
int bp_ctx_witness_dev_stats(bp_ctx* ctx, uint64_t* assigns, uint64_t* gates_from_device, uint64_t* gates_downloaded);

/* `verifier.verify(&proof, &pc_gens, &bp_gens)` (verifier.rs:549-557): consumes the verifier */
int bp_verifier_verify(bp_ctx* ctx, bp_cs* verifier, const uint8_t* proof, size_t proof_len);
/* `batch_verify(prng, instances, &pc_gens, &bp_gens)` (verifier.rs:604-691): instance k = (verifiers[k], the k-th of the
 * concatenated compressed proofs); every verifier is consumed.  Instances whose recordings have the same STRUCTURE (same gadget;
 * coefficient values may differ: public constants, challenge-dependent randomized constraints) are evaluated by one kernel launch
 * per block of 512 from a GPU-resident circuit template.  alphas: count x 4 words (ark Montgomery form), the weights the reference
 * draws per instance from its prng (verifier.rs:649) — REQUIRED for count > 1 (BP_E_ARG otherwise: with equal weights the errors of
 * two invalid proofs can cancel in the one mega-check); NULL is accepted for count == 1 only (Verifier::verify, weight 1).  The same
 * handle twice in one batch is BP_E_ARG at any count.  A verifier created by bp_verifier_new_like that holds fewer commitments than
 * the shared constraints name is BP_E_ARG (the reference would index past its V vector).  check_point_xy (may be NULL): the value
 * of the mega-check MSM, all-zero iff it is the identity.  timing (5 doubles, may be NULL) as in bp_r1cs_batch_verify_scenarios.
 * A batch of like-instances of one recording (bp_verifier_new_like) runs its per-proof front end on the GPU as a whole; a batch that
 * mixes several recordings runs every large enough class of like-instances there and the rest on the host, in one call with one
 * check point ("verifier front end on the device", "Batches of several gadgets" below).  Return value, check point and errors never
 * depend on which of the paths a call took. */
int bp_r1cs_batch_verify(bp_ctx* ctx, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* alphas,
                         double* timing, uint64_t* check_point_xy);
/* The next instance of the SAME gadget without recording it again: a verifier that shares `of`'s phase-1 constraints and its
 * randomized-constraint callbacks (ref-counted, immutable from now on: `of` and the new verifier accept commits and randomized
 * constraints only).  The caller replays just the instance's own transcript traffic: bp_verifier_commit in the same order as on
 * `of`, plus whatever the gadget appends through bp_cs_transcript.  The reference has no such call — every `Verifier` there records
 * its gadget anew (verifier.rs:69-224); with 4096 instances of a 2^14-multiplier circuit that recording is the whole cost. */
int bp_verifier_new_like(bp_cs* of, void* transcript, bp_cs** out);
/* Verification of many proofs with a verdict for EACH: `Verifier::verify` (verifier.rs:549-600) for `count` instances in one call —
 * the loop `for (v, proof) in instances { v.verify(&proof, &pc_gens, &bp_gens) }` of a service that must tell its proofs apart.
 * Instance k = (verifiers[k], the k-th of the concatenated compressed proofs).
 *   status (count): status[k] is exactly what bp_verifier_verify(ctx, verifiers[k], proof_k, len_k) returns for that instance alone:
 *   BP_OK, BP_E_VERIFICATION, BP_E_FORMAT, BP_E_GENS_LENGTH, or the non-zero return of the instance's randomized-phase callback.
 *   Every instance is checked with weight 1: there are no alphas, and nothing one instance does changes another instance's status
 *   or check point.  The call returns the first non-zero status in instance order.
 *   check_points_xy (count x 8 words, may be NULL): the affine value of instance k's own mega-check (verifier.rs:574-595), all-zero
 *   iff it is the identity — and all-zero for an instance that failed before its check ran.
 *   timing (5 doubles, may be NULL; seconds): the whole call, host replay, waits for the GPU, the single-route instances, decoding.
 * Up-front checks, before any work: every verifier live, of the ctx's curve and given once; generators installed.  A failed check
 * returns BP_E_ARG (BP_E_GENS_LENGTH when no generators are installed) and consumes no verifier.  A host-only ctx returns
 * BP_E_NO_DEVICE after the checks and consumes nothing.  Otherwise every verifier is consumed.  count == 0 returns BP_OK.  The
 * transcript of an instance whose status is BP_OK is left in the state bp_verifier_verify leaves it in.  Randomized-phase callbacks
 * of different instances may run concurrently on the ctx's host pool, as in batch verification.
 * Grouping: an instance whose proof claims a padded size N of 2 .. BP_TUNE_DIRECT_MAX that the installed generators and the direct
 * window tables cover (built on first use, as for proving), on a ctx that is not sharded, takes the GROUPED path: the host pool
 * replays the transcripts (an instance that fails anywhere in decode or replay — a malformed or off-curve point, an identity under
 * validate_and_append_point, an L_vec of the wrong length, a callback error — gets its own status and is left out of the launches;
 * the batch goes on), the survivors are grouped by (circuit template, N), and a group — at most BP_TUNE_VERIFY_EACH instances, and
 * what a 256 MB device arena holds for that N — is ONE sequence of launches on the ctx's stream: k_vfy_tables, k_vfy_batch with one
 * chunk per proof (every proof keeps its own g / h rows), k_ve_heads, the table sums of the fixed bases (k_dt_accum_multi), k_ve_tail
 * (the proofs' own points: P short variable-base MSMs), k_ve_check, one copy back of flags and points.  The host waits for the GPU
 * ONCE per group (BP_VERIFY_EACH_WAITS_PER_GROUP), whatever the number of instances or N; the decompression of the call's points
 * is one more wait per call, a circuit template that is not cached yet one per gadget.  Every other instance (N = 1, N beyond the
 * tables' reach, a sharded ctx, a proof whose framing fails) is verified inside the same call by the single-instance route of
 * bp_verifier_verify.  bp_verifier_verify, bp_r1cs_batch_verify and the scenario entry points keep their behaviour and code paths.
 * bp_r1cs_verify_each_scenarios: the same for scenario statements; flat arrays as in bp_r1cs_batch_verify_scenarios, no alpha.
 * bp_ctx_verify_each_stats: instances that took the grouped path / the single route, groups launched, host waits for the GPU made
 * by the groups, since ctx creation. */
#define BP_VERIFY_EACH_WAITS_PER_GROUP 1
int bp_verifier_verify_batch(bp_ctx* ctx, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens, int* status,
                             uint64_t* check_points_xy, double* timing);
int bp_r1cs_verify_each_scenarios(bp_ctx* ctx, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                  const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, int* status,
                                  uint64_t* check_points_xy, double* timing);
int bp_ctx_verify_each_stats(bp_ctx* ctx, uint64_t* grouped_instances, uint64_t* single_instances, uint64_t* groups, uint64_t* host_waits);
/* test hook: `count` independent variable-base MSMs through k_ve_tail alone; job j owns terms [offsets[j], offsets[j + 1]) of
 * bases_xy (ark layout) and scalars (ark Montgomery words, or any 256-bit integers when scalars_canonical); out_xy: count affine
 * points */
int bp_debug_msm_each(bp_ctx* ctx, size_t count, const size_t* offsets, const uint64_t* bases_xy, const uint64_t* scalars, int scalars_canonical, uint64_t* out_xy);
/* test hook, host only: k_ve_tail's own digit and layout functions (csrc/vfy_each.cuh) for job `job` of `count`: *first / *terms = the
 * job's term range; for its term t (t < *terms, scalars: canonical words of ALL terms) and window w < 64: digits[64 t + w] = the 4-bit
 * digit, planes[64 t + w] = its four bit-plane membership bits as the kernel tests them, lanes[w] = first lane of the window's quad,
 * groups[w] = the LDS slot of the group sum the window folds into */
int bp_debug_ve_plan(size_t count, const size_t* offsets, const uint64_t* scalars_canonical, size_t job, uint32_t* first, uint32_t* terms, uint8_t* digits,
                     uint8_t* planes, uint32_t* lanes, uint32_t* groups);
/* Batch verification that NAMES the failing instances: `batch_verify` (verifier.rs:604-691) at its own speed while the batch is
 * valid, and a verdict for each instance when it is not — the loop `for (v, proof) in instances { v.verify(..) }` of a service with
 * large statements, for which bp_verifier_verify_batch falls back to one MSM per proof.  The reference has no such call.
 * Instance k = (verifiers[k], the k-th of the concatenated compressed proofs) with weight alphas[k] (count x 4 words, ark Montgomery
 * form); framing and weights as in bp_r1cs_batch_verify.  Instance k keeps its weight in every pass.
 *   status (count): status[k] is what bp_verifier_verify(ctx, verifiers[k], proof_k, len_k) returns for that instance alone: BP_OK,
 *   BP_E_VERIFICATION, BP_E_FORMAT, BP_E_GENS_LENGTH, or the non-zero return of its randomized-phase callback — with ONE caveat: an
 *   invalid proof is reported BP_OK only if a weighted sum that contains it is the identity, which is the failure probability of
 *   `batch_verify` itself over the caller's weights.  A valid proof is never reported invalid (a subset of valid proofs sums to the
 *   identity whatever the weights), and a subset of one is decided exactly (alpha * C is the identity iff C is, alpha != 0).
 *   The call returns the first non-zero status in instance order; when it returns BP_OK the batch is accepted exactly as
 *   bp_r1cs_batch_verify accepts it.
 *   timing (4 doubles, may be NULL; seconds): the whole call, pass 1, all later passes, snapshot / restore of the instances' states.
 * How: a PASS is one run of the batch verifier's core (the launch chains of bp_r1cs_batch_verify: the device front end for
 * like-instances of one recording, the host replay otherwise) over a subset, gathered through an index map.  Pass 1 covers the
 * batch; a valid batch costs that one pass.  An instance that fails BEFORE its check — a malformed or off-curve point, an identity
 * under validate_and_append_point, an L_vec of the wrong length, too few generators, a callback error — keeps its own status and
 * leaves the batch, the rest go on (bp_verifier_verify_batch's rule, not bp_r1cs_batch_verify's "first error rejects the call"):
 * pass 1 names all of them at once, pass 2 covers the survivors.  A subset whose check fails is halved, lower half floor(n / 2): the
 * lower half is tested; if it passes, the upper half is known to fail and is split without a pass of its own; if it fails, it is
 * searched and the upper half tested after it.  With f >= 1 invalid proofs among n survivors: at most 1 + 2 f ceil(log2 n) passes,
 * and for f = 1 at most 3 n instances in all passes.  Every pass runs its members from the state they had on entry to the call
 * (transcript and recorder are snapshotted before pass 1 and restored before each later pass).
 * BP_TUNE_VERIFY_LOCATE_LEAF: a failing subset of at most this many instances is not split further but decided by the machinery of
 * bp_verifier_verify_batch (exact; grouped where the direct tables reach, the single route elsewhere).  Results never depend on it.
 * Up-front checks, before any work: every verifier live, of the ctx's curve and given once; status non-null; alphas non-null for
 * count > 1 (NULL = weight 1 for count == 1); NO WEIGHT ZERO (a zero weight hides its instance from every sum — a refusal that
 * bp_r1cs_batch_verify does not make); a bp_verifier_new_like handle that holds fewer commitments than the shared constraints name;
 * generators installed.  A failed check returns BP_E_ARG (BP_E_GENS_LENGTH when no generators are installed) and consumes no
 * verifier.  A host-only ctx returns BP_E_NO_DEVICE after the checks and consumes nothing.  count == 0 returns BP_OK.  Otherwise
 * every verifier is consumed.  The transcripts' states after the call are UNSPECIFIED, as after bp_r1cs_batch_verify: a pass that
 * completes on the device front end does not advance the host transcripts, the host replay does, and later passes restart their
 * members from the entry state.  Callbacks of an instance run once per pass that holds it, possibly concurrently with other
 * instances' on the ctx's host pool.  On a sharded ctx every pass works as bp_r1cs_batch_verify does there.
 * bp_r1cs_batch_verify_locate_scenarios: the same for scenario statements; flat arrays and weights (alpha_seed, drawn in instance
 * order; required for count > 1) as in bp_r1cs_batch_verify_scenarios; the recordings are rebuilt in every pass.
 * bp_ctx_verify_locate_stats, since ctx creation: calls; passes; the sum of the passes' subset sizes; instances decided exactly (as a
 * subset of one, or by the leaf machinery). */
int bp_r1cs_batch_verify_locate(bp_ctx* ctx, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens,
                                const uint64_t* alphas, int* status, double* timing);
int bp_r1cs_batch_verify_locate_scenarios(bp_ctx* ctx, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs,
                                          const size_t* proof_lens, const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics,
                                          const size_t* npubs, const uint8_t alpha_seed[32], int* status, double* timing);
int bp_ctx_verify_locate_stats(bp_ctx* ctx, uint64_t* calls, uint64_t* passes, uint64_t* instances_in_passes, uint64_t* exact_leaves);
/* test hook, host only: the planner of bp_r1cs_batch_verify_locate (leaf 1) over a simulated core — a range fails its check iff it
 * holds a fails_check member (count bytes); fails_before members (count bytes, may be NULL) are reported, with BP_E_FORMAT, and
 * dropped by the first pass that holds them.  Pass i covered survivors [pass_lo[i], pass_lo[i] + pass_n[i]) of the list of instances
 * still in the batch at that time, in instance order; pass_failed[i]: 0 passed, 1 failed its check, 2 reported members failing before
 * it.  The pass arrays need room for 2 * count + 2 entries and may be NULL; status: count ints. */
int bp_debug_locate_plan(size_t count, const uint8_t* fails_check, const uint8_t* fails_before, uint32_t* npasses, uint32_t* pass_lo, uint32_t* pass_n,
                         uint8_t* pass_failed, uint64_t* instances_in_passes, int* status);
/* merlin::Transcript <-> bp_transcript handle: Strobe128 {state[200], pos, pos_begin, cur_flags} (merlin 3.0 src/strobe.rs) */
int bp_transcript_export_state(const void* transcript, uint8_t out[203]);
int bp_transcript_import_state(void* transcript, const uint8_t in[203]);
void* bp_transcript_clone(const void* transcript);

/* ---- r1cs::Verifier::verify / batch_verify ------------------------------------------------------------
 * bp_r1cs_verify_scenario replaces `Verifier::new` + commits + gadget + `verify(&proof, &pc_gens, &bp_gens)`
 * (src/r1cs/verifier.rs:252-287, 549-600) for the same scenarios as the prover: returns BP_OK, or
 * BP_E_VERIFICATION / BP_E_FORMAT / BP_E_GENS_LENGTH exactly where the reference returns the matching R1CSError.
 * bp_r1cs_batch_verify_scenarios replaces `batch_verify(prng, instances, pc_gens, bp_gens)` (:604-691):
 * `count` instances with concatenated proofs / commitments / publics, params 8 u64 per instance; the per-proof
 * alpha is `Fr::rand` of a ChaCha20 rng seeded with alpha_seed.  The instances go through in blocks: the host replays the
 * transcripts of one block while the GPU evaluates the previous one.  timing[5] (s): [0] the whole call, [1] host replay
 * inside the block loop (overlapped with the GPU), [2] wait for the GPU after the last block + tail scaling, [3] final MSM,
 * [4] proof decoding (framing + point decompression).  Proof-sharded multi-GPU use: rank r passes its slice of the instances, alpha_skip = number
 * of instances on lower ranks (their alphas are drawn and discarded), and receives the affine value of ITS mega-check
 * in check_point_xy (may be NULL).  The batch is valid iff EVERY rank's call returned BP_OK (then every check point is the
 * identity, and so is their sum — by linearity the reference's single MSM, :685).  A call can fail before its MSM runs (an
 * identity A_I1 / T_i / L_j, mismatched L_vec, malformed bytes: verifier.rs:420-470 return early); check_point_xy is then
 * all-zero, so the point sum alone must never decide — reduce the statuses first (parallel.sharded_batch_verify). */
int bp_r1cs_verify_scenario(bp_ctx* ctx, int scenario, const uint64_t* params, const uint8_t* proof, size_t proof_len, const uint64_t* commit_xy,
                            size_t m, const uint64_t* publics, size_t npub);
int bp_r1cs_batch_verify_scenarios(bp_ctx* ctx, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs,
                                   const size_t* proof_lens, const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics,
                                   const size_t* npubs, const uint8_t alpha_seed[32], double* timing, size_t alpha_skip,
                                   uint64_t* check_point_xy);

/* ---- profiling: HIP-event time of the dominant kernel of the last call, on the ctx stream ---------- */
#define BP_K_MSM_ACCUM 0   /* bucket accumulation (k_msm_accum) */
#define BP_K_MSM_TOTAL 1   /* all MSM kernels of the call, first launch to last */
#define BP_K_IPA_SCALARS 2 /* k_ipa_scalars + k_ipa_ip_finish of one round */
#define BP_K_IPA_FOLD 3    /* k_ipa_fold_ab + k_ipa_fold_pts of one round */
#define BP_K_R1CS_POLY 4   /* k_r1cs_poly_t / k_r1cs_poly_eval */
#define BP_K_VFY_SCALARS 5 /* k_vfy_scalars */
#define BP_K_FOLD_TAB 6     /* k_ipa_fold_tab: the first fold round through the fixed-base tables */
#define BP_K_FOLD_LADDER 7  /* k_ipa_fold_glv / k_ipa_fold_uniform / k_ipa_fold_pts: the scalar-multiplication ladders of a round */
#define BP_K_FOLD_FINISH 8  /* k_ipa_fold_finish: Jacobian -> affine with shared inversions */
#define BP_K_MSM_ACCUM_FS 9 /* k_msm_accum_fs: accumulate of the fixed-shape pipeline (mid-size MSMs) */
#define BP_K_MSM_AGG 10     /* bucket reduction + aggregation (k_msm_reduce*, k_msm_marginals*, k_msm_window_sums) */
#define BP_K_VFY_TABLES 11  /* k_vfy_tables */
#define BP_K_VFE_POINTS 12  /* k_vfe_points: decompression + serialization of a batch's points (device front end of batch verification) */
#define BP_K_VFE_SPONGE 13  /* k_vfe_sponge: transcript replay + challenge derivation, one lane per proof */
#define BP_K_VFE_PREPARE 14 /* k_vfe_consts + k_vfe_wv + k_vfe_sum2: challenge arithmetic, parameter blocks, tail scalars */
#define BP_K_VE_TAIL 15     /* k_ve_tail: the per-proof variable-base sums of bp_verifier_verify_batch */
#define BP_K_MSM_BATCH 16   /* k_msb_accum + k_msb_combine: the bucketed route of bp_msm_batch, one region per group */
#define BP_K_DT_CHECK 17    /* k_dt_check over table 4: the direct window tables' part of bp_gens_direct_tables_check */
#define BP_K_WITNESS_CHECK 18 /* k_r1cs_check* : gates and constraints of the witness check */
#define BP_K_COUNT 19
int bp_ctx_set_profiling(bp_ctx* ctx, int enabled);
/* accumulated milliseconds and launch count since the last reset */
int bp_ctx_kernel_time(bp_ctx* ctx, int which, double* ms_total, uint64_t* launches);
int bp_ctx_reset_profiling(bp_ctx* ctx);

/* Size thresholds at which the engine switches kernels (results never depend on them; the tests lower them to drive the
 * large-input paths with small inputs).  FOLD_BATCH_MIN: output points per IPA fold round from which the affine conversion
 * shares inversions (default 65536); MSM_BIN_MIN: terms from which the MSM uses the two-level sort (default 64);
 * IPA_FREEZE_LEN: vector length from which bp_ipa_create / the prover stop folding G and H and fold per-element coefficients
 * over the frozen vectors instead (default 8192; 0 or 1 = never); MSM_WSUM_MIN: total bucket count from which an MSM aggregates
 * its buckets by running sums instead of bit marginals (default 2^18). */
#define BP_TUNE_FOLD_BATCH_MIN 0
#define BP_TUNE_MSM_BIN_MIN 1
#define BP_TUNE_IPA_FREEZE_LEN 2
#define BP_TUNE_MSM_WSUM_MIN 3
#define BP_TUNE_CYCLIC_MIN 4   /* padded size from which a sharded prover partitions the IPA index-cyclically (default 2^14) */
#define BP_TUNE_MSM_FIXED_MIN 5   /* terms from which an MSM over the generator tables uses the fixed-base rows (default 2^20; >= 4096) */
#define BP_TUNE_HOST_THREADS 6    /* host threads of this ctx's pool for the per-instance transcript replays of batch verification (0 = default:
                                     the machine's hardware threads, at most 32, or ARKBP_HOST_THREADS); callers that keep several batches in
                                     flight on several ctxs divide the cores among them */
#define BP_TUNE_FOLD_QUAD_MAX 8    /* fold rounds of the inner-product argument with at most this many output points (G and H together) run with FOUR lanes per
                                     point (quad-cooperative group arithmetic): shorter rounds, more arithmetic; default 0 = never (a prover that keeps the GPU
                                     full gains nothing); a latency-bound single prover sets 2^14 */
#define BP_TUNE_MSM_GLV_MIN 7     /* terms from which a variable-base MSM on secq256k1 splits its scalars with the endomorphism (default 256; a huge value turns it off) */
#define BP_TUNE_WAIT_SLEEP 10     /* microseconds this ctx's host waits sleep between polls of the GPU event, instead of busy-waiting (what the HIP
                                     synchronisation calls do on this stack: one core per waiting thread); 0 = busy wait (default), 1 = 30 us, at most 1000.
                                     30 us: a third of the host CPU per proof for ~2 % of latency, for a prover that keeps several proofs in flight;
                                     batch verification waits often and shortly: 10 us */
#define BP_TUNE_MSM_CHUNK_CAP 9   /* entries per first-level chunk of the mid-size (fixed-shape) MSM pipeline: 8 .. 64; 0 = default (16 for callers that keep
                                     the GPU full; fitted per MSM to whole waves per SIMD for the bp_msm* entry points).  Results never depend on it */
#define BP_TUNE_VFY_DEVICE 11    /* 1 (default): batch verification of like-instances of one single-phase statement runs its per-proof front end on the
                                  * GPU (see "verifier front end on the device" below); 2: like-instances of two-phase statements
                                  * (specify_randomized_constraints) too; 0: always the host replay (A/B, tests).  Values above 2 act as 2.
                                  * ARKBP_VFY_DEVICE=0/1/2 in the environment sets the default of every ctx created afterwards */
#define BP_TUNE_DIRECT_MAX 12    /* statements whose padded size is at most this (default 8192, at most 2^16; 0 = never) are proved over DIRECT WINDOW
                                  * TABLES of the first generators (d * 16^w * base, 60 KiB per base, built by the first such proof of the ctx): every
                                  * MSM of Prover::prove (src/r1cs/prover.rs:516-649) and of InnerProductProof::create
                                  * (src/inner_product_proof.rs:86-213) becomes a sum of table entries, G and H are never folded.  This is the
                                  * latency path for the reference's own benchmark range (benches/r1cs_secq256k1.rs:152-250, 2 .. 2046 multipliers) */
#define BP_TUNE_PROVE_BATCH 13   /* most instances per lockstep group of bp_prover_prove_batch (0 = default: as many as a 256 MB device arena
                                  * holds; at most 65535, groups above 16384 are split) */
#define BP_TUNE_PROVE_BATCH_FRONT 14   /* 1 (default): bp_prover_prove_batch runs the stages in front of the inner-product argument group-wide
                                  * too (see "Batch proving"); 0: those stages run one instance after the other on the single-proof
                                  * workspaces (A/B, tests).  Results never depend on it */
#define BP_TUNE_VERIFY_EACH 15    /* most instances per group of bp_verifier_verify_batch (0 = default: what a 256 MB device arena holds, at most 4096;
                                  * values above 4096 act as 4096) */
#define BP_TUNE_MSM_BATCH_SHORT 16 /* bp_msm_batch: jobs of at most this many terms take the short route (0 = default: 8) */
#define BP_TUNE_MSM_BATCH_SLICE 17 /* bp_msm_batch: most terms per slice of a bucketed job.  0 = default: the call's bucketed terms / 128, at least 64 and at
                                    * most 512 — many jobs: long slices, few jobs: enough slices to occupy the CUs.  Every value >= 1 is accepted, values
                                    * above 2^30 act as 2^30 */
#define BP_TUNE_MSM_BATCH_MAX 18   /* bp_msm_batch: jobs above the short route and of at most this many terms take the bucketed route, longer ones the single
                                    * route (0 = default: 4096; a value at or below the short one leaves no bucketed route) */
#define BP_TUNE_MSM_BATCH_MIN_JOBS 19 /* bp_msm_batch: a call with fewer short and bucketed jobs than this runs every job on the single route (0 = default: 6;
                                    * 1 = never): a group costs the latency of one serial Horner chain whatever it holds.  Results never depend on the four */
#define BP_TUNE_MSM_PAIR 21        /* (20 stays unassigned: tests/test_msm_batch_cpu.py pins it as the first knob that is refused.)  1 (default): L and R of a round of the inner-product argument — two mid-size MSMs of the same length that do not
                                    * depend on each other — run as two jobs of ONE chain of launches with one host wait (see bp_ctx_msm_pair_stats);
                                    * 0: one MSM after the other (A/B, tests).  Results never depend on it */
#define BP_TUNE_VERIFY_LOCATE_LEAF 22 /* bp_r1cs_batch_verify_locate: a failing subset of at most this many instances is decided by the machinery of
                                      * bp_verifier_verify_batch instead of being split further (0 = default: 1, pure bisection; at most 4096) */
#define BP_TUNE_VFY_CLASS_MIN 24   /* (23, like 20, stays unassigned: tests/test_verify_locate_cpu.py pins it as refused.)  Batches of several gadgets: the
                                    * fewest members a class of like-instances needs to run its front end on the device; smaller classes join the host
                                    * replay of the call's remainder.  0 = default: 65535, i.e. the class path is OPT-IN — measured, see "Batches of
                                    * several gadgets" below; 1 = every class; values above 65535 act as 65535.  Results never depend on it */
int bp_ctx_set_tuning(bp_ctx* ctx, int knob, uint64_t value);

/* The O(N) part of `Verifier::verification_scalars` (src/r1cs/verifier.rs:465-514, s from inner_product_proof.rs:279-311) for a
 * caller that records constraints and replays the transcript itself: from the flattened wL, wR, wO (n each; zero beyond n), the
 * challenges y, x, u (phase-2 separator), the proof's a, b and the k inner-product challenges u_j (creation order), with
 * n1 phase-1 multipliers and padded size N = 2^k:
 *   g[i] = u_or_1(i) * (x * y^-i * wR[i] - a * s[i]),   h[i] = u_or_1(i) * (y^-i * (x * wL[i] + wO[i] - b * s[N-1-i]) - 1),  i < N
 * (u_or_1 = 1 for i < n1, u otherwise), written as CANONICAL integers — the form the mega-check MSM consumes (bp_msm_gens with
 * scalars_canonical = 1).  All inputs ark Montgomery words. */
int bp_r1cs_verification_gh(bp_ctx* ctx, size_t n, size_t n1, const uint64_t* wL, const uint64_t* wR, const uint64_t* wO, const uint64_t y[4],
                            const uint64_t x[4], const uint64_t u[4], const uint64_t a[4], const uint64_t b[4], const uint64_t* ipa_challenges, size_t k,
                            uint64_t* g_out, uint64_t* h_out);

/* ---- unit-test hooks: one field / group operation per element on the GPU -------------------------- */
/* field: 2*curve + (0 base field | 1 scalar field); op: 0 mul, 1 add, 2 sub, 3 sqr, 4 inv */
int bp_debug_field_op(bp_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n);
/* the reference's two fixed-value unit tests, through the kernels' own code paths: out[i] = x^i, i < n (`exp_iter`, src/util.rs:55-58,
 * test :147-157) by the power-table routine the prover / verifier kernels use; and <a, b> over the ctx's scalar field
 * (`inner_product`, src/inner_product_proof.rs:390-399, tests :556-562 and src/util.rs:160-166) by the kernels that form
 * c_L = <a_L, b_R> in InnerProductProof::create.  Inputs / outputs: ark Montgomery words. */
int bp_debug_exp_iter(bp_ctx* ctx, const uint64_t x[4], size_t n, uint64_t* out);
int bp_debug_inner_product(bp_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t out[4]);
/* ark-serialize compressed SW points (33 bytes each: x LE || flag byte) -> affine, on the GPU (the square roots of
 * `R1CSProof::from_bytes`, src/r1cs/proof.rs:83-91); out_ok[i] = 0 for malformed or off-curve encodings */
int bp_debug_decompress(bp_ctx* ctx, const uint8_t* compressed33, size_t n, uint64_t* out_xy, uint32_t* out_ok);
/* host only: GLV split of a fold multiplier t (ark words, curve 0 only): masks = p1[5] m1[5] p2[5] m2[5] signed-digit bit masks
 * with t = t1 + lambda*t2 (mod r); lambda_out = canonical lambda.  The uniform IPA fold (src/inner_product_proof.rs:139-150)
 * runs its ladder over these 130-digit halves on secq256k1. */
int bp_debug_glv_decompose(int curve, const uint64_t t[4], uint32_t masks[20], uint64_t lambda_out[4]);
/* ---- verifier front end on the device (csrc/vfe.hip, csrc/vfe_sched.hpp) ------------------------------------------------------
 * For a batch of like-instances of ONE single-phase statement bp_r1cs_batch_verify / bp_r1cs_batch_verify_scenarios run the
 * per-proof front of `batch_verify` (src/r1cs/verifier.rs:604-691) on the GPU: R1CSProof::from_bytes' point decompression
 * (src/r1cs/proof.rs:83-91), the merlin transcript replay of verification_scalars (verifier.rs:403-460, 516-519;
 * src/inner_product_proof.rs:266-280; src/transcript.rs:45-102: Keccak-f[1600] / STROBE-128 / ChaCha20 -> Fr::rand) and the
 * O(k + m) challenge arithmetic (:462-541).  Anything unusual (malformed bytes, an identity point that
 * validate_and_append_point rejects) takes the host replay instead, which reports the reference's error; see "A reject flag per
 * proof" and "Batches of several gadgets" below for how much of the batch that is.
 * ARKBP_VFY_HOST=1 in the environment forces the host replay (A/B).
 * Two-phase statements (randomized constraints) take this path with BP_TUNE_VFY_DEVICE = 2 only: the device derives every
 * challenge, the gadget challenges of the callbacks included; the host then runs each instance's callbacks with its own
 * challenges preset — on the instance's own handle, so a C callback records through the bp_cs it receives, and
 * bp_cs_challenge_scalar returns the preset value for the expected label — and the device consumes the per-proof coefficient
 * tables they produce.  Instance 0's callbacks run once beforehand on a copy of its live transcript; they fix the labels and
 * the phase-2 structure.  The batch goes to the host replay instead when any instance draws other labels, records another
 * structure (multipliers, constraint offsets, variables, which coefficients are +-1 or shared), or when the per-proof gadget
 * challenges and coefficient tables would exceed 256 MiB.  The callbacks then run again there: nothing they recorded under
 * the preset challenges is kept.
 *
 * bp_debug_vfe_schedule_replay (host only, no GPU): builds the data-independent sponge schedule of one verification — transcript
 * at state203 (bp_transcript_export_state), m commitments (absorbed as items 0..m-1 when absorb_commitments), k rounds, n = the
 * padded multiplier count appended under "n" — and runs it on the CPU over `items` (72 bytes each: a 65-byte uncompressed point
 * or a 32-byte scalar, zero padded; order: [commitments] A_I1 A_O1 S1 A_I2 A_O2 S2 T_1 T_3 T_4 T_5 T_6 L[k] R[k] t_x t_x_blinding
 * e_blinding).  seeds_out: (6 + k) x 32 bytes, the challenge_bytes outputs y z u x w u_1..u_k r; *nblocks_out = permutations.
 * bp_debug_vfe_challenges (GPU): the same through k_vfe_points + k_vfe_sponge for `count` proofs of one shape (proof_len bytes
 * each; commit_xy count x m x 8 words, ark layout; states203: count x 203 bytes, or one when shared_state): seeds_out as above per
 * proof, chal_out the derived challenge scalars (count x (6 + k) x 4 ark words), *status_out the OR of the kernels' reject bits
 * (1 malformed, 2 identity under validation, 4 framing).
 * bp_debug_vfe_schedule_replay_2phase (host only): the same for a two-phase statement whose callbacks draw the gadget challenges
 * labels[0..nlabels) in this order ("r1cs-2phase" separator after S1, the squeezes before A_I2); seeds_out: (6 + k + nlabels) x 32
 * bytes in the order y z u x w u_1..u_k r g_1..g_nlabels.
 * bp_ctx_vfe_stats: batches the device front end completed / batches it handed to the host replay on this ctx (two-phase
 * batches included).
 *
 * A reject flag per proof.  Beside the batch-wide status word k_vfe_points keeps one word per proof with the same bits.  A call
 * whose only obstacle is a flagged proof cannot succeed, so it runs no mega-check: the host replays ONLY the flagged instances (in
 * instance order, as a batch of their own) and the call returns what that replay returns — the host replay's answer for the whole
 * batch, because every instance that fails before its check is among them.  Should that replay find nothing wrong (never expected),
 * the whole batch is replayed as before.  Such a call still counts one host_fallback and no device_batch.  Two-phase batches
 * (BP_TUNE_VFY_DEVICE = 2) learn of a flag in the middle of their chain and replay the whole batch.
 *
 * Batches of several gadgets.  A verifying service sees a few gadget shapes mixed in arrival order.  When the batch as a whole is not
 * one class of like-instances, the instances are partitioned: like-instances share the recording (cs->base of a handle, the source
 * of a scenario statement), the commitment count and form (affine, or wire bytes still pending), the proof length, the transcript
 * position, and being single-phase.  Classes are ordered by size, largest first, ties by their first member; the largest
 * BP_VFY_MAX_CLASSES classes with at least BP_TUNE_VFY_CLASS_MIN members become DEVICE CLASSES.  They run back to back on the
 * ctx's stream — k_vfe_points, k_vfe_sponge, the challenge arithmetic, k_vfy_tables / k_vfy_batch per block of 512, each class on
 * its own slice of one staging area — into ONE pair of g / h accumulators sized for the largest N, ONE tail array, with one result
 * slot per class and block (96 blocks per call over all classes); then one copy back, ONE wait, ONE mega-check MSM.  Everything
 * else is the REMAINDER: smaller classes, classes beyond the eighth or beyond the 96 blocks, two-phase classes (they stay on the
 * host replay, whatever BP_TUNE_VFY_DEVICE says), instances without a shared recording, and every member of a class the front end's
 * own entry conditions decline (k >= 32, too few generators, N != 2^k, the 2^31 limits).  The remainder is ONE host replay with its
 * own check point; pending wire commitments are decoded and committed for its members only, a device class keeps its bytes
 * pending.  The call's check point is the group sum of the two points, which by linearity is the reference's single MSM
 * (verifier.rs:685); the batch is accepted iff no instance failed before its check and that sum is the identity.  A flagged
 * proof in a device class is handled as above: the flagged instances and the remainder are replayed as one subset.  The passes of
 * bp_r1cs_batch_verify_locate take the same path.  A sharded ctx, ARKBP_VFY_HOST and BP_TUNE_VFY_DEVICE = 0 keep the host replay.
 * The default of BP_TUNE_VFY_CLASS_MIN is 65535: measured against the host replay of the same members (tools/exp_vfy_mixed.py,
 * profiles/r15_vfy_mixed.txt; one run on one MI355X, 16 host threads, one call at a time), two classes of cfg4's statement with 8 .. 512
 * members each were SLOWER on the device at every size (7.6 against 1.4 ms at 8, 11.6 against 5.4 ms at 512; 2 x 2048: 21.6 against
 * 16.0 ms), so no crossover exists in that range and the class path is opt-in.  Each class adds the latency of its own k_vfe_sponge
 * (about 3 ms, one lane per proof, whatever the class size) to the one stream.  The host threads a call keeps busy were not
 * measured: a device class costs the host one staging memcpy, the host replay a transcript replay per proof on the ctx's pool.  A
 * service for which that matters more than one call's latency sets the knob to the smallest class it wants on the device.
 * bp_ctx_vfe_class_stats, since ctx creation: calls that took the class path / classes the device finished / their members /
 * instances the host replay took in such calls / instances replayed because the device flagged something, on either path (in a class
 * call: the flagged ones and the remainder, which are replayed together).  bp_ctx_vfe_stats is not touched by an unflagged class call.
 * bp_debug_vfy_class_plan (host only): the partition itself.  keys: one 64-bit class key per instance; eligible (may be NULL: all):
 * 0 keeps an instance in the remainder; class_min / max_classes: 0 = the defaults (the knob's, BP_VFY_MAX_CLASSES).  class_of[k]:
 * the device class of instance k in launch order, or -1 for the remainder; *nclasses: device classes. */
#define BP_VFY_MAX_CLASSES 8
int bp_ctx_vfe_class_stats(bp_ctx* ctx, uint64_t* class_calls, uint64_t* device_classes, uint64_t* device_instances, uint64_t* remainder_instances,
                           uint64_t* flagged_replayed);
int bp_debug_vfy_class_plan(size_t count, const uint64_t* keys, const uint8_t* eligible, uint64_t class_min, uint32_t max_classes, int32_t* class_of, uint32_t* nclasses);
int bp_debug_vfe_schedule_replay(const uint8_t state203[203], int absorb_commitments, uint64_t m, uint32_t k, uint64_t n, const uint8_t* items, uint8_t* seeds_out,
                                 uint32_t* nblocks_out);
int bp_debug_vfe_schedule_replay_2phase(const uint8_t state203[203], int absorb_commitments, uint64_t m, uint32_t k, uint64_t n, const char* const* labels, size_t nlabels,
                                        const uint8_t* items, uint8_t* seeds_out, uint32_t* nblocks_out);
int bp_debug_vfe_challenges(bp_ctx* ctx, size_t count, const uint8_t* proofs, size_t proof_len, const uint64_t* commit_xy, size_t m, const uint8_t* states203,
                            int shared_state, int absorb_commitments, uint8_t* seeds_out, uint64_t* chal_out, uint32_t* status_out);
int bp_ctx_vfe_stats(bp_ctx* ctx, uint64_t* device_batches, uint64_t* host_fallbacks);
/* MSMs over the generator tables that took the fixed-base schedule (bp_gens_msm_tables) on this ctx, and how many of those ran on a
 * rank's share of the terms of a sharded proof (blocks of a commitment's terms, the strided slice of the first IPA round) */
int bp_ctx_msm_stats(bp_ctx* ctx, uint64_t* fixed_base_runs, uint64_t* fixed_base_runs_sharded);
/* The small-statement path (BP_TUNE_DIRECT_MAX): MSMs this ctx answered from its direct window tables, and the number of generators
 * per vector those tables cover (0 = not built yet) */
int bp_ctx_direct_stats(bp_ctx* ctx, uint64_t* direct_msms, size_t* bases_per_vector);
/* Two fold rounds from the tables (bp_gens_fold_tables over 3N/4 bases; src/inner_product_proof.rs:143-155, 219-224): first folds this
 * ctx deferred, and second folds it then produced straight from the tables — on one GPU and, since round 4, on the index-cyclic slice
 * of a sharded prover */
int bp_ctx_fold_stats(bp_ctx* ctx, uint64_t* deferred_first_folds, uint64_t* second_folds_from_tables);
/* Paired MSMs (BP_TUNE_MSM_PAIR): passes in which the L and R MSMs of an inner-product round ran as two jobs of one launch chain on
 * this ctx, and the jobs of those passes that were redone alone on the general path because their scalars overflowed the fixed
 * shape (skewed scalars; the other job's result stands).  A round that does not qualify — sharded ctx, fixed-base rows, direct
 * tables, fewer terms than BP_TUNE_MSM_BIN_MIN, the knob off — runs its two MSMs one after the other and counts nothing */
int bp_ctx_msm_pair_stats(bp_ctx* ctx, uint64_t* paired_passes, uint64_t* jobs_redone);
/* A ctx WITHOUT a device for sanitizer runs of the host layer on machines with no GPU (tools/sanitize/): only bp_r1cs_batch_verify,
 * bp_r1cs_batch_verify_scenarios, bp_ctx_set_tuning and bp_ctx_destroy accept it.  They run the complete host side of batch
 * verification — framing, square roots (on the host here), thread pools, shared recordings, transcript replay (live and lockstep),
 * template cache and eviction, staging — and skip every kernel, copy and the mega-check: NOTHING IS VERIFIED.  The status is that of
 * the host replay (format / validation errors in instance order); check_point_xy receives [checksum of everything the host staged,
 * count, launched groups, 0 ..] so that runs with different thread counts and replay modes can be compared.  gens_capacity: the
 * generator count the ctx pretends to hold. */
int bp_debug_ctx_create_hostonly(int curve, size_t gens_capacity, bp_ctx** out);
/* host only (no GPU): the Fiat-Shamir challenges y z u x w u_1..u_k r of up to eight scenario verifications (flat arrays as in
 * bp_r1cs_batch_verify_scenarios), derived by the per-proof live transcript replay (use_x8 = 0: verify_prepare over the instance's own
 * merlin transcript, src/r1cs/verifier.rs:403-460 + :516-519) or by the lockstep replay of eight same-shaped single-phase instances
 * (use_x8 = 1; AVX-512 Keccak-f x8).  out: count x 40 x 4 ark words, nchal[j] = challenges of instance j.  Returns 1 (not an error
 * code) when the lockstep replay does not apply: fewer than eight instances, differing shapes, a randomized phase, no AVX-512. */
int bp_debug_verify_challenges(int curve, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                               const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, int use_x8, uint64_t* out,
                               size_t* nchal);
/* op: 0 P+Q (general add), 1 P+Q (mixed add), 2 2P, 3 k*P (k canonical, one per element) */
int bp_debug_point_op(bp_ctx* ctx, int op, const uint64_t* p_xy, const uint64_t* q_xy, const uint64_t* k, uint64_t* out_xy, size_t n);
/* The same on RAW representatives: operands and results are the nine 32-bit limbs of the device's radix-2^29 form, no conversion
 * either way, so a test can feed any legal representative (lazy limbs, values in [p, 2p) ..) and inspect the limbs that come back.
 * csrc/dbg_raw.cuh lists the ops (RAW_F_*, RAW_P_*) and is what the CPU harness csrc/fp29_selftest.cpp runs as well.
 * field_raw: in n x 36 words (a | b | c | d), out n x 18 words.  point_raw (the ctx's curve): in n x 54 words (P.X P.Y P.Z Q.X Q.Y
 * Q.Z; the mixed additions read Q.X, Q.Y as the affine operand), out n x 28 words (X Y Z flag) for ops 0..3 (jac_add, jac_madd,
 * jac_dbl, jac_madd_fast with flag = rare) and n x 4 x 28 for the quad-cooperative ops 4..6 (qjac_add, qjac_madd, qjac_dbl): one
 * case runs in four adjacent lanes, 64 different cases per block, and every lane's result comes back. */
int bp_debug_field_raw(bp_ctx* ctx, int field, int op, const uint32_t* in, uint32_t* out, size_t n);
int bp_debug_point_raw(bp_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif
