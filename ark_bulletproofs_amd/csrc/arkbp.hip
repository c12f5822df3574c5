// libarkbp_hip.so — context, workspaces, host orchestration and the C ABI (include/arkbp.h).
// There is no CPU fallback: without a HIP device every compute entry point returns BP_E_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <sys/prctl.h>
#include <time.h>
#include <rccl/rccl.h>   // types only: the entry points are bound with dlsym (rccl_api)
#include <dlfcn.h>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <deque>
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>
#include "../../include/arkbp.h"
#include <atomic>
#include <chrono>
#include "host_proto.hpp"
#include "prove_steps.hpp"
#include "gens_digest.hpp"
#include "ipa_plan.hpp"
#include "vfy_dev_plan.hpp"
#include "r1cs.cuh"
#include "pedersen.cuh"
#include "small.cuh"
#include "small_batch.cuh"
#include "small_batch_front.cuh"
#include "witness_check.cuh"
#include "witness_dev.cuh"
#include "vfy_each.cuh"
#include "msm_batch.cuh"
#include "vfe.hpp"
#include "vfe_sched.hpp"
static_assert(arkbp::vfe::PB_WORDS == arkbp::VFY_PB_WORDS, "parameter block layout shared by vfe.hip and r1cs.cuh");

using namespace arkbp;
using arkbp::host::A4;
using arkbp::host::F4;
using arkbp::host::J4;
using arkbp::host::HostCsc;
using arkbp::host::build_host_csc;
using arkbp::host::HostRowIndex;
using arkbp::host::build_row_index;
using arkbp::host::jac_from_words;
using arkbp::host::to_aff_many;

static thread_local std::string g_err;
const char* bp_last_error(void) { return g_err.c_str(); }

// ---- host-only dry run (sanitizer builds on machines without a GPU; include/arkbp.h bp_debug_ctx_create_hostonly) ------------------
// A ctx created without a device runs the HOST side of batch verification — framing, thread pools, shared recordings, transcript
// replay, template cache and eviction, staging — with every HIP call replaced: "device" buffers are zeroed host memory, copies are
// memcpy, kernels / streams / events are skipped.  Nothing is verified in that mode (the entry points return a checksum of what the
// host staged instead of the mega-check); it exists so that ASan / UBSan / TSan see the multi-threaded host layer (tools/sanitize/).
// g_dry is set, per calling thread, by the entry points that accept such a ctx; the library's own pool threads make no HIP calls.
static thread_local bool g_dry = false;
namespace dry {
static char g_token;   // stands for streams and events
template <class T> static inline hipError_t Malloc(T** p, size_t n) { if (g_dry) { *p = (T*)calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; } return ::hipMalloc(p, n); }
static inline hipError_t Free(void* p) { if (g_dry) { free(p); return hipSuccess; } return ::hipFree(p); }
template <class T> static inline hipError_t HostMalloc(T** p, size_t n, unsigned flags = hipHostMallocDefault) { if (g_dry) { *p = (T*)calloc(1, n ? n : 1); return *p ? hipSuccess : hipErrorOutOfMemory; } return ::hipHostMalloc(p, n, flags); }
static inline hipError_t HostFree(void* p) { if (g_dry) { free(p); return hipSuccess; } return ::hipHostFree(p); }
static inline hipError_t MemcpyAsync(void* d, const void* s_, size_t n, hipMemcpyKind k, hipStream_t st) { if (g_dry) { if (n) memmove(d, s_, n); return hipSuccess; } return ::hipMemcpyAsync(d, s_, n, k, st); }
static inline hipError_t MemsetAsync(void* d, int v, size_t n, hipStream_t st) { if (g_dry) { if (n) memset(d, v, n); return hipSuccess; } return ::hipMemsetAsync(d, v, n, st); }
static inline hipError_t GetLastError() { return g_dry ? hipSuccess : ::hipGetLastError(); }
static inline hipError_t SetDevice(int d) { return g_dry ? hipSuccess : ::hipSetDevice(d); }
static inline hipError_t StreamSynchronize(hipStream_t st) { return g_dry ? hipSuccess : ::hipStreamSynchronize(st); }
static inline hipError_t StreamCreateWithFlags(hipStream_t* st, unsigned f) { if (g_dry) { *st = (hipStream_t)&g_token; return hipSuccess; } return ::hipStreamCreateWithFlags(st, f); }
static inline hipError_t StreamDestroy(hipStream_t st) { return g_dry ? hipSuccess : ::hipStreamDestroy(st); }
static inline hipError_t EventCreate(hipEvent_t* e) { if (g_dry) { *e = (hipEvent_t)&g_token; return hipSuccess; } return ::hipEventCreate(e); }
static inline hipError_t EventCreateWithFlags(hipEvent_t* e, unsigned f) { if (g_dry) { *e = (hipEvent_t)&g_token; return hipSuccess; } return ::hipEventCreateWithFlags(e, f); }
static inline hipError_t EventDestroy(hipEvent_t e) { return g_dry ? hipSuccess : ::hipEventDestroy(e); }
static inline hipError_t EventRecord(hipEvent_t e, hipStream_t st) { return g_dry ? hipSuccess : ::hipEventRecord(e, st); }
static inline hipError_t EventSynchronize(hipEvent_t e) { return g_dry ? hipSuccess : ::hipEventSynchronize(e); }
static inline hipError_t EventQuery(hipEvent_t e) { return g_dry ? hipSuccess : ::hipEventQuery(e); }
static inline hipError_t EventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) { if (g_dry) { *ms = 0; return hipSuccess; } return ::hipEventElapsedTime(ms, a, b); }
}  // namespace dry
#define hipMalloc(...) dry::Malloc(__VA_ARGS__)
#define hipFree(...) dry::Free(__VA_ARGS__)
#define hipHostMalloc(...) dry::HostMalloc(__VA_ARGS__)
#define hipHostFree(...) dry::HostFree(__VA_ARGS__)
#define hipMemcpyAsync(...) dry::MemcpyAsync(__VA_ARGS__)
#define hipMemsetAsync(...) dry::MemsetAsync(__VA_ARGS__)
#define hipGetLastError(...) dry::GetLastError(__VA_ARGS__)
#define hipSetDevice(...) dry::SetDevice(__VA_ARGS__)
#define hipStreamSynchronize(...) dry::StreamSynchronize(__VA_ARGS__)
#define hipStreamCreateWithFlags(...) dry::StreamCreateWithFlags(__VA_ARGS__)
#define hipStreamDestroy(...) dry::StreamDestroy(__VA_ARGS__)
#define hipEventCreate(...) dry::EventCreate(__VA_ARGS__)
#define hipEventCreateWithFlags(...) dry::EventCreateWithFlags(__VA_ARGS__)
#define hipEventDestroy(...) dry::EventDestroy(__VA_ARGS__)
#define hipEventRecord(...) dry::EventRecord(__VA_ARGS__)
#define hipEventSynchronize(...) dry::EventSynchronize(__VA_ARGS__)
#define hipEventQuery(...) dry::EventQuery(__VA_ARGS__)
#define hipEventElapsedTime(...) dry::EventElapsedTime(__VA_ARGS__)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) do { if (!g_dry) { hipLaunchKernelGGLInternal(__VA_ARGS__); } } while (0)

#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                     \
            g_err = std::string(#x) + ": " + hipGetErrorString(e_);                                 \
            return BP_E_HIP;                                                                        \
        }                                                                                           \
    } while (0)
#define BPCHK(x) do { int r_ = (x); if (r_ != BP_OK) return r_; } while (0)

// ---- native collectives: RCCL over xGMI (BASELINE north_star: "final RCCL point-reduce over xGMI") --------------------------------
// The library does not link librccl: it binds the five entry points it needs at run time from the RCCL the process already has
// (a PyTorch-ROCm host brings its own copy) or from the ROCm installation, so a single-GPU host never loads RCCL at all.
struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string why;
};
static RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, [] {
        void* h = nullptr;
        const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
        // ARKBP_RCCL_LIB names the library to bind instead (tests point it at a path that does not exist to drive the error path)
        const char* forced = getenv("ARKBP_RCCL_LIB");
        std::string last_err;
        auto try_open = [&](const char* n, int flags) {
            h = dlopen(n, flags);
            if (!h) { const char* e = dlerror(); if (e) last_err = e; }   // dlerror() clears the message it returns: read it ONCE
            return h != nullptr;
        };
        if (forced) try_open(forced, RTLD_NOW | RTLD_GLOBAL);
        else {
            for (const char* n : names) if (try_open(n, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL)) break;   // the copy the process already mapped
            if (!h) for (const char* n : names) if (try_open(n, RTLD_NOW | RTLD_GLOBAL)) break;
        }
        if (!h) { api.why = std::string("librccl not found: ") + last_err; return; }
        api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(h, "ncclGetUniqueId");
        api.CommInitRank = (decltype(api.CommInitRank))dlsym(h, "ncclCommInitRank");
        api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
        api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
        api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
        api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllGather && api.GetErrorString;
        if (!api.ok) api.why = "librccl lacks an expected entry point";
    });
    return api;
}

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    bool owned = true;  // false: a view of another ctx's allocation (shared generator tables)
    int ensure(size_t bytes) {
        if (bytes <= cap) return BP_OK;
        if (!owned) { g_err = "shared device buffer too small"; return BP_E_ARG; }
        if (p) HIPCHK(hipFree(p));
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        HIPCHK(hipMalloc(&p, want));
        cap = want;
        return BP_OK;
    }
    // exactly `bytes` (the large precomputed tables: the 25 % growth slack of ensure() would be tens of GB)
    int ensure_exact(size_t bytes) {
        if (bytes <= cap) return BP_OK;
        if (!owned) { g_err = "shared device buffer too small"; return BP_E_ARG; }
        if (p) HIPCHK(hipFree(p));
        p = nullptr; cap = 0;
        HIPCHK(hipMalloc(&p, bytes + 256));
        cap = bytes + 256;
        return BP_OK;
    }
    // buffers whose kernels rely on "all zero between uses" (and restore it themselves): zeroed once, when (re)allocated
    int ensure_zeroed(size_t bytes, hipStream_t st) {
        if (bytes <= cap) return BP_OK;
        int rc = ensure(bytes);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(p, 0, cap, st));
        return BP_OK;
    }
    void release() { if (p && owned) (void)hipFree(p); p = nullptr; cap = 0; owned = true; }
    template <class T> T* as() { return (T*)p; }
};
// Pinned host staging that only grows: at least `bytes`, allocated with `slack` bytes on top (each site's own rule)
static int pinned_ensure(void*& p, size_t& cap, size_t bytes, size_t slack) {
    if (cap >= bytes) return BP_OK;
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr; cap = 0;
    HIPCHK(hipHostMalloc(&p, bytes + slack));
    cap = bytes + slack;
    return BP_OK;
}

// Device copies of ONE shared recording's constraint indices (bp_prover_new_like; r1cs_host.inc pl_entry): the column index with its
// imported coefficient table, and — once a guarded proof has used it — the row index.  The key is the recording itself, held weakly:
// an entry whose recording is gone is purged before the next lookup, and a live recording's address cannot have been reused.
static constexpr size_t PL_CACHE_MAX = 8;
struct PlResident {
    std::weak_ptr<const host::FrozenRecording> key;
    DevBuf csc;    // [moff | ment | mc | coefs]
    size_t o_ment = 0, o_mc = 0, o_coefs = 0;
    bool have_csc = false;
    DevBuf row;    // [poff | pinfo | tvar | tcid | lrow | coefs]
    size_t r_pinfo = 0, r_tvar = 0, r_tcid = 0, r_lrow = 0, r_coefs = 0;
    const host::HostRowIndex* row_of = nullptr;   // the host index the row block was made from (owned by the recording)
    uint64_t used = 0;
    size_t bytes() const { return csc.cap + row.cap; }
    ~PlResident() { csc.release(); row.release(); }
};

struct KTimer {
    double ms = 0;
    uint64_t launches = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

struct IpaState {
    const u32 *d_Q = nullptr, *d_Gf = nullptr, *d_Hf = nullptr;
    u32 *d_G = nullptr, *d_H = nullptr, *d_a = nullptr, *d_b = nullptr;
    size_t n = 0;            // current vector length
    size_t round = 0;
    bool first = true;
    // pending common factors of the resident generator vectors: G_true = gamma_G * Ghat, H_true = gamma_H * Hhat
    F4 gamma_G, gamma_H;
    bool pending = false, h_geo = false;  // h_geo: H_true[i] = gamma_H * rho^i * Hhat[i]
    // optional hints of the R1CS prover (see ipa_create_dev)
    bool have_gf = false, have_rho = false;
    F4 gf_halves[2];
    const F4* rho_pw = nullptr;
    const u32* d_rho_pow = nullptr;
    bool lr_done = false;
    // frozen-generator tail (ipa.cuh): from length n0 on, G and H stay as they are and per-element coefficients fold instead
    bool allow_freeze = false, frozen = false;
    size_t n0 = 0;
    u32 *d_cG = nullptr, *d_cH = nullptr;
    // multi-GPU: how the L / R MSMs of this instance treat the ctx's shard mode (see msm_run): -1 = the ctx default (window
    // partition + point-reduce), 2 = this rank's terms are its own slice of the vectors (index-cyclic IPA): all windows, then the
    // point-reduce, 0 = replicated (every rank computes the same small MSM: the frozen tail after the gather)
    // gens_stride > 0: the working vectors are (a slice of) the ctx's generator tables at round 1: d_G[i] = G[gens_first + i*gens_stride]
    u32 gens_first = 0, gens_stride = 0;
    // round 1 may read the generators straight from the ctx's resident tables (no working copy): non-null until the first fold
    const u32 *d_G_in = nullptr, *d_H_in = nullptr;
    bool have_qw = false;      // Q = qw * B (the R1CS prover's Q, prover.rs:779): lets round 1 run as a fixed-base MSM over the tables
    F4 qw;
    int msm_mode = -1;
    // deferred first fold (ipa.cuh "TWO fold rounds from the tables"): round 1's multipliers are kept, G and H stay the generator
    // tables for one more round, and the second fold produces Ghat'' / Hhat'' straight from the tables
    bool deferred = false;
    F4 def_tG, def_tH;
    size_t min_len = 0;         // index-cyclic slices: the local length at which the ranks gather (a deferred fold needs one more local round)
    bool direct = false;        // frozen from round 1 over the ctx's generator tables, L and R as sums over the direct window tables (small.cuh)
    // direct: the fold a challenge asks for is carried out by the NEXT round's k_dt_round (or by k_ipa_fold_ab after the last round)
    bool fold_pending = false;
    F4 pend_u, pend_ui;
    u32 *d_a_alt = nullptr, *d_b_alt = nullptr;   // second buffer pair: a fused fold reads one pair and writes the other
    F4 geo_k0;                  // index-cyclic slices: the geometric H factor of local element j is K * rho^(rank + j*world) = (K * geo_k0) * (rho^world)^j
    bool have_k0 = false;
};

struct bp_ctx {
    int curve = 0, device = 0;
    bool host_only = false;      // no device behind this ctx: the host-side dry run of batch verification (see g_dry)
    hipStream_t stream = nullptr;
    bool profiling = false;
    size_t tune_fold_batch_min = 65536;   // BP_TUNE_FOLD_BATCH_MIN
    size_t tune_msm_bin_min = MsmKnobs().bin_min;         // BP_TUNE_MSM_BIN_MIN
    size_t tune_ipa_freeze_len = 8192;    // BP_TUNE_IPA_FREEZE_LEN (measured at 2^20, one proof at a time: 1024 -> 51.0 ms of inner-product argument, 4096 -> 49.0, 8192 -> 47.5, 16384 -> 46.8 with a slower prove() around it; throughput unchanged)
    size_t tune_msm_wsum_min = MsmKnobs().wsum_min;   // BP_TUNE_MSM_WSUM_MIN: buckets from which running-sum window aggregation replaces the marginals
    KTimer timers[BP_K_COUNT];
    std::vector<hipEvent_t> event_pool;
    // MSM workspaces
    DevBuf canon, hist, lvl_off, totals, cursor, entries, slots, bin_cur, boff, lvA, lvB, Tbuf, io_pts, io_scal, io_out;
    DevBuf fs_bcnt, fs_loff, fs_binch, fs_sums, fs_over;   // fixed-shape MSM pipeline (msm.cuh 7); fs_over: one overflow word per job
    int tune_msm_pair = 1;                        // BP_TUNE_MSM_PAIR: L and R of an inner-product round as two jobs of one launch chain (msm_run_pair)
    uint64_t pair_passes = 0, pair_redone = 0;    // paired passes completed / jobs of those redone on the general path (bp_ctx_msm_pair_stats)
    // IPA workspaces (resident layouts)
    DevBuf ipa_G, ipa_H, ipa_a, ipa_b, ipa_Gf, ipa_Hf, ipa_sL, ipa_sR, ipa_part, ipa_Q, ipa_jac, ipa_pref, ipa_cG, ipa_cH;
    // generator tables (BulletproofGens party 0, PedersenGens), resident layout
    DevBuf d_G, d_H, d_pc;
    DevBuf pc_table;   // fixed-base window tables of B, B_blinding (pedersen.cuh), built on first use
    DevBuf pc_dt;      // direct window tables of B, B_blinding (small.cuh k_dt_commit)
    size_t gens_cap = 0;
    A4 pc_B, pc_Bb;
    bool pc_set = false, pc_custom = false;   // pc_B / pc_Bb hold a pair / one that bp_pedersen_gens_install put there (default() otherwise)
    // R1CS prover / verifier vectors (resident scalar layout)
    DevBuf r_aL, r_aR, r_aO, r_sL, r_sR, r_wL, r_wR, r_wO, r_msmsc, r_ypow, r_part, r_small, r_g, r_h, r_chal, r_tail;
    // batch verification: per-proof parameter blocks, chunk partials; cached circuit templates (VTemplate<C>)
    DevBuf v_params, v_gpart, v_hpart, v_alpha, v_tables, v_dec;
    DevBuf p_moff, p_ment, p_mc, p_coefs, p_ztab;   // prover-side constraint index of the statement being proved (k_r1cs_flatten)
    // verifier front end on the device (vfe.hip; r1cs_host.inc batch_verify_device): raw inputs, serialized items, challenges, scratch
    DevBuf vfe_in, vfe_msg, vfe_chal, vfe_ws, vfe_small, vfe_flags;   // (vfe_flags: the kernels' reject bits per proof, beside the batch-wide word in vfe_small)
    void* h_vfe = nullptr;                    // pinned staging: [proof bytes | commitments | transcript states | small results]
    size_t h_vfe_cap = 0;
    DevBuf vfe2_sched, vfe2_voff, vfe2_vq, vfe2_vcid, vfe2_gch, vfe2_coef;   // two-phase batches: per-batch schedule, terms on commitments, gadget challenges, coefficient tables
    void* h_vfe2 = nullptr;                   // pinned: [gadget challenges | per-proof coefficient tables]
    size_t h_vfe2_cap = 0;
    std::map<std::string, std::shared_ptr<void>> vfe_classes;   // (shared recording, m, k, transcript position) -> VfeClassDev<C>
    int tune_vfy_device = 1;                  // BP_TUNE_VFY_DEVICE: 0 host replay, 1 single-phase like-instances on the device, 2 two-phase ones too
    uint64_t fb_runs = 0, fb_runs_sharded = 0; // fixed-base MSMs completed on this ctx / of those, on a rank's share of the terms of a sharded proof
    uint64_t vfe_batches = 0, vfe_fallbacks = 0;                 // batches the device front end completed / handed to the host replay
    uint64_t tune_vfy_class_min = 0;          // BP_TUNE_VFY_CLASS_MIN (0 = default: VFY_CLASS_MIN_DEFAULT)
    uint64_t vcl_calls = 0, vcl_classes = 0, vcl_instances = 0, vcl_remainder = 0, vcl_flagged = 0;   // bp_ctx_vfe_class_stats
    uint64_t cw_front_end = 0, cw_prologue_gpu = 0, cw_host = 0;  // wire commitments decoded by k_vfe_points / by k_points_decompress / by host roots
    void* h_vstage[2] = {nullptr, nullptr};   // pinned staging halves of the batch-verify pipeline
    size_t h_vstage_cap[2] = {0, 0};
    hipEvent_t vstage_ev[2] = {nullptr, nullptr};
    hipEvent_t vtail_ev[2] = {nullptr, nullptr};   // the tails of a block go up on aux_stream
    std::unique_ptr<host::HostPool> pool;     // host threads of this ctx's data-parallel loops (created on first use)
    hipEvent_t sync_ev = nullptr;             // blocking-sync event of ctx_stream_wait
    void* h_upload = nullptr;                 // pinned slab for the prover's witness uploads (r1cs_host.inc upload_scalars_pinned)
    size_t h_upload_cap = 0;
    void* h_csc = nullptr;                    // pinned staging of the prover's constraint index
    size_t h_csc_cap = 0;
    void* h_dec = nullptr;                    // pinned: x words, points, flags, ok of a batch's compressed points
    size_t h_dec_cap = 0;
    hipStream_t aux_stream = nullptr;         // point decompression runs beside the main stream
    hipEvent_t dec_ev[2] = {nullptr, nullptr};
    std::map<std::string, std::shared_ptr<void>> templates;          // structure digest -> VTemplate<C>
    std::map<std::string, std::shared_ptr<void>> scenario_sources;   // (scenario, params, publics) -> recorded, frozen verifier
    size_t scenario_source_terms = 0;
    void* h_vaux[2] = {nullptr, nullptr};     // pinned: launch order + per-instance coefficient tables of a block
    size_t h_vaux_cap[2] = {0, 0};
    // window-sharded multi-GPU mode (bp_ctx_set_window_shard): every MSM of this ctx accumulates only this rank's Pippenger
    // windows and the ranks' partial points are summed through the host's collective
    int shard_rank = 0, shard_world = 1;
    bp_point_reduce_cb shard_cb = nullptr;
    void* shard_user = nullptr;
    bp_allgather_cb gather_cb = nullptr;   // optional: lets the prover partition the IPA index-cyclically (bp_ctx_set_shard_allgather)
    void* gather_user = nullptr;
    // native collectives (bp_ctx_rccl_init): both exchanges of the sharded mode as ncclAllGather on the ctx's stream
    ncclComm_t nccl = nullptr;
    DevBuf coll_send, coll_recv;
    void* h_coll = nullptr;                // pinned: [send | recv]
    size_t h_coll_cap = 0;
    uint64_t coll_count = 0;
    double coll_seconds = 0;
    size_t tune_cyclic_min = (size_t)1 << 14;   // BP_TUNE_CYCLIC_MIN: padded size from which a sharded prover partitions the IPA
    size_t tune_msm_fixed_min = MsmKnobs().fixed_min;   // BP_TUNE_MSM_FIXED_MIN: terms from which MSMs over the generator tables use the fixed-base rows
    size_t tune_host_threads = 0;                  // BP_TUNE_HOST_THREADS: size of this ctx's host pool (0 = host_pool_threads())
    hipEvent_t sync_ev_aux = nullptr;              // event of ctx_aux_stream_wait
    unsigned tune_wait_sleep = 0;                  // BP_TUNE_WAIT_SLEEP: host waits poll and sleep this many microseconds in between instead of busy-waiting (see event_wait)
    bool msm_latency_first = false;                // set by the bp_msm* entry points for the duration of the call (see msm_use_quad)
    size_t tune_msm_chunk_cap = MsmKnobs().chunk_cap;                 // BP_TUNE_MSM_CHUNK_CAP: entries per level-1 chunk of the fixed-shape MSM pipeline (0 = fs_chunk_cap's choice)
    size_t tune_fold_quad_max = 0;                 // BP_TUNE_FOLD_QUAD_MAX: fold rounds with at most this many output points run four lanes per point (0 = never)
    size_t tune_msm_glv_min = MsmKnobs().glv_min;                 // BP_TUNE_MSM_GLV_MIN: terms from which an MSM on a GLV curve splits its scalars
    DevBuf cyc_a, cyc_b, cyc_Gf, cyc_Hf;
    // fixed-base MSM rows of the generators (bp_gens_msm_tables): row r of a table = 2^(4r) * base, r < FB_ROWS, layout [r][i]
    DevBuf fb_G, fb_H, fb_pc;
    size_t fb_cap = 0;       // bases covered per vector
    // fixed-base tables of the generators for the first fold round (bp_gens_fold_tables; ipa.cuh k_ipa_fold_tab)
    DevBuf ftab_G, ftab_H;
    size_t ftab_n = 0;       // bases covered: G[0..ftab_n), H[0..ftab_n)
    u32 ftab_first = 0, ftab_stride = 1;   // ... or, for a rank's SLICE of the tables (bp_gens_fold_tables_slice): column i = generator ftab_first + i * ftab_stride
    int ftab_w = 0, ftab_nwin = 0;
    // direct window tables of the first generators (small.cuh): bases [B, B_blinding | G[0..dt_cap) | H[0..dt_cap)], built on the first
    // small statement this ctx proves
    DevBuf dt_tab, dt_part, dt_a2, dt_b2, dt_ticket;
    size_t dt_cap = 0;
    size_t tune_direct_max = 8192;   // BP_TUNE_DIRECT_MAX: padded sizes up to this one prove over the direct tables (0 = never)
    u32* h_dt = nullptr;             // pinned: the results of one launch (or its partial points, see msm_direct_launch)
    u32 dt_pending_parts = 1;        // partial points per MSM on their way to h_dt
    u32 dt_last_nblk = 0;            // workgroups per MSM of the last msm_direct_launch (bp_debug_msm_direct reports it)
    uint64_t dt_runs = 0;            // MSMs answered from the direct tables
    // bp_prover_prove_batch: its own device arena and pinned staging (never the single-proof workspaces above), and its counters
    size_t tune_prove_batch = 0;     // BP_TUNE_PROVE_BATCH: most instances per lockstep group (0 = as many as PB_ARENA_BUDGET allows)
    DevBuf pb_arena;
    void* h_pb = nullptr;            // pinned
    size_t h_pb_cap = 0;
    uint64_t pb_lockstep = 0, pb_single = 0, pb_groups = 0;
    double pb_ipa_s = 0;             // seconds of lockstep inner-product rounds in the current call
    // ... and the stages in front of the argument run group-wide (prove_batch.inc "front groups"): what is public lives in pf_aux
    int tune_pb_front = 1;           // BP_TUNE_PROVE_BATCH_FRONT
    DevBuf pf_aux;
    void* h_pf = nullptr;            // pinned: witness staging, the aux block, results
    size_t h_pf_cap = 0;
    uint64_t pf_instances = 0, pf_groups = 0, pf_waits = 0;
    // witness check (witness_check.cuh): its index block on the device, the pinned staging, and the instances the most recent proving call refused
    DevBuf wc_dev;
    void* h_wc = nullptr;            // pinned: [the flags as they come back | the image of wc_dev]
    size_t h_wc_cap = 0;
    std::vector<std::pair<uint64_t, bp_witness_report>> unsat;
    uint64_t bx_scalars = 0, bx_launches = 0;   // BP_BLINDING_EXPANDED: scalars the expansion kernels wrote / their launches (bp_ctx_blinding_stats)
    // like-provers (bp_prover_new_like): device copies of their recordings' constraint indices, and the counters of bp_ctx_prover_like_stats
    std::vector<std::unique_ptr<PlResident>> pl_cache;   // at most PL_CACHE_MAX, the least recently used goes first
    uint64_t pl_clock = 0;
    uint64_t pl_uploads = 0, pl_hits = 0, pl_gates_dev = 0, pl_gates_host = 0;
    // witnesses assigned from device memory (bp_prover_assign_multipliers_dev): the flag words of k_wit_take, their pinned landing place, and the counters of bp_ctx_witness_dev_stats
    DevBuf wd_res;
    void* h_wd = nullptr;
    size_t h_wd_cap = 0;
    uint64_t wd_assigns = 0, wd_gates_dev = 0, wd_gates_down = 0;
    DevBuf pl_ztab;                  // the z^(2^j) of the proof in flight, when the coefficient table it would share a buffer with is resident
    // bp_verifier_verify_batch (verify_each.inc): its device arena and counters
    size_t tune_verify_each = 0;     // BP_TUNE_VERIFY_EACH: most instances per group (0 = what VE_ARENA_BUDGET holds, at most VE_GROUP_MAX)
    DevBuf ve_arena;
    uint64_t ve_grouped = 0, ve_single = 0, ve_groups = 0, ve_waits = 0;
    // bp_r1cs_batch_verify_locate: its knob and counters (calls, passes of the core, instances in them, instances decided exactly)
    size_t tune_verify_locate_leaf = 0;   // BP_TUNE_VERIFY_LOCATE_LEAF (0 = 1: pure bisection)
    uint64_t vl_calls = 0, vl_passes = 0, vl_instances = 0, vl_exact = 0;
    // bp_msm_batch (msm_batch.inc): its knobs (0 = the default) and counters; it stages in ve_arena
    uint64_t tune_msb_short = 0, tune_msb_slice = 0, tune_msb_max = 0, tune_msb_min_jobs = 0;   // BP_TUNE_MSM_BATCH_SHORT / _SLICE / _MAX / _MIN_JOBS
    uint64_t mb_short = 0, mb_bucketed = 0, mb_single = 0, mb_groups = 0, mb_waits = 0;
    uint64_t folds_deferred = 0, folds_tab2 = 0;   // first folds deferred / second folds that came straight from the tables (bp_ctx_fold_stats)
    u32 fold_took = 0;         // which fold kernels the launchers enqueued since the last reset (FOLD_TOOK_*; bp_debug_fold reports it)
    bool gens_derived = false; // the resident generators are a prefix of party 0's derived chain (bp_gens_derive), not caller-installed points
    IpaState ipa_step;         // bp_ipa_begin .. bp_ipa_finish
    bool ipa_step_active = false;
    u32* h_totals = nullptr;  // pinned
    void* h_T = nullptr;      // pinned: the result points of an MSM chain (msm_host_T_ensure)
    size_t h_T_cap = 0;
};

// The ctx's host pool: created by the first data-parallel loop over more than one index (`n`), the calling thread counts as one
static void host_pool_ensure(bp_ctx* ctx, size_t n) {
    if (ctx && n > 1 && !ctx->pool) ctx->pool.reset(new host::HostPool(std::max(1u, ctx->tune_host_threads ? (unsigned)ctx->tune_host_threads : host::host_pool_threads()) - 1));
}
// fn(lo), .., fn(hi - 1): on the pool when the ctx has one, inline otherwise (no ctx, no pool yet, a single index)
static void pool_range(bp_ctx* ctx, size_t lo, size_t hi, const std::function<void(size_t)>& fn) {
    if (hi <= lo) return;
    if (!ctx || !ctx->pool || hi - lo == 1) { for (size_t k = lo; k < hi; k++) fn(k); return; }
    ctx->pool->run(lo, hi, fn);
}
// off[k] = lens[0] + .. + lens[k - 1] for k <= count
static std::vector<size_t> prefix_offsets(const size_t* lens, size_t count) {
    std::vector<size_t> off(count + 1, 0);
    for (size_t k = 0; k < count; k++) off[k + 1] = off[k] + lens[k];
    return off;
}

static int get_event(bp_ctx* c, hipEvent_t* e) {
    if (!c->event_pool.empty()) { *e = c->event_pool.back(); c->event_pool.pop_back(); return BP_OK; }
    HIPCHK(hipEventCreate(e));
    return BP_OK;
}
// Host waits.  hipStreamSynchronize AND hipEventSynchronize busy-wait on this stack — also for events created with
// hipEventBlockingSync: measured 1.00 core of process CPU per waiting thread (tools/wait_cpu.py; a 2^22-term MSM: 117.3 ms of wall,
// 117.3 ms of CPU).  With eight proofs in flight that was seven cores of a 16-CPU quota doing nothing, and the quota was what bounded
// the prover pipeline (bench.py config.host_cpu_in_timed_region: 12.5 cores used, the cgroup throttled in a third of its periods).
// BP_TUNE_WAIT_SLEEP = 1 makes a ctx's waits poll the event and sleep ~50 us in between: one 2^20 proof then costs 20 ms of host CPU
// instead of 68 (wall 67.7 -> 68.9 ms) and the pipeline's throughput is unchanged at 7.9 instead of 12.5 cores — the setting for a
// prover service.  Batch verification waits far more often per millisecond of GPU work and lost 10 % with it, so the default stays
// the busy wait (ARKBP_SYNC=sleep / =spin force either everywhere); the bp_msm* entry points always busy-wait.
static void wait_thread_setup() {
    static thread_local bool done = false;
    if (!done) { done = true; (void)prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0); }   // 2 us of timer slack instead of 50: short sleeps stay short
}
static int wait_env() {   // -1: per ctx (BP_TUNE_WAIT_SLEEP), 0: busy wait everywhere, 1: sleeping waits everywhere
    static const int v = !getenv("ARKBP_SYNC") ? -1 : !strcmp(getenv("ARKBP_SYNC"), "sleep") ? 1 : !strcmp(getenv("ARKBP_SYNC"), "spin") ? 0 : -1;
    return v;
}
static unsigned wait_sleep_us(const bp_ctx* c) { const int e = wait_env(); return e == 0 ? 0u : (c && c->tune_wait_sleep) ? c->tune_wait_sleep : e == 1 ? 30u : 0u; }
static bool wait_sleeps(const bp_ctx* c) { return wait_sleep_us(c) != 0; }
static hipError_t event_wait(const bp_ctx* c, hipEvent_t ev) {
    if (!wait_sleeps(c)) return hipEventSynchronize(ev);
    wait_thread_setup();
    for (int it = 0;; it++) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return hipSuccess;
        if (e != hipErrorNotReady) return e;
        if (it < 3) continue;                              // (a wait that is over within a few microseconds costs no sleep)
        const long ns = (long)wait_sleep_us(c) * 1000L;
        struct timespec ts = {0, it < 40 ? ns : 2 * ns};
        nanosleep(&ts, nullptr);
    }
}
static hipError_t stream_wait(bp_ctx* c, hipStream_t stream, hipEvent_t& ev) {
    if (!wait_sleeps(c)) return hipStreamSynchronize(stream);
    if (!ev) { hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming); if (e != hipSuccess) return e; }
    hipError_t e = hipEventRecord(ev, stream);
    if (e != hipSuccess) return e;
    return event_wait(c, ev);
}
static hipError_t ctx_stream_wait(bp_ctx* c) {
    if (c->msm_latency_first) return hipStreamSynchronize(c->stream);
    return stream_wait(c, c->stream, c->sync_ev);
}
static hipError_t ctx_aux_stream_wait(bp_ctx* c) { return stream_wait(c, c->aux_stream, c->sync_ev_aux); }
// all-gather of `bytes` host bytes per rank -> recv (world x bytes, rank order): ncclAllGather on the ctx's stream between a pinned
// H2D and a pinned D2H copy; the stream order puts it behind the kernels already enqueued
static int ctx_native_allgather(bp_ctx* c, const void* send, size_t bytes, void* recv) {
    RcclApi& api = rccl_api();
    const size_t W = (size_t)c->shard_world;
    const auto t0 = std::chrono::steady_clock::now();
    BPCHK(c->coll_send.ensure(bytes)); BPCHK(c->coll_recv.ensure(bytes * W));
    if (c->h_coll_cap < bytes * (W + 1)) {
        if (c->h_coll) HIPCHK(hipHostFree(c->h_coll));
        c->h_coll = nullptr; c->h_coll_cap = 0;
        HIPCHK(hipHostMalloc(&c->h_coll, bytes * (W + 1) + 4096));
        c->h_coll_cap = bytes * (W + 1) + 4096;
    }
    memcpy(c->h_coll, send, bytes);
    HIPCHK(hipMemcpyAsync(c->coll_send.p, c->h_coll, bytes, hipMemcpyHostToDevice, c->stream));
    const ncclResult_t r = api.AllGather(c->coll_send.p, c->coll_recv.p, bytes, ncclUint8, c->nccl, c->stream);
    if (r != ncclSuccess) { g_err = std::string("ncclAllGather: ") + api.GetErrorString(r); return BP_E_HIP; }
    HIPCHK(hipMemcpyAsync((char*)c->h_coll + bytes, c->coll_recv.p, bytes * W, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    memcpy(recv, (char*)c->h_coll + bytes, bytes * W);
    c->coll_count++;
    c->coll_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return BP_OK;
}
// the two exchanges of the sharded mode, through RCCL when the ctx has a communicator, else through the host's callbacks
static int shard_allgather(bp_ctx* c, const void* send, size_t bytes, void* recv) {
    if (c->nccl) return ctx_native_allgather(c, send, bytes, recv);
    if (!c->gather_cb) { g_err = "sharded mode: no all-gather installed"; return BP_E_ARG; }
    const int rc = c->gather_cb(c->gather_user, send, bytes, recv);
    if (rc) { g_err = "the all-gather callback failed"; return rc < 0 ? rc : BP_E_ARG; }
    return BP_OK;
}
static inline bool shard_has_allgather(const bp_ctx* c) { return c->nccl || c->gather_cb; }

struct ScopedK {  // records start/stop events around a region when profiling is on
    bp_ctx* c; int which; hipEvent_t e0 = nullptr, e1 = nullptr; bool on;
    ScopedK(bp_ctx* c_, int w) : c(c_), which(w), on(c_->profiling) {
        if (on) { if (get_event(c, &e0) || get_event(c, &e1)) { on = false; return; } (void)hipEventRecord(e0, c->stream); }
    }
    void stop() { if (on) { (void)hipEventRecord(e1, c->stream); c->timers[which].pending.push_back({e0, e1}); on = false; } }
    ~ScopedK() { stop(); }
};
static void collect_timers(bp_ctx* c) {
    for (int k = 0; k < BP_K_COUNT; k++) {
        for (auto& pr : c->timers[k].pending) {
            float ms = 0;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                c->timers[k].ms += ms; c->timers[k].launches++;
            }
            c->event_pool.push_back(pr.first); c->event_pool.push_back(pr.second);
        }
        c->timers[k].pending.clear();
    }
}

extern "C" int bp_points_import(bp_ctx* c, const void* d_in, void* d_out, size_t n);

// ---- MSM orchestration ---------------------------------------------------------------------------
// The shapes — windows, bins, slots, chunk sizes, per-job strides — are made by msm_plan.hpp, pure functions of (terms, scalar bits,
// MsmKnobs) that its self-test checks on the CPU; here the knobs are filled and the kernels launched.
// Policy of the latency-first knob (measured, profiles/r03_msm_quad_glv_ab.txt): the GLV split and the quad-cooperative additions in
// the latency-bound kernels of the fixed-shape pipeline (ecq.cuh; against the lane-per-addition kernels: profiles/r03_msm_quad_ab.txt)
// shorten ONE mid-size MSM (2^16 terms: 0.607 -> 0.513 ms wall) but do not lower its arithmetic — the split adds an endomorphism
// product to every second mixed addition, a quad addition issues 20 products where a lane issues 16 — so a caller that keeps the GPU
// full with many MSMs in flight (the prover pipeline: eight streams) gains nothing and pays ~5 % on the accumulate.  They are
// therefore used where the caller waits for the one result: the bp_msm* entry points.  ARKBP_MSM_LATENCY=1 / =0 forces them on / off
// everywhere (A/B).
static int msm_latency_env() { static const int v = getenv("ARKBP_MSM_LATENCY") ? atoi(getenv("ARKBP_MSM_LATENCY")) : -1; return v; }
static bool msm_use_quad(const bp_ctx* ctx) { const int e = msm_latency_env(); return e >= 0 ? e != 0 : ctx->msm_latency_first; }
static bool msm_quad_trees(const bp_ctx* ctx) { static const bool force = getenv("ARKBP_MSM_QUAD_TREES") != nullptr; return force || msm_use_quad(ctx); }   // (experiment: the quad trees without the GLV split)
// what the planners read: the ctx's knobs as they are now (no ctx: the defaults), the environment's experiment switches as they were
// at the first MSM
static MsmKnobs msm_knobs(const bp_ctx* ctx) {
    static const MsmKnobs env = [] {
        const auto num = [](const char* name) { const char* v = getenv(name); return v ? atoi(v) : 0; };
        MsmKnobs e;
        e.env_c = num("ARKBP_MSM_C"); e.env_fs_cap = num("ARKBP_MSM_FS_CAP"); e.env_tpt = num("ARKBP_MSM_TPT"); e.env_fixed_c = num("ARKBP_MSM_FIXED_C");
        e.env_nobin = getenv("ARKBP_MSM_NOBIN") != nullptr; e.env_nofs = getenv("ARKBP_MSM_NOFS") != nullptr;
        e.env_marginals = getenv("ARKBP_MSM_MARGINALS") != nullptr;   // A/B: the bit-marginal bucket aggregation everywhere
        return e;
    }();
    MsmKnobs kn = env;
    if (!ctx) return kn;
    kn.wsum_min = ctx->tune_msm_wsum_min; kn.bin_min = ctx->tune_msm_bin_min; kn.glv_min = ctx->tune_msm_glv_min; kn.chunk_cap = ctx->tune_msm_chunk_cap;
    kn.fixed_min = ctx->tune_msm_fixed_min; kn.quad = msm_use_quad(ctx);
    return kn;
}
// (direct launches in both branches: a kernel template named only inside a conditional expression is not emitted for the device)
#define MSM_LAUNCH_REDUCE_FS(red_g, grid, ...) do { if (msm_quad_trees(ctx) && (red_g) == 4u) hipLaunchKernelGGL((k_msm_reduce_fs<C, true>), grid, dim3(256), 0, st, __VA_ARGS__); \
                                                    else hipLaunchKernelGGL((k_msm_reduce_fs<C, false>), grid, dim3(256), 0, st, __VA_ARGS__); } while (0)
#define MSM_LAUNCH_MARGINALS_FS(grid, ...) do { if (msm_quad_trees(ctx)) hipLaunchKernelGGL((k_msm_marginals_fs<C, 256, true>), grid, dim3(256), 0, st, __VA_ARGS__); \
                                                else hipLaunchKernelGGL((k_msm_marginals_fs<C, 256, false>), grid, dim3(256), 0, st, __VA_ARGS__); } while (0)
// The pinned block the MSM chains copy their result points into
static int msm_host_T_ensure(bp_ctx* ctx, size_t bytes, size_t slack = 4096) { return pinned_ensure(ctx->h_T, ctx->h_T_cap, bytes, slack); }
// Host tail of an MSM: the Horner sum, from the top position down, over the points a chain left in the pinned block (T: 12 words per
// point, Z = 0 for the identity).  Every position costs `dbls` doublings of ONE point — a serial chain that a scalar core runs ~40x
// faster than a GPU lane.  Positions below nlow hold one point each (T[j]); the nhigh positions above hold `parts` points each, behind
// those.  The three forms:
//   bit marginals, sum_{w,k} 2^(c*w+k) T[w][k]:                         nlow = W * c, nhigh = 0, dbls = 1
//   ... with the slot window's bits as top_parts partial points each:   nlow = wb * c, nhigh = top_bits, parts = top_parts, dbls = 1
//   window sums, sum_w 2^(c*w) (sum_j T[w][j]):                         nlow = 0, nhigh = W, parts = workgroups per window, dbls = c
template <class C> static J4 msm_horner_tail(const u64* T, int nlow, int nhigh, u32 parts, int dbls) {
    typedef host::Grp<C> G;
    J4 acc = G::inf();
    auto add_T = [&](size_t idx) {
        const J4 p = jac_from_words(T + idx * 12);
        if (!p.Z.is_zero()) acc = G::add(acc, p);
    };
    for (int j = nlow + nhigh - 1; j >= 0; j--) {
        for (int d = 0; d < dbls; d++) acc = G::dbl(acc);
        if (j >= nlow) { for (u32 q = 0; q < parts; q++) add_T((size_t)nlow + (size_t)(j - nlow) * parts + q); }
        else add_T((size_t)j);
    }
    return acc;
}

// A rank's partial point -> the sum over the ranks of a sharded ctx (one small exchange): RCCL all-gather of the Jacobian partials
// inside the library, or the host's point-reduce callback.
template <class C> static int shard_point_reduce(bp_ctx* ctx, J4& part) {
    typedef host::Grp<C> G;
    if (ctx->nccl) {
        // RCCL point-reduce: group addition is not an RCCL reduce op -> all-gather of the partials + world-1 host additions.  The
        // partial travels as it is — Jacobian, 96 bytes — so no rank pays a field inversion per MSM just to ship it;
        // every rank adds the same points in the same order and normalises its own copy of the sum when the caller asks.
        uint64_t xyz[12];
        memcpy(xyz, part.X.v, 32); memcpy(xyz + 4, part.Y.v, 32); memcpy(xyz + 8, part.Z.v, 32);
        std::vector<uint64_t> all((size_t)ctx->shard_world * 12);
        BPCHK(ctx_native_allgather(ctx, xyz, 96, all.data()));
        J4 sum = G::inf();
        for (int r = 0; r < ctx->shard_world; r++) {
            J4 q; memcpy(q.X.v, &all[(size_t)r * 12], 32); memcpy(q.Y.v, &all[(size_t)r * 12 + 4], 32); memcpy(q.Z.v, &all[(size_t)r * 12 + 8], 32);
            sum = G::add(sum, q);
        }
        part = sum;
        return BP_OK;
    }
    if (!ctx->shard_cb) { g_err = "sharded mode: no point-reduce installed"; return BP_E_ARG; }
    A4 a = G::to_aff(part);      // (the callback's contract is an affine point: include/arkbp.h bp_point_reduce_cb)
    uint64_t xy[8]; memcpy(xy, a.x.v, 32); memcpy(xy + 4, a.y.v, 32);
    const int rc = ctx->shard_cb(ctx->shard_user, xy);
    if (rc) { g_err = "msm: the point-reduce callback failed"; return rc < 0 ? rc : BP_E_ARG; }
    memcpy(a.x.v, xy, 32); memcpy(a.y.v, xy + 4, 32);
    part = G::from_aff(a);
    return BP_OK;
}

// ---- the fixed-shape pipeline (msm.cuh 7) ------------------------------------------------------------------------------------------
// One shape (msm_plan.hpp msm_fs_shape, sh.fits) for J <= MSM_JOBS MSMs of sh.pl.n terms each — own scalars and bases — as ONE chain
// of five launches with the job in grid.z: no host wait before the last kernel, one D2H copy of the J result blocks, one wait, the J
// host Horner tails.  Every job works in its own stride of the ctx's buffers (FsJobs), so each result is the sum it is alone.
// A GLV shape (sh.bp.glv; msm.cuh "GLV split": 2n half-terms of 128 bits) runs the same chain: what differs is the plan — half the
// windows, hence half the buckets for the reduction / aggregation trees and half the doublings (and marginal sums) of the Horner tail
// —, that the kernels read the bases as half-terms (BaseSegs::glv) and the canon stride (MSM_GLV_WORDS words per scalar, in sh.jb).
// over[j]: job j raised its overflow word (skewed scalars) and results[j] is not written; the caller redoes that job on the general
// path, which recomputes everything.
template <class C> static int msm_fs_jobs(bp_ctx* ctx, int J, const BaseSegs* segs, const ScalSegs* scalars, int scalars_mont, const FsShape& sh, J4* results, bool* over) {
    static const bool mtrace = getenv("ARKBP_MSM_TRACE") != nullptr;
    hipStream_t st = ctx->stream;
    const MsmPlan& pl = sh.pl; const BinPlan& bp = sh.bp; const SlotPlan& sp = sh.sp; const FsPlan& fp = sh.fp; const FsJobs& jb = sh.jb;
    const size_t n = pl.n, nj = (size_t)J, maxch = sh.maxch, tc = sh.tc, tb = sh.tb;
    const u32 chl_fs = sh.chl_fs, red_g = sh.red_g;
    if (!sh.fits || J < 1 || J > MSM_JOBS) { g_err = "msm_fs_jobs: a shape that does not fit"; return BP_E_ARG; }
    const auto tfs = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_f0 = mtrace ? tfs() : 0;
    BPCHK(ctx->canon.ensure(nj * jb.canon * 4));
    // hist, the bin cursors and the overflow words are all-zero between MSMs in every job's region: their last readers restore that
    BPCHK(ctx->hist.ensure_zeroed(nj * jb.hist * 4, st));
    BPCHK(ctx->bin_cur.ensure_zeroed(nj * jb.bin_cur * 4, st));
    BPCHK(ctx->fs_over.ensure_zeroed(MSM_JOBS * 4, st));
    BPCHK(ctx->slots.ensure(nj * jb.slots * 4));
    BPCHK(ctx->boff.ensure(nj * jb.buckets * 4));
    BPCHK(ctx->fs_bcnt.ensure(nj * jb.buckets * 4));
    BPCHK(ctx->fs_loff.ensure(nj * jb.buckets * 4));
    BPCHK(ctx->fs_binch.ensure(nj * jb.binch * 4));
    BPCHK(ctx->fs_sums.ensure(nj * jb.sums * 4));
    BPCHK(ctx->lvA.ensure(nj * jb.part * 4));
    BPCHK(ctx->Tbuf.ensure(nj * tb));
    BPCHK(msm_host_T_ensure(ctx, nj * tb));
    PerJob<ScalSegs> sj; memset(&sj, 0, sizeof sj);
    PerJob<BaseSegs> bj; memset(&bj, 0, sizeof bj);
    for (int j = 0; j < J; j++) { sj.j[j] = scalars[j]; bj.j[j] = segs[j]; if (bp.glv) bj.j[j].glv = 1; }
    ScopedK total(ctx, BP_K_MSM_TOTAL);
    u32* d_over = ctx->fs_over.as<u32>();
    u32* d_info = ctx->Tbuf.as<u32>() + tc * 24;
    const int wg = std::max(1, (int)(12288 / bp.NBIN));   // windows per launch: 48 KiB of LDS counters
    const u32 gp = (u32)((n + (size_t)256 * bp.tpt - 1) / ((size_t)256 * bp.tpt));
    const u32 gz = (u32)J;
    for (int wa = 0; wa < (int)bp.wb; wa += wg) {
        const int we = std::min<int>((int)bp.wb, wa + wg);
        hipLaunchKernelGGL(k_msm_bin_partition<C>, dim3(gp, 1, gz), dim3(256), ((size_t)(we - wa) * bp.NBIN + (wa == 0 ? bp.top_nb : 0)) * 4, st, sj, ctx->canon.as<u32>(),
                           ctx->hist.as<u32>(), pl, scalars_mont, bp, sp, ctx->bin_cur.as<u32>(), ctx->slots.as<u32>(), d_over, wa, we, wa == 0 ? 1 : 0, jb);
    }
    hipLaunchKernelGGL(k_msm_bin_sort_fs, dim3(bp.NBIN, bp.wb + fp.has_top, gz), dim3(256), (((size_t)1 << bp.LB) + 8 + bp.cap) * 4, st, ctx->slots.as<u32>(),
                       ctx->bin_cur.as<u32>(), ctx->hist.as<u32>(), ctx->boff.as<u32>(), ctx->fs_bcnt.as<u32>(), ctx->fs_loff.as<u32>(), ctx->fs_binch.as<u32>(),
                       d_over, pl, bp, sp, chl_fs, jb);
    {
        ScopedK acc(ctx, BP_K_MSM_ACCUM_FS);
        hipLaunchKernelGGL(k_msm_accum_fs<C>, dim3((u32)((maxch + 255) / 256), 1, gz), dim3(256), 0, st, bj, ctx->slots.as<u32>(), ctx->fs_bcnt.as<u32>(), ctx->fs_loff.as<u32>(),
                           ctx->boff.as<u32>(), ctx->fs_binch.as<u32>(), ctx->lvA.as<u32>(), pl, bp, fp, chl_fs, d_info, jb);
    }
    {
        ScopedK agg(ctx, BP_K_MSM_AGG);
        MSM_LAUNCH_REDUCE_FS(red_g, dim3((u32)(((size_t)bp.wb * pl.NB * red_g + 255) / 256), 1, gz), ctx->lvA.as<u32>(), ctx->fs_bcnt.as<u32>(), ctx->fs_loff.as<u32>(),
                           ctx->fs_binch.as<u32>(), ctx->fs_sums.as<u32>(), pl, bp, fp, chl_fs, red_g, jb);
        MSM_LAUNCH_MARGINALS_FS(dim3((u32)tc, 1, gz), ctx->fs_sums.as<u32>(), ctx->lvA.as<u32>(), ctx->fs_bcnt.as<u32>(), ctx->fs_loff.as<u32>(),
                           ctx->Tbuf.as<u32>(), pl, bp, fp, chl_fs, d_info, d_over, jb);
    }
    HIPCHK(hipMemcpyAsync(ctx->h_T, ctx->Tbuf.p, nj * tb, hipMemcpyDeviceToHost, st));
    total.stop();
    const double t_f1 = mtrace ? tfs() : 0;
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    const double t_f2 = mtrace ? tfs() : 0;
    for (int jn = 0; jn < J; jn++) {
        const uint8_t* blk = (const uint8_t*)ctx->h_T + (size_t)jn * tb;
        const u32* info = (const u32*)(blk + tc * 96);
        over[jn] = info[2] != 0;
        if (over[jn]) {
            if (mtrace) fprintf(stderr, "[msm-fs] n=%zu glv=%u job %d: overflow, the general path takes over\n", n, bp.glv, jn);
            continue;
        }
        results[jn] = msm_horner_tail<C>((const u64*)blk, (int)bp.wb * pl.c, (int)fp.top_bits, fp.top_parts, 1);
        if (mtrace) fprintf(stderr, "[msm-fs] n=%zu glv=%u job %d/%d c=%d W=%d bins=%u chunks=%u/%u  enqueue %.1f us  wait %.1f us  host tails so far %.1f us\n", n, bp.glv, jn, J, pl.c,
                            pl.W, fp.nbins, info[0], fp.max_chunks, (t_f1 - t_f0) * 1e6, (t_f2 - t_f1) * 1e6, (tfs() - t_f2) * 1e6);
    }
    return BP_OK;
}
// Mid-size MSMs on a curve with the endomorphism, for callers that wait for the one result: the chain over GLV-split scalars.
// *done = false when the GLV shape does not fit or a region overflowed (skewed scalars): the caller then runs the ordinary schedule.
template <class C> static int msm_run_fs_glv(bp_ctx* ctx, const BaseSegs& segs, const ScalSegs& d_scalars, size_t n, int scalars_mont, J4& result, bool& done) {
    done = false;
    const FsShape sh = msm_fs_shape(n, C::Fr::BITS, 1, true, msm_knobs(ctx));
    if (!sh.fits) return BP_OK;
    bool over = false;
    BPCHK(msm_fs_jobs<C>(ctx, 1, &segs, &d_scalars, scalars_mont, sh, &result, &over));
    done = !over;
    return BP_OK;
}
// the mid-size MSM takes the GLV-split pipeline (msm_run_fs_glv) when it applies: callers that wait for one result
template <class C> static bool msm_glv_route(const bp_ctx* ctx, const BaseSegs& segs, size_t n, bool sharded, int w_hi) {
    if constexpr (!C::HAS_GLV) { (void)ctx; (void)segs; (void)n; (void)sharded; (void)w_hi; return false; }
    else {
        static const bool no_glv = getenv("ARKBP_MSM_NOGLV") != nullptr, no_fs0 = getenv("ARKBP_MSM_NOFS") != nullptr;
        return !no_glv && !no_fs0 && !sharded && w_hi < 0 && ctx->shard_world == 1 && !segs.fixed_c4 && msm_glv_sizes(msm_knobs(ctx), n);
    }
}

// The back end that msm_run's general path and the fixed-base schedule share.  The front end has sorted the entries by bucket and
// left the totals on the host (tot[k]: chunks of level k, tot[MSM_NLMAX]: the fullest bucket) and the level offsets in ctx->lvl_off.
// Level 1 is k_msm_accum (one lane per chunk of 2^chl entries: mixed additions of gathered bases; `mode`: how it finds a bucket's
// entries), levels 2 .. K the k_msm_reduce tree, until a bucket holds one point.  special: the buckets from b_gen on (top_nb buckets
// of a narrow top window, a few holding ~n/2 entries each) go through the first spl levels like every other and are finished by
// k_msm_reduce_special in one launch.  finish(points, offsets) enqueues what sums the buckets — inside the BP_K_MSM_AGG region.
// deep: the fullest bucket needs nl levels or more; nothing was launched.  wave (A/B): one wavefront per bucket, no tree above.
template <class C, class Finish>
static int msm_tree_back(bp_ctx* ctx, const BaseSegs& segs, const u32* entries, int mode, const SlotPlan& sp, const MsmPlan& pl, const u32* tot, int nl, int chl,
                         bool special, int spl, u32 b_gen, u32 top_nb, bool wave, int& K, bool& deep, Finish&& finish) {
    hipStream_t st = ctx->stream;
    const int TB = 256;
    const size_t Bp1 = (size_t)pl.B + 1;
    u32* lvl = ctx->lvl_off.as<u32>();
    // levels: 1 = chunks of entries; k >= 2 = chunks of level k-1 partials; stop when a bucket holds <= 1
    K = 1;
    { u64 cap = (u64)1 << chl; while (cap < tot[MSM_NLMAX]) { cap <<= chl; K++; } }
    if (special && K < spl + 1) K = spl + 1;   // the special buckets' partials meet in level spl + 1
    deep = K >= nl;
    if (deep) return BP_OK;
    BPCHK(ctx->lvA.ensure((size_t)tot[1] * 96));
    if (K >= 2) BPCHK(ctx->lvB.ensure((size_t)tot[2] * 96));
    if (wave && !special) {
        // the bucket sums go straight to the last level's slots (<= 1 per bucket)
        ScopedK acc(ctx, BP_K_MSM_ACCUM);
        hipLaunchKernelGGL(k_msm_accum_wave<C>, dim3((pl.B + 3) / 4), dim3(256), 0, st, segs, entries, lvl, lvl + Bp1 * K, ctx->lvA.as<u32>(), pl.B, mode, sp, (u32)pl.NB,
                           ctx->boff.as<u32>());
        acc.stop();
        finish(ctx->lvA.as<u32>(), lvl + Bp1 * K);
        return BP_OK;
    }
    {
        ScopedK acc(ctx, BP_K_MSM_ACCUM);
        hipLaunchKernelGGL(k_msm_accum<C>, dim3((tot[1] + TB - 1) / TB), dim3(TB), 0, st, segs, entries, lvl, lvl + Bp1, ctx->lvA.as<u32>(), pl.B, tot[1], mode, sp, (u32)pl.NB,
                           ctx->boff.as<u32>(), chl);
    }
    u32* cur = ctx->lvA.as<u32>();
    u32* nxt = ctx->lvB.as<u32>();
    ScopedK agg(ctx, BP_K_MSM_AGG);
    for (int k = 2; k <= K; k++) {
        hipLaunchKernelGGL(k_msm_reduce<C>, dim3((tot[k] + TB - 1) / TB), dim3(TB), 0, st, cur, lvl + Bp1 * (k - 1), lvl + Bp1 * k, nxt, pl.B, tot[k], chl,
                           (k == spl + 1 && special) ? b_gen : pl.B);
        if (k == spl + 1 && special)
            hipLaunchKernelGGL(k_msm_reduce_special<C>, dim3(top_nb), dim3(256), 0, st, cur, lvl + Bp1 * spl, lvl + Bp1 * (spl + 1), nxt, b_gen, pl.B);
        u32* t = cur; cur = nxt; nxt = t;
    }
    finish(cur, lvl + Bp1 * K);
    return BP_OK;
}

template <class C> static int msm_run(bp_ctx* ctx, const BaseSegs& segs, const u32* d_scalars_one, size_t n, int scalars_mont, J4& result,
                                      int w_lo = 0, int w_hi = -1 /* window range for multi-GPU window sharding; default all */,
                                      int shard_mode = -1 /* -1: the ctx's mode (window partition + reduce when world > 1); 0: none (replicated);
                                                             2: the terms are this rank's own share: all windows, then the point-reduce */,
                                      const ScalSegs* sseg = nullptr /* the scalars as runs read in place (then d_scalars_one is unused) */,
                                      bool no_fixed_shape = false /* straight to the general path: a job of msm_run_pair whose fixed-shape pass overflowed */) {
    ScalSegs d_scalars; memset(&d_scalars, 0, sizeof d_scalars);
    if (sseg) d_scalars = *sseg; else { d_scalars.nseg = 1; d_scalars.ptr[0] = d_scalars_one; d_scalars.start[0] = 0; d_scalars.start[1] = (u32)n; }
    typedef host::Grp<C> G;
    result = G::inf();
    if (n == 0) return BP_OK;
    if (n >= (1u << 31)) { g_err = "msm: n too large"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    const MsmKnobs kn = msm_knobs(ctx);
    MsmPlan pl = msm_plan(n, C::Fr::BITS, kn);
    const bool sharded = w_hi < 0 && ctx->shard_world > 1 && shard_mode != 0;
    if (sharded && shard_mode != 2) {   // contiguous block partition of the windows (the same rule as parallel.shard_range)
        const int base = pl.W / ctx->shard_world, rem = pl.W % ctx->shard_world, r = ctx->shard_rank;
        w_lo = r * base + std::min(r, rem);
        w_hi = w_lo + base + (r < rem ? 1 : 0);
    }
    auto finish_sharded = [&](J4& part) -> int {   // partial point -> sum over the ranks (one small exchange)
        if (!sharded) return BP_OK;
        return shard_point_reduce<C>(ctx, part);
    };
    if (!no_fixed_shape && msm_glv_route<C>(ctx, segs, n, sharded, w_hi)) {
        // mid-size MSMs on a curve with the endomorphism: the fixed-shape pipeline over GLV-split scalars (half the windows)
        bool done = false;
        BPCHK(msm_run_fs_glv<C>(ctx, segs, d_scalars, n, scalars_mont, result, done));
        if (done) return BP_OK;
    }
    if (w_hi >= 0) { pl.w_lo = std::max(0, w_lo); pl.w_hi = std::min(pl.W, w_hi); }
    if (pl.w_lo >= pl.w_hi) return finish_sharded(result);  // this rank owns no window: the identity
    constexpr int NL = MSM_NLMAX;
    int nl = 2;  // levels 0..nl-1 can be needed: 16^(nl-1) >= n
    { u64 cap = MSM_CH; while (cap < n && nl < NL) { cap *= MSM_CH; nl++; } }   // sized for the smaller fan-in
    if (nl < 4) nl = 4;   // the special buckets of the top window meet one level after spl <= 2
    const int spl = n > ((size_t)1 << 17) ? 2 : 1;   // hot bucket ~ n/2 entries: keep the special kernel at <= 32 partials per lane
    const size_t Bp1 = (size_t)pl.B + 1;
    const u32 ntiles = (pl.B + MSM_SCAN_TILE - 1) / MSM_SCAN_TILE;
    BPCHK(ctx->canon.ensure(n * 32));
    // hist, the bin cursors and the overflow flag are all-zero between MSMs: their last readers (k_msm_scan_apply, k_msm_bin_sort,
    // the host) restore that, so no memset is enqueued per MSM
    BPCHK(ctx->hist.ensure_zeroed(pl.B * 4, st));
    BPCHK(ctx->lvl_off.ensure(Bp1 * NL * 4));
    BPCHK(ctx->totals.ensure_zeroed((NL + 2) * 4 + (size_t)ntiles * (NL + 1) * 4, st));
    BPCHK(ctx->cursor.ensure(pl.B * 4));
    const bool use_marginals = msm_use_marginals(kn, pl);
    const u32 nblk_ws = (u32)((pl.NB + 256 * MSM_SEG - 1) / (256 * MSM_SEG));   // workgroups per window of k_msm_window_sums
    const size_t tcount = use_marginals ? (size_t)pl.W * pl.c : (size_t)pl.W * nblk_ws;
    BPCHK(ctx->Tbuf.ensure(tcount * 96));
    if (!ctx->h_totals) HIPCHK(hipHostMalloc((void**)&ctx->h_totals, 64));
    const size_t tbytes = tcount * 96;
    BPCHK(msm_host_T_ensure(ctx, tbytes));
    if (pl.W > MSM_MAXW) { g_err = "msm: too many windows"; return BP_E_ARG; }
    // the fixed-shape pipeline's shape; its window and bin plans also serve the general path
    const FsShape sh = msm_fs_shape(n, C::Fr::BITS, 1, false, kn, pl.w_lo, pl.w_hi, segs.fixed_c4 != 0);
    const BinPlan& bp = sh.bp;
    bool binned = sh.binned;
    auto make_slots = [&](SlotPlan& sp, int w_first, size_t first_slot) -> size_t { return msm_make_slots(pl, C::Fr::BITS, n, false, sp, w_first, first_slot); };
    SlotPlan sp;
    u32* lvl = ctx->lvl_off.as<u32>();
    u32* d_tot = ctx->totals.as<u32>();
    u32* d_tiles = d_tot + (NL + 2);
    u32* d_over = d_tot + (NL + 1);
    const int TB = 256;
    const u32 gb = (u32)((n + TB - 1) / TB);
    // front end: digits, histogram, placement, scans; leaves the totals (and the overflow flag) in h_totals
    int chl = MSM_CHL;
    u32 b_gen = pl.B;   // buckets below b_gen go through the generic reduction tree; the rest (narrow top window) are special
    auto front_end = [&](bool bins) -> int {
        static const int chl_env = getenv("ARKBP_MSM_CHL") ? atoi(getenv("ARKBP_MSM_CHL")) : 0;
        chl = bins ? (chl_env >= 2 && chl_env <= 6 ? chl_env : MSM_CHL_BINNED) : MSM_CHL;
        static const bool no_special = getenv("ARKBP_MSM_NOSPECIAL") != nullptr;
        b_gen = (bins && bp.top_nb && bp.top_nb <= 16 && !no_special) ? (u32)bp.wb * (u32)pl.NB : pl.B;   // few, huge buckets only: a wider top window fits the generic tree
        const size_t nslots = make_slots(sp, bins ? (int)bp.wb : 0, bins ? (size_t)bp.wb * bp.NBIN * bp.cap : 0);
        if (nslots >= ((size_t)1 << 32)) { g_err = "msm: slot array too large"; return BP_E_ARG; }
        BPCHK(ctx->slots.ensure(nslots * 4));
        if (bins) {
            BPCHK(ctx->bin_cur.ensure_zeroed((size_t)pl.W * bp.NBIN * 4, st));
            BPCHK(ctx->boff.ensure((size_t)pl.B * 4));
            const int wg = std::max(1, (int)(12288 / bp.NBIN));   // windows per launch: 48 KiB of LDS counters
            const u32 gp = (u32)((n + (size_t)256 * bp.tpt - 1) / ((size_t)256 * bp.tpt));
            for (int wa = 0; wa < (int)bp.wb; wa += wg) {
                const int we = std::min<int>((int)bp.wb, wa + wg);
                hipLaunchKernelGGL(k_msm_bin_partition<C>, dim3(gp), dim3(256), ((size_t)(we - wa) * bp.NBIN + (wa == 0 ? bp.top_nb : 0)) * 4, st, PerJob<ScalSegs>{{d_scalars}}, ctx->canon.as<u32>(),
                                   ctx->hist.as<u32>(), pl, scalars_mont, bp, sp, ctx->bin_cur.as<u32>(), ctx->slots.as<u32>(), d_over, wa, we, wa == 0 ? 1 : 0, FsJobs{});
            }
            hipLaunchKernelGGL(k_msm_bin_sort, dim3(bp.NBIN, pl.W), dim3(256), (((size_t)1 << bp.LB) + 4 + bp.cap) * 4, st, ctx->slots.as<u32>(),
                               ctx->bin_cur.as<u32>(), ctx->hist.as<u32>(), ctx->boff.as<u32>(), pl, bp, sp);
        } else {
            const u32 lds_hist = gb == 1 && (size_t)pl.B <= 12288 ? (u32)pl.B : 0u;   // one workgroup: count in LDS (48 KiB of counters at most)
            hipLaunchKernelGGL(k_msm_digits<C>, dim3(gb), dim3(TB), (size_t)lds_hist * 4, st, d_scalars, ctx->canon.as<u32>(), ctx->hist.as<u32>(), pl, scalars_mont, sp,
                               ctx->slots.as<u32>(), d_over, lds_hist);
        }
        hipLaunchKernelGGL(k_msm_scan_tiles, dim3(ntiles), dim3(256), 0, st, ctx->hist.as<u32>(), d_tiles, pl.B, nl, chl, b_gen, spl);
        hipLaunchKernelGGL(k_msm_scan_top, dim3(1), dim3(64), 0, st, d_tiles, ntiles, d_tot, lvl, pl.B);
        hipLaunchKernelGGL(k_msm_scan_apply, dim3(ntiles), dim3(256), 0, st, ctx->hist.as<u32>(), d_tiles, lvl, pl.B, nl, chl, b_gen, spl);
        HIPCHK(hipMemcpyAsync(ctx->h_totals, d_tot, (NL + 2) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        if (ctx->h_totals[NL + 1] != 0) HIPCHK(hipMemsetAsync(d_over, 0, 4, st));   // the overflow flag was raised: lower it for the next pass / MSM
        return BP_OK;
    };
    static const bool mtrace = getenv("ARKBP_MSM_TRACE") != nullptr;   // host-side phase times of every MSM on stderr
    // ---- the fixed-shape pipeline (msm.cuh 7): no host wait before the last kernel; falls through to the general path on overflow ----
    if (!no_fixed_shape && sh.fits) {
        bool over = false;
        BPCHK(msm_fs_jobs<C>(ctx, 1, &segs, &d_scalars, scalars_mont, sh, &result, &over));
        if (!over) return finish_sharded(result);
    }
    ScopedK total(ctx, BP_K_MSM_TOTAL);
    const auto tnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_m0 = mtrace ? tnow() : 0;
    BPCHK(front_end(binned));
    const double t_m1 = mtrace ? tnow() : 0;
    if (binned && ctx->h_totals[NL + 1] != 0) {   // a bin region overflowed (skewed scalars): one-pass slots for every window
        binned = false;
        BPCHK(front_end(false));
    }
    const bool slotted = ctx->h_totals[NL + 1] == 0;
    const u32* entries_ptr = ctx->slots.as<u32>();
    if (!slotted) {  // some bucket outgrew its slots (skewed scalars): exact counting-sort scatter
        BPCHK(ctx->entries.ensure(n * pl.W * 4));
        HIPCHK(hipMemcpyAsync(ctx->cursor.p, lvl, pl.B * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_msm_scatter, dim3(gb), dim3(TB), 0, st, ctx->canon.as<u32>(), ctx->cursor.as<u32>(), ctx->entries.as<u32>(), pl);
        entries_ptr = ctx->entries.as<u32>();
    }
    const u32* tot = ctx->h_totals;
    if (tot[0] == 0) { total.stop(); return finish_sharded(result); }  // every digit zero: the identity
    static const bool accum_wave = getenv("ARKBP_MSM_ACCUM") && !strcmp(getenv("ARKBP_MSM_ACCUM"), "wave");   // A/B: one wavefront per bucket
    int K = 1; bool deep = false;
    BPCHK(msm_tree_back<C>(ctx, segs, entries_ptr, slotted ? (binned ? 2 : 1) : 0, sp, pl, tot, nl, chl, b_gen < pl.B, spl, b_gen, bp.top_nb, accum_wave, K, deep,
                           [&](const u32* pts, const u32* off) {
        if (use_marginals) hipLaunchKernelGGL(k_msm_marginals<C>, dim3(pl.W, pl.c), dim3(256), 0, st, pts, off, ctx->Tbuf.as<u32>(), pl);
        else hipLaunchKernelGGL(k_msm_window_sums<C>, dim3(nblk_ws, pl.W), dim3(256), 0, st, pts, off, ctx->Tbuf.as<u32>(), pl, nblk_ws);
    }));
    if (deep) { g_err = "msm: bucket population exceeds the reduction depth"; return BP_E_ARG; }
    HIPCHK(hipMemcpyAsync(ctx->h_T, ctx->Tbuf.p, tbytes, hipMemcpyDeviceToHost, st));
    total.stop();
    const double t_m2 = mtrace ? tnow() : 0;
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    const double t_m3 = mtrace ? tnow() : 0;
    result = use_marginals ? msm_horner_tail<C>((const u64*)ctx->h_T, pl.W * pl.c, 0, 0, 1) : msm_horner_tail<C>((const u64*)ctx->h_T, 0, pl.W, nblk_ws, pl.c);
    if (mtrace) fprintf(stderr, "[msm] n=%zu c=%d W=%d K=%d  front(enqueue+sync) %.1f us  back enqueue %.1f us  back wait %.1f us  host tail %.1f us\n", n, pl.c, pl.W, K,
                        (t_m1 - t_m0) * 1e6, (t_m2 - t_m1) * 1e6, (t_m3 - t_m2) * 1e6, (tnow() - t_m3) * 1e6);
    return finish_sharded(result);
}

// ---- fixed-base MSM over the generator tables (msm.cuh 1c) -----------------------------------------------------------------
// A run of generator-table bases of a fixed-base MSM: which table (0 = G, 1 = H, 2 = PedersenGens {B, B_blinding}), first index, count
struct FbRun { int table; size_t first, count; size_t stride = 1; };   // stride: base j of the run is table[first + j * stride] (an index-cyclic slice)
// the rows of `count` bases, slab by slab through the caller's scratch (tmp: 96 B, pref: 32 B, outb: 64 B per row and slab base)
template <class C> static int fb_rows_build(hipStream_t st, const u32* gens, u32* table, size_t count, size_t table_cap, size_t slab, DevBuf& tmp, DevBuf& pref, DevBuf& outb) {
    for (size_t lo = 0; lo < count; lo += slab) {
        const size_t m = std::min(slab, count - lo);
        const u32 gb = (u32)((m + 255) / 256);
        hipLaunchKernelGGL(k_msm_fb_rows<C>, dim3(gb), dim3(256), 0, st, gens + lo * 16, tmp.as<u32>(), (u32)m, FB_ROWS);
        hipLaunchKernelGGL(k_ftab_normalize<C>, dim3(gb), dim3(256), 0, st, tmp.as<u32>(), pref.as<u32>(), outb.as<u32>(), (u32)m, FB_ROWS);
        HIPCHK(hipGetLastError());
        for (u32 r = 0; r < FB_ROWS; r++)   // [r][i] of the slab -> [r][lo + i] of the table
            HIPCHK(hipMemcpyAsync(table + ((size_t)r * table_cap + lo) * 16, outb.as<u32>() + (size_t)r * m * 16, m * 64, hipMemcpyDeviceToDevice, st));
    }
    return BP_OK;
}
template <class C> static int fb_tables_build(bp_ctx* ctx, size_t cap) {
    hipStream_t st = ctx->stream;
    if (cap == 0 || cap > ctx->gens_cap) { g_err = "msm tables: more bases than installed generators"; return BP_E_GENS_LENGTH; }
    if (!ctx->d_G.owned) { g_err = "msm tables: build them on the ctx that owns the generator tables, then bp_gens_share"; return BP_E_ARG; }
    ctx->fb_cap = 0;
    BPCHK(ctx->fb_G.ensure_exact((size_t)FB_ROWS * cap * 64)); BPCHK(ctx->fb_H.ensure_exact((size_t)FB_ROWS * cap * 64)); BPCHK(ctx->fb_pc.ensure((size_t)FB_ROWS * 2 * 64));
    const size_t slab = std::min<size_t>(cap, (size_t)1 << 18);   // bounds the Jacobian scratch: 65 rows x 2^18 x 96 B = 1.6 GB
    DevBuf tmp, pref, outb;
    BPCHK(tmp.ensure(FB_ROWS * slab * 96)); BPCHK(pref.ensure(FB_ROWS * slab * 32)); BPCHK(outb.ensure(FB_ROWS * slab * 64));
    auto build = [&](const u32* gens, u32* table, size_t count, size_t table_cap) -> int { return fb_rows_build<C>(st, gens, table, count, table_cap, slab, tmp, pref, outb); };
    BPCHK(build(ctx->d_G.as<u32>(), ctx->fb_G.as<u32>(), cap, cap));
    BPCHK(build(ctx->d_H.as<u32>(), ctx->fb_H.as<u32>(), cap, cap));
    BPCHK(build(ctx->d_pc.as<u32>(), ctx->fb_pc.as<u32>(), 2, 2));
    HIPCHK(ctx_stream_wait(ctx));
    tmp.release(); pref.release(); outb.release();
    ctx->fb_cap = cap;
    return BP_OK;
}
// sum_t s_t * Base(t) for bases given as runs of the generator tables; *done = false when the fixed-base path does not apply
// (no tables, a run beyond them, skewed scalars overflowing a bin region, window-sharded ctx): the caller then runs the
// ordinary MSM over the same bases.
template <class C>
static int msm_fixed_run_one(bp_ctx* ctx, const FbRun* runs, int nruns, const ScalSegs& ssegs, size_t n, int scalars_mont, J4& result, bool& done, int shard_mode) {
    typedef host::Grp<C> G;
    done = false;
    static const bool fbtrace = getenv("ARKBP_FB_TRACE") != nullptr;
#define FBX(k) do { if (fbtrace) fprintf(stderr, "[fixed-base] declined at exit %d (n = %zu, runs = %d, world = %d, mode = %d)\n", k, n, nruns, ctx->shard_world, shard_mode); return BP_OK; } while (0)
    const bool reduce_after = ctx->shard_world > 1 && shard_mode == 2;
    if (ctx->shard_world > 1 && !reduce_after) FBX(1);
    static const bool off = getenv("ARKBP_MSM_NOFIXED") != nullptr;   // A/B switch
    if (off || !ctx->fb_cap || nruns > MSM_MAXSEG) FBX(2);
    const FbPlan fb = fb_plan(n, C::Fr::BITS, msm_knobs(ctx));   // window width, entry word, bins (msm_plan.hpp)
    if (fb.decline == 2) FBX(2);
    BaseSegs segs; memset(&segs, 0, sizeof segs);
    u32 at = 0;
    for (int k = 0; k < nruns; k++) {
        const size_t cap = runs[k].table == 2 ? 2 : ctx->fb_cap;
        if (runs[k].count && runs[k].first + (runs[k].count - 1) * runs[k].stride + 1 > cap) FBX(3);
        const DevBuf& tb = runs[k].table == 0 ? ctx->fb_G : runs[k].table == 1 ? ctx->fb_H : ctx->fb_pc;
        segs.ptr[k] = (const u32*)tb.p + runs[k].first * 16;
        segs.row_words[k] = (u64)cap * 16;
        segs.stride[k] = (u32)runs[k].stride;
        segs.start[k] = at; at += (u32)runs[k].count;
    }
    segs.start[nruns] = at; segs.nseg = nruns;
    if (at != n) { g_err = "msm_fixed: runs and term count differ"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    if (fb.decline) FBX(fb.decline);
    const MsmPlan& pl = fb.pl; const BinPlan& bp = fb.bp;
    const u32 nbin = bp.NBIN, tbits = fb.tbits;
    const size_t cap = bp.cap;
    const int LB = (int)bp.LB, nl = fb.nl;
    SlotPlan sp; memset(&sp, 0, sizeof sp);
    constexpr int NL = MSM_NLMAX;
    const size_t Bp1 = (size_t)pl.B + 1;
    const u32 ntiles = (pl.B + MSM_SCAN_TILE - 1) / MSM_SCAN_TILE;
    const u32 nblk_ws = (u32)((pl.NB + 256 * MSM_SEG - 1) / (256 * MSM_SEG));
    BPCHK(ctx->canon.ensure(n * 32)); BPCHK(ctx->hist.ensure_zeroed((size_t)pl.B * 4, st)); BPCHK(ctx->lvl_off.ensure(Bp1 * NL * 4));
    BPCHK(ctx->totals.ensure_zeroed((NL + 2) * 4 + (size_t)ntiles * (NL + 1) * 4, st)); BPCHK(ctx->bin_cur.ensure_zeroed((size_t)nbin * 4, st)); BPCHK(ctx->boff.ensure((size_t)pl.B * 4));
    BPCHK(ctx->slots.ensure((size_t)nbin * cap * 4)); BPCHK(ctx->Tbuf.ensure(((size_t)nblk_ws + 1) * 96));
    if (!ctx->h_totals) HIPCHK(hipHostMalloc((void**)&ctx->h_totals, 64));
    BPCHK(msm_host_T_ensure(ctx, 96, 4000));
    ScopedK total(ctx, BP_K_MSM_TOTAL);
    u32* lvl = ctx->lvl_off.as<u32>();
    u32* d_tot = ctx->totals.as<u32>();
    u32* d_tiles = d_tot + (NL + 2);
    u32* d_over = d_tot + (NL + 1);
    const int chl = MSM_CHL_BINNED;
    const u32 gp = (u32)((n + (size_t)256 * bp.tpt - 1) / ((size_t)256 * bp.tpt));
    hipLaunchKernelGGL(k_msm_fb_partition<C>, dim3(gp), dim3(256), (size_t)nbin * 4, st, ssegs, ctx->canon.as<u32>(), pl, scalars_mont, bp, tbits, ctx->bin_cur.as<u32>(),
                       ctx->slots.as<u32>(), d_over);
    MsmPlan pl1 = pl; pl1.W = 1;   // one bucket set from here on
    hipLaunchKernelGGL(k_msm_bin_sort, dim3(nbin, 1), dim3(256), (((size_t)1 << LB) + 4 + cap) * 4, st, ctx->slots.as<u32>(), ctx->bin_cur.as<u32>(), ctx->hist.as<u32>(),
                       ctx->boff.as<u32>(), pl1, bp, sp);
    hipLaunchKernelGGL(k_msm_scan_tiles, dim3(ntiles), dim3(256), 0, st, ctx->hist.as<u32>(), d_tiles, pl.B, nl, chl, pl.B, 1);
    hipLaunchKernelGGL(k_msm_scan_top, dim3(1), dim3(64), 0, st, d_tiles, ntiles, d_tot, lvl, pl.B);
    hipLaunchKernelGGL(k_msm_scan_apply, dim3(ntiles), dim3(256), 0, st, ctx->hist.as<u32>(), d_tiles, lvl, pl.B, nl, chl, pl.B, 1);
    HIPCHK(hipMemcpyAsync(ctx->h_totals, d_tot, (NL + 2) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    const u32* tot = ctx->h_totals;
    if (tot[NL + 1] != 0) {   // a bin region overflowed (skewed scalars): the ordinary MSM handles those
        HIPCHK(hipMemsetAsync(d_over, 0, 4, st));
        total.stop();
        FBX(7);
    }
    result = G::inf();
    done = true;
    if (tot[0] == 0) { total.stop(); return BP_OK; }
    segs.fixed_c4 = (u32)(pl.c / 4); segs.tbits = tbits;
    int K = 1; bool deep = false;
    BPCHK(msm_tree_back<C>(ctx, segs, ctx->slots.as<u32>(), 2, sp, pl, tot, nl, chl, false, 1, pl.B, 0, false, K, deep, [&](const u32* pts, const u32* offs) {
        hipLaunchKernelGGL(k_msm_window_sums<C>, dim3(nblk_ws, 1), dim3(256), 0, st, pts, offs, ctx->Tbuf.as<u32>(), pl1, nblk_ws);
        hipLaunchKernelGGL(k_msm_sum_partials<C>, dim3(1), dim3(256), 0, st, ctx->Tbuf.as<u32>(), nblk_ws, ctx->Tbuf.as<u32>() + (size_t)nblk_ws * 24);
    }));
    if (deep) { done = false; total.stop(); return BP_OK; }
    HIPCHK(hipMemcpyAsync(ctx->h_T, ctx->Tbuf.as<u32>() + (size_t)nblk_ws * 24, 96, hipMemcpyDeviceToHost, st));
    total.stop();
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    const J4 pnt = jac_from_words((const u64*)ctx->h_T);
    if (!pnt.Z.is_zero()) result = pnt;   // no Horner tail: the rows already carry the powers of two
    return BP_OK;
}
#undef FBX
// The entry word of the fixed-base sort packs (window, term, fine bucket, sign) into 32 bits: one call holds up to 2^22 terms.  Longer
// MSMs — the commitments of a 2^22-constraint proof have 2^23 + 1 terms — go through in pieces of the logical term range (runs and
// scalar segments cut alike), the partial points added on the host: the schedule's 13 mixed additions per term instead of the
// ordinary 17-18 at every size.  On a sharded ctx (shard_mode 2: the runs are THIS RANK'S share of the terms — all windows here, the
// single-GPU schedule at 1/world of the terms) ONE point-reduce follows, whatever the number of pieces; any other mode steps aside.
static constexpr size_t FB_MAX_TERMS = (size_t)1 << 22;
template <class C>
static int msm_fixed_run(bp_ctx* ctx, const FbRun* runs, int nruns, const ScalSegs& ssegs, size_t n, int scalars_mont, J4& result, bool& done, int shard_mode = -1) {
    typedef host::Grp<C> G;
    done = false;
    const bool reduce_after = ctx->shard_world > 1 && shard_mode == 2;
    if (n <= FB_MAX_TERMS) {
        BPCHK(msm_fixed_run_one<C>(ctx, runs, nruns, ssegs, n, scalars_mont, result, done, shard_mode));
    } else {
        if (ctx->shard_world > 1 && !reduce_after) return BP_OK;
        const size_t pieces = (n + FB_MAX_TERMS - 1) / FB_MAX_TERMS, per = (n + pieces - 1) / pieces;
        J4 acc = G::inf();
        bool all = true;
        for (size_t t0 = 0; t0 < n && all; t0 += per) {
            const size_t t1 = std::min(n, t0 + per);
            FbRun rs[MSM_MAXSEG]; int nr = 0;
            ScalSegs ss; memset(&ss, 0, sizeof ss);
            size_t at = 0;
            for (int k = 0; k < nruns; k++) {          // the runs' share of [t0, t1)
                const size_t lo = std::max(at, t0), hi = std::min(at + runs[k].count, t1);
                if (lo < hi) { rs[nr] = runs[k]; rs[nr].first = runs[k].first + (lo - at) * runs[k].stride; rs[nr].count = hi - lo; nr++; }
                at += runs[k].count;
            }
            u32 sat = 0;
            for (int k = 0; k < ssegs.nseg; k++) {      // the scalar segments' share
                const size_t lo = std::max<size_t>(ssegs.start[k], t0), hi = std::min<size_t>(ssegs.start[k + 1], t1);
                if (lo < hi) { ss.ptr[ss.nseg] = ssegs.ptr[k] + (lo - ssegs.start[k]) * 8; ss.start[ss.nseg] = sat; sat += (u32)(hi - lo); ss.nseg++; }
            }
            ss.start[ss.nseg] = sat;
            J4 part; bool ok = false;
            BPCHK(msm_fixed_run_one<C>(ctx, rs, nr, ss, t1 - t0, scalars_mont, part, ok, shard_mode));
            if (!ok) all = false; else acc = G::add(acc, part);
        }
        if (all) { result = acc; done = true; }
    }
    if (!done) return BP_OK;
    ctx->fb_runs++;
    if (reduce_after) { ctx->fb_runs_sharded++; return shard_point_reduce<C>(ctx, result); }
    return BP_OK;
}

// MSM over the resident generator tables (no base upload): bases = G[off..off+n) (if use_G) || H[off..off+n) (if use_H) || extras
struct MsmLatencyScope { bp_ctx* c; bool prev; MsmLatencyScope(bp_ctx* c_) : c(c_), prev(c_->msm_latency_first) { c->msm_latency_first = true; } ~MsmLatencyScope() { c->msm_latency_first = prev; } };
template <class C> static int msm_gens_entry(bp_ctx* c, int use_G, int use_H, size_t off, size_t n, const uint64_t* extra_xy, size_t n_extra,
                                             const uint64_t* scalars, int canonical, uint64_t out_xy[8]) {
    MsmLatencyScope latency(c);
    const size_t ng = use_G ? n : 0, nh = use_H ? n : 0, total = ng + nh + n_extra;
    if (total == 0) { memset(out_xy, 0, 64); return BP_OK; }
    BPCHK(c->io_scal.ensure(total * 32));
    HIPCHK(hipMemcpyAsync(c->io_scal.p, scalars, total * 32, hipMemcpyHostToDevice, c->stream));
    if (!n_extra && (ng || nh)) {   // only generator-table bases: the fixed-base schedule when the rows are installed (bp_gens_msm_tables)
        FbRun runs[2]; int nr = 0;
        if (ng) runs[nr++] = FbRun{0, off, ng};
        if (nh) runs[nr++] = FbRun{1, off, nh};
        ScalSegs ss; memset(&ss, 0, sizeof ss);
        ss.nseg = 1; ss.ptr[0] = c->io_scal.as<u32>(); ss.start[0] = 0; ss.start[1] = (u32)total;
        J4 r; bool done = false;
        BPCHK(msm_fixed_run<C>(c, runs, nr, ss, total, canonical ? 0 : 1, r, done));
        if (done) {
            A4 a = host::Grp<C>::to_aff(r);
            memcpy(out_xy, a.x.v, 32); memcpy(out_xy + 4, a.y.v, 32);
            if (c->profiling) collect_timers(c);
            return BP_OK;
        }
    }
    if (n_extra) {
        BPCHK(c->io_pts.ensure(n_extra * 64));
        HIPCHK(hipMemcpyAsync(c->io_pts.p, extra_xy, n_extra * 64, hipMemcpyHostToDevice, c->stream));
        BPCHK(bp_points_import(c, c->io_pts.p, c->io_pts.p, n_extra));
    }
    BaseSegs sg; memset(&sg, 0, sizeof sg);
    int k = 0; u32 at = 0;
    if (ng) { sg.ptr[k] = c->d_G.as<u32>() + off * 16; sg.start[k] = at; at += (u32)ng; k++; }
    if (nh) { sg.ptr[k] = c->d_H.as<u32>() + off * 16; sg.start[k] = at; at += (u32)nh; k++; }
    if (n_extra) { sg.ptr[k] = c->io_pts.as<u32>(); sg.start[k] = at; at += (u32)n_extra; k++; }
    sg.start[k] = at; sg.nseg = k;
    J4 r;
    BPCHK(msm_run<C>(c, sg, c->io_scal.as<u32>(), total, canonical ? 0 : 1, r));
    A4 a = host::Grp<C>::to_aff(r);
    memcpy(out_xy, a.x.v, 32); memcpy(out_xy + 4, a.y.v, 32);
    if (c->profiling) collect_timers(c);
    return BP_OK;
}
template <class C> static void aff_out(uint64_t out[8], const A4& a) { memcpy(out, a.x.v, 32); memcpy(out + 4, a.y.v, 32); }

template <class C> static int msm_dev_entry(bp_ctx* ctx, const void* d_bases, const void* d_scalars, size_t n, int canonical, uint64_t out_xy[8],
                                            int w_lo = 0, int w_hi = -1) {
    MsmLatencyScope latency(ctx);
    BaseSegs segs; memset(&segs, 0, sizeof segs);
    segs.nseg = 1; segs.ptr[0] = (const u32*)d_bases; segs.start[0] = 0; segs.start[1] = (u32)n;
    J4 r;
    BPCHK(msm_run<C>(ctx, segs, (const u32*)d_scalars, n, canonical ? 0 : 1, r, w_lo, w_hi));
    A4 a = host::Grp<C>::to_aff(r);
    memcpy(out_xy, a.x.v, 32); memcpy(out_xy + 4, a.y.v, 32);
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}


// ---- InnerProductProof::create orchestration (src/inner_product_proof.rs:37-239) ------------------------
// All vectors are device-resident in the engine's layouts and are consumed (folded in place), like the
// reference's by-value Vec arguments.  `challenge` is the Fiat-Shamir step (:132-137): it receives affine
// L, R (ark layout) and returns u (ark Montgomery words).
typedef std::function<int(const uint64_t* L_xy, const uint64_t* R_xy, uint64_t* u_out)> ChallengeFn;

template <class F> static Words8 words_of(const F4& x) { Words8 w; memcpy(w.w, x.v, 32); return w; }
// non-adjacent form of the canonical value of x: sum_i (plus_i - minus_i) 2^i, no two adjacent non-zero digits
template <class S> static Naf naf_of(const F4& x) {
    Naf r; memset(&r, 0, sizeof r);
    uint64_t k[5] = {0, 0, 0, 0, 0};
    S::to_canon(k, x);
    for (int i = 0; i < 258; i++) {
        if (!(k[0] | k[1] | k[2] | k[3] | k[4])) break;
        if (k[0] & 1) {
            if ((k[0] & 3) == 1) { r.plus[i >> 5] |= 1u << (i & 31); k[0] &= ~(uint64_t)1; }
            else { r.minus[i >> 5] |= 1u << (i & 31); for (int j = 0; j < 5; j++) { if (++k[j]) break; } }  // k += 1
        }
        for (int j = 0; j < 4; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 63);
        k[4] >>= 1;
    }
    return r;
}

// ---- GLV decomposition on the host (once per round: the fold scalar is uniform) ---------------------------------------
// round(num / r) for a 512-bit num (8 limbs) and the 256-bit modulus r: binary long division, then round half up
static void div_round_512(const uint64_t num[8], const uint64_t r[4], uint64_t quot[8]) {
    uint64_t rem[5] = {0, 0, 0, 0, 0};
    memset(quot, 0, 64);
    auto geq = [&](const uint64_t* a /*5*/) { if (a[4]) return true; for (int i = 3; i >= 0; i--) { if (a[i] != r[i]) return a[i] > r[i]; } return true; };
    auto sub = [&](uint64_t* a) { unsigned __int128 br = 0; for (int i = 0; i < 4; i++) { unsigned __int128 t = (unsigned __int128)a[i] - r[i] - (uint64_t)br; a[i] = (uint64_t)t; br = (t >> 64) & 1; } a[4] -= (uint64_t)br; };
    for (int bit = 511; bit >= 0; bit--) {
        for (int i = 4; i > 0; i--) rem[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
        rem[0] = (rem[0] << 1) | ((num[bit >> 6] >> (bit & 63)) & 1);
        if (geq(rem)) { sub(rem); quot[bit >> 6] |= (uint64_t)1 << (bit & 63); }
    }
    // round: if 2*rem >= r, quot += 1
    uint64_t dbl[5];
    for (int i = 4; i > 0; i--) dbl[i] = (rem[i] << 1) | (rem[i - 1] >> 63);
    dbl[0] = rem[0] << 1;
    if (geq(dbl)) { for (int i = 0; i < 8; i++) if (++quot[i]) break; }
}
static void mul_256x192(const uint64_t a[4], const uint64_t b[3], uint64_t out[8]) {
    memset(out, 0, 64);
    for (int i = 0; i < 4; i++) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 3; j++) { c += (unsigned __int128)a[i] * b[j] + out[i + j]; out[i + j] = (uint64_t)c; c >>= 64; }
        for (int j = i + 3; j < 8 && c; j++) { c += out[j]; out[j] = (uint64_t)c; c >>= 64; }
    }
}
// NAF digit masks of a non-negative integer < 2^160 given as 3 limbs; `negate` swaps the +1 / -1 masks
static void naf_masks(const uint64_t k_in[3], bool negate, u32 plus[5], u32 minus[5]) {
    uint64_t k[3] = {k_in[0], k_in[1], k_in[2]};
    memset(plus, 0, 20); memset(minus, 0, 20);
    for (int i = 0; i < 160; i++) {
        if (!(k[0] | k[1] | k[2])) break;
        if (k[0] & 1) {
            const bool is_plus = (k[0] & 3) == 1;
            if (is_plus) k[0] &= ~(uint64_t)1; else { for (int j = 0; j < 3; j++) if (++k[j]) break; }
            u32* dst = (is_plus != negate) ? plus : minus;
            dst[i >> 5] |= 1u << (i & 31);
        }
        k[0] = (k[0] >> 1) | (k[1] << 63); k[1] = (k[1] >> 1) | (k[2] << 63); k[2] >>= 1;
    }
}
// t (field element) -> t1 + t2*lambda with short t1, t2; fills the four masks of one vector.  false if a half exceeds 129 bits.
struct GlvRaw { uint64_t mg1[3], mg2[3]; bool n1, n2; };   // t = (n1 ? -mg1 : mg1) + lambda * (n2 ? -mg2 : mg2)
template <class C> static bool glv_decompose(const F4& t, u32 p1[5], u32 m1[5], u32 p2[5], u32 m2[5], GlvRaw* raw = nullptr) {
    if constexpr (C::HAS_GLV) {
        typedef host::Fld<typename C::Fr> S;
        uint64_t tc[4]; S::to_canon(tc, t);
        uint64_t prod[8], c1[8], c2[8];
        mul_256x192(tc, C::GLV_B2, prod); div_round_512(prod, C::Fr::P64, c1);    // c1 = round(b2 * t / r)
        mul_256x192(tc, C::GLV_NB1, prod); div_round_512(prod, C::Fr::P64, c2);   // c2 = round(-b1 * t / r)
        auto small = [&](const uint64_t v[3]) { uint64_t c[4] = {v[0], v[1], v[2], 0}; return S::from_canon(c); };
        const F4 fc1 = S::from_canon(c1), fc2 = S::from_canon(c2);   // c1, c2 < 2^130: the low 4 limbs hold them
        // k2 = -c1*b1 - c2*b2 = c1*|b1| - c2*b2 ;  k1 = t - k2*lambda      (mod r; both are short up to sign)
        F4 lam; memcpy(lam.v, C::LAMBDA64, 32);
        const F4 k2 = S::sub(S::mul(fc1, small(C::GLV_NB1)), S::mul(fc2, small(C::GLV_B2)));
        const F4 k1 = S::sub(t, S::mul(k2, lam));
        auto split = [&](const F4& k, uint64_t mag[3], bool& neg) {
            uint64_t c[4]; S::to_canon(c, k);
            neg = false;
            if (c[3] | (c[2] >> 1)) {   // not short: it is r - |k|
                F4 nk = S::neg(k); S::to_canon(c, nk); neg = true;
                if (c[3] | (c[2] >> 1)) return false;
            }
            mag[0] = c[0]; mag[1] = c[1]; mag[2] = c[2];
            return true;
        };
        uint64_t mg1[3], mg2[3]; bool n1, n2;
        if (!split(k1, mg1, n1) || !split(k2, mg2, n2)) return false;
        if (raw) { memcpy(raw->mg1, mg1, 24); memcpy(raw->mg2, mg2, 24); raw->n1 = n1; raw->n2 = n2; return true; }
        naf_masks(mg1, n1, p1, m1);
        naf_masks(mg2, n2, p2, m2);
        return true;
    } else {
        (void)t; (void)p1; (void)m1; (void)p2; (void)m2; (void)raw;
        return false;
    }
}
template <class C> static bool glv_pair(const F4& tG, const F4& tH, Naf2& g, Naf2& h) {
    return glv_decompose<C>(tG, g.p1, g.m1, g.p2, g.m2) && glv_decompose<C>(tH, h.p1, h.m1, h.p2, h.m2);
}
// Rounds with at least 2^16 output points convert to affine through k_ipa_fold_finish (one inversion per m points); smaller
// rounds are launch/latency bound and keep the in-lane inversion.
struct FoldFinish { u32* jac = nullptr; u32* pref = nullptr; u32 m = 0; };
// what a fold launcher enqueued (bp_ctx::fold_took; include/arkbp.h bp_debug_fold)
enum : u32 { FOLD_TOOK_GLV = 1, FOLD_TOOK_NAF = 2, FOLD_TOOK_QUAD = 4, FOLD_TOOK_FINISH = 8, FOLD_TOOK_TAB = 16, FOLD_TOOK_TAB2 = 32 };
static int fold_finish_plan(bp_ctx* ctx, size_t lanes, FoldFinish& ff) {
    static const bool off = getenv("ARKBP_FOLD_NOBATCH") != nullptr;
    ff = FoldFinish();
    if (off || lanes < ctx->tune_fold_batch_min) return BP_OK;
    BPCHK(ctx->ipa_jac.ensure(lanes * 96));
    BPCHK(ctx->ipa_pref.ensure(lanes * 32));
    ff.jac = ctx->ipa_jac.as<u32>(); ff.pref = ctx->ipa_pref.as<u32>();
    ff.m = (u32)std::min<size_t>(8, std::max<size_t>(2, lanes / 32768));   // keep >= 2^15 lanes busy
    return BP_OK;
}
template <class C> static void fold_finish_launch(bp_ctx* ctx, const FoldFinish& ff, u32* d_G, u32* d_H, size_t n, int which, size_t lanes) {
    if (!ff.jac) return;
    ctx->fold_took |= FOLD_TOOK_FINISH;
    ScopedK tk(ctx, BP_K_FOLD_FINISH);
    const u32 threads = (u32)((lanes + ff.m - 1) / ff.m);
    hipLaunchKernelGGL(k_ipa_fold_finish<C>, dim3((threads + 255) / 256), dim3(256), 0, ctx->stream, ff.jac, ff.pref, d_G, d_H, (u32)n, which, (u32)lanes, ff.m);
}
// launches the uniform fold for multipliers (tG, tH): GLV ladder where the curve has the endomorphism, plain NAF ladder otherwise
// (force_naf: the NAF ladder there too — the route a multiplier without a short GLV split takes; bp_debug_fold)
template <class C> static int launch_uniform_fold(bp_ctx* ctx, u32* d_G, u32* d_H, size_t n, const F4& tG, const F4& tH, int which, bool force_naf = false) {
    typedef host::Fld<typename C::Fr> S;
    hipStream_t st = ctx->stream;
    const u32 lanes = (u32)(which == 3 ? 2 * n : n);
    FoldFinish ff;
    BPCHK(fold_finish_plan(ctx, lanes, ff));
    bool done = false;
    // rounds whose points leave most of the chip idle: four lanes per point (ecq.cuh) — ~1.6x less latency per round for 2.5x the
    // VALU work (profiles/r03_fold_quad_ab.txt); BP_TUNE_FOLD_QUAD_MAX = the largest round (in points) that takes this form
    const bool quad = lanes >= 64 && lanes <= ctx->tune_fold_quad_max;
    const u32 grid = quad ? (lanes * 4 + 255) / 256 : (lanes + 255) / 256;
    {
    ScopedK tk(ctx, BP_K_FOLD_LADDER);
    if constexpr (C::HAS_GLV) {
        Naf2 g, h;
        if (!force_naf && glv_pair<C>(tG, tH, g, h)) {
            if (quad) hipLaunchKernelGGL((k_ipa_fold_glv<C, true>), dim3(grid), dim3(256), 0, st, d_G, d_H, (u32)n, g, h, which, ff.jac);
            else hipLaunchKernelGGL((k_ipa_fold_glv<C, false>), dim3(grid), dim3(256), 0, st, d_G, d_H, (u32)n, g, h, which, ff.jac);
            done = true;
            ctx->fold_took |= FOLD_TOOK_GLV;
        }
    }
    if (!done) {
        ctx->fold_took |= FOLD_TOOK_NAF;
        Naf a = naf_of<S>(tG), b = naf_of<S>(tH);
        if (quad) hipLaunchKernelGGL((k_ipa_fold_uniform<C, true>), dim3(grid), dim3(256), 0, st, d_G, d_H, (u32)n, a, b, which, ff.jac);
        else hipLaunchKernelGGL((k_ipa_fold_uniform<C, false>), dim3(grid), dim3(256), 0, st, d_G, d_H, (u32)n, a, b, which, ff.jac);
    }
    if (quad) ctx->fold_took |= FOLD_TOOK_QUAD;
    }
    fold_finish_launch<C>(ctx, ff, d_G, d_H, n, which, lanes);
    return BP_OK;
}

// ---- fixed-base tables for the first fold round (ipa.cuh: k_ftab_window, k_ftab_normalize, k_ipa_fold_tab) --------------------
// signed w-bit digits of a non-negative integer (limbs little-endian, `nl` of them), least significant window first
static void ftab_recode(const uint64_t* mag, int nl, bool negate, int w, int nwin, unsigned short* e, unsigned long long& negmask) {
    uint64_t k[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < nl; i++) k[i] = mag[i];
    const uint64_t full = (uint64_t)1 << w, half = full >> 1;
    negmask = 0;
    for (int j = 0; j < nwin; j++) {
        uint64_t d = k[0] & (full - 1);
        for (int i = 0; i < 4; i++) k[i] = (k[i] >> w) | (k[i + 1] << (64 - w));
        k[4] >>= w;
        bool neg = false;
        if (d > half) { d = full - d; neg = true; for (int i = 0; i < 5; i++) if (++k[i]) break; }   // digit d - 2^w, carry 1
        e[j] = (unsigned short)d;
        if (d && (neg != negate)) negmask |= 1ull << j;
    }
}
template <class C> static int ftab_nwin_for(int w) { return (C::HAS_GLV ? 130 : 256) / w + 1; }
// element j of a rank's index-cyclic slice of a vector: in[rank + j * world] (32-byte scalars, 64-byte points)
template <class W8> __global__ void k_cyclic_gather(const u32* __restrict__ in, u32* __restrict__ out, u32 n_loc, u32 rank, u32 world) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_loc) return;
    const W8* src = (const W8*)in + ((size_t)rank + (size_t)j * world);
    ((W8*)out)[j] = *src;
}
struct Blk32 { uint4 a, b; };
struct Blk64 { uint4 a, b, c, d; };
template <class C> static bool ftab_digits(const bp_ctx* ctx, const F4& t, FtabDigits& d) {
    typedef host::Fld<typename C::Fr> S;
    memset(&d, 0, sizeof d);
    d.nwin = (u32)ctx->ftab_nwin;
    if (d.nwin > 44) return false;
    if constexpr (C::HAS_GLV) {
        GlvRaw raw; u32 dummy[5];
        if (!glv_decompose<C>(t, dummy, dummy, dummy, dummy, &raw)) return false;
        ftab_recode(raw.mg1, 3, raw.n1, ctx->ftab_w, ctx->ftab_nwin, d.e1, d.neg1);
        ftab_recode(raw.mg2, 3, raw.n2, ctx->ftab_w, ctx->ftab_nwin, d.e2, d.neg2);
    } else {
        uint64_t c[4]; S::to_canon(c, t);
        ftab_recode(c, 4, false, ctx->ftab_w, ctx->ftab_nwin, d.e1, d.neg1);
    }
    return true;
}
// Builds the tables for G[0..n), H[0..n) of the installed generators.  w = 0: the widest window (<= 8 bits) whose tables fit in
// `budget_bytes` (0 = 3/4 of the free device memory).
// first / stride: the tables of the generators first + i * stride, i < n — 1/world of the memory for a rank of a sharded prover whose
// inner-product argument works on that index-cyclic slice (these are the ctx's own tables then, whoever owns the generators).
template <class C> static int ftab_build(bp_ctx* ctx, size_t n, int w, size_t budget_bytes, u32 first = 0, u32 stride = 1) {
    hipStream_t st = ctx->stream;
    if (n == 0 || stride == 0 || (size_t)first + (n - 1) * (size_t)stride >= ctx->gens_cap) { g_err = "fold tables: more bases than installed generators"; return BP_E_GENS_LENGTH; }
    if (!ctx->d_G.owned && stride == 1) { g_err = "fold tables: build them on the ctx that owns the generator tables, then bp_gens_share"; return BP_E_ARG; }
    for (DevBuf* b : {&ctx->ftab_G, &ctx->ftab_H}) { if (!b->owned) { b->p = nullptr; b->cap = 0; b->owned = true; } else b->release(); }   // (a shared view is let go, not freed)
    ctx->ftab_n = 0; ctx->ftab_first = 0; ctx->ftab_stride = 1;
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (!budget_bytes) budget_bytes = free_b / 4 * 3;
    auto bytes_for = [&](int ww) { const size_t E = (size_t)1 << (ww - 1); return 2 * (size_t)ftab_nwin_for<C>(ww) * E * n * 64 + E * n * (96 + 32) + n * 96; };
    if (w == 0) { w = 8; while (w > 2 && bytes_for(w) > budget_bytes) w--; }
    if (w < 2 || w > 8 || bytes_for(w) > free_b) { g_err = "fold tables: not enough device memory"; return BP_E_ARG; }
    const size_t E = (size_t)1 << (w - 1);
    const int nwin = ftab_nwin_for<C>(w);
    const size_t per_vec = (size_t)nwin * E * n * 64;
    BPCHK(ctx->ftab_G.ensure_exact(per_vec)); BPCHK(ctx->ftab_H.ensure_exact(per_vec));
    DevBuf tmp, pref, state, gsl;
    BPCHK(tmp.ensure_exact(E * n * 96)); BPCHK(pref.ensure_exact(E * n * 32)); BPCHK(state.ensure_exact(n * 96));
    const u32 gb = (u32)((n + 255) / 256);
    if (stride > 1 || first) BPCHK(gsl.ensure_exact(n * 64));
    for (int v = 0; v < 2; v++) {
        const u32* gens = v ? ctx->d_H.as<u32>() : ctx->d_G.as<u32>();
        if (gsl.p) {   // the slice as a compact vector: the builder below then runs unchanged
            hipLaunchKernelGGL(k_cyclic_gather<Blk64>, dim3(gb), dim3(256), 0, st, gens, gsl.as<u32>(), (u32)n, first, stride);
            gens = gsl.as<u32>();
        }
        u32* T = v ? ctx->ftab_H.as<u32>() : ctx->ftab_G.as<u32>();
        for (int j = 0; j < nwin; j++) {
            hipLaunchKernelGGL(k_ftab_window<C>, dim3(gb), dim3(256), 0, st, gens, state.as<u32>(), tmp.as<u32>(), (u32)n, (u32)E, j == 0 ? 1 : 0);
            hipLaunchKernelGGL(k_ftab_normalize<C>, dim3(gb), dim3(256), 0, st, tmp.as<u32>(), pref.as<u32>(), T + (size_t)j * E * n * 16, (u32)n, (u32)E);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));
    tmp.release(); pref.release(); state.release(); gsl.release();
    ctx->ftab_n = n; ctx->ftab_w = w; ctx->ftab_nwin = nwin; ctx->ftab_first = first; ctx->ftab_stride = stride;
    return BP_OK;
}
// Walks every entry of the fold tables and of the fixed-base MSM rows (ipa.cuh "integrity check"); counts the entries that break
// the chain rule.  ~0.3 s for 146 GB of fold tables.
template <class C> static int tables_check(bp_ctx* ctx, uint64_t* bad_fold, uint64_t* bad_rows) {
    hipStream_t st = ctx->stream;
    BPCHK(ctx->io_out.ensure(64));
    unsigned long long* d_bad = ctx->io_out.as<unsigned long long>();
    HIPCHK(hipMemsetAsync(d_bad, 0, 16, st));
    if (ctx->ftab_n) {
        const u32 n = (u32)ctx->ftab_n, E = 1u << (ctx->ftab_w - 1), gb = (n + 255) / 256;
        hipLaunchKernelGGL(k_ftab_check<C>, dim3(gb), dim3(256), 0, st, ctx->d_G.as<u32>(), ctx->ftab_G.as<u32>(), n, E, (u32)ctx->ftab_nwin, d_bad, ctx->ftab_first, ctx->ftab_stride);
        hipLaunchKernelGGL(k_ftab_check<C>, dim3(gb), dim3(256), 0, st, ctx->d_H.as<u32>(), ctx->ftab_H.as<u32>(), n, E, (u32)ctx->ftab_nwin, d_bad, ctx->ftab_first, ctx->ftab_stride);
    }
    if (ctx->fb_cap) {
        const u32 n = (u32)ctx->fb_cap, gb = (n + 255) / 256;
        hipLaunchKernelGGL(k_fb_rows_check<C>, dim3(gb), dim3(256), 0, st, ctx->d_G.as<u32>(), ctx->fb_G.as<u32>(), n, (size_t)n, FB_ROWS, d_bad + 1);
        hipLaunchKernelGGL(k_fb_rows_check<C>, dim3(gb), dim3(256), 0, st, ctx->d_H.as<u32>(), ctx->fb_H.as<u32>(), n, (size_t)n, FB_ROWS, d_bad + 1);
        hipLaunchKernelGGL(k_fb_rows_check<C>, dim3(1), dim3(256), 0, st, ctx->d_pc.as<u32>(), ctx->fb_pc.as<u32>(), 2u, (size_t)2, FB_ROWS, d_bad + 1);
    }
    HIPCHK(hipGetLastError());
    unsigned long long h[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(h, d_bad, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    if (bad_fold) *bad_fold = h[0];
    if (bad_rows) *bad_rows = h[1];
    return BP_OK;
}
// The same for the tables of the small-statement path and of the commitments, and for the resident points they are anchored at
// (small.cuh k_dt_check, pedersen.cuh k_pc_table_check, msm.cuh k_points_on_curve): every launch first, then one copy back and one
// wait.  Reads what is there — a view of another ctx's generators and direct tables included — and builds nothing.
template <class C> static int direct_tables_check(bp_ctx* ctx, uint64_t* bad, uint64_t* first_bad, uint64_t* checked) {
    hipStream_t st = ctx->stream;
    BPCHK(ctx->io_out.ensure(2 * BP_TABLES_KINDS * 8));
    unsigned long long* d_bad = ctx->io_out.as<unsigned long long>();
    unsigned long long* d_first = d_bad + BP_TABLES_KINDS;
    HIPCHK(hipMemsetAsync(d_bad, 0, BP_TABLES_KINDS * 8, st));
    HIPCHK(hipMemsetAsync(d_first, 0xff, BP_TABLES_KINDS * 8, st));
    uint64_t seen[BP_TABLES_KINDS] = {0, 0, 0, 0};
    const u32* pc = ctx->d_pc.as<u32>();
    const size_t cap = ctx->dt_cap, nb = 2 + 2 * cap;
    if (cap && pc && cap <= ctx->gens_cap && ctx->dt_tab.p && ctx->dt_tab.cap >= nb * DT_BASE_BYTES) {
        const size_t entries = nb * DT_PER_BASE;
        ScopedK tk(ctx, BP_K_DT_CHECK);
        hipLaunchKernelGGL(k_dt_check<C>, dim3((u32)((entries + 255) / 256)), dim3(256), 0, st, pc, ctx->d_G.as<u32>(), ctx->d_H.as<u32>(), (u32)cap, ctx->dt_tab.as<u32>(),
                           (u32)nb, d_bad + BP_TABLES_DIRECT, d_first + BP_TABLES_DIRECT);
        seen[BP_TABLES_DIRECT] = entries;
    }
    if (pc && ctx->pc_dt.p && ctx->pc_dt.cap >= (size_t)2 * DT_BASE_BYTES) {
        hipLaunchKernelGGL(k_dt_check<C>, dim3((2 * DT_PER_BASE + 255) / 256), dim3(256), 0, st, pc, (const u32*)nullptr, (const u32*)nullptr, 0u, ctx->pc_dt.as<u32>(), 2u,
                           d_bad + BP_TABLES_PC_DIRECT, d_first + BP_TABLES_PC_DIRECT);
        seen[BP_TABLES_PC_DIRECT] = 2 * DT_PER_BASE;
    }
    if (pc && ctx->pc_table.p && ctx->pc_table.cap >= PC_TABLE_BYTES) {
        hipLaunchKernelGGL(k_pc_table_check<C>, dim3(2 * PC_WINDOWS * PC_DIGITS / 256), dim3(256), 0, st, pc, ctx->pc_table.as<u32>(), d_bad + BP_TABLES_PC_WIDE,
                           d_first + BP_TABLES_PC_WIDE);
        seen[BP_TABLES_PC_WIDE] = 2 * PC_WINDOWS * PC_DIGITS;
    }
    if (pc) {
        hipLaunchKernelGGL(k_points_on_curve<C>, dim3(1), dim3(256), 0, st, pc, 2u, 0u, d_bad + BP_TABLES_RESIDENT, d_first + BP_TABLES_RESIDENT);
        seen[BP_TABLES_RESIDENT] = 2;
        if (const u32 n = (u32)ctx->gens_cap) {
            const u32 gb = (n + 255) / 256;
            hipLaunchKernelGGL(k_points_on_curve<C>, dim3(gb), dim3(256), 0, st, ctx->d_G.as<u32>(), n, 2u, d_bad + BP_TABLES_RESIDENT, d_first + BP_TABLES_RESIDENT);
            hipLaunchKernelGGL(k_points_on_curve<C>, dim3(gb), dim3(256), 0, st, ctx->d_H.as<u32>(), n, 2u + n, d_bad + BP_TABLES_RESIDENT, d_first + BP_TABLES_RESIDENT);
            seen[BP_TABLES_RESIDENT] += 2 * (uint64_t)n;
        }
    }
    HIPCHK(hipGetLastError());
    unsigned long long h[2 * BP_TABLES_KINDS];
    HIPCHK(hipMemcpyAsync(h, d_bad, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    for (int k = 0; k < BP_TABLES_KINDS; k++) {
        if (bad) bad[k] = h[k];
        if (first_bad) first_bad[k] = h[BP_TABLES_KINDS + k];
        if (checked) checked[k] = seen[k];
    }
    return BP_OK;
}
// Table columns of a state's local elements: element j (generator gens_first + j * gens_stride) is column c0 + j * cs of the ctx's
// fold tables — whole tables (column = generator index) or a rank's slice of them; false when the elements do not lie on the columns
static bool ftab_cols(const bp_ctx* ctx, const IpaState& s, u32& c0, u32& cs) {
    const u32 ts = ctx->ftab_stride ? ctx->ftab_stride : 1u, tf = ctx->ftab_first;
    if (!s.gens_stride || s.gens_stride % ts || s.gens_first < tf || (s.gens_first - tf) % ts) return false;
    c0 = (s.gens_first - tf) / ts; cs = s.gens_stride / ts;
    return true;
}
// the first-round uniform fold through the tables; false when they do not apply (then the ladder kernels run)
template <class C> static int launch_tab_fold(bp_ctx* ctx, const IpaState& s, u32* d_G, u32* d_H, size_t n, const F4& tG, const F4& tH, bool& done) {
    done = false;
    static const bool off = getenv("ARKBP_FOLD_NOTAB") != nullptr;   // A/B switch
    u32 c0 = 0, cs = 1;
    if (off || !ctx->ftab_n || n < 64 || !ftab_cols(ctx, s, c0, cs)) return BP_OK;
    if ((size_t)c0 + (n - 1) * (size_t)cs >= ctx->ftab_n) return BP_OK;   // left half reaches past the tabled bases
    FtabDigits dG, dH;
    if (!ftab_digits<C>(ctx, tG, dG) || !ftab_digits<C>(ctx, tH, dH)) return BP_OK;
    const u32 lanes = (u32)(2 * n);
    FoldFinish ff;
    BPCHK(fold_finish_plan(ctx, lanes, ff));
    {
    ScopedK tk(ctx, BP_K_FOLD_TAB);
    hipLaunchKernelGGL(k_ipa_fold_tab<C>, dim3((lanes + 255) / 256), dim3(256), 0, ctx->stream, ctx->ftab_G.as<u32>(), ctx->ftab_H.as<u32>(), (u32)ctx->ftab_n,
                       1u << (ctx->ftab_w - 1), d_G, d_H, (u32)n, dG, dH, 3, c0, cs, ff.jac, s.d_G_in, s.d_H_in);
    }
    ctx->fold_took |= FOLD_TOOK_TAB;
    fold_finish_launch<C>(ctx, ff, d_G, d_H, n, 3, lanes);
    done = true;
    return BP_OK;
}

// whether the first fold of a prover round can be deferred (ipa.cuh "TWO fold rounds from the tables"): the vectors are the ctx's
// generator tables read in place, the fold tables cover the bases [0, n + n/2), both multipliers have table digits, and neither this
// round nor the next reaches the frozen-tail length
template <class C> static bool fold_can_defer(bp_ctx* ctx, const IpaState& s, size_t n, const F4& tG1, const F4& tH1) {
    static const bool off = getenv("ARKBP_FOLD_NODEFER") != nullptr || getenv("ARKBP_FOLD_NOTAB") != nullptr;   // A/B switches
    u32 c0 = 0, cs = 1;
    if (off || !ctx->ftab_n || !s.d_G_in || !s.d_H_in || !ftab_cols(ctx, s, c0, cs)) return false;
    // either the whole vectors on one GPU, or this rank's index-cyclic slice (local element j = table base first + j * stride; its
    // MSMs are partial sums followed by the point-reduce) with one more LOCAL round to come
    const bool whole = s.gens_stride == 1 && s.gens_first == 0 && ctx->shard_world == 1 && s.msm_mode == -1;
    const bool slice = s.msm_mode == 2 && ctx->shard_world > 1 && s.first && n > s.min_len;
    if (!whole && !slice) return false;
    if (n < 256 || (n & 1) || (size_t)c0 + (n + n / 2 - 1) * (size_t)cs >= ctx->ftab_n) return false;
    if (s.allow_freeze && n / 2 <= std::max<size_t>(ctx->tune_ipa_freeze_len, 2)) return false;
    if (!s.have_rho) return false;
    FtabDigits d;
    return ftab_digits<C>(ctx, tG1, d) && ftab_digits<C>(ctx, tH1, d);
}
// the second fold after a deferred first one, straight from the tables: m outputs per vector; false when a multiplier has no digits
template <class C> static int launch_tab_fold2(bp_ctx* ctx, const IpaState& s, u32* d_G, u32* d_H, size_t m, const F4& t2G, const F4& t2H, bool& done) {
    typedef host::Fld<typename C::Fr> S;
    done = false;
    FtabDigits3 dG, dH;
    u32 c0 = 0, cs = 1;
    if (!ftab_cols(ctx, s, c0, cs)) return BP_OK;
    if (!ftab_digits<C>(ctx, s.def_tG, dG.d[0]) || !ftab_digits<C>(ctx, t2G, dG.d[1]) || !ftab_digits<C>(ctx, S::mul(s.def_tG, t2G), dG.d[2])) return BP_OK;
    if (!ftab_digits<C>(ctx, s.def_tH, dH.d[0]) || !ftab_digits<C>(ctx, t2H, dH.d[1]) || !ftab_digits<C>(ctx, S::mul(s.def_tH, t2H), dH.d[2])) return BP_OK;
    const u32 lanes = (u32)(2 * m);
    FoldFinish ff;
    BPCHK(fold_finish_plan(ctx, lanes, ff));
    {
        ScopedK tk(ctx, BP_K_FOLD_TAB);
        hipLaunchKernelGGL(k_ipa_fold_tab2<C>, dim3((lanes + 255) / 256), dim3(256), 0, ctx->stream, ctx->ftab_G.as<u32>(), ctx->ftab_H.as<u32>(), (u32)ctx->ftab_n,
                           1u << (ctx->ftab_w - 1), d_G, d_H, (u32)m, dG, dH, ff.jac, s.d_G_in, s.d_H_in, c0, cs);
    }
    ctx->fold_took |= FOLD_TOOK_TAB2;
    fold_finish_launch<C>(ctx, ff, d_G, d_H, m, 3, lanes);
    done = true;
    return BP_OK;
}
// test hook: one fold through the launchers above with caller-chosen multipliers (include/arkbp.h bp_debug_fold).  Everything a
// kernel would read is checked here first: the launchers themselves rely on the prover's rounds for that.
template <class C> static int dbg_fold(bp_ctx* ctx, int route, size_t n, const uint64_t* tGw, const uint64_t* tHw, const uint64_t* t2Gw, const uint64_t* t2Hw, u32 first,
                                       u32 stride, const uint64_t* G_xy, const uint64_t* H_xy, uint64_t* G_out, uint64_t* H_out, u32* took) {
    hipStream_t st = ctx->stream;
    *took = 0;
    const bool ladder = route == BP_DEBUG_FOLD_LADDER || route == BP_DEBUG_FOLD_LADDER_NAF, tab2 = route == BP_DEBUG_FOLD_TAB2;
    const size_t in_pts = tab2 ? 4 * n : 2 * n;   // elements of each vector the fold reads
    const bool whole = first == 0 && stride == 1;
    F4 tG, tH, t2G, t2H;
    memcpy(tG.v, tGw, 32); memcpy(tH.v, tHw, 32);
    if (tab2) { memcpy(t2G.v, t2Gw, 32); memcpy(t2H.v, t2Hw, 32); }
    IpaState s;
    if (!ladder) {
        if (!ctx->ftab_n || !ctx->ftab_G.p || !ctx->ftab_H.p) { g_err = "bp_debug_fold: the fold tables are not built (bp_gens_fold_tables)"; return BP_E_ARG; }
        if (!stride || (size_t)first + (in_pts - 1) * (size_t)stride >= ctx->gens_cap) { g_err = "bp_debug_fold: an element lies outside the installed generators"; return BP_E_ARG; }
        s.gens_first = first; s.gens_stride = stride;
        u32 c0 = 0, cs = 1;
        const size_t tabled = tab2 ? 3 * n : n;   // the elements that are looked up: [0, n), or [0, n + n/2) of the 2n a deferred fold spans
        if (!ftab_cols(ctx, s, c0, cs) || (size_t)c0 + (tabled - 1) * (size_t)cs >= ctx->ftab_n) { g_err = "bp_debug_fold: an element lies outside the fold tables"; return BP_E_ARG; }
    }
    DevBuf wG, wH, out;
    auto done = [&](int rc) { wG.release(); wH.release(); out.release(); return rc; };
#define DFCHK(x) do { int rc__ = (x); if (rc__ != BP_OK) return done(rc__); } while (0)
#define DFHIP(x) do { if ((x) != hipSuccess) { g_err = "bp_debug_fold: HIP error"; return done(BP_E_HIP); } } while (0)
    DFCHK(wG.ensure_exact(in_pts * 64)); DFCHK(wH.ensure_exact(in_pts * 64)); DFCHK(out.ensure_exact(2 * n * 64));
    u32 *d_G = wG.as<u32>(), *d_H = wH.as<u32>();
    if (ladder) {
        DFHIP(hipMemcpyAsync(d_G, G_xy, 2 * n * 64, hipMemcpyHostToDevice, st));
        DFHIP(hipMemcpyAsync(d_H, H_xy, 2 * n * 64, hipMemcpyHostToDevice, st));
        DFCHK(bp_points_import(ctx, d_G, d_G, 2 * n)); DFCHK(bp_points_import(ctx, d_H, d_H, 2 * n));
    } else if (whole) {   // the resident tables read in place; the working vectors only receive
        s.d_G_in = ctx->d_G.as<u32>(); s.d_H_in = ctx->d_H.as<u32>();
    } else {              // the slice as a compact copy, which is also where the results go (ipa_create_cyclic)
        const u32 gb = (u32)((in_pts + 255) / 256);
        hipLaunchKernelGGL(k_cyclic_gather<Blk64>, dim3(gb), dim3(256), 0, st, ctx->d_G.as<u32>(), d_G, (u32)in_pts, first, stride);
        hipLaunchKernelGGL(k_cyclic_gather<Blk64>, dim3(gb), dim3(256), 0, st, ctx->d_H.as<u32>(), d_H, (u32)in_pts, first, stride);
        s.d_G_in = d_G; s.d_H_in = d_H;
    }
    ctx->fold_took = 0;
    bool ran = true;
    if (ladder) DFCHK(launch_uniform_fold<C>(ctx, d_G, d_H, n, tG, tH, 3, route == BP_DEBUG_FOLD_LADDER_NAF));
    else if (!tab2) DFCHK(launch_tab_fold<C>(ctx, s, d_G, d_H, n, tG, tH, ran));
    else { s.def_tG = tG; s.def_tH = tH; DFCHK(launch_tab_fold2<C>(ctx, s, d_G, d_H, n, t2G, t2H, ran)); }
    DFHIP(hipGetLastError());
    *took = ran ? ctx->fold_took : 0;
    if (ran) {
        DFCHK(bp_points_export(ctx, d_G, out.p, n)); DFCHK(bp_points_export(ctx, d_H, out.as<u32>() + n * 16, n));
        DFHIP(hipMemcpyAsync(G_out, out.p, n * 64, hipMemcpyDeviceToHost, st));
        DFHIP(hipMemcpyAsync(H_out, out.as<u32>() + n * 16, n * 64, hipMemcpyDeviceToHost, st));
    }
    DFHIP(ctx_stream_wait(ctx));
#undef DFCHK
#undef DFHIP
    return done(BP_OK);
}

// ---- direct window tables of the first generators (small.cuh): the small-statement path --------------------------------------------
static inline u32 dt_base_pc(int which /* 0 = B, 1 = B_blinding */) { return (u32)which; }
static inline u32 dt_base_G(const bp_ctx* ctx, size_t i) { (void)ctx; return (u32)(2 + i); }
static inline u32 dt_base_H(const bp_ctx* ctx, size_t i) { return (u32)(2 + ctx->dt_cap + i); }
// true when statements of padded size N go over the direct tables on this ctx (building them on first use)
template <class C> static int dt_ensure(bp_ctx* ctx, size_t N, bool& ready) {
    ready = false;
    if (!ctx->tune_direct_max || N == 0 || N > ctx->tune_direct_max || ctx->shard_world > 1 || ctx->gens_cap < N) return BP_OK;
    if (ctx->dt_cap >= N) { ready = true; return BP_OK; }
    if (!ctx->dt_tab.owned && ctx->dt_tab.p) { ctx->dt_tab.p = nullptr; ctx->dt_tab.cap = 0; ctx->dt_tab.owned = true; }   // (a shared table that is too short: build our own)
    hipStream_t st = ctx->stream;
    const size_t cap = std::min(ctx->gens_cap, ctx->tune_direct_max), nb = 2 + 2 * cap;
    ctx->dt_cap = 0;
    BPCHK(ctx->dt_tab.ensure_exact(nb * DT_BASE_BYTES));
    DevBuf ws;
    BPCHK(ws.ensure(nb * DT_WINDOWS * 96));
    auto part = [&](const u32* bases, size_t first, size_t count) -> int {
        hipLaunchKernelGGL(k_dt_window_bases<C>, dim3((u32)((count + 63) / 64)), dim3(64), 0, st, bases, (u32)count, ws.as<u32>() + first * DT_WINDOWS * 24);
        return BP_OK;
    };
    BPCHK(part(ctx->d_pc.as<u32>(), 0, 2));
    BPCHK(part(ctx->d_G.as<u32>(), 2, cap));
    BPCHK(part(ctx->d_H.as<u32>(), 2 + cap, cap));
    const size_t entries = nb * DT_PER_BASE;
    hipLaunchKernelGGL(k_dt_entries<C>, dim3((u32)((entries + 255) / 256)), dim3(256), 0, st, ws.as<u32>(), (u32)nb, ctx->dt_tab.as<u32>());
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));
    ws.release();
    ctx->dt_cap = cap;
    ready = true;
    return BP_OK;
}
static constexpr u32 DT_HOST_SUM_MAX = 16;
// nout MSMs over the direct tables in one launch (+ one finishing launch when more than one workgroup per MSM is worth it): the
// launch half leaves the results on their way to pinned memory, the collect half reads them after the caller's stream wait
template <class C> static int msm_direct_launch(bp_ctx* ctx, const DtJobs& jobs, int nout) {
    hipStream_t st = ctx->stream;
    u32 maxterms = 0;
    for (int o = 0; o < nout; o++) maxterms = std::max(maxterms, jobs.job[o].terms);
    // A quad-cooperative mixed addition is ~4.5 us with a SIMD to itself, the workgroup's tree six levels of the same: one unit (four
    // additions) per quad while that leaves at most one workgroup per CU, two units beyond (the waves then share their SIMDs)
    const size_t units = (size_t)maxterms * DT_UNITS_PER_TERM;
    u32 nblk = (u32)std::max<size_t>(1, (units + 63) / 64);
    if ((size_t)nblk * nout > 256) nblk = (u32)std::min<size_t>(1024, (units + 127) / 128);
    BPCHK(ctx->dt_part.ensure((size_t)DT_MAXOUT * (nblk + 1) * 96));
    if (!ctx->h_dt) HIPCHK(hipHostMalloc((void**)&ctx->h_dt, (size_t)DT_MAXOUT * DT_HOST_SUM_MAX * 96));
    u32* part = ctx->dt_part.as<u32>();
    u32* res = part + (size_t)DT_MAXOUT * nblk * 24;
    // up to DT_HOST_SUM_MAX partial points per MSM are added by the HOST (0.4 us per addition there) instead of a second launch whose
    // six-level tree costs ~35 us however few points it adds
    const bool host_sum = nblk > 1 && nblk <= DT_HOST_SUM_MAX;
    {
        ScopedK tk(ctx, BP_K_MSM_ACCUM);
        hipLaunchKernelGGL(k_dt_accum<C>, dim3(nblk, (u32)nout), dim3(256), 0, st, ctx->dt_tab.as<u32>(), jobs, nblk == 1 ? res : part);
        if (nblk > 1 && !host_sum) hipLaunchKernelGGL(k_dt_finish<C>, dim3((u32)nout), dim3(256), 0, st, part, nblk, res);
    }
    ctx->dt_pending_parts = host_sum ? nblk : 1u;
    ctx->dt_last_nblk = nblk;
    HIPCHK(hipMemcpyAsync(ctx->h_dt, host_sum ? part : res, (size_t)nout * ctx->dt_pending_parts * 96, hipMemcpyDeviceToHost, st));
    return BP_OK;
}
template <class C> static void msm_direct_collect(bp_ctx* ctx, int nout, J4* results) {
    typedef host::Grp<C> G;
    const u64* T = (const u64*)ctx->h_dt;
    const u32 np = ctx->dt_pending_parts;
    for (int o = 0; o < nout; o++) {
        J4 acc = G::inf();
        for (u32 j = 0; j < np; j++) {
            const u64* P = T + 12 * ((size_t)o * np + j);
            const J4 pnt = jac_from_words(P);
            if (pnt.Z.is_zero()) continue;
            acc = np == 1 ? pnt : G::add(acc, pnt);
        }
        results[o] = acc;
    }
    ctx->dt_runs += (uint64_t)nout;
}
template <class C> static int msm_direct(bp_ctx* ctx, const DtJobs& jobs, int nout, J4* results) {
    BPCHK(msm_direct_launch<C>(ctx, jobs, nout));
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    msm_direct_collect<C>(ctx, nout, results);
    return BP_OK;
}
// Two MSMs of n terms each that do not depend on each other — L and R of an inner-product round — as two jobs of ONE fixed-shape
// launch chain (msm_fs_jobs): half the launches and one host wait instead of two, and the two latency-bound trees run side by side.
// Where the pair does not go through that pipeline alone on this ctx, the two msm_run calls run as they always did, in order: a
// sharded ctx or instance (the order of the collectives must not change), fixed-base rows, the GLV route of the latency-first
// entry points, a shape outside the pipeline, BP_TUNE_MSM_PAIR = 0.  A job whose scalars overflow the fixed shape is redone alone on
// the general path; the other job's result stands.
template <class C> static int msm_run_pair(bp_ctx* ctx, const BaseSegs segs[2], const u32* const d_scalars[2], size_t n, int scalars_mont, J4 results[2], int shard_mode = -1) {
    typedef host::Grp<C> G;
    auto two_calls = [&]() -> int {
        for (int j = 0; j < 2; j++) BPCHK(msm_run<C>(ctx, segs[j], d_scalars[j], n, scalars_mont, results[j], 0, -1, shard_mode));
        return BP_OK;
    };
    if (!ctx->tune_msm_pair || n == 0 || n >= (1u << 31) || ctx->shard_world > 1 || shard_mode != -1) return two_calls();
    for (int j = 0; j < 2; j++)
        if (msm_glv_route<C>(ctx, segs[j], n, false, -1)) return two_calls();
    const FsShape sh = msm_fs_shape(n, C::Fr::BITS, 2, false, msm_knobs(ctx), 0, -1, segs[0].fixed_c4 || segs[1].fixed_c4);   // (does not fit below tune_msm_bin_min)
    if (!sh.fits) return two_calls();
    ScalSegs ss[2]; memset(ss, 0, sizeof ss);
    for (int j = 0; j < 2; j++) { ss[j].nseg = 1; ss[j].ptr[0] = d_scalars[j]; ss[j].start[0] = 0; ss[j].start[1] = (u32)n; results[j] = G::inf(); }
    bool over[2] = {false, false};
    BPCHK(msm_fs_jobs<C>(ctx, 2, segs, ss, scalars_mont, sh, results, over));
    ctx->pair_passes++;
    for (int j = 0; j < 2; j++) {
        if (!over[j]) continue;
        ctx->pair_redone++;
        BPCHK(msm_run<C>(ctx, segs[j], d_scalars[j], n, scalars_mont, results[j], 0, -1, shard_mode, nullptr, true));
    }
    return BP_OK;
}
// ... and their affine forms in ark words (one shared inversion)
template <class C> static int msm_run_pair_aff(bp_ctx* ctx, const BaseSegs segs[2], const u32* const d_scalars[2], size_t n, int scalars_mont, uint64_t out0[8], uint64_t out1[8],
                                               int shard_mode = -1) {
    J4 r[2]; A4 a[2];
    BPCHK(msm_run_pair<C>(ctx, segs, d_scalars, n, scalars_mont, r, shard_mode));
    to_aff_many<C>(r, 2, a);
    memcpy(out0, a[0].x.v, 32); memcpy(out0 + 4, a[0].y.v, 32);
    memcpy(out1, a[1].x.v, 32); memcpy(out1 + 4, a[1].y.v, 32);
    return BP_OK;
}

// test hook: msm_run_pair on caller-chosen device arrays (include/arkbp.h bp_debug_msm_pair)
template <class C> static int dbg_msm_pair(bp_ctx* c, const void* const* base_ptrs, const size_t* base_counts, const void* const* d_scalars, size_t n, int canonical,
                                           int latency_first, uint64_t* out_xy) {
    BaseSegs segs[2]; memset(segs, 0, sizeof segs);
    for (int j = 0; j < 2; j++) {
        size_t at = 0; int k = 0;
        for (int r = 0; r < MSM_MAXSEG && base_counts[j * MSM_MAXSEG + r]; r++, k++) {
            if (!base_ptrs[j * MSM_MAXSEG + r]) { g_err = "bp_debug_msm_pair: a run without a pointer"; return BP_E_ARG; }
            segs[j].ptr[k] = (const u32*)base_ptrs[j * MSM_MAXSEG + r]; segs[j].start[k] = (u32)at; at += base_counts[j * MSM_MAXSEG + r];
        }
        segs[j].start[k] = (u32)at; segs[j].nseg = k;
        if (at != n) { g_err = "bp_debug_msm_pair: a job's runs do not add up to n"; return BP_E_ARG; }
    }
    const u32* const scs[2] = {(const u32*)d_scalars[0], (const u32*)d_scalars[1]};
    const bool prev = c->msm_latency_first;
    c->msm_latency_first = latency_first != 0;
    const int rc = msm_run_pair_aff<C>(c, segs, scs, n, canonical ? 0 : 1, out_xy, out_xy + 8);
    c->msm_latency_first = prev;
    return rc;
}

// State of one InnerProductProof::create in flight (the loop body of src/inner_product_proof.rs:70-237 cut at the Fiat-Shamir
// step): ipa_round_lr computes L, R of the current round, ipa_round_fold consumes the challenge.  ipa_create_dev drives it with a
// callback; bp_ipa_begin / bp_ipa_round_LR / bp_ipa_round_fold / bp_ipa_finish expose the same steps for hosts that keep the
// transcript on their side of the boundary, and for the index-cyclic multi-GPU partition (parallel.py), where L and R of a
// round are sums of per-rank partials.
static inline int ipa_lg2(size_t x) { int k = 0; while (((size_t)1 << k) < x) k++; return k; }

template <class C> static int ipa_begin_dev(bp_ctx* ctx, IpaState& s, const u32* d_Q, const u32* d_Gf, const u32* d_Hf, u32* d_G, u32* d_H, u32* d_a, u32* d_b,
                                            size_t n, const F4* gf_halves, const F4* rho_pw, const u32* d_rho_pow, bool allow_freeze = false) {
    typedef host::Fld<typename C::Fr> S;
    if (n == 0 || (n & (n - 1))) { g_err = "ipa_create: n must be a power of two (reference asserts, src/inner_product_proof.rs:66)"; return BP_E_ARG; }
    s = IpaState();
    s.d_Q = d_Q; s.d_Gf = d_Gf; s.d_Hf = d_Hf; s.d_G = d_G; s.d_H = d_H; s.d_a = d_a; s.d_b = d_b; s.n = n;
    s.gamma_G = S::one(); s.gamma_H = S::one();
    if (gf_halves) { s.have_gf = true; s.gf_halves[0] = gf_halves[0]; s.gf_halves[1] = gf_halves[1]; }
    if (rho_pw && d_rho_pow) { s.have_rho = true; s.rho_pw = rho_pw; s.d_rho_pow = d_rho_pow; }
    s.allow_freeze = allow_freeze;
    const size_t fz = std::max<size_t>(ctx->tune_ipa_freeze_len, 2);
    BPCHK(ctx->ipa_sL.ensure((std::max(n, 2 * fz) + 2) * 32));
    BPCHK(ctx->ipa_sR.ensure((std::max(n, 2 * fz) + 2) * 32));
    BPCHK(ctx->ipa_part.ensure(((std::max(n / 2, fz) + 255) / 256 + 1) * 64));
    return BP_OK;
}
// ---- one side of a round's plan (ipa_plan.hpp) as what each MSM runner takes
// the fixed-base rows: the side's runs; Q = qw * B is row 0 of the Pedersen table, its scalar the inner product scaled by qw
static inline int ipa_fb_runs(const IpaSide& sd, const u32* sc, FbRun runs[IPA_MAXSEG], ScalSegs& ss) {
    for (int k = 0; k < sd.nseg; k++) runs[k] = FbRun{sd.seg[k].table, sd.seg[k].first, sd.seg[k].count, sd.seg[k].stride};
    memset(&ss, 0, sizeof ss);
    ss.nseg = 2; ss.ptr[0] = sc; ss.start[0] = 0; ss.start[1] = (u32)sd.ip_slot; ss.ptr[1] = sc + (sd.ip_slot + 1) * 8; ss.start[2] = (u32)sd.terms;
    return sd.nseg;
}
// an ordinary MSM over compact vectors (a plan of IpaShape::compact()): G, H name element 0 of the working vectors or of the round's inputs
static inline BaseSegs ipa_base_segs(const IpaSide& sd, const u32* G, const u32* H, const u32* Q) {
    const u32* const tab[3] = {G, H, Q};
    BaseSegs sg; memset(&sg, 0, sizeof sg);
    sg.nseg = sd.nseg;
    size_t at = 0;
    for (int k = 0; k < sd.nseg; k++) { sg.ptr[k] = tab[sd.seg[k].table] + sd.seg[k].first * 16; sg.start[k] = (u32)at; at += sd.seg[k].count; }
    sg.start[sd.nseg] = (u32)at;
    return sg;
}
// the direct window tables, L and R of a frozen round of half length n: [G | H | B] with c * Q = (c * qw) * B.  Every base belongs to
// exactly one of L, R (k_ipa_frozen_scalars): L takes G where the element sits in the upper half of its period of the current length
// and H in the lower half, R the other way round — only those are visited
static inline void ipa_direct_jobs(const bp_ctx* ctx, const IpaPlan& p, size_t n, const u32* sL, const u32* sR, DtJob jobs[2]) {
    for (int o = 0; o < 2; o++) {
        const IpaSide& sd = p.side[o];
        const u32* sc = o ? sR : sL;
        DtJob& jb = jobs[o];
        memset(&jb, 0, sizeof jb);
        jb.nseg = (u32)sd.nseg;
        size_t at = 0;
        for (int k = 0; k < sd.nseg; at += sd.seg[k].count, k++) {
            const IpaSeg& g = sd.seg[k];
            if (g.table == IPA_Q) jb.seg[k] = DtSeg{sc + (sd.ip_slot + 1) * 8, dt_base_pc(0), 1, 0, 0, 0};
            else jb.seg[k] = DtSeg{sc + at * 8, g.table == IPA_G ? dt_base_G(ctx, g.first) : dt_base_H(ctx, g.first), (u32)(g.count / 2), 0, (u32)n, (u32)g.half};
            jb.terms += jb.seg[k].count;
        }
    }
}
// L, R of the current round (affine, ark layout): src/inner_product_proof.rs:78-131 (first round) / :166-213
template <class C> static int ipa_round_lr(bp_ctx* ctx, IpaState& s, uint64_t Lw[8], uint64_t Rw[8]) {
    typedef host::Fld<typename C::Fr> S;
    if (s.n <= 1 || s.lr_done) { g_err = "ipa: round_LR out of sequence"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    const size_t n = s.n / 2;
    u32* sL = ctx->ipa_sL.as<u32>();
    u32* sR = ctx->ipa_sR.as<u32>();
    const u32* const sc[2] = {sL, sR};
    // the layout of L and R over compact vectors: the working vectors, or the inputs a first or deferred round still reads (an
    // index-cyclic rank's vectors are its compact copy of the slice first + j * stride of the generator tables)
    const IpaShape sh = {s.frozen ? IPA_FROZEN : s.deferred ? IPA_DEFERRED : IPA_PLAIN, n, s.n, s.n0, 0, 0, 1};
    const IpaPlan plan = ipa_plan(sh);
    const size_t terms = plan.side[0].terms, ip = plan.side[0].ip_slot;
    // 1. the scalars of both sides in the order of that layout, the inner products behind them (scaled by qw in the slot after)
    {
        ScopedK tk(ctx, BP_K_IPA_SCALARS);
        const size_t len = s.frozen ? s.n0 : n;
        const u32 gb = (u32)((len + 255) / 256);
        const int pend = s.pending ? (s.h_geo ? 2 : 1) : 0;
        if (s.direct) {
            // one launch: the fold the previous challenge asked for (into the other buffer pair), the scalars, the inner products
            hipLaunchKernelGGL(k_dt_round<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, s.d_a_alt, s.d_b_alt, s.d_cG, s.d_cH, (u32)n, (u32)s.n0, s.fold_pending ? 1 : 0,
                               words_of<S>(s.pend_u), words_of<S>(s.pend_ui), sL, sR, ctx->ipa_part.as<u32>(), ctx->dt_ticket.as<u32>(), words_of<S>(s.qw));
            if (s.fold_pending) { std::swap(s.d_a, s.d_a_alt); std::swap(s.d_b, s.d_b_alt); s.fold_pending = false; }
        } else if (s.frozen) {
            hipLaunchKernelGGL(k_ipa_frozen_scalars<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, s.d_cG, s.d_cH, (u32)n, (u32)s.n0, sL, sR, ctx->ipa_part.as<u32>());
        } else if (s.deferred) {
            // the round after a deferred first fold: L and R over the generator tables themselves with split scalars
            hipLaunchKernelGGL(k_ipa_scalars_deferred<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, (u32)n, sL, sR, ctx->ipa_part.as<u32>(), pend, words_of<S>(s.gamma_G),
                               words_of<S>(s.gamma_H), s.d_rho_pow, words_of<S>(s.def_tG), words_of<S>(s.def_tH));
        } else {
            hipLaunchKernelGGL(k_ipa_scalars<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, s.d_Gf, s.d_Hf, s.first ? 1 : 0, (u32)n, sL, sR, ctx->ipa_part.as<u32>(), pend,
                               words_of<S>(s.gamma_G), words_of<S>(s.gamma_H), s.d_rho_pow);
        }
        if (!s.direct)
            hipLaunchKernelGGL(k_ipa_ip_finish<C>, dim3(1), dim3(256), 0, st, ctx->ipa_part.as<u32>(), gb, sL + ip * 8, sR + ip * 8, words_of<S>(s.qw), !s.frozen && s.have_qw ? 1 : 0);
    }
    // 2. who computes the sums, and over what
    const bool tables = s.d_G_in != nullptr;   // (never once frozen)
    const IpaPolicy pol = ipa_policy({s.frozen, s.direct, s.deferred, s.first, tables, s.have_qw, ctx->fb_cap != 0, s.msm_mode, s.gens_stride});
    BaseSegs segs[2];
    for (int o = 0; o < 2; o++) segs[o] = ipa_base_segs(plan.side[o], tables ? s.d_G_in : s.d_G, tables ? s.d_H_in : s.d_H, s.d_Q);
    IpaPlan rows = plan;   // the same layout in the resident tables' own indices
    if (pol.rows != IPA_ROWS_NONE) {
        IpaShape rs = sh;
        if (s.msm_mode == 2) { rs.g_first = rs.h_first = s.gens_first; rs.stride = s.gens_stride; }
        else { rs.g_first = (size_t)(s.d_G_in - ctx->d_G.as<u32>()) / 16; rs.h_first = (size_t)(s.d_H_in - ctx->d_H.as<u32>()) / 16; }
        rows = ipa_plan(rs);
    }
    // 3. the fixed-base rows of the resident tables first where the policy says so (Q = qw * B rides along as a row of the Pedersen
    // table; a slice reads the rows with its stride), then what they declined.  Every MSM of a slice ends in exactly one point-reduce.
    J4 P[2]; bool done[2] = {false, false};
    for (int o = 0; o < 2; o++) {
        if (pol.rows == IPA_ROWS_EACH || (pol.rows == IPA_ROWS_L_THEN_R && (o == 0 || done[0]))) {
            FbRun runs[IPA_MAXSEG]; ScalSegs ss;
            const int nruns = ipa_fb_runs(rows.side[o], sc[o], runs, ss);
            BPCHK(msm_fixed_run<C>(ctx, runs, nruns, ss, terms, 0, P[o], done[o], pol.rows == IPA_ROWS_EACH ? 2 : -1));
        }
        if (pol.fallback == IPA_FB_SIDE && !done[o]) BPCHK(msm_run<C>(ctx, segs[o], sc[o], terms, 0, P[o], 0, -1, s.msm_mode));
    }
    if (pol.fallback == IPA_FB_DIRECT) {
        DtJobs jobs; memset(&jobs, 0, sizeof jobs);
        ipa_direct_jobs(ctx, plan, n, sL, sR, jobs.job);
        BPCHK(msm_direct<C>(ctx, jobs, 2, P));
    } else if (pol.fallback == IPA_FB_PAIR && !(done[0] && done[1])) {
        BPCHK(msm_run_pair<C>(ctx, segs, sc, terms, 0, P, s.msm_mode));
    } else if (pol.fallback == IPA_FB_TWO && !(done[0] && done[1])) {
        for (int o = 0; o < 2; o++) BPCHK(msm_run<C>(ctx, segs[o], sc[o], terms, 0, P[o], 0, -1, s.msm_mode));
    }
    // 4. the one exit
    A4 LR[2];
    to_aff_many<C>(P, 2, LR);
    aff_out<C>(Lw, LR[0]); aff_out<C>(Rw, LR[1]);
    s.lr_done = true;
    return BP_OK;
}
// the folds of the round for challenge u (ark words): :137-155 (first round) / :214-224
template <class C> static int ipa_round_fold(bp_ctx* ctx, IpaState& s, const uint64_t uw[4]) {
    typedef host::Fld<typename C::Fr> S;
    if (!s.lr_done) { g_err = "ipa: round_fold before round_LR"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    const size_t n = s.n / 2;
    const u32 gb = (u32)((n + 255) / 256);
    u32 *d_G = s.d_G, *d_H = s.d_H;
    const bool first = s.first;
    F4 u; memcpy(u.v, uw, 32);
    F4 ui = S::inv(u);
    auto advance = [&]() { s.round++; s.n = n; s.lr_done = false; };   // every exit: the round is over
    // the ladder kernels fold in place: they need the round-1 inputs in the working vectors (the table fold reads them from the
    // resident generator tables and needs no copy)
    auto working_copy = [&]() -> int {
        if (!s.d_G_in) return BP_OK;
        if (s.d_G_in == s.d_G) { s.d_G_in = s.d_H_in = nullptr; return BP_OK; }   // (an index-cyclic slice: the working vectors ARE the compact copy)
        HIPCHK(hipMemcpyAsync(s.d_G, s.d_G_in, 2 * n * 64, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(s.d_H, s.d_H_in, 2 * n * 64, hipMemcpyDeviceToDevice, st));
        s.d_G_in = s.d_H_in = nullptr;
        return BP_OK;
    };
    if (s.direct) {
        // the next round's k_dt_round folds (a, b and the coefficients); after the last round only a[0], b[0] are left to form
        if (n == 1) {
            ScopedK tk(ctx, BP_K_IPA_FOLD);
            hipLaunchKernelGGL(k_ipa_fold_ab<C>, dim3(1), dim3(256), 0, st, s.d_a, s.d_b, 1u, words_of<S>(u), words_of<S>(ui));
            tk.stop();
            HIPCHK(hipGetLastError());
        } else {
            s.fold_pending = true; s.pend_u = u; s.pend_ui = ui;
        }
        advance();
        return BP_OK;
    }
    if (s.frozen) {
        ScopedK tk(ctx, BP_K_IPA_FOLD);
        hipLaunchKernelGGL(k_ipa_fold_ab<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, (u32)n, words_of<S>(u), words_of<S>(ui));
        hipLaunchKernelGGL(k_ipa_frozen_fold<C>, dim3((u32)((s.n0 + 255) / 256)), dim3(256), 0, st, s.d_cG, s.d_cH, (u32)n, (u32)s.n0, words_of<S>(u), words_of<S>(ui));
        tk.stop();
        HIPCHK(hipGetLastError());
        advance();
        return BP_OK;
    }
    {
        ScopedK tk(ctx, BP_K_IPA_FOLD);
        hipLaunchKernelGGL(k_ipa_fold_ab<C>, dim3(gb), dim3(256), 0, st, s.d_a, s.d_b, (u32)n, words_of<S>(u), words_of<S>(ui));
        const bool gf_ok = first && s.have_gf && !s.gf_halves[0].is_zero() && !s.gf_halves[1].is_zero();
        if (gf_ok && s.have_rho) {
            // both halves uniform.  G as below.  H: u*gL*rho^i*H_L + u^-1*gR*rho^(n+i)*H_R = (u^-1*gR*rho^n) * rho^i * (H_R + t*H_L),
            // t = u^2 * (gL/gR) * rho^-n: the pending factor of H stays geometric, K * rho^i.
            const int k = ipa_lg2(n);
            const F4 s2 = S::mul(u, s.gf_halves[1]);
            const F4 ginv = S::inv(s.gf_halves[1]);
            const F4 tG1 = S::mul(S::mul(ui, s.gf_halves[0]), S::inv(s2)), tH1 = S::mul(S::mul(S::sqr(u), S::mul(s.gf_halves[0], ginv)), s.rho_pw[k]);
            bool tab_done = false;
            if (fold_can_defer<C>(ctx, s, n, tG1, tH1)) {
                // TWO rounds from the tables: nothing is materialised now; the next round's L / R run over the tables with split scalars
                // and its fold (below, `s.deferred`) computes Ghat'' / Hhat'' directly
                s.deferred = true; s.def_tG = tG1; s.def_tH = tH1;
                tab_done = true;
                ctx->folds_deferred++;
            } else
            BPCHK(launch_tab_fold<C>(ctx, s, d_G, d_H, n, tG1, tH1, tab_done));   // the bases are the generator tables themselves: fixed-base look-ups
            if (!tab_done) { BPCHK(working_copy()); BPCHK(launch_uniform_fold<C>(ctx, d_G, d_H, n, tG1, tH1, 3)); }
            s.gamma_G = S::mul(s.gamma_G, s2);
            s.gamma_H = S::mul(S::mul(ui, s.gf_halves[1]), s.rho_pw[32 + k]);
            if (s.have_k0) s.gamma_H = S::mul(s.gamma_H, s.geo_k0);
            s.pending = true; s.h_geo = true;
        } else if (gf_ok) {
            BPCHK(working_copy());
            // G: u^-1*gL*G_L + u*gR*G_R = (u*gR) * (G_R + t*G_L), t = u^-1*gL / (u*gR): uniform, one NAF ladder; H: per-lane factors
            const F4 s2 = S::mul(u, s.gf_halves[1]);
            const F4 tG = S::mul(S::mul(ui, s.gf_halves[0]), S::inv(s2));
            BPCHK(launch_uniform_fold<C>(ctx, d_G, d_H, n, tG, tG, 1));
            FoldFinish ff;
            BPCHK(fold_finish_plan(ctx, n, ff));
            hipLaunchKernelGGL(k_ipa_fold_pts<C>, dim3(gb), dim3(256), 0, st, d_G, d_H, s.d_Gf, s.d_Hf, 1, (u32)n, words_of<S>(u), words_of<S>(ui), 2, ff.jac);
            fold_finish_launch<C>(ctx, ff, d_G, d_H, n, 2, n);
            s.gamma_G = S::mul(s.gamma_G, s2);
            s.pending = true;
        } else if (first) {
            BPCHK(working_copy());
            FoldFinish ff;
            BPCHK(fold_finish_plan(ctx, 2 * n, ff));
            hipLaunchKernelGGL(k_ipa_fold_pts<C>, dim3((u32)((2 * n + 255) / 256)), dim3(256), 0, st, d_G, d_H, s.d_Gf, s.d_Hf, 1, (u32)n, words_of<S>(u),
                               words_of<S>(ui), 3, ff.jac);
            fold_finish_launch<C>(ctx, ff, d_G, d_H, n, 3, 2 * n);
        } else {
            // Ghat' = G_R + u^-2 * G_L, gamma_G *= u;   Hhat' = H_R + u^2 * H_L, gamma_H *= u^-1
            // (geometric pending factor: c[i]/c[n+i] = rho^-n joins t, and K picks up rho^n)
            const int k = ipa_lg2(n);
            const F4 t2G = S::sqr(ui), t2H = s.h_geo ? S::mul(S::sqr(u), s.rho_pw[k]) : S::sqr(u);
            if (s.deferred) {
                bool done2 = false;
                BPCHK(launch_tab_fold2<C>(ctx, s, d_G, d_H, n, t2G, t2H, done2));
                if (done2) ctx->folds_tab2++;
                if (!done2) {   // (a multiplier whose digits do not fit: materialise round 1 after all, then the ladder)
                    bool done1 = false;
                    BPCHK(launch_tab_fold<C>(ctx, s, d_G, d_H, 2 * n, s.def_tG, s.def_tH, done1));
                    if (!done1) {
                        if (s.d_G_in != d_G) {
                        HIPCHK(hipMemcpyAsync(d_G, s.d_G_in, 4 * n * 64, hipMemcpyDeviceToDevice, st));
                        HIPCHK(hipMemcpyAsync(d_H, s.d_H_in, 4 * n * 64, hipMemcpyDeviceToDevice, st));
                        }
                        BPCHK(launch_uniform_fold<C>(ctx, d_G, d_H, 2 * n, s.def_tG, s.def_tH, 3));
                    }
                    BPCHK(launch_uniform_fold<C>(ctx, d_G, d_H, n, t2G, t2H, 3));
                }
                s.deferred = false;
            } else
            BPCHK(launch_uniform_fold<C>(ctx, d_G, d_H, n, t2G, t2H, 3));
            s.gamma_G = S::mul(s.gamma_G, u);
            s.gamma_H = s.h_geo ? S::mul(S::mul(s.gamma_H, ui), s.rho_pw[32 + k]) : S::mul(s.gamma_H, ui);
            s.pending = true;
        }
    }
    HIPCHK(hipGetLastError());
    s.first = false;
    if (!s.deferred) s.d_G_in = s.d_H_in = nullptr;   // (a deferred fold keeps reading the generator tables for one more round)
    advance();
    if (s.allow_freeze && n >= 2 && n <= ctx->tune_ipa_freeze_len) {   // the vectors just reached the freeze length: coefficients from here on
        BPCHK(ctx->ipa_cG.ensure(n * 32)); BPCHK(ctx->ipa_cH.ensure(n * 32));
        s.d_cG = ctx->ipa_cG.as<u32>(); s.d_cH = ctx->ipa_cH.as<u32>();
        hipLaunchKernelGGL(k_ipa_freeze_init<C>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, s.d_cG, s.d_cH, (u32)n, s.pending ? (s.h_geo ? 2 : 1) : 0,
                           words_of<S>(s.gamma_G), words_of<S>(s.gamma_H), s.d_rho_pow);
        HIPCHK(hipGetLastError());
        s.frozen = true; s.n0 = n;
    }
    return BP_OK;
}
// a[0], b[0] -> ark layout on the host (:226-231)
template <class C> static int ipa_finish_dev(bp_ctx* ctx, IpaState& s, uint64_t a_out[4], uint64_t b_out[4]) {
    if (s.n != 1) { g_err = "ipa: finish before the last round"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    BPCHK(ctx->io_out.ensure(64));
    hipLaunchKernelGGL(k_scalars_export<typename C::Fr>, dim3(1), dim3(64), 0, st, s.d_a, ctx->io_out.as<u32>(), 1u);
    hipLaunchKernelGGL(k_scalars_export<typename C::Fr>, dim3(1), dim3(64), 0, st, s.d_b, ctx->io_out.as<u32>() + 8, 1u);
    uint64_t ab[8];
    HIPCHK(hipMemcpyAsync(ab, ctx->io_out.p, 64, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    memcpy(a_out, ab, 32); memcpy(b_out, ab + 4, 32);
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}
// the rounds down to length stop_len: L and R of a round into its row of L_out / R_out, the challenge from the callback, the folds
template <class C> static int ipa_rounds(bp_ctx* ctx, IpaState& s, size_t stop_len, const ChallengeFn& challenge, uint64_t* L_out, uint64_t* R_out) {
    while (s.n > stop_len) {
        uint64_t *Lw = L_out + 8 * s.round, *Rw = R_out + 8 * s.round, uw[4];
        BPCHK(ipa_round_lr<C>(ctx, s, Lw, Rw));
        int rc = challenge(Lw, Rw, uw);
        if (rc) { g_err = "ipa_create: challenge callback failed"; return rc < 0 ? rc : BP_E_ARG; }
        BPCHK(ipa_round_fold<C>(ctx, s, uw));
    }
    return BP_OK;
}
static inline size_t ipa_gather_len(const bp_ctx* ctx) { return ipa_gather_len(ctx->tune_ipa_freeze_len, (size_t)ctx->shard_world); }

// ---- InnerProductProof::create orchestration (src/inner_product_proof.rs:37-239): all vectors device-resident in the engine's
// layouts and consumed (folded in place), like the reference's by-value Vec arguments.
template <class C>
static int ipa_create_dev(bp_ctx* ctx, const u32* d_Q, const u32* d_Gf, const u32* d_Hf, u32* d_G, u32* d_H, u32* d_a, u32* d_b, size_t n,
                          const ChallengeFn& challenge, uint64_t* L_out, uint64_t* R_out, uint64_t a_out[4], uint64_t b_out[4],
                          const F4* gf_halves = nullptr /* optional hint: G_factors == gf_halves[0] on [0,n/2) and gf_halves[1] on [n/2,n) */,
                          const F4* rho_pw = nullptr /* optional hint (with gf_halves): H_factors[i] = rho^i * G_factors[i];
                                                        rho_pw[k] = rho^-(2^k), rho_pw[32+k] = rho^(2^k), k < 32 */,
                          const u32* d_rho_pow = nullptr /* device table of rho^(2^k), resident words */,
                          bool gens_are_tables = false /* d_G, d_H stand for the ctx's generator tables G[0..n), H[0..n) */,
                          bool gens_in_place = false /* ... and were NOT copied: round 1 reads ctx->d_G / d_H, d_G / d_H receive its output */,
                          const F4* q_scalar = nullptr /* Q = q_scalar * B (PedersenGens::B) */,
                          bool direct = false /* (with gens_are_tables and q_scalar, n within the ctx's direct window tables) never fold G and H:
                                                 the coefficients start as the factor vectors, every round's L and R are sums over the tables */) {
    IpaState s;
    BPCHK(ipa_begin_dev<C>(ctx, s, d_Q, d_Gf, d_Hf, d_G, d_H, d_a, d_b, n, gf_halves, rho_pw, d_rho_pow, true));
    if (gens_are_tables) { s.gens_first = 0; s.gens_stride = 1; }
    if (gens_in_place) { s.d_G_in = ctx->d_G.as<u32>(); s.d_H_in = ctx->d_H.as<u32>(); }
    if (n == 1) s.d_G_in = s.d_H_in = nullptr;
    if (q_scalar) { s.have_qw = true; s.qw = *q_scalar; }
    if (direct && gens_are_tables && q_scalar && n >= 2 && ctx->dt_cap >= n) {
        BPCHK(ctx->ipa_cG.ensure(n * 32)); BPCHK(ctx->ipa_cH.ensure(n * 32));
        BPCHK(ctx->ipa_sL.ensure((2 * n + 2) * 32)); BPCHK(ctx->ipa_sR.ensure((2 * n + 2) * 32));
        BPCHK(ctx->ipa_part.ensure(((n + 255) / 256 + 1) * 64));
        HIPCHK(hipMemcpyAsync(ctx->ipa_cG.p, d_Gf, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->ipa_cH.p, d_Hf, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
        BPCHK(ctx->dt_a2.ensure(n * 16)); BPCHK(ctx->dt_b2.ensure(n * 16));   // (the folded vectors: at most n / 2 elements)
        BPCHK(ctx->dt_ticket.ensure(64));
        HIPCHK(hipMemsetAsync(ctx->dt_ticket.p, 0, 64, ctx->stream));   // (the last workgroup of k_dt_round leaves it at zero; an aborted launch would not)
        s.d_cG = ctx->ipa_cG.as<u32>(); s.d_cH = ctx->ipa_cH.as<u32>();
        s.d_a_alt = ctx->dt_a2.as<u32>(); s.d_b_alt = ctx->dt_b2.as<u32>();
        s.d_G_in = s.d_H_in = nullptr;
        s.frozen = true; s.direct = true; s.n0 = n;
    }
    BPCHK(ipa_rounds<C>(ctx, s, 1, challenge, L_out, R_out));
    return ipa_finish_dev<C>(ctx, s, a_out, b_out);
}

// ---- index-cyclic InnerProductProof::create inside a sharded prover -------------------------------------------
// Rank r of `world` keeps the elements i = r + j*world of a, b, G, H and of the factor vectors: element i and its fold partner
// i + n/2 live on the same rank while n >= 2*world, so every fold is local and 1/world of the single-GPU work.  A round's L and R
// are sums of per-rank partial MSMs (the <a_L, b_R> * Q term is linear too): the ctx's point-reduce callback.  When the global
// length reaches the frozen-tail length the ranks all-gather what is left (a few hundred elements) and every rank finishes the
// remaining rounds over the frozen generators, replicated.  L, R, a, b are bit-identical to the single-GPU result.
template <class C>
static int ipa_create_cyclic(bp_ctx* ctx, const u32* d_Q, const u32* d_Gf, const u32* d_Hf, const u32* d_Gtab, const u32* d_Htab, const u32* d_a, const u32* d_b,
                             size_t N, const ChallengeFn& challenge, uint64_t* L_out, uint64_t* R_out, uint64_t a_out[4], uint64_t b_out[4],
                             const F4* gf_halves, const F4* rho_pw, const u32* d_rho_pow, const F4* qw = nullptr /* Q = qw * B (the R1CS prover's Q) */) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    hipStream_t st = ctx->stream;
    const size_t W = (size_t)ctx->shard_world, r = (size_t)ctx->shard_rank;
    const int w = ipa_lg2(W);
    const size_t n_loc = N / W;
    const size_t S_glob = ipa_gather_len(ctx), S_loc = S_glob / W;   // global, local length at which the ranks gather
    // this rank's slices (the generator tables are read in place: no full working copy)
    BPCHK(ctx->cyc_a.ensure(std::max(n_loc, S_glob) * 32)); BPCHK(ctx->cyc_b.ensure(std::max(n_loc, S_glob) * 32));
    BPCHK(ctx->cyc_Gf.ensure(n_loc * 32)); BPCHK(ctx->cyc_Hf.ensure(n_loc * 32));
    BPCHK(ctx->ipa_G.ensure(std::max(n_loc, S_glob) * 64)); BPCHK(ctx->ipa_H.ensure(std::max(n_loc, S_glob) * 64));
    const u32 gb = (u32)((n_loc + 255) / 256);
    hipLaunchKernelGGL(k_cyclic_gather<Blk32>, dim3(gb), dim3(256), 0, st, d_a, ctx->cyc_a.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    hipLaunchKernelGGL(k_cyclic_gather<Blk32>, dim3(gb), dim3(256), 0, st, d_b, ctx->cyc_b.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    hipLaunchKernelGGL(k_cyclic_gather<Blk32>, dim3(gb), dim3(256), 0, st, d_Gf, ctx->cyc_Gf.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    hipLaunchKernelGGL(k_cyclic_gather<Blk32>, dim3(gb), dim3(256), 0, st, d_Hf, ctx->cyc_Hf.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    hipLaunchKernelGGL(k_cyclic_gather<Blk64>, dim3(gb), dim3(256), 0, st, d_Gtab, ctx->ipa_G.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    hipLaunchKernelGGL(k_cyclic_gather<Blk64>, dim3(gb), dim3(256), 0, st, d_Htab, ctx->ipa_H.as<u32>(), (u32)n_loc, (u32)r, (u32)W);
    HIPCHK(hipGetLastError());
    // local geometric hint: H_factors[r + j*W] = rho^r * (rho^W)^j * G_factors: tables of rho^W = the global tables shifted by lg W
    F4 rho_loc[64];
    const bool geo = gf_halves && rho_pw && d_rho_pow;
    if (geo) for (int k = 0; k < 32; k++) { rho_loc[k] = k + w < 32 ? rho_pw[k + w] : S::one(); rho_loc[32 + k] = k + w < 32 ? rho_pw[32 + k + w] : S::one(); }
    IpaState s;
    BPCHK(ipa_begin_dev<C>(ctx, s, d_Q, ctx->cyc_Gf.as<u32>(), ctx->cyc_Hf.as<u32>(), ctx->ipa_G.as<u32>(), ctx->ipa_H.as<u32>(), ctx->cyc_a.as<u32>(),
                           ctx->cyc_b.as<u32>(), n_loc, gf_halves, geo ? rho_loc : nullptr, geo ? d_rho_pow + (size_t)w * 8 : nullptr, false));
    s.msm_mode = 2;
    s.gens_first = (u32)r; s.gens_stride = (u32)W;
    s.d_G_in = s.d_G; s.d_H_in = s.d_H;   // round 1 reads the slice where it lies (and may defer its fold: two rounds from the tables, as on one GPU)
    s.min_len = S_loc;
    if (qw) { s.qw = *qw; s.have_qw = true; }
    F4 rho_r = S::one(), rho_mr = S::one();   // rho^rank, rho^-rank
    if (geo) for (int k = 0; k < w; k++) if ((r >> k) & 1) { rho_r = S::mul(rho_r, rho_pw[32 + k]); rho_mr = S::mul(rho_mr, rho_pw[k]); }
    s.geo_k0 = rho_r; s.have_k0 = geo;
    BPCHK(ipa_rounds<C>(ctx, s, S_loc, challenge, L_out, R_out));
    // gather: [a | b | G | H] of the S_loc local elements, ark layouts, from every rank; global index = rank + j * W
    const size_t m = s.n;   // == S_loc
    const size_t per = m * (32 + 32 + 64 + 64);
    std::vector<host::u8> send(per), recv(per * W);
    {
        const u32 g2 = (u32)((m + 255) / 256);
        BPCHK(ctx->io_out.ensure(per));
        u32* o = ctx->io_out.as<u32>();
        hipLaunchKernelGGL(k_scalars_export<FrP>, dim3(g2), dim3(256), 0, st, s.d_a, o, (u32)m);
        hipLaunchKernelGGL(k_scalars_export<FrP>, dim3(g2), dim3(256), 0, st, s.d_b, o + m * 8, (u32)m);
        hipLaunchKernelGGL(k_points_dev_to_ark<C>, dim3(g2), dim3(256), 0, st, s.d_G, o + m * 16, (u32)m);
        hipLaunchKernelGGL(k_points_dev_to_ark<C>, dim3(g2), dim3(256), 0, st, s.d_H, o + m * 32, (u32)m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(send.data(), o, per, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx_stream_wait(ctx));
    }
    BPCHK(shard_allgather(ctx, send.data(), per, recv.data()));
    std::vector<F4> ga(S_glob), gbv(S_glob);
    std::vector<A4> gG(S_glob), gH(S_glob);
    for (size_t rr = 0; rr < W; rr++) {
        const host::u8* blk = recv.data() + rr * per;
        for (size_t j = 0; j < m; j++) {
            const size_t i = rr + j * W;
            memcpy(&ga[i], blk + j * 32, 32); memcpy(&gbv[i], blk + m * 32 + j * 32, 32);
            memcpy(&gG[i], blk + m * 64 + j * 64, 64); memcpy(&gH[i], blk + m * 128 + j * 64, 64);
        }
    }
    BPCHK(upload_scalars<C>(ctx, ctx->cyc_a.as<u32>(), ga.data(), S_glob));
    BPCHK(upload_scalars<C>(ctx, ctx->cyc_b.as<u32>(), gbv.data(), S_glob));
    HIPCHK(hipMemcpyAsync(ctx->ipa_G.p, gG.data(), S_glob * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_H.p, gH.data(), S_glob * 64, hipMemcpyHostToDevice, st));
    BPCHK(bp_points_import(ctx, ctx->ipa_G.p, ctx->ipa_G.p, S_glob));
    BPCHK(bp_points_import(ctx, ctx->ipa_H.p, ctx->ipa_H.p, S_glob));
    // the tail: generators frozen as gathered, their pending factors as per-element coefficients.  In the global index the
    // geometric factor is K_common * rho^i with K_common = (this rank's K) * rho^-rank — the same on every rank.
    IpaState t;
    BPCHK(ipa_begin_dev<C>(ctx, t, d_Q, nullptr, nullptr, ctx->ipa_G.as<u32>(), ctx->ipa_H.as<u32>(), ctx->cyc_a.as<u32>(), ctx->cyc_b.as<u32>(), S_glob, nullptr, nullptr,
                           nullptr, false));
    BPCHK(ctx->ipa_sL.ensure((2 * S_glob + 1) * 32)); BPCHK(ctx->ipa_sR.ensure((2 * S_glob + 1) * 32));
    BPCHK(ctx->ipa_part.ensure(((S_glob + 255) / 256 + 1) * 64));
    t.round = s.round; t.first = false; t.msm_mode = 0;
    BPCHK(ctx->ipa_cG.ensure(S_glob * 32)); BPCHK(ctx->ipa_cH.ensure(S_glob * 32));
    t.d_cG = ctx->ipa_cG.as<u32>(); t.d_cH = ctx->ipa_cH.as<u32>();
    const F4 kH = s.h_geo ? S::mul(s.gamma_H, rho_mr) : s.gamma_H;
    hipLaunchKernelGGL(k_ipa_freeze_init<C>, dim3((u32)((S_glob + 255) / 256)), dim3(256), 0, st, t.d_cG, t.d_cH, (u32)S_glob, s.pending ? (s.h_geo ? 2 : 1) : 0,
                       words_of<S>(s.gamma_G), words_of<S>(kH), d_rho_pow);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));   // ga .. gH are locals
    t.frozen = true; t.n0 = S_glob;
    BPCHK(ipa_rounds<C>(ctx, t, 1, challenge, L_out, R_out));
    return ipa_finish_dev<C>(ctx, t, a_out, b_out);
}
// whether a sharded prover can partition an IPA of padded size N this way
static inline bool ipa_cyclic_applies(const bp_ctx* ctx, size_t N) {
    const size_t W = (size_t)ctx->shard_world;
    if (W <= 1 || !shard_has_allgather(ctx) || (W & (W - 1)) || N < ctx->tune_cyclic_min) return false;
    return N >= 2 * ipa_gather_len(ctx) && N / W >= 2;   // at least one partitioned round
}

// uploads the host vectors of an IPA instance into the ctx's working buffers (engine layouts)
template <class C>
static int ipa_upload_host(bp_ctx* ctx, const uint64_t* Q, const uint64_t* Gf, const uint64_t* Hf, const uint64_t* Gv, const uint64_t* Hv, const uint64_t* a,
                           const uint64_t* b, size_t n) {
    typedef typename C::Fr Fr;
    hipStream_t st = ctx->stream;
    BPCHK(ctx->ipa_G.ensure(n * 64)); BPCHK(ctx->ipa_H.ensure(n * 64));
    BPCHK(ctx->ipa_a.ensure(n * 32)); BPCHK(ctx->ipa_b.ensure(n * 32));
    BPCHK(ctx->ipa_Gf.ensure(n * 32)); BPCHK(ctx->ipa_Hf.ensure(n * 32));
    BPCHK(ctx->ipa_Q.ensure(64));
    HIPCHK(hipMemcpyAsync(ctx->ipa_G.p, Gv, n * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_H.p, Hv, n * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_Q.p, Q, 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_a.p, a, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_b.p, b, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_Gf.p, Gf, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_Hf.p, Hf, n * 32, hipMemcpyHostToDevice, st));
    BPCHK(bp_points_import(ctx, ctx->ipa_G.p, ctx->ipa_G.p, n));
    BPCHK(bp_points_import(ctx, ctx->ipa_H.p, ctx->ipa_H.p, n));
    BPCHK(bp_points_import(ctx, ctx->ipa_Q.p, ctx->ipa_Q.p, 1));
    const u32 gb = (u32)((n + 255) / 256);
    DevBuf* sc[] = {&ctx->ipa_a, &ctx->ipa_b, &ctx->ipa_Gf, &ctx->ipa_Hf};
    for (auto s : sc) hipLaunchKernelGGL(k_scalars_import<Fr>, dim3(gb), dim3(256), 0, st, s->as<u32>(), s->as<u32>(), (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));   // the host buffers are the caller's: done with them before returning
    return BP_OK;
}
template <class C>
static int ipa_create_host_entry(bp_ctx* ctx, const uint64_t* Q, const uint64_t* Gf, const uint64_t* Hf, const uint64_t* Gv, const uint64_t* Hv,
                                 const uint64_t* a, const uint64_t* b, size_t n, const ChallengeFn& fn, uint64_t* L_out, uint64_t* R_out,
                                 uint64_t* a_out, uint64_t* b_out) {
    BPCHK(ipa_upload_host<C>(ctx, Q, Gf, Hf, Gv, Hv, a, b, n));
    return ipa_create_dev<C>(ctx, ctx->ipa_Q.as<u32>(), ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), ctx->ipa_G.as<u32>(), ctx->ipa_H.as<u32>(),
                             ctx->ipa_a.as<u32>(), ctx->ipa_b.as<u32>(), n, fn, L_out, R_out, a_out, b_out);
}
template <class C>
static int ipa_begin_host_entry(bp_ctx* ctx, const uint64_t* Q, const uint64_t* Gf, const uint64_t* Hf, const uint64_t* Gv, const uint64_t* Hv,
                                const uint64_t* a, const uint64_t* b, size_t n) {
    ctx->ipa_step_active = false;
    if (n == 0 || (n & (n - 1))) { g_err = "ipa_begin: n must be a power of two (reference asserts, src/inner_product_proof.rs:66)"; return BP_E_ARG; }
    BPCHK(ipa_upload_host<C>(ctx, Q, Gf, Hf, Gv, Hv, a, b, n));
    BPCHK(ipa_begin_dev<C>(ctx, ctx->ipa_step, ctx->ipa_Q.as<u32>(), ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), ctx->ipa_G.as<u32>(), ctx->ipa_H.as<u32>(),
                           ctx->ipa_a.as<u32>(), ctx->ipa_b.as<u32>(), n, nullptr, nullptr, nullptr));
    ctx->ipa_step_active = true;
    return BP_OK;
}
// current a, b, G, H (first n_cur elements, ark layout) and the pending factors: G_true[i] = gamma_G * G[i], H_true[i] = gamma_H * H[i]
template <class C>
static int ipa_export_host(bp_ctx* ctx, uint64_t* a, uint64_t* b, uint64_t* G_xy, uint64_t* H_xy, uint64_t gG[4], uint64_t gH[4], size_t* n_cur) {
    typedef typename C::Fr Fr;
    IpaState& s = ctx->ipa_step;
    if (s.lr_done) { g_err = "ipa_export: between round_LR and round_fold"; return BP_E_ARG; }
    hipStream_t st = ctx->stream;
    const size_t n = s.n;
    const u32 gb = (u32)((n + 255) / 256);
    BPCHK(ctx->io_out.ensure(n * 64 * 2 + n * 32 * 2));
    u32* o = ctx->io_out.as<u32>();
    hipLaunchKernelGGL(k_points_dev_to_ark<C>, dim3(gb), dim3(256), 0, st, s.d_G, o, (u32)n);
    hipLaunchKernelGGL(k_points_dev_to_ark<C>, dim3(gb), dim3(256), 0, st, s.d_H, o + n * 16, (u32)n);
    hipLaunchKernelGGL(k_scalars_export<Fr>, dim3(gb), dim3(256), 0, st, s.d_a, o + n * 32, (u32)n);
    hipLaunchKernelGGL(k_scalars_export<Fr>, dim3(gb), dim3(256), 0, st, s.d_b, o + n * 40, (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(G_xy, o, n * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(H_xy, o + n * 16, n * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(a, o + n * 32, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(b, o + n * 40, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    memcpy(gG, s.gamma_G.v, 32); memcpy(gH, s.gamma_H.v, 32);
    *n_cur = n;
    return BP_OK;
}

#include "r1cs_host.inc"

// ---- unit-test kernels -----------------------------------------------------------------------------
template <class F> __global__ void k_dbg_field(int op, const u32* a, const u32* b, u32* out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 wa[8], wb[8];
    load_words8(wa, a + (size_t)i * 8); load_words8(wb, b + (size_t)i * 8);
    Fe x = fe_load_ark<F>(wa), y = fe_load_ark<F>(wb), r;
    switch (op) {
        case 0: r = fe_mul<F>(x, y); break;
        case 1: r = fe_norm(fe_add(x, y)); break;
        case 2: r = fe_sub<F, 2>(x, y); break;
        case 3: r = fe_sqr<F>(x); break;
        default: r = fe_inv<F>(x); break;
    }
    fe_store_ark<F>(wa, r);
    store_words8(out + (size_t)i * 8, wa);
}
template <class C> __global__ void k_dbg_point(int op, const u32* p, const u32* q, const u32* k, u32* out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[16];
    load_words8(w, p + (size_t)i * 16); load_words8(w + 8, p + (size_t)i * 16 + 8);
    Aff P = aff_load_ark<C>(w);
    load_words8(w, q + (size_t)i * 16); load_words8(w + 8, q + (size_t)i * 16 + 8);
    Aff Q = aff_load_ark<C>(w);
    Jac r;
    if (op == 0) r = jac_add<C>(jac_from_aff<C>(P), jac_from_aff<C>(Q));
    else if (op == 1) r = jac_madd<C>(jac_from_aff<C>(P), Q);
    else if (op == 2) r = jac_dbl<C>(jac_from_aff<C>(P));
    else {
        u32 kk[8];
        load_words8(kk, k + (size_t)i * 8);
        r = jac_inf<C>();
        for (int b = 255; b >= 0; b--) {
            r = jac_dbl<C>(r);
            if ((kk[b >> 5] >> (b & 31)) & 1) r = jac_madd<C>(r, P);
        }
    }
    Aff a = jac_to_aff<C>(r);
    aff_store_ark<C>(w, a);
    store_words8(out + (size_t)i * 16, w); store_words8(out + (size_t)i * 16 + 8, w + 8);
}
// raw-representative unit ops: the kernels live in a translation unit of their own (csrc/dbg_raw.hip), so that this unit's device code
// is not touched by them; word counts per case as in csrc/dbg_raw.cuh
namespace arkbp {
int dbg_raw_launch_field(hipStream_t st, int field, int op, const u32* in, u32* out, u32 n);
int dbg_raw_launch_point(hipStream_t st, int curve, int op, const u32* in, u32* out, u32 n);
}
static constexpr int RAW_F_IN = 36, RAW_F_OUT = 18, RAW_F_COUNT = 13, RAW_P_IN = 54, RAW_P_OUT = 28, RAW_P_COUNT = 7, RAW_P_QADD = 4;

template <class C> static int dbg_rng_draws(void* transcript, const uint64_t* witness, size_t nw, const uint8_t* seeds, int lanes, size_t count, uint64_t* out) {
    typedef typename C::Fr FrP; typedef host::Fld<FrP> S;
    std::vector<std::unique_ptr<host::TranscriptRng>> rngs;
    for (int j = 0; j < lanes; j++) {
        rngs.emplace_back(new host::TranscriptRng(*(host::Transcript*)transcript));
        for (size_t i = 0; i < nw; i++) { F4 w; memcpy(w.v, witness + 4 * i, 32); host::u8 b[32]; S::to_bytes(b, w); rngs[j]->rekey("v_blinding", b, 32); }
        host::ChaChaRng ext(seeds + 32 * j);
        rngs[j]->finalize(ext);
    }
    if (lanes == 1) { for (size_t i = 0; i < count; i++) { F4 x = host::rand_fe<FrP>(*rngs[0]); memcpy(out + 4 * i, x.v, 32); } return BP_OK; }
#if defined(__x86_64__)
    if (lanes != 8 || !host::cpu_has_avx512() || count < 3) return BP_E_ARG;
    host::TranscriptRng* rp[8];
    for (int j = 0; j < 8; j++) {
        for (size_t i = 0; i < 3; i++) { F4 x = host::rand_fe<FrP>(*rngs[j]); memcpy(out + 4 * (j * count + i), x.v, 32); }
        rp[j] = rngs[j].get();
        if (rp[j]->s.pos != 8 || rp[j]->s.pos_begin != 0) return BP_E_ARG;
    }
    std::vector<u64> words((count - 3) * 4 * 8);
    host::transcript_rng_x8_words(rp, words.data(), (count - 3) * 4);
    for (int j = 0; j < 8; j++)
        for (size_t i = 3; i < count; i++)
            for (int w = 0; w < 4; w++) {
                u64 x = words[(4 * (i - 3) + w) * 8 + j];
                if (w == 3 && FrP::BITS < 256) x &= (~(u64)0) >> (256 - FrP::BITS);  // Fp::rand masks the top limb
                out[4 * (j * count + i) + w] = x;
            }
    // the scalar continuation from the x8 state must also agree: one more draw each, returned in place of the last one
    for (int j = 0; j < 8; j++) { F4 x = host::rand_fe<FrP>(*rngs[j]); (void)x; }
    return BP_OK;
#else
    return BP_E_ARG;
#endif
}

// ---- recorder handles (see include/arkbp.h): a Prover<G, T> or Verifier<G, T> of the reference as seen through the C ABI ----
struct bp_cs {
    int curve = 0;
    bool proving = false;
    host::Transcript* tr = nullptr;                 // the caller's transcript handle (borrowed, like `T: BorrowMut<Transcript>`)
    std::unique_ptr<host::Transcript> owned_tr;     // statements own theirs
    std::unique_ptr<host::ConstraintSystem<Secq>> cs0;
    std::unique_ptr<host::ConstraintSystem<Zorro>> cs1;
    ProvePre<Secq> pre0;
    ProvePre<Zorro> pre1;
    std::unique_ptr<HostCsc> csc;                   // constraint index of a single-phase statement (built on first need, outside prove())
    bool csc_tried = false;
    std::shared_ptr<const HostCsc> csc_shared;      // ... or the index of the recording it shares (bp_prover_new_like), owned by the recording
    host::u8 rng32[32] = {0};                       // what prove() draws from the external rng
    bool have_rng = false;
    bool consumed = false;                          // prove(self) / verify(self)
    bool running = false;                           // inside prove / verify: the randomized-phase callbacks may still record
    bool check = false;                             // prover: the witness-check guard (bp_prover_set_check)
    std::vector<A4> commitments;                    // V points in commit order (both modes)
    A4 pc_B, pc_Bb;                                 // prover: the pc_gens of Prover::new when they are not PedersenGens::default() (bp_prover_new_gens)
    bool pc_custom = false;
    std::vector<uint8_t> wire;                      // verifier: pending wire commitments, 33 bytes each (bp_verifier_commit_compressed_batch, defer)
    host::Strobe wire_state;                        // the transcript's state when the first of them was stored
    size_t wire_count() const { return wire.size() / 33; }
    virtual ~bp_cs() {}
    template <class C> host::ConstraintSystem<C>* cs();
    size_t num_vars() const { return curve == 0 ? cs0->num_vars : cs1->num_vars; }
    size_t num_constraints() const { return curve == 0 ? cs0->num_constraints() : cs1->num_constraints(); }
};
template <> host::ConstraintSystem<Secq>* bp_cs::cs<Secq>() { return cs0.get(); }
template <> host::ConstraintSystem<Zorro>* bp_cs::cs<Zorro>() { return cs1.get(); }
// scenario statements: a prover handle plus what the scenario made public
struct bp_stmt : bp_cs {
    int scenario = 0;
    host::StatementIO io;
};

template <class C> static void cs_handle_init(bp_cs* h, bool proving, host::Transcript* tr) {
    h->curve = C::ID; h->proving = proving; h->tr = tr;
    auto* cs = new host::ConstraintSystem<C>();
    cs->tr = tr; cs->proving = proving; cs->owner = h;
    if (C::ID == 0) h->cs0.reset((host::ConstraintSystem<Secq>*)cs); else h->cs1.reset((host::ConstraintSystem<Zorro>*)cs);
    host::TP<C>::r1cs_domain_sep(*tr);   // Prover::new (prover.rs:291-308) / Verifier::new (verifier.rs:252-263)
}
// the pair a prover handle commits under: Prover::new(&pc_gens, ..) keeps a reference to it (prover.rs:291-308)
template <class C> static host::PedersenGens<C> cs_pair(const bp_cs* h) {
    if (!h->pc_custom) return host::PedersenGens<C>::default_ref();
    host::PedersenGens<C> pc; pc.B = h->pc_B; pc.B_blinding = h->pc_Bb;
    return pc;
}
template <class C> static void cs_pair_set(bp_cs* h, const A4& B, const A4& Bb) {
    const auto& d = host::PedersenGens<C>::default_ref();
    h->pc_custom = !(B == d.B && Bb == d.B_blinding);
    h->pc_B = B; h->pc_Bb = Bb;
}
// a prover and the ctx it commits or proves on must hold the same pair: the reference's Prover has ONE pc_gens for both
template <class C> static bool cs_pair_matches_t(const bp_cs* h, bp_ctx* c) {
    host::PedersenGens<C> cp; pc_pair<C>(c, cp);
    const host::PedersenGens<C> hp = cs_pair<C>(h);
    return hp.B == cp.B && hp.B_blinding == cp.B_blinding;
}
static int cs_pair_check(const char* who, bp_ctx* c, const bp_cs* h, size_t instance) {
    if (h->curve == 0 ? cs_pair_matches_t<Secq>(h, c) : cs_pair_matches_t<Zorro>(h, c)) return BP_OK;
    g_err = std::string(who) + ": the Pedersen generators of prover " + std::to_string(instance) + " are not the ctx's (bp_prover_new_gens / bp_pedersen_gens_install)";
    return BP_E_ARG;
}
template <class C> static int stmt_build(bp_stmt* s, const uint64_t* params, const uint8_t* seed, bp_ctx* ctx = nullptr) {
    s->owned_tr.reset(new host::Transcript(host::scenario_label(s->scenario)));
    cs_handle_init<C>(s, true, s->owned_tr.get());
    host::ChaChaRng prng(seed);
    host::PedersenGens<C> pc = host::PedersenGens<C>::default_ref();
    if (ctx) { pc_pair<C>(ctx, pc); cs_pair_set<C>(s, pc.B, pc.B_blinding); pedersen_attach<C>(ctx, pc); }   // (the host-only form stays on the default pair)
    int rc = host::scenario_prover<C>(*s->cs<C>(), pc, prng, s->scenario, params, s->io);
    if (rc) return rc;
    s->commitments = s->io.commitments;
    prng.fill_bytes(s->rng32, 32); s->have_rng = true;   // the scenario's external rng is consumed by prove() for exactly these bytes
    s->csc.reset(new HostCsc());
    if (!build_host_csc<C>(*s->cs<C>(), *s->csc)) s->csc.reset();
    s->csc_tried = true;
    return BP_OK;
}
// The constraint index of a single-phase statement (null: two-phase, or not indexable): statement construction, not prove().  Built on
// first need; a prover that shares a recording and recorded nothing itself gets the recording's own, built once for all of them.
template <class C> static const HostCsc* cs_index(bp_cs* s) {
    const host::ConstraintSystem<C>& cs = *s->cs<C>();
    if (cs.base && cs.own_empty() && cs.deferred.empty()) {
        if (!s->csc_shared) s->csc_shared = host::shared_host_csc<C>(*cs.base);
        return s->csc_shared.get();
    }
    if (!s->csc_tried) {
        s->csc.reset(new HostCsc());
        if (!build_host_csc<C>(cs, *s->csc)) s->csc.reset();
        s->csc_tried = true;
    }
    return s->csc.get();
}
// what a like-prover (bp_prover_new_like) must hold before anything of it is consumed: its witness, and every commitment the shared
// constraints name
template <class C> static bool cs_like_ready_t(const bp_cs* s, std::string& why) {
    const host::ConstraintSystem<C>& cs = *const_cast<bp_cs*>(s)->cs<C>();
    if (!cs.like) return true;
    if (!cs.assigned) { why = "a like-prover has no witness (bp_prover_assign_multipliers)"; return false; }
    if (cs.base) for (const host::VTerm& t : cs.base->vterms) if (t.j >= cs.v.size()) { why = "a like-prover holds fewer commitments than the shared constraints name"; return false; }
    return true;
}
static int cs_like_ready(const char* who, const bp_cs* s, size_t instance) {
    std::string why;
    if (s->curve == 0 ? cs_like_ready_t<Secq>(s, why) : cs_like_ready_t<Zorro>(s, why)) return BP_OK;
    g_err = std::string(who) + ": instance " + std::to_string(instance) + ": " + why;
    return BP_E_ARG;
}
// a prover whose witness lies in device memory (bp_prover_assign_multipliers_dev) proves, checks and joins a batch only on a ctx of
// that device: asked before anything is consumed
static int cs_dev_witness_check(const char* who, const bp_ctx* c, const bp_cs* s, size_t instance) {
    const host::DevWitness& w = s->curve == 0 ? s->cs0->dev : s->cs1->dev;
    if (!w.held() || (c && !c->host_only && c->device == w.device)) return BP_OK;
    g_err = std::string(who) + ": instance " + std::to_string(instance) + ": its witness lies in the memory of device " + std::to_string(w.device) + ", which is not this ctx's";
    return BP_E_ARG;
}
// ... and to the host with it, where a route reads it there (a host-assigned prover is left alone)
static int cs_dev_witness_to_host(bp_ctx* c, bp_cs* s) {
    if (!(s->curve == 0 ? s->cs0->dev : s->cs1->dev).held()) return BP_OK;
    return s->curve == 0 ? prove_need_aO<Secq>(c, *s->cs0) : prove_need_aO<Zorro>(c, *s->cs1);
}
template <class C> static int cs_prove(bp_ctx* c, bp_cs* s, uint8_t* proof_out, size_t* proof_len, double* timing) {
    host::ProofData pf;
    StageTimes tm;
    auto* pre = C::ID == 0 ? (ProvePre<C>*)&s->pre0 : (ProvePre<C>*)&s->pre1;
    const HostCsc* csc = cs_index<C>(s);
    WcGuard guard; guard.on = s->check;
    c->unsat.clear();
    int rc = r1cs_prove<C>(c, *s->cs<C>(), s->rng32, pf, tm, pre, csc, nullptr, nullptr, s->check ? &guard : nullptr);
    s->cs<C>()->drop_dev_witness(c);   // (the prover is consumed: a witness still in device memory is wiped and freed)
    if (rc == BP_E_UNSATISFIED) c->unsat.emplace_back((uint64_t)0, guard.report);
    if (rc) return rc;
    std::vector<host::u8> bytes = host::proof_to_bytes<C>(pf);
    if (bytes.size() > *proof_len) { g_err = "prove: output buffer too small"; return BP_E_ARG; }
    memcpy(proof_out, bytes.data(), bytes.size()); *proof_len = bytes.size();
    if (timing) { timing[0] = tm.total; timing[1] = 0; timing[2] = tm.rng; timing[3] = tm.upload; timing[4] = tm.commit_msm; timing[5] = tm.flatten; timing[6] = tm.poly; timing[7] = tm.ipa; }
    return BP_OK;
}
// `count` live provers of one curve: the host twin without a device, else one index upload, one launch sequence and one wait for all
template <class C> static int cs_check_batch(bp_ctx* c, size_t count, bp_cs* const* hs, bp_witness_report* out) {
    for (size_t k = 0; k < count; k++) BPCHK(prove_need_aO<C>(c, *hs[k]->cs<C>()));   // (the host twin and this call's own upload read the witness and a_O on the host)
    if (!c || c->host_only) {
        for (size_t k = 0; k < count; k++) host::witness_check_host<C>(*hs[k]->cs<C>(), out[k]);
        return BP_OK;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(ctx_stream_wait(c));   // (the staging's previous use is complete)
    WcRun<C> wc;
    wc.own.resize(count);
    std::vector<char> ok(count, 1);
    host_pool_ensure(c, count);
    // (a prover that shares a recording and recorded nothing itself: the recording's index, built once, resident on this ctx)
    std::vector<std::shared_ptr<const HostRowIndex>> shared(count);
    auto index = [&](size_t k, const host::RowIndexPar& par) {
        const host::ConstraintSystem<C>& cs = *hs[k]->cs<C>();
        if (cs.base && cs.own_empty()) shared[k] = host::shared_row_index<C>(*cs.base, cs.v.size(), WC_PIECE, par);
        ok[k] = shared[k] || build_row_index<C>(cs, WC_PIECE, wc.own[k], par) ? 1 : 0;
    };
    if (count == 1) { if (hs[0]->cs<C>()->num_terms() > ((size_t)1 << 16)) host_pool_ensure(c, 2); index(0, [&](size_t cnt, const std::function<void(size_t)>& fn) { pool_range(c, 0, cnt, fn); }); }
    else pool_range(c, 0, count, [&](size_t k) { index(k, nullptr); });
    for (size_t k = 0; k < count; k++) {
        if (!ok[k]) { g_err = "prover_check: the constraints of instance " + std::to_string(k) + " cannot be indexed"; return BP_E_ARG; }
        WcItem<C> it; it.cs = hs[k]->cs<C>(); it.idx = shared[k] ? shared[k].get() : &wc.own[k];
        if (shared[k] && count == 1 && c->shard_world <= 1) BPCHK(pl_row<C>(c, it.cs->base, *shared[k], it.dev));   // (one call's items never outnumber the cache: a single one)
        wc.items.push_back(it);
    }
    int rc = wc_enqueue<C>(c, wc, nullptr);
    if (!rc) rc = wc_fetch<C>(c, wc);
    const int rcw = wc_wipe_dev<C>(c, wc);
    const hipError_t e = ctx_stream_wait(c);
    wc_wipe_host<C>(c, wc);
    if (!rc) rc = rcw;
    if (!rc && e != hipSuccess) { g_err = std::string("prover_check: ") + hipGetErrorString(e); rc = BP_E_HIP; }
    if (rc) return rc;
    for (size_t k = 0; k < count; k++) host::witness_report_from_flags<C>(*hs[k]->cs<C>(), wc.flags(c, k), out[k]);
    if (c->profiling) collect_timers(c);
    return BP_OK;
}
template <class C> static int cs_precompute_batch(bp_cs** hs, size_t count) {
    for (size_t g = 0; g < count; g += 8) {
        const size_t c = std::min<size_t>(8, count - g);
        host::ConstraintSystem<C>* css[8]; ProvePre<C>* pres[8]; const host::u8* rngs[8];
        for (size_t j = 0; j < c; j++) {
            css[j] = hs[g + j]->cs<C>(); rngs[j] = hs[g + j]->rng32;
            pres[j] = C::ID == 0 ? (ProvePre<C>*)&hs[g + j]->pre0 : (ProvePre<C>*)&hs[g + j]->pre1;
        }
        prove_precompute_batch<C>(css, rngs, pres, c);
    }
    return BP_OK;
}
// ---- verifier commitments from the wire (include/arkbp.h: bp_verifier_commit_compressed_batch) ---------------------------------
// A verifier handle may hold its commitments as the 33-byte encodings it received (bp_cs::wire) next to the transcript state of
// that moment.  They become Verifier::commit calls either here (wire_materialize: one decode for all instances of a call, then the
// appends on the pool) or never: k_vfe_points decodes them for a batch the device front end takes (VfyDevBatch::commit_wire).
template <class C> static int verifier_commit(bp_cs* h, const uint64_t* V_xy, size_t count, bp_var* vars);
static bool strobe_eq(const host::Strobe& a, const host::Strobe& b) { return !memcmp(a.st.b, b.st.b, 200) && a.pos == b.pos && a.pos_begin == b.pos_begin && a.cur == b.cur; }
// n encodings -> affine ark words; a rejected one gives zero words and ok = 0 (ark-serialize's rules, host_math.hpp deser_compressed).
// With a device: framing on the pool, the roots in ONE k_points_decompress launch.  Without (null or host-only ctx): host roots.
template <class C> static int wire_decode(bp_ctx* ctx, const uint8_t* c33, size_t n, A4* out, uint8_t* ok) {
    typedef host::Fld<typename C::Fq> Fq;
    if (!n) return BP_OK;
    if (!ctx || ctx->host_only) {
        host_pool_ensure(ctx, n);
        pool_range(ctx, 0, n, [&](size_t i) { A4 p; const bool good = host::Grp<C>::deser_compressed(p, c33 + 33 * i); out[i] = good ? p : A4{}; ok[i] = good ? 1 : 0; });
        return BP_OK;
    }
    std::vector<F4> xs(n); std::vector<u32> fl(n);
    host_pool_ensure(ctx, (n + 255) / 256);
    pool_range(ctx, 0, (n + 255) / 256, [&](size_t c) {
        for (size_t i = c * 256, hi = std::min(n, i + 256); i < hi; i++) {
            const uint8_t* d = c33 + 33 * i;
            fl[i] = d[32];
            bool good = !(fl[i] & 0x3f) && (fl[i] & 0xc0) != 0xc0 && Fq::from_bytes(xs[i], d);
            if (good && (fl[i] & 0x40) && !xs[i].is_zero()) good = false;
            if (!good) { xs[i] = F4{{0, 0, 0, 0}}; fl[i] = 0xFFu; }   // malformed framing: not ok below, whatever the kernel makes of it
        }
    });
    std::vector<A4> pts; std::vector<u32> okv;
    BPCHK(decompress_points<C>(ctx, xs.data(), fl.data(), n, pts, okv));
    for (size_t i = 0; i < n; i++) { ok[i] = fl[i] != 0xFFu && okv[i]; out[i] = ok[i] ? pts[i] : A4{}; }
    return BP_OK;
}
// every use of pending commitments: the borrowed transcript must still be where it was when they were stored
static int wire_check_states(const char* who, size_t count, bp_cs* const* vs) {
    for (size_t k = 0; k < count; k++) {
        const bp_cs* h = vs[k];
        if (h->wire.empty()) continue;
        if (!h->tr || !strobe_eq(h->tr->s, h->wire_state)) {
            g_err = std::string(who) + ": instance " + std::to_string(k) + ": the transcript changed while wire commitments were pending (bp_verifier_materialize before binding more data)";
            return BP_E_ARG;
        }
    }
    return BP_OK;
}
// what every entry point over an array of verifier handles asks of it (`who` opens the message): each handle live, a verifier and
// on the ctx's curve; none given twice (two pool threads on one recorder would race, and verify(self) takes one instance): any count
static int verifiers_check(const char* who, const bp_ctx* c, size_t count, bp_cs* const* verifiers) {
    for (size_t k = 0; k < count; k++) {
        const bp_cs* h = verifiers[k];
        if (!h || h->consumed || h->proving || h->curve != c->curve) { g_err = std::string(who) + ": every instance needs a live verifier of the ctx's curve"; return BP_E_ARG; }
    }
    if (count > 1) {
        std::vector<const bp_cs*> sorted(verifiers, verifiers + count);
        std::sort(sorted.begin(), sorted.end(), std::less<const bp_cs*>());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { g_err = std::string(who) + ": a verifier is consumed by ONE instance"; return BP_E_ARG; }
    }
    return BP_OK;
}
// bp_r1cs_batch_verify_locate only: a like-instance holds every commitment the shared constraints name (else verify_prepare refuses it mid-pass)
template <class C> static int verifiers_cover_constraints(const char* who, size_t count, bp_cs* const* verifiers) {
    const host::FrozenRecording* seen = nullptr;
    size_t need = 0;
    for (size_t k = 0; k < count; k++) {
        const host::ConstraintSystem<C>* cs = verifiers[k]->cs<C>();
        const host::FrozenRecording* b = cs->base.get();
        if (!b) continue;
        if (b != seen) { seen = b; need = 0; for (const auto& vt : b->vterms) need = std::max(need, (size_t)vt.j + 1); }
        if (cs->V.size() + verifiers[k]->wire_count() < need) { g_err = std::string(who) + ": the constraints refer to more commitments than a verifier holds (bp_verifier_commit)"; return BP_E_ARG; }
    }
    return BP_OK;
}
// verify(self) over an array of handles: consumed on entry, `running` (the randomized-phase callbacks may record) until the call leaves, however it leaves
struct VerifyingScope {
    bp_cs* const* vs;
    size_t count;
    VerifyingScope(bp_cs* const* vs_, size_t count_) : vs(vs_), count(count_) { for (size_t k = 0; k < count; k++) { vs[k]->consumed = true; vs[k]->running = true; } }
    ~VerifyingScope() { for (size_t k = 0; k < count; k++) vs[k]->running = false; }
    VerifyingScope(const VerifyingScope&) = delete;
};
// instances 0 .. n of a call over recorded handles: the array itself (idx null) or the members idx names (the passes of
// bp_r1cs_batch_verify_locate).  Two pointers: closures hold it by value.
struct CsView {
    bp_cs* const* vs;
    const uint32_t* idx;
    bp_cs* operator()(size_t j) const { return vs[idx ? idx[j] : j]; }
};
// the pending commitments of instances at(0 .. count): decoded together, then Verifier::commit per instance on the pool.  st[k] =
// BP_E_FORMAT for an instance with a rejected encoding: it keeps its pending bytes, handle and transcript untouched.
template <class C> static int wire_materialize(bp_ctx* ctx, size_t count, CsView at, int* st) {
    std::vector<size_t> off(count + 1, 0);
    for (size_t k = 0; k < count; k++) { st[k] = BP_OK; off[k + 1] = off[k] + at(k)->wire_count(); }
    const size_t tot = off[count];
    if (!tot) return BP_OK;
    std::vector<uint8_t> all(tot * 33), ok(tot);
    std::vector<A4> pts(tot);
    host_pool_ensure(ctx, count);
    pool_range(ctx, 0, count, [&](size_t k) { const bp_cs* h = at(k); if (!h->wire.empty()) memcpy(all.data() + off[k] * 33, h->wire.data(), h->wire.size()); });
    BPCHK(wire_decode<C>(ctx, all.data(), tot, pts.data(), ok.data()));
    if (ctx) (ctx->host_only ? ctx->cw_host : ctx->cw_prologue_gpu) += tot;
    pool_range(ctx, 0, count, [&](size_t k) {
        bp_cs* h = at(k);
        const size_t mk = off[k + 1] - off[k];
        if (!mk) return;
        for (size_t j = 0; j < mk; j++) if (!ok[off[k] + j]) { st[k] = BP_E_FORMAT; return; }
        h->wire.clear();
        st[k] = verifier_commit<C>(h, (const uint64_t*)(pts.data() + off[k]), mk, nullptr);
    });
    return BP_OK;
}
// the device front end's view of a batch of like-instances: all commitments pending (same count), or none
template <class C> static bool wire_dev_form(size_t n, CsView at, bool& wire, size_t& m) {
    bp_cs* h0 = at(0);
    wire =!h0->wire.empty();
    m = wire ? h0->wire_count() : h0->cs<C>()->V.size();
    for (size_t k = 0; k < n; k++) {
        bp_cs* h = at(k);
        if (wire ? (h->wire_count() != m || !h->cs<C>()->V.empty()) : !h->wire.empty()) return false;
    }
    return true;
}

template <class C> static int points_compress_t(const uint64_t* xy, size_t n, uint8_t* out) {
    for (size_t i = 0; i < n; i++) {
        A4 p; memcpy(&p, xy + 8 * i, 64);
        if (!host::Grp<C>::on_curve(p)) { g_err = "bp_points_compress: point " + std::to_string(i) + " is not on the curve"; return BP_E_ARG; }
        host::Grp<C>::ser_compressed(out + 33 * i, p);
    }
    return BP_OK;
}
template <class C>
static int verifier_commit_wire_batch(bp_ctx* c, size_t count, bp_cs* const* vs, const size_t* m_each, const uint8_t* c33, int defer, bp_var* vars_out, int* status) {
    const std::vector<size_t> off = prefix_offsets(m_each, count);
    for (size_t k = 0; k < count; k++) {   // the variables are known before anything is decoded: Committed(i) in commit order
        if (status) status[k] = BP_OK;
        const size_t first = vs[k]->cs<C>()->V.size() + vs[k]->wire_count();
        if (vars_out) for (size_t j = 0; j < m_each[k]; j++) { vars_out[off[k] + j].kind = BP_VAR_COMMITTED; vars_out[off[k] + j].index = (uint32_t)(first + j); }
    }
    if (defer) {
        for (size_t k = 0; k < count; k++) {
            bp_cs* h = vs[k];
            if (!m_each[k]) continue;
            if (h->wire.empty()) h->wire_state = h->tr->s;   // (a later deferred call keeps the first snapshot: checked equal on entry)
            h->wire.insert(h->wire.end(), c33 + 33 * off[k], c33 + 33 * off[k + 1]);
        }
        return BP_OK;
    }
    // immediate: one decode for the whole call, then Verifier::commit per verifier on the pool
    const size_t tot = off[count];
    std::vector<A4> pts(tot);
    std::vector<uint8_t> ok(tot);
    BPCHK(wire_decode<C>(c, c33, tot, pts.data(), ok.data()));
    (c->host_only ? c->cw_host : c->cw_prologue_gpu) += tot;
    std::vector<int> st(count, BP_OK);
    host_pool_ensure(c, count);
    pool_range(c, 0, count, [&](size_t k) {
        for (size_t j = off[k]; j < off[k + 1]; j++) if (!ok[j]) { st[k] = BP_E_FORMAT; return; }
        if (m_each[k]) st[k] = verifier_commit<C>(vs[k], (const uint64_t*)(pts.data() + off[k]), m_each[k], nullptr);
    });
    int first = BP_OK;
    for (size_t k = 0; k < count; k++) { if (status) status[k] = st[k]; if (st[k] && !first) first = st[k]; }
    if (first == BP_E_FORMAT) g_err = "bp_verifier_commit_compressed_batch: a commitment's encoding was rejected";
    return first;
}

// The provider (r1cs_host.inc VfyProvider) over instances at(0 .. n) of recorded verifier handles, for every entry point that takes
// such handles.  The closures hold the view by value: they outlive the scope a subset was formed in (bp_r1cs_batch_verify_locate).
template <class C> static void cs_provider(bp_ctx* c, size_t n, CsView at, VfyProvider<C>& prov) {
    typedef host::ConstraintSystem<C> CS;
    prov.m_of = [at](size_t k) { return at(k)->cs<C>()->V.size(); };
    prov.get = [at](size_t k, VfyInstance<C>& out) -> int { out.cs = at(k)->cs<C>(); return BP_OK; };
    // like-instances of one recording (bp_verifier_new_like): the device front end continues their transcripts from where
    // Verifier::commit left them.  Randomized constraints (BP_TUNE_VFY_DEVICE = 2): every instance's callbacks run on its own handle
    // (a C callback records through the handle it receives), with the challenges its transcript produced on the device
    const bool two_ok = c->tune_vfy_device >= 2;
    prov.dev_batch = [at, n, two_ok](VfyDevBatch<C>& db) -> bool {
        const CS* c0 = at(0)->cs<C>();
        if (!c0->base || !c0->tr || (!c0->deferred.empty() && !two_ok)) return false;
        for (size_t k = 0; k < n; k++) {
            const CS* ck = at(k)->cs<C>();
            if (ck->base != c0->base || ck->cs_off.size() != 1 || ck->deferred.size() != c0->deferred.size() || ck->phase2 || ck->num_vars != c0->num_vars || ck->V.size() != c0->V.size() ||
                !ck->tr)
                return false;
        }
        bool wire; size_t m;
        if (!wire_dev_form<C>(n, at, wire, m)) return false;
        db.src = c0; db.m = m; db.absorb_commitments = wire; db.shared_state = false;
        db.state_of = [at](size_t k) { return (const host::Strobe*)&at(k)->cs<C>()->tr->s; };   // (pending commitments: the pre-commit state, checked on entry)
        if (wire) db.commit_wire = [at](size_t k) { return (const uint8_t*)at(k)->wire.data(); };   // (the bytes stay pending: a later pass reuses them)
        else db.commit_xy = [at](size_t k) { return (const uint64_t*)at(k)->cs<C>()->V.data(); };
        if (!c0->deferred.empty()) db.cs_of = [at](size_t k) { return at(k)->cs<C>(); };
        return true;
    };
    // batches of several gadgets: what makes a handle a like-instance of others, and a class of them as the front end sees it
    prov.class_id = [at](size_t k, VfyClassId& id) -> bool {
        bp_cs* h = at(k);
        const CS* ck = h->cs<C>();
        if (!ck->base || !ck->tr || ck->cs_off.size() != 1 || ck->phase2 || ck->num_vars != ck->base->num_vars) return false;
        id.wire = !h->wire.empty();
        if (id.wire && !ck->V.empty()) return false;   // (some commitments committed, some pending: the host replay's)
        id.rec = ck->base.get(); id.m = id.wire ? h->wire_count() : ck->V.size(); id.two = !ck->deferred.empty();
        id.pos = ck->tr->s.pos; id.pos_begin = ck->tr->s.pos_begin;
        return true;
    };
    prov.dev_class = [at](const uint32_t* idx, size_t cnt, VfyDevBatch<C>& db) -> bool {
        bp_cs* h0 = at(idx[0]);
        const bool wire = !h0->wire.empty();
        db.src = h0->cs<C>(); db.m = wire ? h0->wire_count() : h0->cs<C>()->V.size(); db.absorb_commitments = wire; db.shared_state = false;
        db.state_of = [at, idx](size_t j) { return (const host::Strobe*)&at(idx[j])->cs<C>()->tr->s; };
        if (wire) db.commit_wire = [at, idx](size_t j) { return (const uint8_t*)at(idx[j])->wire.data(); };
        else db.commit_xy = [at, idx](size_t j) { return (const uint64_t*)at(idx[j])->cs<C>()->V.data(); };
        (void)cnt;
        return true;
    };
    prov.prologue = [c, n, at](const uint32_t* idx, size_t cnt, int* st) -> int {
        if (!idx) return wire_materialize<C>(c, n, at, st);
        std::vector<uint32_t> map(cnt);   // (a view holds one index map: the two composed)
        for (size_t j = 0; j < cnt; j++) map[j] = at.idx ? at.idx[idx[j]] : idx[j];
        return wire_materialize<C>(c, cnt, CsView{at.vs, map.data()}, st);
    };
}
// the weights of a call over recorded handles: the caller's words, or 1 for Verifier::verify's single instance
template <class C> static std::vector<F4> cs_weights(const uint64_t* alphas, size_t count) {
    std::vector<F4> al(count);
    for (size_t k = 0; k < count; k++) { if (alphas) memcpy(al[k].v, alphas + 4 * k, 32); else al[k] = host::Fld<typename C::Fr>::one(); }
    return al;
}

// batch_verify over recorded verifier handles (each consumed, like `verify(self)`)
template <class C>
static int cs_batch_verify(bp_ctx* c, size_t count, bp_cs* const* vs, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* alphas, double* timing,
                           uint64_t* point_out) {
    const std::vector<size_t> poff = prefix_offsets(proof_lens, count);
    const std::vector<F4> al = cs_weights<C>(alphas, count);
    VfyProvider<C> prov;
    cs_provider<C>(c, count, CsView{vs, nullptr}, prov);
    VerifyingScope scope(vs, count);
    return batch_verify_core<C>(c, count, prov, proofs, poff.data(), al.data(), timing, point_out);
}

// ---- debug hooks for the reference-held constants (src/util.rs:147-166, src/inner_product_proof.rs:556-562) ----
// out[i] = x^i for i < n, through pow_table — the device function with which the prover / verifier kernels form y^i, y^-i and z^q
// (the reference's exp_iter, util.rs:55-58).  xtab: x^(2^k), k < 32, resident words.
// host only: the challenge sequence of up to eight scenario verifications, from the per-proof live transcript (verify_prepare_t over
// LiveTr) or from the lockstep replay (replay_challenges_x8) — both must follow ONE Fiat-Shamir schedule
template <class C> struct LogLiveTr {
    LiveTr<C> in;
    std::vector<F4>* log;
    void append_u64(const char* l, uint64_t x) { in.append_u64(l, x); }
    bool vpoint(const char* l, const A4& p) { return in.vpoint(l, p); }
    void point(const char* l, const A4& p) { in.point(l, p); }
    void scalar(const char* l, const F4& x) { in.scalar(l, x); }
    F4 chal(const char* l) { const F4 c = in.chal(l); log->push_back(c); return c; }
    void ipp(uint64_t n) { in.ipp(n); }
    F4 chal_r() { const F4 c = in.chal_r(); log->push_back(c); return c; }
    bool inverse(F4&) { return false; }
};
template <class C>
static int dbg_verify_challenges(size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* commit_xy,
                                 const size_t* ms, const uint64_t* publics, const size_t* npubs, int use_x8, uint64_t* out, size_t* nchal) {
    std::vector<std::unique_ptr<host::Transcript>> trs(count);
    std::vector<std::unique_ptr<host::ConstraintSystem<C>>> css(count);
    std::vector<host::ProofData> pfs(count);
    size_t po = 0, co = 0, uo = 0;
    for (size_t k = 0; k < count; k++) {
        host::StatementIO io;
        io.commitments.resize(ms[k]); io.publics.resize(npubs[k]);
        if (ms[k]) memcpy(io.commitments.data(), commit_xy + 8 * co, ms[k] * 64);
        if (npubs[k]) memcpy(io.publics.data(), publics + 4 * uo, npubs[k] * 32);
        trs[k].reset(new host::Transcript(host::scenario_label(scenarios[k])));
        css[k].reset(new host::ConstraintSystem<C>());
        BPCHK(build_verifier_cs<C>(*css[k], *trs[k], scenarios[k], params + 8 * k, io));
        BPCHK(host::proof_from_bytes<C>(pfs[k], proofs + po, proof_lens[k]));
        po += proof_lens[k]; co += ms[k]; uo += npubs[k];
    }
    if (use_x8) {
#if defined(__x86_64__)
        if (count != 8 || !host::cpu_has_avx512()) return 1;
        host::ConstraintSystem<C>* csp[8]; const host::ProofData* pfp[8];
        for (int j = 0; j < 8; j++) { csp[j] = css[j].get(); pfp[j] = &pfs[j]; }
        std::vector<F4> ch[8];
        if (!replay_challenges_x8<C>(csp, pfp, ch)) return 1;
        for (int j = 0; j < 8; j++) { nchal[j] = ch[j].size(); if (ch[j].size() > 40) return BP_E_ARG; if (!ch[j].empty()) memcpy(out + (size_t)j * 40 * 4, ch[j].data(), ch[j].size() * 32); }
        return BP_OK;
#else
        return 1;
#endif
    }
    for (size_t k = 0; k < count; k++) {
        std::vector<F4> log;
        LogLiveTr<C> T{LiveTr<C>{*trs[k]}, &log};
        VerifyPrep<C> vp;
        const int rc = verify_prepare_t<C>(*css[k], pfs[k], (size_t)-1, vp, T);
        if (rc) return rc;
        if (log.size() > 40) return BP_E_ARG;
        nchal[k] = log.size();
        if (!log.empty()) memcpy(out + k * 40 * 4, log.data(), log.size() * 32);
    }
    return BP_OK;
}
template <class C> __global__ void k_dbg_scalars_to_ark(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    fe_store_ark<typename C::Fr>(w, load_fe_dev<typename C::Fr>(in + (size_t)i * 8));
    store_words8(out + (size_t)i * 8, w);
}
template <class F> __global__ void k_dbg_exp_iter(const u32* __restrict__ xtab, u32 n, u32* __restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 w[8];
    fe_store_ark<F>(w, pow_table<F>(xtab, i));
    store_words8(out + (size_t)i * 8, w);
}
template <class C> static int dbg_exp_iter(bp_ctx* ctx, const uint64_t* x, size_t n, uint64_t* out) {
    typedef host::Fld<typename C::Fr> S;
    F4 tab[32]; memcpy(tab[0].v, x, 32);
    for (int k = 1; k < 32; k++) tab[k] = S::sqr(tab[k - 1]);
    BPCHK(ctx->r_ypow.ensure(64 * 32)); BPCHK(ctx->io_out.ensure(std::max<size_t>(n, 1) * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->r_ypow.as<u32>(), tab, 32));
    hipLaunchKernelGGL(k_dbg_exp_iter<typename C::Fr>, dim3((u32)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->r_ypow.as<u32>(), (u32)n, ctx->io_out.as<u32>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, ctx->io_out.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx_stream_wait(ctx));
    return BP_OK;
}
// <a, b> over the scalar field with the kernels InnerProductProof::create uses for c_L = <a_L, b_R> (k_ipa_scalars +
// k_ipa_ip_finish; inner_product_proof.rs:83-84, 390-399): the inputs are laid out as a || 0 and 0 || b, so c_L = <a, b>, c_R = 0.
template <class C> static int dbg_inner_product(bp_ctx* ctx, const uint64_t* a, const uint64_t* b, size_t n, uint64_t* out) {
    typedef host::Fld<typename C::Fr> S;
    hipStream_t st = ctx->stream;
    std::vector<F4> av(2 * n, S::zero()), bv(2 * n, S::zero()), ones(2 * n, S::one());
    memcpy(av.data(), a, n * 32); memcpy(bv.data() + n, b, n * 32);
    BPCHK(ctx->ipa_a.ensure(2 * n * 32)); BPCHK(ctx->ipa_b.ensure(2 * n * 32)); BPCHK(ctx->ipa_Gf.ensure(2 * n * 32)); BPCHK(ctx->ipa_Hf.ensure(2 * n * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->ipa_a.as<u32>(), av.data(), 2 * n)); BPCHK(upload_scalars<C>(ctx, ctx->ipa_b.as<u32>(), bv.data(), 2 * n));
    BPCHK(upload_scalars<C>(ctx, ctx->ipa_Gf.as<u32>(), ones.data(), 2 * n)); BPCHK(upload_scalars<C>(ctx, ctx->ipa_Hf.as<u32>(), ones.data(), 2 * n));
    const u32 gb = (u32)((n + 255) / 256);
    BPCHK(ctx->ipa_sL.ensure((2 * n + 1) * 32)); BPCHK(ctx->ipa_sR.ensure((2 * n + 1) * 32)); BPCHK(ctx->ipa_part.ensure((size_t)gb * 64));
    u32* sL = ctx->ipa_sL.as<u32>();
    u32* sR = ctx->ipa_sR.as<u32>();
    Words8 zero; memset(&zero, 0, sizeof zero);
    hipLaunchKernelGGL(k_ipa_scalars<C>, dim3(gb), dim3(256), 0, st, ctx->ipa_a.as<u32>(), ctx->ipa_b.as<u32>(), ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), 0, (u32)n, sL, sR,
                       ctx->ipa_part.as<u32>(), 0, zero, zero, (const u32*)nullptr);
    hipLaunchKernelGGL(k_ipa_ip_finish<C>, dim3(1), dim3(256), 0, st, ctx->ipa_part.as<u32>(), gb, sL + 2 * n * 8, sR + 2 * n * 8, zero, 0);
    HIPCHK(hipGetLastError());
    uint64_t canon[4];
    HIPCHK(hipMemcpyAsync(canon, sL + 2 * n * 8, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    F4 r = S::from_canon(canon);
    memcpy(out, r.v, 32);
    return BP_OK;
}

// ---- helpers of the bp_cs entry points (templates cannot live inside extern "C") ----
#define CS_DISPATCH(h, expr0, expr1) ((h)->curve == 0 ? (expr0) : (expr1))
// ---- r1cs::Prover / Verifier / ConstraintSystem for a caller's own gadgets -----------------------------------------------------
static inline bool cs_live(bp_cs* h) { return h && (!h->consumed || h->running); }
static inline void terms_in(std::vector<host::Term>& out, const bp_var* vars, const uint64_t* coefs, size_t n) {
    out.resize(n);
    for (size_t i = 0; i < n; i++) { out[i].v.k = (host::VKind)vars[i].kind; out[i].v.i = vars[i].index; memcpy(out[i].c.v, coefs + 4 * i, 32); }
}
template <class C> static bool terms_valid(bp_cs* h, const bp_var* vars, size_t n) {
    const host::ConstraintSystem<C>& cs = *h->cs<C>();
    const size_t m = cs.proving ? cs.v.size() : cs.V.size() + h->wire_count();   // (pending wire commitments are variables already)
    for (size_t i = 0; i < n; i++) {
        if (vars[i].kind > BP_VAR_ONE) return false;
        if (vars[i].kind == BP_VAR_COMMITTED ? vars[i].index >= m : vars[i].kind != BP_VAR_ONE && vars[i].index >= cs.num_vars) return false;
    }
    return true;
}
static inline bp_var var_out(const host::Var& v) { bp_var o; o.kind = (uint32_t)v.k; o.index = v.i; return o; }
template <class C> static int verifier_new_like(bp_cs* of, host::Transcript* tr, bp_cs** out) {
    host::ConstraintSystem<C>& src = *of->cs<C>();
    BPCHK(src.freeze());
    bp_cs* h = new bp_cs();
    cs_handle_init<C>(h, false, tr);
    h->cs<C>()->init_like(src);
    *out = h;
    return BP_OK;
}

template <class C> static int prover_new_like(bp_cs* of, host::Transcript* tr, bp_cs** out) {
    host::ConstraintSystem<C>& src = *of->cs<C>();
    BPCHK(src.freeze(true));
    of->csc.reset(); of->csc_tried = false;   // (its index is the recording's from here)
    bp_cs* h = new bp_cs();
    cs_handle_init<C>(h, true, tr);
    h->cs<C>()->init_like_prover(src);
    h->pc_custom = of->pc_custom; h->pc_B = of->pc_B; h->pc_Bb = of->pc_Bb;
    *out = h;
    return BP_OK;
}
template <class C> static int prover_assign_multipliers(bp_cs* h, const uint64_t* left, const uint64_t* right, size_t count) {
    host::ConstraintSystem<C>& cs = *h->cs<C>();
    if (!cs.like || cs.assigned || cs.phase2 || !cs.base || count != cs.base->num_vars) { g_err = "assign_multipliers: needs a like-prover (bp_prover_new_like) without a witness, and as many values as the recording has multipliers"; return BP_E_ARG; }
    for (size_t i = 0; i < 4 * count; i += 4)
        if (host::Fld<typename C::Fr>::geq_p(left + i) || host::Fld<typename C::Fr>::geq_p(right + i)) { g_err = "assign_multipliers: a value is not a reduced scalar"; return BP_E_ARG; }
    cs.assign_multipliers((const F4*)left, (const F4*)right, count);
    return BP_OK;
}

template <class C> static int prover_commit(bp_cs* h, bp_ctx* ctx, const uint64_t* v, const uint64_t* blind, size_t count, uint64_t* V_xy, bp_var* vars) {
    host::ConstraintSystem<C>& cs = *h->cs<C>();
    if (cs.phase2) return BP_E_ARG;
    host::PedersenGens<C> pc = cs_pair<C>(h);
    if (ctx) pedersen_attach<C>(ctx, pc);   // (the entry point has checked that the ctx's tables are multiples of this pair)
    std::vector<A4> pts(count);
    BPCHK(pc.commit_many((const F4*)v, (const F4*)blind, count, pts.data()));
    for (size_t i = 0; i < count; i++) {   // Prover::commit (prover.rs:327-341), in order
        const u32 idx = (u32)cs.v.size();
        F4 a, b; memcpy(a.v, v + 4 * i, 32); memcpy(b.v, blind + 4 * i, 32);
        cs.v.push_back(a); cs.v_blinding.push_back(b);
        host::TP<C>::append_point(*cs.tr, "V", pts[i]);
        h->commitments.push_back(pts[i]);
        if (V_xy) memcpy(V_xy + 8 * i, &pts[i], 64);
        if (vars) { vars[i].kind = BP_VAR_COMMITTED; vars[i].index = idx; }
    }
    return BP_OK;
}
template <class C> static int verifier_commit(bp_cs* h, const uint64_t* V_xy, size_t count, bp_var* vars) {
    host::ConstraintSystem<C>& cs = *h->cs<C>();
    if (cs.phase2) return BP_E_ARG;
    for (size_t i = 0; i < count; i++) {   // Verifier::commit (verifier.rs:279-287)
        A4 p; memcpy(&p, V_xy + 8 * i, 64);
        const u32 idx = (u32)cs.V.size();
        cs.V.push_back(p);
        host::TP<C>::append_point(*cs.tr, "V", p);
        h->commitments.push_back(p);
        if (vars) { vars[i].kind = BP_VAR_COMMITTED; vars[i].index = idx; }
    }
    return BP_OK;
}
// a like-instance shares its source's phase-1 constraints: recording more of them there would fork the shared structure
template <class C> static bool cs_can_record(bp_cs* h) { const auto& cs = *h->cs<C>(); return cs.phase2 || !cs.base; }

template <class C> static int cs_multiply_t(bp_cs* h, const bp_var* lv, const uint64_t* lc, size_t nl, const bp_var* rv, const uint64_t* rc, size_t nr, bp_var out[3]) {
    if (!terms_valid<C>(h, lv, nl) || !terms_valid<C>(h, rv, nr)) return BP_E_ARG;
    std::vector<host::Term> l, r; terms_in(l, lv, lc, nl); terms_in(r, rv, rc, nr);
    host::Var o[3];
    h->cs<C>()->multiply(l.data(), nl, r.data(), nr, o);
    for (int i = 0; i < 3; i++) out[i] = var_out(o[i]);
    h->csc_tried = false; h->csc.reset();
    return BP_OK;
}
template <class C> static int cs_allocate_t(bp_cs* h, const uint64_t* assignment, bp_var* out) {
    F4 a; if (assignment) memcpy(a.v, assignment, 32);
    host::Var o;
    int rc = h->cs<C>()->allocate(assignment ? &a : nullptr, o);
    if (rc) return rc;
    *out = var_out(o);
    return BP_OK;
}
template <class C> static int cs_allocate_multiplier_t(bp_cs* h, const uint64_t* l, const uint64_t* r, bp_var out[3]) {
    F4 a, b; if (l) memcpy(a.v, l, 32); if (r) memcpy(b.v, r, 32);
    host::Var o[3];
    int rc = h->cs<C>()->allocate_multiplier(l ? &a : nullptr, r ? &b : nullptr, o);
    if (rc) return rc;
    for (int i = 0; i < 3; i++) out[i] = var_out(o[i]);
    return BP_OK;
}
template <class C> static int cs_constrain_t(bp_cs* h, const bp_var* vars, const uint64_t* coefs, size_t n) {
    if (!terms_valid<C>(h, vars, n)) return BP_E_ARG;
    std::vector<host::Term> t; terms_in(t, vars, coefs, n);
    h->cs<C>()->constrain(t.data(), n);
    h->csc_tried = false; h->csc.reset();
    return BP_OK;
}
// bulk forms: one call per gadget instead of one per gate
template <class C> static int cs_allocate_multipliers_t(bp_cs* h, const uint64_t* l, const uint64_t* r, size_t count, uint32_t* first) {
    host::ConstraintSystem<C>& cs = *h->cs<C>();
    if (cs.proving && (!l || !r)) return BP_E_MISSING;
    if (first) *first = (uint32_t)cs.num_vars;
    cs.reserve(count, 0, 0);
    for (size_t i = 0; i < count; i++) {
        host::Var o[3];
        if (cs.proving) { F4 a, b; memcpy(a.v, l + 4 * i, 32); memcpy(b.v, r + 4 * i, 32); cs.allocate_multiplier(&a, &b, o); }
        else cs.allocate_multiplier(nullptr, nullptr, o);
    }
    return BP_OK;
}
template <class C> static int cs_constrain_many_t(bp_cs* h, const bp_var* vars, const uint64_t* coefs, const size_t* offsets, size_t nc) {
    host::ConstraintSystem<C>& cs = *h->cs<C>();
    const size_t nt = offsets[nc];
    if (!terms_valid<C>(h, vars, nt)) return BP_E_ARG;
    for (size_t q = 0; q < nc; q++) if (offsets[q] > offsets[q + 1]) return BP_E_ARG;
    cs.reserve(0, nc, nt);
    std::vector<host::Term> t; terms_in(t, vars, coefs, nt);
    for (size_t q = 0; q < nc; q++) cs.constrain(t.data() + offsets[q], offsets[q + 1] - offsets[q]);
    h->csc_tried = false; h->csc.reset();
    return BP_OK;
}
template <class C> static int cs_specify_t(bp_cs* h, bp_randomize_cb cb, void* user) {
    // the closure receives the handle the randomized phase runs on: the recorder passes itself, and a like-instance's copy of the
    // closure must reach ITS handle — so the handle is found through the recorder, not captured
    h->cs<C>()->specify_randomized_constraints([cb, user](host::ConstraintSystem<C>& cs) -> int { return cb(user, (bp_cs*)cs.owner); });
    return BP_OK;
}
#define CS_RECORD_GUARD(h) do { if (!cs_live(h)) return BP_E_ARG; if (!CS_DISPATCH(h, cs_can_record<Secq>(h), cs_can_record<Zorro>(h))) { g_err = (h)->proving ? "this prover shares its phase-1 constraints (bp_prover_new_like): only commits and randomized constraints can be added" : "this verifier shares its phase-1 constraints (bp_verifier_new_like): only commits and randomized constraints can be added"; return BP_E_ARG; } } while (0)

// ---- C ABI ----------------------------------------------------------------------------------------
#if defined(__x86_64__)
template <class C> __attribute__((target("avx512f"))) static void dbg_append_points_x8(void* const* trs, int lanes, const char* label, const uint64_t* xy, size_t npts) {
    host::StrobeX8 sx;
    sx.broadcast(((host::Transcript*)trs[0])->s);
    uint8_t ser[8][72];
    const uint8_t* ptr[8];
    for (int l = 0; l < 8; l++) { ptr[l] = ser[l]; memset(ser[l], 0, 72); }
    for (size_t v = 0; v < npts; v++) {
        for (int l = 0; l < lanes; l++) {
            A4 p; memcpy(p.x.v, xy + ((size_t)l * npts + v) * 8, 32); memcpy(p.y.v, xy + ((size_t)l * npts + v) * 8 + 4, 32);
            host::Grp<C>::ser_uncompressed(ser[l], p);
        }
        sx.append_message_each(label, ptr, 65);
    }
    host::Strobe* outs[8];
    for (int l = 0; l < lanes; l++) outs[l] = &((host::Transcript*)trs[l])->s;
    sx.scatter(outs, lanes);
}
#endif

#if defined(__x86_64__)
__attribute__((target("avx512f"))) static int dbg_challenge_x8(void* const* trs, const char* msg_label, const uint8_t* msg, size_t msg_len, const char* chal_label, size_t nbytes,
                                                                uint8_t* out) {
    host::StrobeX8 sx;
    const host::Strobe* in[8];
    for (int l = 0; l < 8; l++) in[l] = &((host::Transcript*)trs[l])->s;
    if (!sx.gather(in)) return BP_E_ARG;
    sx.append_message_same(msg_label, msg, msg_len);
    uint8_t buf[8][64];
    uint8_t* wp[8];
    for (int l = 0; l < 8; l++) wp[l] = buf[l];
    sx.challenge_bytes_each(chal_label, wp, nbytes);
    for (int l = 0; l < 8; l++) memcpy(out + (size_t)l * nbytes, buf[l], nbytes);
    host::Strobe* outs[8];
    for (int l = 0; l < 8; l++) outs[l] = &((host::Transcript*)trs[l])->s;
    sx.scatter(outs, 8);
    return BP_OK;
}
#endif

#include "prove_batch.inc"   // bp_prover_prove_batch, bp_prover_commit_batch (the C entry points are declared extern "C" by the header)
#include "verify_each.inc"   // bp_verifier_verify_batch, bp_r1cs_verify_each_scenarios, bp_debug_msm_each
#include "msm_batch.inc"     // bp_msm_batch, bp_msm_batch_dev, bp_ctx_msm_batch_stats, bp_debug_msm_batch_plan

// ---- bp_r1cs_batch_verify_locate: batch verification that names the failing instances --------------------------------------------
// The planner (verify_locate.inc) asks for passes over subsets of the batch; a pass is ONE call of batch_verify_core over the
// subset's own provider, proofs and weights, gathered through an index map.  Instance k keeps weight k in every pass.
#include "verify_locate.inc"
// sub(idx, n, out): the provider of instances idx[0 .. n) of the batch.  restore(idx, n): puts those instances back into the state
// they had on entry to the call (recorded handles; scenario providers build their recordings anew in every pass).
template <class C> using LocateSubFn = std::function<void(const uint32_t*, size_t, VfyProvider<C>&)>;
template <class C>
static int locate_core(bp_ctx* ctx, size_t count, const LocateSubFn<C>& sub, const std::function<void(const uint32_t*, size_t)>& restore, const uint8_t* proofs,
                       const size_t* poff /* count + 1 */, const F4* alphas, int* status, double* timing, double snap_s) {
    const double t_entry = now_s(), snap0 = snap_s;
    double t_first = 0, t_later = 0;
    const size_t leaf = ctx->tune_verify_locate_leaf ? ctx->tune_verify_locate_leaf : 1;
    LocatePlanner plan(count, leaf, status);
    std::vector<uint8_t> buf;
    std::vector<size_t> spoff;
    std::vector<F4> sal;
    // the subset's proofs in one contiguous buffer with its own offsets, its weights likewise; the whole batch is used in place
    auto gather = [&](const uint32_t* idx, size_t n, const uint8_t*& pr, const size_t*& po, const F4*& al) {
        if (n == count) { pr = proofs; po = poff; al = alphas; return; }   // (a contiguous range of the survivors that holds every instance)
        spoff.assign(n + 1, 0);
        for (size_t j = 0; j < n; j++) spoff[j + 1] = spoff[j] + (poff[idx[j] + 1] - poff[idx[j]]);
        buf.resize(spoff[n] ? spoff[n] : 1);
        sal.resize(n);
        for (size_t j = 0; j < n; j++) { memcpy(buf.data() + spoff[j], proofs + poff[idx[j]], spoff[j + 1] - spoff[j]); sal[j] = alphas[idx[j]]; }
        pr = buf.data(); po = spoff.data(); al = sal.data();
    };
    bool first = true;
    auto enter = [&](const uint32_t* idx, size_t n) {   // every pass but the first starts its members from their entry state
        if (first) { first = false; return; }
        const double t0 = now_s();
        restore(idx, n);
        snap_s += now_s() - t0;
    };
    const LocatePlanner::RunFn run = [&](size_t lo, size_t n, LocateOutcome& out) -> int {
        const double t0 = now_s();
        const bool was_first = first;
        const uint32_t* idx = plan.survivors().data() + lo;
        enter(idx, n);
        const uint8_t* pr; const size_t* po; const F4* al;
        gather(idx, n, pr, po, al);
        VfyProvider<C> prov;
        sub(idx, n, prov);
        std::vector<int> st(n, BP_OK);
        const int rc = batch_verify_core<C>(ctx, n, prov, pr, po, al, nullptr, nullptr, st.data());
        ctx->vl_passes++; ctx->vl_instances += n;
        (was_first ? t_first : t_later) += now_s() - t0;
        for (size_t j = 0; j < n; j++) if (st[j]) out.before.emplace_back(j, st[j]);
        if (!out.before.empty()) { out.kind = LocateOutcome::FAILED_BEFORE; return BP_OK; }
        if (rc == BP_OK) { out.kind = LocateOutcome::PASSED; return BP_OK; }
        if (rc == BP_E_VERIFICATION) { out.kind = LocateOutcome::FAILED_CHECK; return BP_OK; }
        return rc;   // (a HIP error, two structures under one digest: the call cannot go on)
    };
    // a failing range of at most BP_TUNE_VERIFY_LOCATE_LEAF members: the machinery of bp_verifier_verify_batch, a verdict for each
    const LocatePlanner::ExactFn exact = [&](size_t lo, size_t n, int* st) -> int {
        const double t0 = now_s();
        const uint32_t* idx = plan.survivors().data() + lo;
        enter(idx, n);
        const uint8_t* pr; const size_t* po; const F4* al;
        gather(idx, n, pr, po, al);
        VfyProvider<C> prov;
        sub(idx, n, prov);
        prov.dev_batch = nullptr;
        std::fill(st, st + n, BP_OK);
        const int rc = verify_each_core<C>(ctx, n, prov, pr, po, st, nullptr, nullptr);
        t_later += now_s() - t0;
        int want = BP_OK;
        for (size_t j = 0; j < n && !want; j++) want = st[j];
        return rc == want ? BP_OK : rc;   // (it returns the first status; anything else is an error of the call itself)
    };
    const int prc = plan.plan(run, exact, BP_E_VERIFICATION);
    ctx->vl_calls++; ctx->vl_exact += plan.exact_leaves();
    if (timing) { timing[0] = now_s() - t_entry + snap0; timing[1] = t_first; timing[2] = t_later; timing[3] = snap_s; }
    if (prc) return prc > 0 ? BP_E_ARG : prc;
    for (size_t k = 0; k < count; k++) if (status[k]) return status[k];
    return BP_OK;
}
// over recorded verifier handles (each consumed, like `verify(self)`)
template <class C>
static int cs_batch_verify_locate(bp_ctx* c, size_t count, bp_cs* const* vs, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* alphas, int* status,
                                  double* timing) {
    typedef host::ConstraintSystem<C> CS;
    const std::vector<size_t> poff = prefix_offsets(proof_lens, count);
    const std::vector<F4> al = cs_weights<C>(alphas, count);
    // entry states: the transcript (the host replay advances it) and what the randomized phase changes in the recorder
    const double t_snap = now_s();
    std::vector<host::Strobe> tr0(count);
    std::vector<typename CS::RandSnap> cs0(count);
    for (size_t k = 0; k < count; k++) { CS* ck = vs[k]->cs<C>(); if (ck->tr) tr0[k] = ck->tr->s; ck->snapshot(cs0[k]); }
    const double snap_s = now_s() - t_snap;
    const std::function<void(const uint32_t*, size_t)> restore = [&](const uint32_t* idx, size_t n) {
        for (size_t j = 0; j < n; j++) { CS* ck = vs[idx[j]]->cs<C>(); if (ck->tr) ck->tr->s = tr0[idx[j]]; ck->restore(cs0[idx[j]]); }
    };
    const LocateSubFn<C> sub = [&](const uint32_t* idx, size_t n, VfyProvider<C>& prov) {
        const CsView at{vs, idx};
        cs_provider<C>(c, n, at, prov);
        // a pass the device front end declines commits the members' pending commitments: from then on THAT is their entry state
        prov.prologue = [materialize = prov.prologue, at, &tr0](const uint32_t* idx, size_t cnt, int* st) -> int {
            auto member = [idx](size_t j) { return idx ? (size_t)idx[j] : j; };
            std::vector<char> had(cnt);
            for (size_t j = 0; j < cnt; j++) had[j] = !at(member(j))->wire.empty();
            BPCHK(materialize(idx, cnt, st));
            for (size_t j = 0; j < cnt; j++) if (had[j] && !st[j]) tr0[at.idx[member(j)]] = at(member(j))->tr->s;
            return BP_OK;
        };
    };
    VerifyingScope scope(vs, count);
    return locate_core<C>(c, count, sub, restore, proofs, poff.data(), al.data(), status, timing, snap_s);
}
// scenario statements: batch_verify_scenarios' sources, recorders and weights; a subset's provider goes through the index map
template <class C>
static int scenarios_batch_verify_locate(bp_ctx* c, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                         const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, const uint8_t* alpha_seed, int* status,
                                         double* timing) {
    const VfyCoreFn<C> core = [&](const VfyProvider<C>& full, const size_t* poff, const F4* alphas) -> int {
        for (size_t k = 0; k < count; k++) if (alphas[k].is_zero()) { g_err = "batch_verify_locate: a weight is zero"; return BP_E_ARG; }
        const LocateSubFn<C> sub = [&](const uint32_t* idx, size_t n, VfyProvider<C>& prov) {
            if (n == count) prov = full;   // (the lockstep heads need consecutive instances: the whole batch only)
            else provider_subset<C>(full, idx, prov);
        };
        const std::function<void(const uint32_t*, size_t)> restore = [](const uint32_t*, size_t) {};
        return locate_core<C>(c, count, sub, restore, proofs, poff, alphas, status, timing, 0.0);
    };
    return batch_verify_scenarios<C>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, alpha_seed, nullptr, 0, nullptr, &core);
}

int bp_r1cs_batch_verify_locate(bp_ctx* c, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* alphas, int* status,
                                double* timing) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!verifiers || !proofs || !proof_lens || !status) return BP_E_ARG;
    if (count > 1 && !alphas) { g_err = "batch_verify_locate: per-instance weights (alphas) are required for more than one instance"; return BP_E_ARG; }
    if (alphas) for (size_t k = 0; k < count; k++) {   // (zero is zero in Montgomery form too)
        if (!(alphas[4 * k] | alphas[4 * k + 1] | alphas[4 * k + 2] | alphas[4 * k + 3])) { g_err = "batch_verify_locate: a zero weight hides its instance from every sum"; return BP_E_ARG; }
    }
    BPCHK(verifiers_check("batch_verify_locate", c, count, verifiers));
    BPCHK(CS_DISPATCH(c, verifiers_cover_constraints<Secq>("batch_verify_locate", count, verifiers), verifiers_cover_constraints<Zorro>("batch_verify_locate", count, verifiers)));
    if (!c->gens_cap) { g_err = "batch_verify_locate: generators not installed"; return BP_E_GENS_LENGTH; }
    if (c->host_only) { g_err = "batch_verify_locate: a host-only ctx has no device to verify on"; return BP_E_NO_DEVICE; }
    BPCHK(wire_check_states("batch_verify_locate", count, verifiers));
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? cs_batch_verify_locate<Secq>(c, count, verifiers, proofs, proof_lens, alphas, status, timing)
                         : cs_batch_verify_locate<Zorro>(c, count, verifiers, proofs, proof_lens, alphas, status, timing);
}
int bp_r1cs_batch_verify_locate_scenarios(bp_ctx* c, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                          const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, const uint8_t alpha_seed[32],
                                          int* status, double* timing) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!scenarios || !params || !proofs || !proof_lens || !ms || !npubs || !status) return BP_E_ARG;
    if (count > 1 && !alpha_seed) { g_err = "batch_verify_locate: the weights' seed is required for more than one instance"; return BP_E_ARG; }
    size_t tm = 0, tp = 0;
    for (size_t k = 0; k < count; k++) { tm += ms[k]; tp += npubs[k]; }
    if ((tm && !commit_xy) || (tp && !publics)) return BP_E_ARG;
    if (!c->gens_cap) { g_err = "batch_verify_locate: generators not installed"; return BP_E_GENS_LENGTH; }
    if (c->host_only) { g_err = "batch_verify_locate: a host-only ctx has no device to verify on"; return BP_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? scenarios_batch_verify_locate<Secq>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, alpha_seed, status, timing)
                         : scenarios_batch_verify_locate<Zorro>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, alpha_seed, status, timing);
}
int bp_ctx_verify_locate_stats(bp_ctx* c, uint64_t* calls, uint64_t* passes, uint64_t* instances_in_passes, uint64_t* exact_leaves) {
    if (!c) return BP_E_ARG;
    if (calls) *calls = c->vl_calls;
    if (passes) *passes = c->vl_passes;
    if (instances_in_passes) *instances_in_passes = c->vl_instances;
    if (exact_leaves) *exact_leaves = c->vl_exact;
    return BP_OK;
}
// test hook, host only: the planner over a simulated core
int bp_debug_locate_plan(size_t count, const uint8_t* fails_check, const uint8_t* fails_before, uint32_t* npasses, uint32_t* pass_lo, uint32_t* pass_n,
                         uint8_t* pass_failed, uint64_t* instances_in_passes, int* status) {
    if (!status || (count && !fails_check) || count >= ((size_t)1 << 31)) return BP_E_ARG;
    LocatePlanner plan(count, 1, status);
    uint32_t np = 0;
    const LocatePlanner::RunFn run = [&](size_t lo, size_t n, LocateOutcome& out) -> int {
        const uint32_t* idx = plan.survivors().data() + lo;
        for (size_t j = 0; j < n; j++) if (fails_before && fails_before[idx[j]]) out.before.emplace_back(j, BP_E_FORMAT);
        if (!out.before.empty()) out.kind = LocateOutcome::FAILED_BEFORE;
        else { out.kind = LocateOutcome::PASSED; for (size_t j = 0; j < n; j++) if (fails_check[idx[j]]) out.kind = LocateOutcome::FAILED_CHECK; }
        if (pass_lo) pass_lo[np] = (uint32_t)lo;
        if (pass_n) pass_n[np] = (uint32_t)n;
        if (pass_failed) pass_failed[np] = (uint8_t)out.kind;
        np++;
        return BP_OK;
    };
    const LocatePlanner::ExactFn exact = [&](size_t lo, size_t n, int* st) -> int {   // (not reached with leaf 1 and this simulator)
        const uint32_t* idx = plan.survivors().data() + lo;
        for (size_t j = 0; j < n; j++) st[j] = fails_before && fails_before[idx[j]] ? BP_E_FORMAT : fails_check[idx[j]] ? BP_E_VERIFICATION : BP_OK;
        return BP_OK;
    };
    const int rc = plan.plan(run, exact, BP_E_VERIFICATION);
    if (npasses) *npasses = np;
    if (instances_in_passes) *instances_in_passes = plan.instances_in_passes();
    return rc ? BP_E_ARG : BP_OK;
}

// test hook: the production msm_direct on caller-chosen jobs (include/arkbp.h bp_debug_msm_direct).  Everything a job would read is
// checked here on the host — k_dt_accum itself trusts its descriptors
template <class C>
static int dbg_msm_direct(bp_ctx* ctx, size_t njobs, const uint32_t* desc, const uint64_t* imm, const uint64_t* const* scalars, const size_t* scalar_lens,
                          uint64_t* out_xy, uint32_t* workgroups) {
    typedef typename C::Fr FrP;
    hipStream_t st = ctx->stream;
    const size_t nbases = 2 + 2 * ctx->dt_cap;
    DtJobs jobs; memset(&jobs, 0, sizeof jobs);
    size_t seg_off[DT_MAXOUT][DT_MAXSEG], seg_len[DT_MAXOUT][DT_MAXSEG], total = 0;
    for (size_t j = 0; j < njobs; j++) {
        const uint32_t* d = desc + j * BP_DEBUG_DT_DESC_WORDS;
        DtJob& jb = jobs.job[j];
        if (d[0] > (uint32_t)DT_MAXSEG || d[1] > 1) { g_err = "bp_debug_msm_direct: bad segment count or immediate flag"; return BP_E_ARG; }
        jb.nseg = d[0]; jb.has_imm = d[1]; jb.imm_base = d[1] ? d[2] : 0;
        if (jb.has_imm) {
            if (!imm || jb.imm_base >= nbases) { g_err = "bp_debug_msm_direct: the immediate term's base is outside the tables"; return BP_E_ARG; }
            memcpy(jb.imm, imm + 4 * j, 32);
        }
        size_t terms = jb.has_imm;
        for (uint32_t s = 0; s < jb.nseg; s++) {
            const uint32_t* sd = d + 3 + 5 * s;
            const size_t base0 = sd[0], count = sd[1], fn = sd[3];
            if (!count || sd[2] > 2 || sd[4] > 1) { g_err = "bp_debug_msm_direct: empty segment, or bad format / fold_hi"; return BP_E_ARG; }
            // the last element term count - 1 stands for (small.cuh DtSeg::fold_n); the remapping is monotonic in the term
            const size_t last = fn ? ((count - 1) / fn) * 2 * fn + (count - 1) % fn + (sd[4] ? fn : 0) : count - 1;
            if (base0 >= nbases || last >= nbases - base0) { g_err = "bp_debug_msm_direct: a segment leaves the tables"; return BP_E_ARG; }
            if (!scalars || !scalar_lens || !scalars[j * DT_MAXSEG + s] || scalar_lens[j * DT_MAXSEG + s] <= last) {
                g_err = "bp_debug_msm_direct: a scalar array is shorter than the elements its segment visits"; return BP_E_ARG;
            }
            seg_off[j][s] = total; seg_len[j][s] = last + 1;
            total += last + 1;
            terms += count;
            jb.seg[s].base0 = (u32)base0; jb.seg[s].count = (u32)count; jb.seg[s].resident = sd[2]; jb.seg[s].fold_n = (u32)fn; jb.seg[s].fold_hi = sd[4];
        }
        if (!terms) { g_err = "bp_debug_msm_direct: a job without terms"; return BP_E_ARG; }
        jb.terms = (u32)terms;
    }
    BPCHK(ctx->io_scal.ensure(std::max<size_t>(total, 1) * 32));
    u32* d_sc = ctx->io_scal.as<u32>();
    for (size_t j = 0; j < njobs; j++) {
        for (uint32_t s = 0; s < jobs.job[j].nseg; s++) {
            DtSeg& sg = jobs.job[j].seg[s];
            u32* dst = d_sc + seg_off[j][s] * 8;
            const size_t n = seg_len[j][s];
            HIPCHK(hipMemcpyAsync(dst, scalars[j * DT_MAXSEG + s], n * 32, hipMemcpyHostToDevice, st));
            if (sg.resident == 1) hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, dst, dst, (u32)n);
            sg.sc = dst;
        }
    }
    HIPCHK(hipGetLastError());
    J4 r[DT_MAXOUT];
    A4 a[DT_MAXOUT];
    BPCHK(msm_direct<C>(ctx, jobs, (int)njobs, r));
    if (workgroups) *workgroups = ctx->dt_last_nblk;
    to_aff_many<C>(r, njobs, a);
    for (size_t j = 0; j < njobs; j++) { memcpy(out_xy + 8 * j, a[j].x.v, 32); memcpy(out_xy + 8 * j + 4, a[j].y.v, 32); }
    return BP_OK;
}

extern "C" {

int bp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int bp_ctx_create(int curve, int device, bp_ctx** out) {
    if (!out || (curve != BP_CURVE_SECQ256K1 && curve != BP_CURVE_ZORRO)) { g_err = "bp_ctx_create: bad argument"; return BP_E_ARG; }
    int n = bp_device_count();
    if (n <= 0 || device < 0 || device >= n) { g_err = "bp_ctx_create: no HIP device (the engine has no CPU fallback)"; return BP_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(device));
    bp_ctx* c = new bp_ctx();
    c->curve = curve; c->device = device;
    if (const char* v = getenv("ARKBP_VFY_DEVICE")) { if (*v >= '0' && *v <= '2' && !v[1]) c->tune_vfy_device = *v - '0'; }   // the default of BP_TUNE_VFY_DEVICE
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; g_err = hipGetErrorString(e); return BP_E_HIP; }
    *out = c;
    return BP_OK;
}
void bp_ctx_destroy(bp_ctx* c) {
    if (!c) return;
    g_dry = c->host_only;
    c->pool.reset();             // (the pool's threads end before the buffers they may have touched go away)
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    collect_timers(c);
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->sync_ev) (void)hipEventDestroy(c->sync_ev);
    if (c->sync_ev_aux) (void)hipEventDestroy(c->sync_ev_aux);
    DevBuf* bufs[] = {&c->fs_over, &c->canon, &c->hist, &c->lvl_off, &c->totals, &c->cursor, &c->entries, &c->slots, &c->bin_cur, &c->boff, &c->lvA, &c->lvB, &c->Tbuf, &c->io_pts, &c->io_scal, &c->io_out,
                      &c->ipa_G, &c->ipa_H, &c->ipa_a, &c->ipa_b, &c->ipa_Gf, &c->ipa_Hf, &c->ipa_sL, &c->ipa_sR, &c->ipa_part, &c->ipa_Q, &c->ipa_jac, &c->ipa_pref, &c->ipa_cG, &c->ipa_cH,
                      &c->d_G, &c->d_H, &c->d_pc, &c->pc_table, &c->r_aL, &c->r_aR, &c->r_aO, &c->r_sL, &c->r_sR, &c->r_wL, &c->r_wR, &c->r_wO, &c->r_msmsc,
                      &c->r_ypow, &c->r_part, &c->r_small, &c->r_g, &c->r_h, &c->r_chal, &c->r_tail, &c->v_params, &c->v_gpart, &c->v_hpart, &c->v_alpha, &c->v_tables, &c->v_dec, &c->ve_arena, &c->cyc_a, &c->cyc_b, &c->cyc_Gf, &c->cyc_Hf, &c->ftab_G, &c->ftab_H, &c->fb_G, &c->fb_H, &c->fb_pc, &c->p_moff, &c->p_ment, &c->p_mc, &c->p_coefs, &c->p_ztab, &c->fs_bcnt, &c->fs_loff, &c->fs_binch, &c->fs_sums};
    c->templates.clear();
    c->vfe_classes.clear();
    c->pl_cache.clear();
    c->pl_ztab.release();
    for (auto b : bufs) b->release();
    DevBuf* vbufs[] = {&c->vfe_in, &c->vfe_msg, &c->vfe_chal, &c->vfe_ws, &c->vfe_small, &c->vfe_flags, &c->vfe2_sched, &c->vfe2_voff, &c->vfe2_vq, &c->vfe2_vcid, &c->vfe2_gch, &c->vfe2_coef};
    for (auto b : vbufs) b->release();
    if (c->h_vfe) (void)hipHostFree(c->h_vfe);
    if (c->h_vfe2) (void)hipHostFree(c->h_vfe2);
    c->dt_tab.release(); c->dt_part.release(); c->pc_dt.release(); c->dt_a2.release(); c->dt_b2.release(); c->dt_ticket.release();
    c->pb_arena.release();
    c->pf_aux.release();
    c->wc_dev.release();
    if (c->h_wc) (void)hipHostFree(c->h_wc);
    c->wd_res.release();
    if (c->h_wd) (void)hipHostFree(c->h_wd);
    if (c->h_pf) (void)hipHostFree(c->h_pf);
    if (c->h_pb) (void)hipHostFree(c->h_pb);
    if (c->h_dt) (void)hipHostFree(c->h_dt);
    if (c->h_totals) (void)hipHostFree(c->h_totals);
    if (c->h_T) (void)hipHostFree(c->h_T);
    for (int i = 0; i < 2; i++) { if (c->h_vstage[i]) (void)hipHostFree(c->h_vstage[i]); if (c->vstage_ev[i]) (void)hipEventDestroy(c->vstage_ev[i]); if (c->vtail_ev[i]) (void)hipEventDestroy(c->vtail_ev[i]); if (c->dec_ev[i]) (void)hipEventDestroy(c->dec_ev[i]); }
    for (int i = 0; i < 2; i++) if (c->h_vaux[i]) (void)hipHostFree(c->h_vaux[i]);
    if (c->h_upload) (void)hipHostFree(c->h_upload);
    if (c->h_csc) (void)hipHostFree(c->h_csc);
    if (c->h_dec) (void)hipHostFree(c->h_dec);
    if (c->aux_stream) { (void)hipStreamSynchronize(c->aux_stream); (void)hipStreamDestroy(c->aux_stream); }
    if (c->nccl) { (void)rccl_api().CommDestroy(c->nccl); c->nccl = nullptr; }
    c->coll_send.release(); c->coll_recv.release();
    if (c->h_coll) (void)hipHostFree(c->h_coll);
    (void)hipStreamDestroy(c->stream);
    delete c;
    g_dry = false;
}
int bp_debug_ctx_create_hostonly(int curve, size_t gens_capacity, bp_ctx** out) {
    if (!out || (curve != BP_CURVE_SECQ256K1 && curve != BP_CURVE_ZORRO)) return BP_E_ARG;
    bp_ctx* c = new bp_ctx();
    c->curve = curve; c->device = -1; c->host_only = true; c->gens_cap = gens_capacity;
    c->stream = (hipStream_t)&dry::g_token;
    *out = c;
    return BP_OK;
}
int bp_ctx_set_window_shard(bp_ctx* c, int rank, int world, bp_point_reduce_cb cb, void* user) {
    if (!c || world < 1 || rank < 0 || rank >= world || (world > 1 && !cb)) return BP_E_ARG;
    c->shard_rank = rank; c->shard_world = world; c->shard_cb = cb; c->shard_user = user;
    return BP_OK;
}
int bp_rccl_unique_id(uint8_t out[128]) {
    if (!out) return BP_E_ARG;
    RcclApi& api = rccl_api();
    if (!api.ok) { g_err = "RCCL unavailable: " + api.why; return BP_E_HIP; }
    ncclUniqueId id;
    const ncclResult_t r = api.GetUniqueId(&id);
    if (r != ncclSuccess) { g_err = std::string("ncclGetUniqueId: ") + api.GetErrorString(r); return BP_E_HIP; }
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(out, &id, 128);
    return BP_OK;
}
int bp_ctx_rccl_init(bp_ctx* c, const uint8_t unique_id[128], int rank, int world) {
    if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return BP_E_ARG;
    RcclApi& api = rccl_api();
    if (!api.ok) { g_err = "RCCL unavailable: " + api.why; return BP_E_HIP; }
    HIPCHK(hipSetDevice(c->device));
    if (c->nccl) { (void)api.CommDestroy(c->nccl); c->nccl = nullptr; }
    ncclUniqueId id; memcpy(&id, unique_id, 128);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = api.CommInitRank(&comm, world, id, rank);
    if (r != ncclSuccess) { g_err = std::string("ncclCommInitRank: ") + api.GetErrorString(r); return BP_E_HIP; }
    c->nccl = comm;
    c->shard_rank = rank; c->shard_world = world;
    c->shard_cb = nullptr; c->shard_user = nullptr; c->gather_cb = nullptr; c->gather_user = nullptr;
    c->coll_count = 0; c->coll_seconds = 0;
    return BP_OK;
}
int bp_ctx_rccl_shutdown(bp_ctx* c) {
    if (!c) return BP_E_ARG;
    if (c->nccl) { HIPCHK(hipSetDevice(c->device)); HIPCHK(ctx_stream_wait(c)); (void)rccl_api().CommDestroy(c->nccl); c->nccl = nullptr; }
    c->shard_rank = 0; c->shard_world = 1;
    return BP_OK;
}
int bp_ctx_collective_stats(bp_ctx* c, uint64_t* count, double* seconds) {
    if (!c) return BP_E_ARG;
    if (count) *count = c->coll_count;
    if (seconds) *seconds = c->coll_seconds;
    return BP_OK;
}
int bp_debug_rccl_allgather(bp_ctx* c, const uint8_t* send, size_t bytes, uint8_t* recv) {
    if (!c || !send || !recv || !bytes) return BP_E_ARG;
    if (!c->nccl) { g_err = "no RCCL communicator on this ctx (bp_ctx_rccl_init)"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return ctx_native_allgather(c, send, bytes, recv);
}
int bp_ctx_set_shard_allgather(bp_ctx* c, bp_allgather_cb cb, void* user) {
    if (!c) return BP_E_ARG;
    c->gather_cb = cb; c->gather_user = user;
    return BP_OK;
}
int bp_ctx_set_tuning(bp_ctx* c, int knob, uint64_t value) {
    if (!c) return BP_E_ARG;
    switch (knob) {
        case BP_TUNE_CYCLIC_MIN: c->tune_cyclic_min = (size_t)value; return BP_OK;
        case BP_TUNE_MSM_FIXED_MIN: c->tune_msm_fixed_min = (size_t)value; return BP_OK;
        case BP_TUNE_HOST_THREADS: if (value > 256) return BP_E_ARG; c->tune_host_threads = (size_t)value; c->pool.reset(); return BP_OK;
        case BP_TUNE_FOLD_BATCH_MIN: c->tune_fold_batch_min = (size_t)value; return BP_OK;
        case BP_TUNE_MSM_BIN_MIN: c->tune_msm_bin_min = (size_t)value; return BP_OK;
        case BP_TUNE_IPA_FREEZE_LEN: c->tune_ipa_freeze_len = (size_t)value; return BP_OK;
        case BP_TUNE_MSM_WSUM_MIN: c->tune_msm_wsum_min = (size_t)value; return BP_OK;
        case BP_TUNE_MSM_GLV_MIN: c->tune_msm_glv_min = (size_t)value; return BP_OK;
        case BP_TUNE_FOLD_QUAD_MAX: c->tune_fold_quad_max = (size_t)value; return BP_OK;
        case BP_TUNE_WAIT_SLEEP: if (value > 1000) return BP_E_ARG; c->tune_wait_sleep = value == 1 ? 30u : (unsigned)value; return BP_OK;
        case BP_TUNE_MSM_CHUNK_CAP: if (value && (value < 8 || value > 64)) return BP_E_ARG; c->tune_msm_chunk_cap = (size_t)value; return BP_OK;
        case BP_TUNE_VFY_DEVICE: c->tune_vfy_device = value >= 2 ? 2 : (int)value; return BP_OK;
        case BP_TUNE_PROVE_BATCH: if (value > 65535) return BP_E_ARG; c->tune_prove_batch = (size_t)value; return BP_OK;
        case BP_TUNE_VERIFY_EACH: c->tune_verify_each = (size_t)std::min<uint64_t>(value, 4096); return BP_OK;
        case BP_TUNE_PROVE_BATCH_FRONT: if (value > 1) return BP_E_ARG; c->tune_pb_front = (int)value; return BP_OK;
        case BP_TUNE_DIRECT_MAX: if (value > ((uint64_t)1 << 16)) return BP_E_ARG; c->tune_direct_max = (size_t)value; return BP_OK;
        case BP_TUNE_MSM_BATCH_SHORT: c->tune_msb_short = value; return BP_OK;   // (the four take every value: 0 = the default)
        case BP_TUNE_MSM_BATCH_MIN_JOBS: c->tune_msb_min_jobs = value; return BP_OK;
        case BP_TUNE_MSM_BATCH_SLICE: c->tune_msb_slice = value; return BP_OK;
        case BP_TUNE_MSM_BATCH_MAX: c->tune_msb_max = value; return BP_OK;
        case BP_TUNE_MSM_PAIR: if (value > 1) return BP_E_ARG; c->tune_msm_pair = (int)value; return BP_OK;
        case BP_TUNE_VERIFY_LOCATE_LEAF: if (value > 4096) return BP_E_ARG; c->tune_verify_locate_leaf = (size_t)value; return BP_OK;
        case BP_TUNE_VFY_CLASS_MIN: c->tune_vfy_class_min = std::min<uint64_t>(value, 65535); return BP_OK;
    }
    return BP_E_ARG;
}
int bp_ctx_sync(bp_ctx* c) {
    if (!c) return BP_E_ARG;
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}

int bp_dev_alloc(bp_ctx* c, size_t bytes, void** dptr) {
    if (!c || !dptr) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMalloc(dptr, bytes ? bytes : 1));
    return BP_OK;
}
int bp_dev_free(bp_ctx* c, void* dptr) {
    if (!c) return BP_E_ARG;
    HIPCHK(ctx_stream_wait(c));
    HIPCHK(hipFree(dptr));
    return BP_OK;
}
int bp_dev_upload(bp_ctx* c, void* dptr, const void* hostp, size_t bytes) {
    if (!c || (!dptr && bytes) || (!hostp && bytes)) return BP_E_ARG;
    HIPCHK(hipMemcpyAsync(dptr, hostp, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
int bp_dev_download(bp_ctx* c, void* hostp, const void* dptr, size_t bytes) {
    if (!c || (!dptr && bytes) || (!hostp && bytes)) return BP_E_ARG;
    HIPCHK(hipMemcpyAsync(hostp, dptr, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
int bp_points_import(bp_ctx* c, const void* d_in, void* d_out, size_t n) {
    if (!c || ((!d_in || !d_out) && n)) return BP_E_ARG;
    if (!n) return BP_OK;
    const u32 gb = (u32)((n + 255) / 256);
    if (c->curve == 0) hipLaunchKernelGGL(k_points_ark_to_dev<Secq>, dim3(gb), dim3(256), 0, c->stream, (const u32*)d_in, (u32*)d_out, (u32)n);
    else hipLaunchKernelGGL(k_points_ark_to_dev<Zorro>, dim3(gb), dim3(256), 0, c->stream, (const u32*)d_in, (u32*)d_out, (u32)n);
    HIPCHK(hipGetLastError());
    return BP_OK;
}
int bp_points_export(bp_ctx* c, const void* d_in, void* d_out, size_t n) {
    if (!c || ((!d_in || !d_out) && n)) return BP_E_ARG;
    if (!n) return BP_OK;
    const u32 gb = (u32)((n + 255) / 256);
    if (c->curve == 0) hipLaunchKernelGGL(k_points_dev_to_ark<Secq>, dim3(gb), dim3(256), 0, c->stream, (const u32*)d_in, (u32*)d_out, (u32)n);
    else hipLaunchKernelGGL(k_points_dev_to_ark<Zorro>, dim3(gb), dim3(256), 0, c->stream, (const u32*)d_in, (u32*)d_out, (u32)n);
    HIPCHK(hipGetLastError());
    return BP_OK;
}

int bp_msm_dev(bp_ctx* c, const void* d_bases, const void* d_scalars, size_t n, int canonical, uint64_t out_xy[8]) {
    if (!c || !out_xy || ((!d_bases || !d_scalars) && n)) { g_err = "bp_msm_dev: bad argument"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_dev_entry<Secq>(c, d_bases, d_scalars, n, canonical, out_xy) : msm_dev_entry<Zorro>(c, d_bases, d_scalars, n, canonical, out_xy);
}
int bp_debug_msm_pair(bp_ctx* c, const void* const* base_ptrs, const size_t* base_counts, const void* const* d_scalars, size_t n, int canonical, int latency_first,
                      uint64_t* out_xy) {
    if (!c || !base_ptrs || !base_counts || !d_scalars || !d_scalars[0] || !d_scalars[1] || !out_xy || n == 0 || n >= ((size_t)1 << 31)) { g_err = "bp_debug_msm_pair: bad argument"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_msm_pair<Secq>(c, base_ptrs, base_counts, d_scalars, n, canonical, latency_first, out_xy)
                         : dbg_msm_pair<Zorro>(c, base_ptrs, base_counts, d_scalars, n, canonical, latency_first, out_xy);
}
int bp_msm_gens(bp_ctx* c, int use_G, int use_H, size_t off, size_t n, const uint64_t* extra_bases_xy, size_t n_extra, const uint64_t* scalars,
                int canonical, uint64_t out_xy[8]) {
    if (!c || !out_xy || (n_extra && !extra_bases_xy)) { g_err = "bp_msm_gens: bad argument"; return BP_E_ARG; }
    const size_t total = (use_G ? n : 0) + (use_H ? n : 0) + n_extra;
    if (total && !scalars) { g_err = "bp_msm_gens: bad argument"; return BP_E_ARG; }
    if ((use_G || use_H) && n && off + n > c->gens_cap) { g_err = "bp_msm_gens: range exceeds the installed generator tables"; return BP_E_GENS_LENGTH; }
    if (total >= ((size_t)1 << 31)) { g_err = "bp_msm_gens: too many terms"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_gens_entry<Secq>(c, use_G, use_H, off, n, extra_bases_xy, n_extra, scalars, canonical, out_xy)
                         : msm_gens_entry<Zorro>(c, use_G, use_H, off, n, extra_bases_xy, n_extra, scalars, canonical, out_xy);
}
int bp_msm_window_count(int curve, size_t n, int* windows, int* window_bits) {
    if ((curve != 0 && curve != 1) || !windows) return BP_E_ARG;
    MsmPlan pl = msm_plan(n ? n : 1, curve == 0 ? Secq::Fr::BITS : Zorro::Fr::BITS, msm_knobs(nullptr));
    *windows = pl.W;
    if (window_bits) *window_bits = pl.c;
    return BP_OK;
}
int bp_msm_dev_windows(bp_ctx* c, const void* d_bases, const void* d_scalars, size_t n, int canonical, int w_lo, int w_hi, uint64_t out_xy[8]) {
    if (!c || !out_xy || ((!d_bases || !d_scalars) && n) || w_lo < 0 || w_hi < w_lo) { g_err = "bp_msm_dev_windows: bad argument"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_dev_entry<Secq>(c, d_bases, d_scalars, n, canonical, out_xy, w_lo, w_hi)
                         : msm_dev_entry<Zorro>(c, d_bases, d_scalars, n, canonical, out_xy, w_lo, w_hi);
}
int bp_msm(bp_ctx* c, const uint64_t* bases_xy, const uint64_t* scalars, size_t n, int canonical, uint64_t out_xy[8]) {
    if (!c || !out_xy || ((!bases_xy || !scalars) && n)) { g_err = "bp_msm: bad argument"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    if (n == 0) { memset(out_xy, 0, 64); return BP_OK; }
    BPCHK(c->io_pts.ensure(n * 64));
    BPCHK(c->io_scal.ensure(n * 32));
    HIPCHK(hipMemcpyAsync(c->io_pts.p, bases_xy, n * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->io_scal.p, scalars, n * 32, hipMemcpyHostToDevice, c->stream));
    BPCHK(bp_points_import(c, c->io_pts.p, c->io_pts.p, n));
    return bp_msm_dev(c, c->io_pts.p, c->io_scal.p, n, canonical, out_xy);
}


int bp_ipa_create(bp_ctx* c, const uint64_t Q_xy[8], const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t* G_xy, const uint64_t* H_xy,
                  const uint64_t* a, const uint64_t* b, size_t n, bp_challenge_cb cb, void* user, uint64_t* L_out_xy, uint64_t* R_out_xy, uint64_t a_out[4],
                  uint64_t b_out[4]) {
    if (!c || !Q_xy || !G_factors || !H_factors || !G_xy || !H_xy || !a || !b || !cb || !a_out || !b_out || (n > 1 && (!L_out_xy || !R_out_xy))) {
        g_err = "bp_ipa_create: bad argument"; return BP_E_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    ChallengeFn fn = [cb, user](const uint64_t* L, const uint64_t* R, uint64_t* u) { return cb(user, L, R, u); };
    return c->curve == 0 ? ipa_create_host_entry<Secq>(c, Q_xy, G_factors, H_factors, G_xy, H_xy, a, b, n, fn, L_out_xy, R_out_xy, a_out, b_out)
                         : ipa_create_host_entry<Zorro>(c, Q_xy, G_factors, H_factors, G_xy, H_xy, a, b, n, fn, L_out_xy, R_out_xy, a_out, b_out);
}

int bp_ipa_begin(bp_ctx* c, const uint64_t Q_xy[8], const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t* G_xy, const uint64_t* H_xy,
                 const uint64_t* a, const uint64_t* b, size_t n) {
    if (!c || !Q_xy || !G_factors || !H_factors || !G_xy || !H_xy || !a || !b) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? ipa_begin_host_entry<Secq>(c, Q_xy, G_factors, H_factors, G_xy, H_xy, a, b, n)
                         : ipa_begin_host_entry<Zorro>(c, Q_xy, G_factors, H_factors, G_xy, H_xy, a, b, n);
}
int bp_ipa_round_LR(bp_ctx* c, uint64_t L_xy[8], uint64_t R_xy[8]) {
    if (!c || !L_xy || !R_xy) return BP_E_ARG;
    if (!c->ipa_step_active) { g_err = "bp_ipa_round_LR: no bp_ipa_begin"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? ipa_round_lr<Secq>(c, c->ipa_step, L_xy, R_xy) : ipa_round_lr<Zorro>(c, c->ipa_step, L_xy, R_xy);
}
int bp_ipa_round_fold(bp_ctx* c, const uint64_t u[4]) {
    if (!c || !u) return BP_E_ARG;
    if (!c->ipa_step_active) { g_err = "bp_ipa_round_fold: no bp_ipa_begin"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? ipa_round_fold<Secq>(c, c->ipa_step, u) : ipa_round_fold<Zorro>(c, c->ipa_step, u);
}
int bp_ipa_finish(bp_ctx* c, uint64_t a[4], uint64_t b[4]) {
    if (!c || !a || !b) return BP_E_ARG;
    if (!c->ipa_step_active) { g_err = "bp_ipa_finish: no bp_ipa_begin"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    int rc = c->curve == 0 ? ipa_finish_dev<Secq>(c, c->ipa_step, a, b) : ipa_finish_dev<Zorro>(c, c->ipa_step, a, b);
    if (rc == BP_OK) c->ipa_step_active = false;
    return rc;
}
int bp_ipa_export(bp_ctx* c, uint64_t* a, uint64_t* b, uint64_t* G_xy, uint64_t* H_xy, uint64_t gamma_G[4], uint64_t gamma_H[4], size_t* n_cur) {
    if (!c || !a || !b || !G_xy || !H_xy || !gamma_G || !gamma_H || !n_cur) return BP_E_ARG;
    if (!c->ipa_step_active) { g_err = "bp_ipa_export: no bp_ipa_begin"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? ipa_export_host<Secq>(c, a, b, G_xy, H_xy, gamma_G, gamma_H, n_cur) : ipa_export_host<Zorro>(c, a, b, G_xy, H_xy, gamma_G, gamma_H, n_cur);
}

// ---- generators -------------------------------------------------------------------------------------
int bp_gens_derive(bp_ctx* c, size_t cap) {
    if (!c || !cap) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? gens_derive<Secq>(c, cap) : gens_derive<Zorro>(c, cap);
}
int bp_gens_upload(bp_ctx* c, const uint64_t* G_xy, const uint64_t* H_xy, size_t cap) {
    if (!c || !G_xy || !H_xy || !cap) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? gens_install<Secq>(c, G_xy, H_xy, cap) : gens_install<Zorro>(c, G_xy, H_xy, cap);
}
int bp_gens_msm_tables(bp_ctx* c, size_t count, size_t* bytes_out) {
    if (!c) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (count == 0) { if (c->fb_G.owned) { c->fb_G.release(); c->fb_H.release(); c->fb_pc.release(); } c->fb_cap = 0; return BP_OK; }
    const int rc = c->curve == 0 ? fb_tables_build<Secq>(c, count) : fb_tables_build<Zorro>(c, count);
    if (rc) return rc;
    if (bytes_out) *bytes_out = 2 * (size_t)FB_ROWS * count * 64;
    return BP_OK;
}
int bp_gens_direct_tables(bp_ctx* c, size_t count, size_t* bytes_out) {
    if (!c) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (bytes_out) *bytes_out = 0;
    if (count == 0) { if (c->dt_tab.owned) c->dt_tab.release(); else { c->dt_tab.p = nullptr; c->dt_tab.cap = 0; c->dt_tab.owned = true; } c->dt_cap = 0; return BP_OK; }
    if (!c->gens_cap) { g_err = "direct tables: no generators installed"; return BP_E_GENS_LENGTH; }
    if (c->shard_world > 1 || !c->tune_direct_max) { g_err = "direct tables: the small-statement path is off on this ctx (sharded, or BP_TUNE_DIRECT_MAX = 0)"; return BP_E_ARG; }
    const size_t want = std::min(std::min(count, c->gens_cap), c->tune_direct_max);
    // dt_ensure builds for min(generators, BP_TUNE_DIRECT_MAX): narrow the knob for the build so that `count` is what is built
    const size_t keep = c->tune_direct_max;
    c->tune_direct_max = want;
    if (c->dt_cap != want) c->dt_cap = 0;
    bool ready = false;
    const int rc = c->curve == 0 ? dt_ensure<Secq>(c, want, ready) : dt_ensure<Zorro>(c, want, ready);
    c->tune_direct_max = keep;
    if (rc) return rc;
    if (bytes_out) *bytes_out = (2 + 2 * c->dt_cap) * DT_BASE_BYTES;
    return BP_OK;
}
int bp_gens_fold_tables(bp_ctx* c, size_t count, int window_bits, size_t budget_bytes, int* window_bits_out, size_t* bytes_out) {
    if (!c || window_bits < 0 || window_bits == 1 || window_bits > 8) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (count == 0) { if (c->ftab_G.owned) { c->ftab_G.release(); c->ftab_H.release(); } c->ftab_n = 0; c->ftab_first = 0; c->ftab_stride = 1; return BP_OK; }
    const int rc = c->curve == 0 ? ftab_build<Secq>(c, count, window_bits, budget_bytes) : ftab_build<Zorro>(c, count, window_bits, budget_bytes);
    if (rc) return rc;
    if (window_bits_out) *window_bits_out = c->ftab_w;
    if (bytes_out) *bytes_out = 2 * (size_t)c->ftab_nwin * ((size_t)1 << (c->ftab_w - 1)) * c->ftab_n * 64;
    return BP_OK;
}
int bp_gens_fold_tables_slice(bp_ctx* c, size_t count, int window_bits, size_t budget_bytes, int rank, int world, int* window_bits_out, size_t* bytes_out) {
    if (!c || window_bits < 0 || window_bits == 1 || window_bits > 8 || world < 1 || rank < 0 || rank >= world || count == 0 || count % (size_t)world) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    const size_t cols = count / (size_t)world;
    const int rc = c->curve == 0 ? ftab_build<Secq>(c, cols, window_bits, budget_bytes, (u32)rank, (u32)world) : ftab_build<Zorro>(c, cols, window_bits, budget_bytes, (u32)rank, (u32)world);
    if (rc) return rc;
    if (window_bits_out) *window_bits_out = c->ftab_w;
    if (bytes_out) *bytes_out = 2 * (size_t)c->ftab_nwin * ((size_t)1 << (c->ftab_w - 1)) * c->ftab_n * 64;
    return BP_OK;
}
int bp_gens_tables_check(bp_ctx* c, uint64_t* bad_fold_entries, uint64_t* bad_msm_rows) {
    if (!c) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (!c->gens_cap) { g_err = "tables_check: generators not installed"; return BP_E_GENS_LENGTH; }
    return c->curve == 0 ? tables_check<Secq>(c, bad_fold_entries, bad_msm_rows) : tables_check<Zorro>(c, bad_fold_entries, bad_msm_rows);
}
int bp_gens_direct_tables_check(bp_ctx* c, uint64_t bad[BP_TABLES_KINDS], uint64_t first_bad[BP_TABLES_KINDS], uint64_t checked[BP_TABLES_KINDS]) {
    if (!c) { g_err = "bp_gens_direct_tables_check: null ctx"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? direct_tables_check<Secq>(c, bad, first_bad, checked) : direct_tables_check<Zorro>(c, bad, first_bad, checked);
}
int bp_gens_check(bp_ctx* c, bp_gens_report* out) {
    if (!c || !out) { g_err = "bp_gens_check: null ctx or report"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    if (!c->gens_cap) { g_err = "bp_gens_check: generators not installed"; return BP_E_GENS_LENGTH; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? gens_check<Secq>(c, out) : gens_check<Zorro>(c, out);
}
int bp_gens_digest(bp_ctx* c, size_t n, uint8_t out[128]) {
    if (!c || !out) { g_err = "bp_gens_digest: null ctx or output"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    if (!n) { g_err = "bp_gens_digest: n must be at least 1"; return BP_E_ARG; }
    if (n > c->gens_cap) { g_err = "bp_gens_digest: n exceeds the installed generators"; return BP_E_GENS_LENGTH; }
    HIPCHK(hipSetDevice(c->device));
    return gens_digest_dev(c, n, out);
}
int bp_host_gens_digest(int curve, const uint64_t* G_xy, const uint64_t* H_xy, size_t n, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8], uint8_t out[128]) {
    if ((curve != 0 && curve != 1) || !G_xy || !H_xy || !n || !B_xy || !B_blinding_xy || !out) { g_err = "bp_host_gens_digest: bad argument"; return BP_E_ARG; }
    host::gens_digest(curve, G_xy, H_xy, n, B_xy, B_blinding_xy, out);
    return BP_OK;
}
int bp_debug_tables_ptr(bp_ctx* c, int which, void** dptr, size_t* nbytes) {
    if (!c || !dptr || !nbytes || which < 0 || which > 9) return BP_E_ARG;
    if (which >= 7) {   // the resident points themselves
        DevBuf& t = which == 7 ? c->d_pc : which == 8 ? c->d_G : c->d_H;
        const size_t size = which == 7 ? (size_t)128 : c->gens_cap * 64;
        const bool there = t.p && size && t.cap >= size;
        *dptr = there ? t.p : nullptr; *nbytes = there ? size : 0;
        return BP_OK;
    }
    if (which >= 4) {   // the direct window tables (small.cuh) and the 8-bit Pedersen tables (pedersen.cuh)
        DevBuf& t = which == 4 ? c->dt_tab : which == 5 ? c->pc_dt : c->pc_table;
        const size_t size = which == 4 ? (c->dt_cap ? (2 + 2 * c->dt_cap) * DT_BASE_BYTES : 0) : which == 5 ? (size_t)2 * DT_BASE_BYTES : PC_TABLE_BYTES;
        const bool built = t.p && size && t.cap >= size;
        *dptr = built ? t.p : nullptr; *nbytes = built ? size : 0;
        return BP_OK;
    }
    DevBuf& b = which == 0 ? c->ftab_G : which == 1 ? c->ftab_H : which == 2 ? c->fb_G : c->fb_H;
    const size_t used = which < 2 ? (c->ftab_n ? (size_t)c->ftab_nwin * ((size_t)1 << (c->ftab_w - 1)) * c->ftab_n * 64 : 0) : (size_t)FB_ROWS * c->fb_cap * 64;
    *dptr = used ? b.p : nullptr; *nbytes = used;
    return BP_OK;
}
int bp_debug_fold(bp_ctx* c, int route, size_t n, const uint64_t tG[4], const uint64_t tH[4], const uint64_t t2G[4], const uint64_t t2H[4], uint32_t gens_first,
                  uint32_t gens_stride, const uint64_t* G_xy, const uint64_t* H_xy, uint64_t* G_out_xy, uint64_t* H_out_xy, uint32_t* took) {
    if (!c || route < BP_DEBUG_FOLD_LADDER || route > BP_DEBUG_FOLD_TAB2 || !n || n >= ((size_t)1 << 28) || !tG || !tH || !G_out_xy || !H_out_xy || !took) {
        g_err = "bp_debug_fold: bad argument"; return BP_E_ARG;
    }
    if (route == BP_DEBUG_FOLD_TAB2 && (!t2G || !t2H)) { g_err = "bp_debug_fold: the second multipliers are missing"; return BP_E_ARG; }
    if (route <= BP_DEBUG_FOLD_LADDER_NAF && (!G_xy || !H_xy)) { g_err = "bp_debug_fold: the ladder routes fold the caller's points"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_fold<Secq>(c, route, n, tG, tH, t2G, t2H, gens_first, gens_stride, G_xy, H_xy, G_out_xy, H_out_xy, took)
                         : dbg_fold<Zorro>(c, route, n, tG, tH, t2G, t2H, gens_first, gens_stride, G_xy, H_xy, G_out_xy, H_out_xy, took);
}
int bp_debug_msm_direct(bp_ctx* c, size_t njobs, const uint32_t* desc, const uint64_t* imm, const uint64_t* const* scalars, const size_t* scalar_lens,
                        uint64_t* out_xy, uint32_t* workgroups) {
    if (!c || !desc || !out_xy || njobs < 1 || njobs > (size_t)DT_MAXOUT) { g_err = "bp_debug_msm_direct: bad argument"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    if (!c->dt_cap || !c->dt_tab.p) { g_err = "bp_debug_msm_direct: the direct tables are not built (bp_gens_direct_tables)"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_msm_direct<Secq>(c, njobs, desc, imm, scalars, scalar_lens, out_xy, workgroups)
                         : dbg_msm_direct<Zorro>(c, njobs, desc, imm, scalars, scalar_lens, out_xy, workgroups);
}
int bp_gens_download(bp_ctx* c, uint64_t* G_xy, uint64_t* H_xy, size_t n) {
    if (!c || !G_xy || !H_xy || n > c->gens_cap) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    BPCHK(c->io_pts.ensure(n * 64));
    for (int k = 0; k < 2; k++) {
        BPCHK(bp_points_export(c, k ? c->d_H.p : c->d_G.p, c->io_pts.p, n));
        HIPCHK(hipMemcpyAsync(k ? H_xy : G_xy, c->io_pts.p, n * 64, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(ctx_stream_wait(c));
    }
    return BP_OK;
}
int bp_pedersen_gens(int curve, uint64_t B_xy[8], uint64_t B_blinding_xy[8]) {
    if (!B_xy || !B_blinding_xy) return BP_E_ARG;
    A4 B, Bb;
    if (curve == 0) { auto g = host::PedersenGens<Secq>::make_default(); B = g.B; Bb = g.B_blinding; }
    else if (curve == 1) { auto g = host::PedersenGens<Zorro>::make_default(); B = g.B; Bb = g.B_blinding; }
    else return BP_E_ARG;
    memcpy(B_xy, B.x.v, 32); memcpy(B_xy + 4, B.y.v, 32); memcpy(B_blinding_xy, Bb.x.v, 32); memcpy(B_blinding_xy + 4, Bb.y.v, 32);
    return BP_OK;
}
int bp_pedersen_gens_install(bp_ctx* c, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8]) {
    if (!c) { g_err = "bp_pedersen_gens_install: null ctx"; return BP_E_ARG; }
    if (!B_xy != !B_blinding_xy) { g_err = "bp_pedersen_gens_install: both points, or neither for PedersenGens::default()"; return BP_E_ARG; }
    if (c->host_only) return BP_E_NO_DEVICE;
    if (c->d_pc.p && !c->d_pc.owned) { g_err = "bp_pedersen_gens_install: this ctx holds another ctx's generators (bp_gens_share): install on the owner"; return BP_E_ARG; }
    A4 B, Bb;
    if (B_xy) {
        const bool ok = c->curve == 0 ? pc_point_ok<Secq>(B_xy, B) && pc_point_ok<Secq>(B_blinding_xy, Bb) : pc_point_ok<Zorro>(B_xy, B) && pc_point_ok<Zorro>(B_blinding_xy, Bb);
        if (!ok) { g_err = "bp_pedersen_gens_install: B and B_blinding must be points of the curve other than the identity, coordinates below p"; return BP_E_ARG; }
    }
    HIPCHK(hipSetDevice(c->device));
    const int rc = c->curve == 0 ? pedersen_install<Secq>(c, B_xy ? &B : nullptr, &Bb) : pedersen_install<Zorro>(c, B_xy ? &B : nullptr, &Bb);
    if (rc) return rc;
    A4 dB, dBb;
    if (c->curve == 0) { const auto& d = host::PedersenGens<Secq>::default_ref(); dB = d.B; dBb = d.B_blinding; }
    else { const auto& d = host::PedersenGens<Zorro>::default_ref(); dB = d.B; dBb = d.B_blinding; }
    c->pc_custom = !(c->pc_B == dB && c->pc_Bb == dBb);
    return BP_OK;
}
int bp_ctx_pedersen_gens(bp_ctx* c, uint64_t B_xy[8], uint64_t B_blinding_xy[8], int* is_default) {
    if (!c) { g_err = "bp_ctx_pedersen_gens: null ctx"; return BP_E_ARG; }
    A4 B, Bb;
    if (c->curve == 0) { host::PedersenGens<Secq> pc; pc_pair<Secq>(c, pc); B = pc.B; Bb = pc.B_blinding; }
    else { host::PedersenGens<Zorro> pc; pc_pair<Zorro>(c, pc); B = pc.B; Bb = pc.B_blinding; }
    if (B_xy) { memcpy(B_xy, B.x.v, 32); memcpy(B_xy + 4, B.y.v, 32); }
    if (B_blinding_xy) { memcpy(B_blinding_xy, Bb.x.v, 32); memcpy(B_blinding_xy + 4, Bb.y.v, 32); }
    if (is_default) *is_default = c->pc_custom ? 0 : 1;
    return BP_OK;
}
int bp_host_derive_generators(int curve, int which_H, uint32_t party, size_t count, uint64_t* out_xy) {
    if (!out_xy) return BP_E_ARG;
    std::vector<A4> v;
    if (curve == 0) host::derive_generators<Secq>(v, which_H ? 'H' : 'G', party, count);
    else if (curve == 1) host::derive_generators<Zorro>(v, which_H ? 'H' : 'G', party, count);
    else return BP_E_ARG;
    if (count) memcpy(out_xy, v.data(), count * 64);
    return BP_OK;
}

// ---- host transcript (the product's own merlin restatement), exposed for CPU-side tests and for shims ----
void* bp_transcript_new(const uint8_t* label, size_t n) { return new host::Transcript(label, n); }
void bp_transcript_free(void* t) { delete (host::Transcript*)t; }
void bp_transcript_append_message(void* t, const char* label, const uint8_t* m, size_t n) { ((host::Transcript*)t)->append_message(label, m, n); }
void bp_transcript_challenge_bytes(void* t, const char* label, uint8_t* out, size_t n) { ((host::Transcript*)t)->challenge_bytes(label, out, n); }
int bp_transcript_append_point(int curve, void* t, const char* label, const uint64_t xy[8]) {
    A4 p; memcpy(p.x.v, xy, 32); memcpy(p.y.v, xy + 4, 32);
    if (curve == 0) host::TP<Secq>::append_point(*(host::Transcript*)t, label, p);
    else if (curve == 1) host::TP<Zorro>::append_point(*(host::Transcript*)t, label, p);
    else return BP_E_ARG;
    return BP_OK;
}
int bp_debug_append_points_x8(int curve, void* const* transcripts, int lanes, const char* label, const uint64_t* points_xy, size_t npts) {
    if (!transcripts || lanes < 2 || lanes > 8 || !label || (npts && !points_xy) || (curve != 0 && curve != 1)) return BP_E_ARG;
#if defined(__x86_64__)
    if (!host::cpu_has_avx512()) return BP_E_ARG;
    if (curve == 0) dbg_append_points_x8<Secq>(transcripts, lanes, label, points_xy, npts); else dbg_append_points_x8<Zorro>(transcripts, lanes, label, points_xy, npts);
    return BP_OK;
#else
    return BP_E_ARG;
#endif
}
// test hook of the rest of the lockstep replay (host::StrobeX8::gather / append_message_same / challenge_bytes_each / scatter): the
// eight transcripts (any states at the same STROBE position) take `msg` under `msg_label` and then give `nbytes` (<= 64) challenge
// bytes each under `chal_label`: out = [8][nbytes].  Must equal bp_transcript_append_message + challenge bytes lane by lane.
int bp_debug_challenge_x8(void* const* transcripts, const char* msg_label, const uint8_t* msg, size_t msg_len, const char* chal_label, size_t nbytes, uint8_t* out) {
    if (!transcripts || !msg_label || !chal_label || !out || nbytes == 0 || nbytes > 64 || (msg_len && !msg)) return BP_E_ARG;
#if defined(__x86_64__)
    if (!host::cpu_has_avx512()) return BP_E_ARG;
    return dbg_challenge_x8(transcripts, msg_label, msg, msg_len, chal_label, nbytes, out);
#else
    return BP_E_ARG;
#endif
}
int bp_transcript_challenge_scalar(int curve, void* t, const char* label, uint64_t out[4]) {
    F4 r;
    if (curve == 0) r = host::TP<Secq>::challenge_scalar(*(host::Transcript*)t, label);
    else if (curve == 1) r = host::TP<Zorro>::challenge_scalar(*(host::Transcript*)t, label);
    else return BP_E_ARG;
    memcpy(out, r.v, 32);
    return BP_OK;
}
int bp_host_sha3_512(const uint8_t* m, size_t n, uint8_t out[64]) { host::sha3_512(out, m, n); return BP_OK; }
// test hook (host only): the prover's TranscriptRng (build_rng, rekey "v_blinding" per witness scalar, finalize with
// ChaCha20(seed)), then `count` Fr::rand draws.  lanes = 1: scalar path; lanes = 8: eight rngs (seeds[8][32]) advanced by the
// AVX-512 x8 stream after 3 scalar draws each, out = 8 x count scalars.  Returns BP_E_ARG when lanes = 8 is unavailable.
int bp_debug_rng_draws(int curve, void* transcript, const uint64_t* witness, size_t nw, const uint8_t* seeds, int lanes, size_t count, uint64_t* out) {
    if (!transcript || !seeds || !out || (nw && !witness)) return BP_E_ARG;
    return curve == 0 ? dbg_rng_draws<Secq>(transcript, witness, nw, seeds, lanes, count, out)
         : curve == 1 ? dbg_rng_draws<Zorro>(transcript, witness, nw, seeds, lanes, count, out) : BP_E_ARG;
}
// sum of `count` affine points on the host: the "point-reduce" after an all-gather of per-GPU partial results
int bp_host_points_sum(int curve, const uint64_t* pts_xy, size_t count, uint64_t out_xy[8]) {
    if ((!pts_xy && count) || !out_xy) return BP_E_ARG;
    A4 r;
    if (curve == 0) { J4 acc = host::Grp<Secq>::inf(); for (size_t i = 0; i < count; i++) { A4 p; memcpy(p.x.v, pts_xy + 8 * i, 32); memcpy(p.y.v, pts_xy + 8 * i + 4, 32); acc = host::Grp<Secq>::madd(acc, p); } r = host::Grp<Secq>::to_aff(acc); }
    else if (curve == 1) { J4 acc = host::Grp<Zorro>::inf(); for (size_t i = 0; i < count; i++) { A4 p; memcpy(p.x.v, pts_xy + 8 * i, 32); memcpy(p.y.v, pts_xy + 8 * i + 4, 32); acc = host::Grp<Zorro>::madd(acc, p); } r = host::Grp<Zorro>::to_aff(acc); }
    else return BP_E_ARG;
    memcpy(out_xy, r.x.v, 32); memcpy(out_xy + 4, r.y.v, 32);
    return BP_OK;
}

// ---- R1CS prove (scenario-level driver) ---------------------------------------------------------------
int bp_r1cs_prove_scenario(bp_ctx* c, int scenario, const uint64_t* params, const uint8_t seed[32], uint8_t* proof_out, size_t* proof_len,
                           uint64_t* commit_xy, size_t m_cap, size_t* m_out, uint64_t* publics, size_t* npub, double* timing) {
    if (!c || !params || !seed || !proof_out || !proof_len || !commit_xy || !m_out || !publics || !npub) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    std::vector<host::u8> bytes;
    host::StatementIO io;
    int rc = c->curve == 0 ? prove_scenario<Secq>(c, scenario, params, seed, bytes, io, timing) : prove_scenario<Zorro>(c, scenario, params, seed, bytes, io, timing);
    if (rc) return rc;
    if (bytes.size() > *proof_len || io.commitments.size() > m_cap || io.publics.size() > 8) { g_err = "prove: output buffer too small"; return BP_E_ARG; }
    memcpy(proof_out, bytes.data(), bytes.size()); *proof_len = bytes.size();
    if (!io.commitments.empty()) memcpy(commit_xy, io.commitments.data(), io.commitments.size() * 64);   // (memcpy's pointers must be valid even for 0 bytes: UBSan)
    *m_out = io.commitments.size();
    if (!io.publics.empty()) memcpy(publics, io.publics.data(), io.publics.size() * 32);
    *npub = io.publics.size();
    return BP_OK;
}

// ---- R1CS verify / batch verify (scenario-level drivers) ------------------------------------------------
int bp_r1cs_verify_scenario(bp_ctx* c, int scenario, const uint64_t* params, const uint8_t* proof, size_t proof_len, const uint64_t* commit_xy, size_t m,
                            const uint64_t* publics, size_t npub) {
    if (!c || !params || !proof || (m && !commit_xy) || (npub && !publics)) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (!c->gens_cap) { g_err = "verify: generators not installed"; return BP_E_GENS_LENGTH; }
    return c->curve == 0 ? verify_scenario<Secq>(c, scenario, params, proof, proof_len, commit_xy, m, publics, npub)
                         : verify_scenario<Zorro>(c, scenario, params, proof, proof_len, commit_xy, m, publics, npub);
}
int bp_r1cs_batch_verify_scenarios(bp_ctx* c, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                   const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, const uint8_t alpha_seed[32],
                                   double* timing, size_t alpha_skip, uint64_t* check_point_xy) {
    if (!c) return BP_E_ARG;
    if (count == 0) { if (check_point_xy) memset(check_point_xy, 0, 64); return BP_OK; }   // the reference's mega-check of nothing is the identity (verifier.rs:685-690)
    if (!scenarios || !params || !proofs || !proof_lens || !commit_xy || !ms || !npubs || !alpha_seed) return BP_E_ARG;
    g_dry = c->host_only;
    HIPCHK(hipSetDevice(c->device));
    if (!c->gens_cap) { g_err = "batch_verify: generators not installed"; g_dry = false; return BP_E_GENS_LENGTH; }
    const int rc = c->curve == 0 ? batch_verify_scenarios<Secq>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, alpha_seed, timing, alpha_skip, check_point_xy)
                                 : batch_verify_scenarios<Zorro>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, alpha_seed, timing, alpha_skip, check_point_xy);
    g_dry = false;
    return rc;
}

// ---- statements: Prover::new + commits + gadget, separated from prove() ----------------------------------
int bp_stmt_prover_create(int curve, int scenario, const uint64_t* params, const uint8_t seed[32], bp_stmt** out) {
    if (!params || !seed || !out || (curve != 0 && curve != 1)) return BP_E_ARG;
    bp_stmt* s = new bp_stmt();
    s->scenario = scenario;
    int rc = curve == 0 ? stmt_build<Secq>(s, params, seed) : stmt_build<Zorro>(s, params, seed);
    if (rc) { delete s; return rc; }
    *out = s;
    return BP_OK;
}
// as bp_stmt_prover_create, with the statement's Pedersen commitments computed on ctx's GPU in one batch
int bp_stmt_prover_create_dev(bp_ctx* c, int scenario, const uint64_t* params, const uint8_t seed[32], bp_stmt** out) {
    if (!c || !params || !seed || !out) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    bp_stmt* s = new bp_stmt();
    s->scenario = scenario;
    int rc = c->curve == 0 ? stmt_build<Secq>(s, params, seed, c) : stmt_build<Zorro>(s, params, seed, c);
    if (rc) { delete s; return rc; }
    *out = s;
    return BP_OK;
}
int bp_pedersen_commit_batch(bp_ctx* c, const uint64_t* v, const uint64_t* blind, size_t m, uint64_t* out_xy) {
    if (!c || (m && (!v || !blind || !out_xy))) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? pedersen_commit_batch<Secq>(c, v, blind, m, out_xy) : pedersen_commit_batch<Zorro>(c, v, blind, m, out_xy);
}
void bp_stmt_free(bp_stmt* s) { delete s; }
int bp_stmt_info(bp_stmt* s, uint64_t* commit_xy, size_t m_cap, size_t* m_out, uint64_t* publics, size_t* npub, size_t* multipliers, size_t* constraints) {
    if (!s || !m_out || !npub) return BP_E_ARG;
    if (s->io.commitments.size() > m_cap || s->io.publics.size() > 8) return BP_E_ARG;
    if (commit_xy && !s->io.commitments.empty()) memcpy(commit_xy, s->io.commitments.data(), s->io.commitments.size() * 64);   // (an empty vector's data() may be null: UB for memcpy even with 0 bytes — found by the UBSan build, tests/sanitize)
    if (publics && !s->io.publics.empty()) memcpy(publics, s->io.publics.data(), s->io.publics.size() * 32);
    *m_out = s->io.commitments.size(); *npub = s->io.publics.size();
    if (multipliers) *multipliers = s->num_vars();
    if (constraints) *constraints = s->num_constraints();
    return BP_OK;
}
bp_cs* bp_stmt_as_prover(bp_stmt* s) { return s; }
int bp_stmt_prove(bp_ctx* c, bp_stmt* s, uint8_t* proof_out, size_t* proof_len, double* timing) { return bp_prover_prove(c, s, nullptr, proof_out, proof_len, timing); }
int bp_stmt_precompute(bp_stmt* s) { return bp_prover_precompute(s, nullptr); }
int bp_stmt_precompute_batch(bp_stmt** stmts, size_t count) { return bp_prover_precompute_batch((bp_cs**)stmts, count); }


int bp_prover_new(int curve, void* transcript, bp_cs** out) {
    if (!transcript || !out || (curve != 0 && curve != 1)) return BP_E_ARG;
    bp_cs* h = new bp_cs();
    if (curve == 0) cs_handle_init<Secq>(h, true, (host::Transcript*)transcript); else cs_handle_init<Zorro>(h, true, (host::Transcript*)transcript);
    *out = h;
    return BP_OK;
}
int bp_prover_new_gens(int curve, void* transcript, const uint64_t B_xy[8], const uint64_t B_blinding_xy[8], bp_cs** out) {
    if (!transcript || !out || !B_xy || !B_blinding_xy || (curve != 0 && curve != 1)) { g_err = "bp_prover_new_gens: bad argument"; return BP_E_ARG; }
    A4 B, Bb;
    const bool ok = curve == 0 ? pc_point_ok<Secq>(B_xy, B) && pc_point_ok<Secq>(B_blinding_xy, Bb) : pc_point_ok<Zorro>(B_xy, B) && pc_point_ok<Zorro>(B_blinding_xy, Bb);
    if (!ok) { g_err = "bp_prover_new_gens: B and B_blinding must be points of the curve other than the identity, coordinates below p"; return BP_E_ARG; }
    const int rc = bp_prover_new(curve, transcript, out);
    if (rc) return rc;
    if (curve == 0) cs_pair_set<Secq>(*out, B, Bb); else cs_pair_set<Zorro>(*out, B, Bb);
    return BP_OK;
}
int bp_verifier_new(int curve, void* transcript, bp_cs** out) {
    if (!transcript || !out || (curve != 0 && curve != 1)) return BP_E_ARG;
    bp_cs* h = new bp_cs();
    if (curve == 0) cs_handle_init<Secq>(h, false, (host::Transcript*)transcript); else cs_handle_init<Zorro>(h, false, (host::Transcript*)transcript);
    *out = h;
    return BP_OK;
}
int bp_verifier_new_like(bp_cs* of, void* transcript, bp_cs** out) {
    if (!cs_live(of) || of->proving || !transcript || !out) { g_err = "bp_verifier_new_like: needs a live verifier handle"; return BP_E_ARG; }
    return CS_DISPATCH(of, verifier_new_like<Secq>(of, (host::Transcript*)transcript, out), verifier_new_like<Zorro>(of, (host::Transcript*)transcript, out));
}
int bp_prover_new_like(bp_cs* of, void* transcript, bp_cs** out) {
    if (!of || !of->proving || of->consumed || of->running || !transcript || !out) { g_err = "bp_prover_new_like: needs a live prover handle that is not inside prove"; return BP_E_ARG; }
    if (of->pre0.rng || of->pre1.rng) { g_err = "bp_prover_new_like: the head of prove() has run on this prover"; return BP_E_ARG; }
    if (CS_DISPATCH(of, of->cs0->phase2, of->cs1->phase2)) { g_err = "bp_prover_new_like: inside the randomized phase"; return BP_E_ARG; }
    return CS_DISPATCH(of, prover_new_like<Secq>(of, (host::Transcript*)transcript, out), prover_new_like<Zorro>(of, (host::Transcript*)transcript, out));
}
int bp_prover_assign_multipliers(bp_cs* h, const uint64_t* left, const uint64_t* right, size_t count) {
    if (!h || !h->proving || h->consumed || h->running || (count && (!left || !right))) { g_err = "assign_multipliers: needs a live like-prover and both vectors"; return BP_E_ARG; }
    if (h->pre0.rng || h->pre1.rng) { g_err = "assign_multipliers: the head of prove() has run on this prover"; return BP_E_ARG; }
    return CS_DISPATCH(h, prover_assign_multipliers<Secq>(h, left, right, count), prover_assign_multipliers<Zorro>(h, left, right, count));
}
int bp_ctx_prover_like_stats(bp_ctx* c, uint64_t* index_uploads, uint64_t* index_hits, uint64_t* resident_bytes, uint64_t* gates_on_device, uint64_t* gates_on_host) {
    if (!c) return BP_E_ARG;
    if (index_uploads) *index_uploads = c->pl_uploads;
    if (index_hits) *index_hits = c->pl_hits;
    if (resident_bytes) *resident_bytes = pl_resident_bytes(c);
    if (gates_on_device) *gates_on_device = c->pl_gates_dev;
    if (gates_on_host) *gates_on_host = c->pl_gates_host;
    return BP_OK;
}
int bp_prover_assign_multipliers_dev(bp_cs* h, bp_ctx* c, const void* d_left, const void* d_right, size_t count) {
    // the handle's rules first, those of bp_prover_assign_multipliers: the ctx is looked at only for a handle that could take a witness
    if (!h || !h->proving || h->consumed || h->running) { g_err = "assign_multipliers_dev: needs a live like-prover"; return BP_E_ARG; }
    if (h->pre0.rng || h->pre1.rng) { g_err = "assign_multipliers_dev: the head of prove() has run on this prover"; return BP_E_ARG; }
    auto fits = [&](auto* cs) { return cs->like && !cs->assigned && !cs->phase2 && cs->base && count == cs->base->num_vars; };
    if (!(h->curve == 0 ? fits(h->cs0.get()) : fits(h->cs1.get()))) { g_err = "assign_multipliers_dev: needs a like-prover (bp_prover_new_like) without a witness, and as many values as the recording has multipliers"; return BP_E_ARG; }
    if (!c || (count && (!d_left || !d_right))) { g_err = "assign_multipliers_dev: needs a ctx and both vectors"; return BP_E_ARG; }
    if (c->host_only) { g_err = "assign_multipliers_dev: a host-only ctx has no device memory"; return BP_E_NO_DEVICE; }
    if (c->curve != h->curve) { g_err = "assign_multipliers_dev: the ctx is of the other curve"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return h->curve == 0 ? wd_assign<Secq>(c, *h->cs0, d_left, d_right, count) : wd_assign<Zorro>(c, *h->cs1, d_left, d_right, count);
}
int bp_witness_range_bits_dev(bp_ctx* c, const void* d_values, size_t count, unsigned nbits, void* d_left, void* d_right) {
    if (!c || nbits < 1 || nbits > 64) { g_err = "witness_range_bits_dev: needs a ctx and 1 to 64 bits per value"; return BP_E_ARG; }
    if (count >= ((size_t)1 << 31) || count * nbits >= ((size_t)1 << 31)) { g_err = "witness_range_bits_dev: count * nbits reaches 2^31"; return BP_E_ARG; }
    if (c->host_only) { g_err = "witness_range_bits_dev: a host-only ctx has no device to build on"; return BP_E_NO_DEVICE; }
    if (count && (!d_values || !d_left || !d_right)) { g_err = "witness_range_bits_dev: needs the values and both outputs"; return BP_E_ARG; }
    if (!count) return BP_OK;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? wd_range_bits<Secq>(c, d_values, count * nbits, nbits, d_left, d_right) : wd_range_bits<Zorro>(c, d_values, count * nbits, nbits, d_left, d_right);
}
int bp_ctx_witness_dev_stats(bp_ctx* c, uint64_t* assigns, uint64_t* gates_from_device, uint64_t* gates_downloaded) {
    if (!c) return BP_E_ARG;
    if (assigns) *assigns = c->wd_assigns;
    if (gates_from_device) *gates_from_device = c->wd_gates_dev;
    if (gates_downloaded) *gates_downloaded = c->wd_gates_down;
    return BP_OK;
}
void bp_cs_free(bp_cs* h) { delete h; }
void* bp_cs_transcript(bp_cs* h) { return h ? h->tr : nullptr; }
int bp_cs_metrics(bp_cs* h, size_t* multipliers, size_t* constraints, size_t* commitments) {
    if (!h) return BP_E_ARG;
    if (multipliers) *multipliers = h->num_vars();
    if (constraints) *constraints = h->num_constraints();
    if (commitments) *commitments = h->commitments.size();
    return BP_OK;
}
int bp_prover_commit(bp_cs* h, bp_ctx* ctx, const uint64_t* v, const uint64_t* v_blinding, size_t count, uint64_t* V_xy_out, bp_var* vars_out) {
    if (!cs_live(h) || !h->proving || (count && (!v || !v_blinding))) return BP_E_ARG;
    if (ctx) { if (ctx->curve != h->curve) return BP_E_ARG; BPCHK(cs_pair_check("prover_commit", ctx, h, 0)); HIPCHK(hipSetDevice(ctx->device)); }
    return CS_DISPATCH(h, prover_commit<Secq>(h, ctx, v, v_blinding, count, V_xy_out, vars_out), prover_commit<Zorro>(h, ctx, v, v_blinding, count, V_xy_out, vars_out));
}
int bp_verifier_commit(bp_cs* h, const uint64_t* V_xy, size_t count, bp_var* vars_out) {
    if (!cs_live(h) || h->proving || (count && !V_xy)) return BP_E_ARG;
    if (!h->wire.empty()) { g_err = "bp_verifier_commit: wire commitments are pending on this verifier (bp_verifier_materialize first)"; return BP_E_ARG; }
    return CS_DISPATCH(h, verifier_commit<Secq>(h, V_xy, count, vars_out), verifier_commit<Zorro>(h, V_xy, count, vars_out));
}
// ---- the wire codec and verifier commitments from compressed bytes ----
int bp_points_decompress(bp_ctx* c, const uint8_t* c33, size_t n, uint64_t* out_xy, uint8_t* ok) {
    if (!c || (n && (!c33 || !out_xy || !ok))) return BP_E_ARG;
    if (!c->host_only) HIPCHK(hipSetDevice(c->device));
    static_assert(sizeof(A4) == 64, "affine points are x || y, 4 + 4 words");
    return c->curve == 0 ? wire_decode<Secq>(c, c33, n, (A4*)out_xy, ok) : wire_decode<Zorro>(c, c33, n, (A4*)out_xy, ok);
}
int bp_points_compress(int curve, const uint64_t* xy, size_t n, uint8_t* c33_out) {
    if ((curve != 0 && curve != 1) || (n && (!xy || !c33_out))) return BP_E_ARG;
    return curve == 0 ? points_compress_t<Secq>(xy, n, c33_out) : points_compress_t<Zorro>(xy, n, c33_out);
}
int bp_verifier_commit_compressed_batch(bp_ctx* c, size_t count, bp_cs* const* verifiers, const size_t* m_each, const uint8_t* c33, int defer, bp_var* vars_out, int* status) {
    if (!c && !defer) return BP_E_ARG;   // (the deferred form decodes nothing: it may go without a ctx, the handles then agree among themselves)
    if (count == 0) return BP_OK;
    if (!verifiers || !m_each || !verifiers[0]) return BP_E_ARG;
    const int curve = c ? c->curve : verifiers[0]->curve;
    size_t tot = 0;
    for (size_t k = 0; k < count; k++) {
        bp_cs* h = verifiers[k];
        if (!cs_live(h) || h->proving || h->curve != curve || !h->tr) { g_err = "bp_verifier_commit_compressed_batch: every handle must be a live verifier of the ctx's curve"; return BP_E_ARG; }
        if (CS_DISPATCH(h, h->cs0->phase2, h->cs1->phase2)) { g_err = "bp_verifier_commit_compressed_batch: commit inside the randomized phase"; return BP_E_ARG; }
        tot += m_each[k];
    }
    if (count > 1) {
        std::vector<const bp_cs*> sorted(verifiers, verifiers + count);
        std::sort(sorted.begin(), sorted.end(), std::less<const bp_cs*>());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { g_err = "bp_verifier_commit_compressed_batch: a handle is given twice"; return BP_E_ARG; }
    }
    if (tot && !c33) return BP_E_ARG;
    // commitments already pending: more may join them (or be committed behind them) only while the transcript stands where it stood
    BPCHK(wire_check_states("bp_verifier_commit_compressed_batch", count, verifiers));
    if (!defer) for (size_t k = 0; k < count; k++) if (!verifiers[k]->wire.empty()) {
        g_err = "bp_verifier_commit_compressed_batch: instance " + std::to_string(k) + " has pending wire commitments (bp_verifier_materialize first)"; return BP_E_ARG;
    }
    if (!defer && !c->host_only) HIPCHK(hipSetDevice(c->device));
    return curve == 0 ? verifier_commit_wire_batch<Secq>(c, count, verifiers, m_each, c33, defer, vars_out, status)
                         : verifier_commit_wire_batch<Zorro>(c, count, verifiers, m_each, c33, defer, vars_out, status);
}
int bp_verifier_materialize(bp_ctx* c, bp_cs* h) {
    if (!cs_live(h) || h->proving || (c && c->curve != h->curve)) return BP_E_ARG;
    if (h->wire.empty()) return BP_OK;
    BPCHK(wire_check_states("bp_verifier_materialize", 1, &h));
    if (c && !c->host_only) HIPCHK(hipSetDevice(c->device));
    int st = BP_OK;
    const CsView at{&h, nullptr};
    BPCHK(CS_DISPATCH(h, wire_materialize<Secq>(c, 1, at, &st), wire_materialize<Zorro>(c, 1, at, &st)));
    if (st == BP_E_FORMAT) g_err = "bp_verifier_materialize: a commitment's encoding was rejected";
    return st;
}
int bp_ctx_commit_wire_stats(bp_ctx* c, uint64_t* by_front_end, uint64_t* by_prologue_gpu, uint64_t* on_host) {
    if (!c) return BP_E_ARG;
    if (by_front_end) *by_front_end = c->cw_front_end;
    if (by_prologue_gpu) *by_prologue_gpu = c->cw_prologue_gpu;
    if (on_host) *on_host = c->cw_host;
    return BP_OK;
}
int bp_cs_multiply(bp_cs* h, const bp_var* lv, const uint64_t* lc, size_t nl, const bp_var* rv, const uint64_t* rc, size_t nr, bp_var out[3]) {
    CS_RECORD_GUARD(h);
    if (!out || (nl && (!lv || !lc)) || (nr && (!rv || !rc))) return BP_E_ARG;
    return CS_DISPATCH(h, cs_multiply_t<Secq>(h, lv, lc, nl, rv, rc, nr, out), cs_multiply_t<Zorro>(h, lv, lc, nl, rv, rc, nr, out));
}
int bp_cs_allocate(bp_cs* h, const uint64_t* assignment, bp_var* out) {
    CS_RECORD_GUARD(h);
    if (!out) return BP_E_ARG;
    return CS_DISPATCH(h, cs_allocate_t<Secq>(h, assignment, out), cs_allocate_t<Zorro>(h, assignment, out));
}
int bp_cs_allocate_multiplier(bp_cs* h, const uint64_t* left, const uint64_t* right, bp_var out[3]) {
    CS_RECORD_GUARD(h);
    if (!out) return BP_E_ARG;
    return CS_DISPATCH(h, cs_allocate_multiplier_t<Secq>(h, left, right, out), cs_allocate_multiplier_t<Zorro>(h, left, right, out));
}
int bp_cs_constrain(bp_cs* h, const bp_var* vars, const uint64_t* coefs, size_t n) {
    CS_RECORD_GUARD(h);
    if (n && (!vars || !coefs)) return BP_E_ARG;
    return CS_DISPATCH(h, cs_constrain_t<Secq>(h, vars, coefs, n), cs_constrain_t<Zorro>(h, vars, coefs, n));
}
int bp_cs_allocate_multipliers(bp_cs* h, const uint64_t* left, const uint64_t* right, size_t count, uint32_t* first_index) {
    CS_RECORD_GUARD(h);
    return CS_DISPATCH(h, cs_allocate_multipliers_t<Secq>(h, left, right, count, first_index), cs_allocate_multipliers_t<Zorro>(h, left, right, count, first_index));
}
int bp_cs_constrain_many(bp_cs* h, const bp_var* vars, const uint64_t* coefs, const size_t* offsets, size_t nconstraints) {
    CS_RECORD_GUARD(h);
    if (!offsets || (offsets[nconstraints] && (!vars || !coefs))) return BP_E_ARG;
    return CS_DISPATCH(h, cs_constrain_many_t<Secq>(h, vars, coefs, offsets, nconstraints), cs_constrain_many_t<Zorro>(h, vars, coefs, offsets, nconstraints));
}
int bp_cs_specify_randomized_constraints(bp_cs* h, bp_randomize_cb cb, void* user) {
    if (!cs_live(h) || !cb) return BP_E_ARG;
    if (CS_DISPATCH(h, h->cs0->phase2, h->cs1->phase2)) { g_err = "specify_randomized_constraints inside the randomized phase"; return BP_E_ARG; }
    CS_RECORD_GUARD(h);
    return CS_DISPATCH(h, cs_specify_t<Secq>(h, cb, user), cs_specify_t<Zorro>(h, cb, user));
}
int bp_cs_challenge_scalar(bp_cs* h, const char* label, uint64_t out[4]) {
    if (!cs_live(h) || !label || !out) return BP_E_ARG;
    if (!CS_DISPATCH(h, h->cs0->phase2, h->cs1->phase2)) { g_err = "challenge_scalar is only available to randomized constraints (RandomizedConstraintSystem)"; return BP_E_ARG; }
    F4 r = CS_DISPATCH(h, h->cs0->challenge_scalar(label), h->cs1->challenge_scalar(label));
    memcpy(out, r.v, 32);
    return BP_OK;
}
int bp_prover_precompute(bp_cs* h, const uint8_t rng_bytes[32]) {
    if (!cs_live(h) || !h->proving) return BP_E_ARG;
    BPCHK(cs_like_ready("precompute", h, 0));
    if (rng_bytes) { memcpy(h->rng32, rng_bytes, 32); h->have_rng = true; }
    if (!h->have_rng) { g_err = "prove: the external rng bytes are missing"; return BP_E_ARG; }
    if (h->curve == 0) { if (!h->pre0.rng) prove_precompute<Secq>(*h->cs0, h->rng32, h->pre0); }
    else { if (!h->pre1.rng) prove_precompute<Zorro>(*h->cs1, h->rng32, h->pre1); }
    return BP_OK;
}
// the same for a batch: groups of 8 same-shaped statements share one AVX-512 Keccak-f x8 stream; others go one by one
int bp_prover_precompute_batch(bp_cs** hs, size_t count) {
    if (!hs) return BP_E_ARG;
    for (size_t i = 0; i < count; i++) if (!cs_live(hs[i]) || !hs[i]->proving || !hs[i]->have_rng || hs[i]->curve != hs[0]->curve) return BP_E_ARG;
    for (size_t i = 0; i < count; i++) BPCHK(cs_like_ready("precompute_batch", hs[i], i));
    if (!count) return BP_OK;
    return hs[0]->curve == 0 ? cs_precompute_batch<Secq>(hs, count) : cs_precompute_batch<Zorro>(hs, count);
}
// how prove() obtains s_L, s_R (include/arkbp.h): fixed once the head of prove() has drawn from the TranscriptRng
int bp_prover_set_blinding(bp_cs* h, int mode) {
    if (!h || !h->proving) { g_err = "set_blinding: not a prover handle"; return BP_E_ARG; }
    if (mode != BP_BLINDING_TRANSCRIPT && mode != BP_BLINDING_EXPANDED) { g_err = "set_blinding: unknown mode"; return BP_E_ARG; }
    if (h->consumed || h->pre0.rng || h->pre1.rng) { g_err = "set_blinding: the head of prove() has run on this prover"; return BP_E_ARG; }
    h->pre0.mode = h->pre1.mode = mode;
    return BP_OK;
}
int bp_prover_blinding(bp_cs* h, int* mode_out) {
    if (!h || !h->proving || !mode_out) return BP_E_ARG;
    *mode_out = h->pre0.mode;
    return BP_OK;
}
int bp_host_blind_expand(int curve, const uint64_t kappa[4], uint64_t j0, size_t count, uint64_t* sL, uint64_t* sR) {
    if ((curve != 0 && curve != 1) || !kappa || (count && (!sL || !sR)) || j0 > ((uint64_t)1 << 31) || count > ((uint64_t)1 << 31) - j0) return BP_E_ARG;
    F4 k; memcpy(k.v, kappa, 32);
    if (curve == 0 ? host::Fld<SecqFr>::geq_p(k.v) : host::Fld<ZorroFr>::geq_p(k.v)) { g_err = "blind_expand: kappa is not a reduced scalar"; return BP_E_ARG; }
    if (curve == 0) host_blind_expand<Secq>(k, j0, count, (F4*)sL, (F4*)sR); else host_blind_expand<Zorro>(k, j0, count, (F4*)sL, (F4*)sR);
    return BP_OK;
}
int bp_debug_blind_expand(bp_ctx* c, const uint64_t kappa[4], uint64_t j0, size_t count, uint64_t* sL, uint64_t* sR) {
    if (!c || !kappa || !sL || !sR || !count || count > ((size_t)1 << 24) || j0 > ((uint64_t)1 << 31) || count > ((uint64_t)1 << 31) - j0) return BP_E_ARG;
    if (c->host_only) return BP_E_NO_DEVICE;
    F4 k; memcpy(k.v, kappa, 32);
    if (c->curve == 0 ? host::Fld<SecqFr>::geq_p(k.v) : host::Fld<ZorroFr>::geq_p(k.v)) { g_err = "blind_expand: kappa is not a reduced scalar"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_blind_expand<Secq>(c, k, j0, count, sL, sR) : dbg_blind_expand<Zorro>(c, k, j0, count, sL, sR);
}
int bp_ctx_blinding_stats(bp_ctx* c, uint64_t* expanded_scalars, uint64_t* launches) {
    if (!c) return BP_E_ARG;
    if (expanded_scalars) *expanded_scalars = c->bx_scalars;
    if (launches) *launches = c->bx_launches;
    return BP_OK;
}
int bp_prover_set_rng(bp_cs* h, const uint8_t rng_bytes[32]) {
    if (!cs_live(h) || !h->proving || !rng_bytes) return BP_E_ARG;
    memcpy(h->rng32, rng_bytes, 32); h->have_rng = true;
    return BP_OK;
}
int bp_prover_prove(bp_ctx* c, bp_cs* h, const uint8_t rng_bytes[32], uint8_t* proof_out, size_t* proof_len, double* timing) {
    if (!c || !h || !h->proving || !proof_out || !proof_len || h->curve != c->curve) return BP_E_ARG;
    if (h->consumed) { g_err = "prove: the prover was already consumed (Prover::prove takes self)"; return BP_E_ARG; }
    if (rng_bytes) {
        if (h->have_rng && (h->pre0.rng || h->pre1.rng) && memcmp(h->rng32, rng_bytes, 32)) { g_err = "prove: rng bytes differ from the precomputed ones"; return BP_E_ARG; }
        memcpy(h->rng32, rng_bytes, 32); h->have_rng = true;
    }
    if (!h->have_rng) { g_err = "prove: the external rng bytes are missing"; return BP_E_ARG; }
    BPCHK(cs_like_ready("prove", h, 0));
    BPCHK(cs_dev_witness_check("prove", c, h, 0));
    BPCHK(cs_pair_check("prove", c, h, 0));   // (before the prover is consumed)
    HIPCHK(hipSetDevice(c->device));
    if (!c->gens_cap) { g_err = "prove: generators not installed (bp_gens_derive / bp_gens_upload / bp_gens_share)"; return BP_E_GENS_LENGTH; }
    h->consumed = true; h->running = true;
    const int rc = c->curve == 0 ? cs_prove<Secq>(c, h, proof_out, proof_len, timing) : cs_prove<Zorro>(c, h, proof_out, proof_len, timing);
    h->running = false;
    return rc;
}
// ---- witness check (include/arkbp.h) ----------------------------------------------------------------------------------------------
size_t bp_witness_check_piece(void) { return WC_PIECE; }
static bool wc_prover_ok(const bp_cs* h) { return h && h->proving && !h->consumed; }
int bp_prover_check(bp_ctx* c, bp_cs* h, bp_witness_report* out) {
    if (!wc_prover_ok(h) || !out || (c && c->curve != h->curve)) { g_err = "prover_check: needs a live prover handle of the ctx's curve and a report"; return BP_E_ARG; }
    BPCHK(cs_like_ready("prover_check", h, 0));
    BPCHK(cs_dev_witness_check("prover_check", c, h, 0));
    bp_witness_report r;
    const int rc = h->curve == 0 ? cs_check_batch<Secq>(c, 1, &h, &r) : cs_check_batch<Zorro>(c, 1, &h, &r);
    if (!rc) *out = r;
    return rc;
}
int bp_prover_check_batch(bp_ctx* c, size_t count, bp_cs* const* provers, bp_witness_report* out) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!provers || !out) return BP_E_ARG;
    for (size_t k = 0; k < count; k++)
        if (!wc_prover_ok(provers[k]) || provers[k]->curve != c->curve) { g_err = "prover_check_batch: every instance needs a live prover of the ctx's curve"; return BP_E_ARG; }
    for (size_t k = 0; k < count; k++) BPCHK(cs_like_ready("prover_check_batch", provers[k], k));
    for (size_t k = 0; k < count; k++) BPCHK(cs_dev_witness_check("prover_check_batch", c, provers[k], k));
    {
        std::vector<const void*> hv(provers, provers + count);
        std::sort(hv.begin(), hv.end());
        if (std::adjacent_find(hv.begin(), hv.end()) != hv.end()) { g_err = "prover_check_batch: a prover appears twice"; return BP_E_ARG; }
    }
    std::vector<bp_witness_report> r(count);
    const int rc = c->curve == 0 ? cs_check_batch<Secq>(c, count, provers, r.data()) : cs_check_batch<Zorro>(c, count, provers, r.data());
    if (!rc) memcpy(out, r.data(), count * sizeof(bp_witness_report));
    return rc;
}
int bp_prover_set_check(bp_cs* h, int on) {
    if (!wc_prover_ok(h)) { g_err = "set_check: needs a live prover handle"; return BP_E_ARG; }
    h->check = on != 0;
    return BP_OK;
}
int bp_prover_checking(bp_cs* h, int* on_out) {
    if (!h || !h->proving || !on_out) return BP_E_ARG;
    *on_out = h->check ? 1 : 0;
    return BP_OK;
}
int bp_ctx_last_unsatisfied(bp_ctx* c, size_t cap, uint64_t* instance, bp_witness_report* reports, size_t* count) {
    if (!c || !count || (cap && (!instance || !reports))) return BP_E_ARG;
    *count = c->unsat.size();
    for (size_t i = 0; i < c->unsat.size() && i < cap; i++) { instance[i] = c->unsat[i].first; reports[i] = c->unsat[i].second; }
    return BP_OK;
}
int bp_debug_prover_poke_witness(bp_cs* h, int vec, size_t index, const uint64_t value[4]) {
    if (!wc_prover_ok(h) || !value || vec < 0 || vec > 3) return BP_E_ARG;
    F4 x; memcpy(x.v, value, 32);
    if (h->curve == 0 ? host::Fld<SecqFr>::geq_p(x.v) : host::Fld<ZorroFr>::geq_p(x.v)) { g_err = "poke_witness: the value is not a reduced scalar"; return BP_E_ARG; }
    auto poke = [&](auto* cs) -> int {
        if (vec != 3 && cs->dev.held()) BPCHK(prove_need_aO(nullptr, *cs));   // (a witness in device memory comes to the host to be poked)
        if (vec == 2) BPCHK(prove_need_aO(nullptr, *cs));   // (a like-prover's a_O exists on the host from here: the poked value is the truth)
        std::vector<F4>& t = vec == 0 ? cs->a_L : vec == 1 ? cs->a_R : vec == 2 ? cs->a_O : cs->v;
        if (index >= t.size()) return BP_E_ARG;
        t[index] = x;
        return BP_OK;
    };
    return h->curve == 0 ? poke(h->cs0.get()) : poke(h->cs1.get());
}

int bp_r1cs_batch_verify(bp_ctx* c, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens, const uint64_t* alphas, double* timing,
                         uint64_t* check_point_xy) {
    if (!c) return BP_E_ARG;
    if (count == 0) { if (check_point_xy) memset(check_point_xy, 0, 64); return BP_OK; }   // the reference's mega-check of nothing is the identity (verifier.rs:685-690)
    if (!verifiers || !proofs || !proof_lens) return BP_E_ARG;
    // The reference weights every instance with a fresh random scalar (verifier.rs:649): with equal weights the errors of two
    // invalid proofs can cancel in the single mega-check.  Only Verifier::verify (one instance) may leave the weight at 1.
    if (count > 1 && !alphas) { g_err = "batch_verify: per-instance weights (alphas) are required for more than one instance"; return BP_E_ARG; }
    BPCHK(verifiers_check("batch_verify", c, count, verifiers));
    BPCHK(wire_check_states("batch_verify", count, verifiers));
    g_dry = c->host_only;
    HIPCHK(hipSetDevice(c->device));
    if (!c->gens_cap) { g_err = "batch_verify: generators not installed"; g_dry = false; return BP_E_GENS_LENGTH; }
    const int rc = c->curve == 0 ? cs_batch_verify<Secq>(c, count, verifiers, proofs, proof_lens, alphas, timing, check_point_xy)
                                 : cs_batch_verify<Zorro>(c, count, verifiers, proofs, proof_lens, alphas, timing, check_point_xy);
    g_dry = false;
    return rc;
}
int bp_verifier_verify(bp_ctx* c, bp_cs* v, const uint8_t* proof, size_t proof_len) {
    return bp_r1cs_batch_verify(c, 1, &v, proof, &proof_len, nullptr, nullptr, nullptr);
}
// merlin::Transcript state for hosts that keep their own merlin: 200 bytes of Keccak state, then pos, pos_begin, cur_flags
int bp_transcript_export_state(const void* t, uint8_t out[203]) {
    if (!t || !out) return BP_E_ARG;
    const host::Transcript* tr = (const host::Transcript*)t;
    memcpy(out, tr->s.st.b, 200); out[200] = tr->s.pos; out[201] = tr->s.pos_begin; out[202] = tr->s.cur;
    return BP_OK;
}
int bp_transcript_import_state(void* t, const uint8_t in[203]) {
    if (!t || !in || in[200] >= host::Strobe::RATE || in[201] > host::Strobe::RATE) return BP_E_ARG;
    host::Transcript* tr = (host::Transcript*)t;
    memcpy(tr->s.st.b, in, 200); tr->s.pos = in[200]; tr->s.pos_begin = in[201]; tr->s.cur = in[202];
    return BP_OK;
}
void* bp_transcript_clone(const void* t) { return t ? new host::Transcript(*(const host::Transcript*)t) : nullptr; }

// dst uses src's resident generator tables (same device, same curve) without copying; src must outlive dst
int bp_gens_share(bp_ctx* dst, bp_ctx* src) {
    if (!dst || !src || dst == src || dst->curve != src->curve || dst->device != src->device || !src->gens_cap) return BP_E_ARG;
    DevBuf* d[] = {&dst->d_G, &dst->d_H, &dst->d_pc};
    DevBuf* sr[] = {&src->d_G, &src->d_H, &src->d_pc};
    for (int i = 0; i < 3; i++) { d[i]->release(); d[i]->p = sr[i]->p; d[i]->cap = sr[i]->cap; d[i]->owned = false; }
    dst->gens_cap = src->gens_cap; dst->gens_derived = src->gens_derived; dst->pc_B = src->pc_B; dst->pc_Bb = src->pc_Bb;
    if (dst->pc_custom || src->pc_custom) { dst->pc_table.release(); dst->pc_dt.release(); }   // the view's own tables 5 and 6 were multiples of another pair
    dst->pc_set = src->pc_set; dst->pc_custom = src->pc_custom;
    DevBuf* dt[] = {&dst->ftab_G, &dst->ftab_H, &dst->fb_G, &dst->fb_H, &dst->fb_pc};
    DevBuf* stb[] = {&src->ftab_G, &src->ftab_H, &src->fb_G, &src->fb_H, &src->fb_pc};
    for (int i = 0; i < 5; i++) { dt[i]->release(); dt[i]->p = stb[i]->p; dt[i]->cap = stb[i]->cap; dt[i]->owned = false; }
    dst->dt_tab.release(); dst->dt_cap = 0;
    if (src->dt_cap) { dst->dt_tab.p = src->dt_tab.p; dst->dt_tab.cap = src->dt_tab.cap; dst->dt_tab.owned = false; dst->dt_cap = src->dt_cap; }
    dst->fb_cap = src->fb_cap;
    dst->ftab_n = src->ftab_n; dst->ftab_w = src->ftab_w; dst->ftab_nwin = src->ftab_nwin; dst->ftab_first = src->ftab_first; dst->ftab_stride = src->ftab_stride;
    return BP_OK;
}

int bp_r1cs_verification_gh(bp_ctx* c, size_t n, size_t n1, const uint64_t* wL, const uint64_t* wR, const uint64_t* wO, const uint64_t y[4],
                            const uint64_t x[4], const uint64_t u[4], const uint64_t a[4], const uint64_t b[4], const uint64_t* ipa_challenges, size_t k,
                            uint64_t* g_out, uint64_t* h_out) {
    if (!c || !y || !x || !u || !a || !b || !g_out || !h_out || (n && (!wL || !wR || !wO)) || (k && !ipa_challenges) || k >= 32) { g_err = "bp_r1cs_verification_gh: bad argument"; return BP_E_ARG; }
    if (n > ((size_t)1 << k) || n1 > n) { g_err = "bp_r1cs_verification_gh: n exceeds the padded size 2^k"; return BP_E_ARG; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? verification_gh_host_entry<Secq>(c, n, n1, wL, wR, wO, y, x, u, a, b, ipa_challenges, k, g_out, h_out)
                         : verification_gh_host_entry<Zorro>(c, n, n1, wL, wR, wO, y, x, u, a, b, ipa_challenges, k, g_out, h_out);
}
int bp_ipa_verify(bp_ctx* c, size_t n, const uint64_t* G_factors, const uint64_t* H_factors, const uint64_t P_xy[8], const uint64_t Q_xy[8],
                  const uint64_t* G_xy, const uint64_t* H_xy, const uint64_t* L_xy, const uint64_t* R_xy, size_t lg_n, const uint64_t* challenges,
                  const uint64_t a[4], const uint64_t b[4]) {
    if (!c || !n || !G_factors || !H_factors || !P_xy || !Q_xy || !G_xy || !H_xy || !a || !b || (lg_n && (!L_xy || !R_xy || !challenges))) {
        g_err = "bp_ipa_verify: bad argument"; return BP_E_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? ipa_verify_host_entry<Secq>(c, n, G_factors, H_factors, P_xy, Q_xy, G_xy, H_xy, L_xy, R_xy, lg_n, challenges, a, b)
                         : ipa_verify_host_entry<Zorro>(c, n, G_factors, H_factors, P_xy, Q_xy, G_xy, H_xy, L_xy, R_xy, lg_n, challenges, a, b);
}

// test hook (host only): the GLV split of the uniform fold multiplier t (ark words): masks = p1[5] m1[5] p2[5] m2[5],
// t = sum (p1-m1)_i 2^i + lambda * sum (p2-m2)_i 2^i (mod r).  BP_E_ARG for a curve without the endomorphism.
int bp_debug_glv_decompose(int curve, const uint64_t t[4], uint32_t masks[20], uint64_t lambda_out[4]) {
    if (curve != 0 || !t || !masks || !lambda_out) return BP_E_ARG;
    F4 x; memcpy(x.v, t, 32);
    if (!glv_decompose<Secq>(x, masks, masks + 5, masks + 10, masks + 15)) { g_err = "glv_decompose: half longer than 129 bits"; return BP_E_ARG; }
    F4 lam; memcpy(lam.v, Secq::LAMBDA64, 32);
    host::Fld<Secq::Fr>::to_canon(lambda_out, lam);
    return BP_OK;
}

int bp_debug_decompress(bp_ctx* c, const uint8_t* compressed33, size_t n, uint64_t* out_xy, uint32_t* out_ok) {   // (the test hook's name for bp_points_decompress)
    if (!c || (n && (!compressed33 || !out_xy || !out_ok))) return BP_E_ARG;
    std::vector<uint8_t> ok(n);
    BPCHK(bp_points_decompress(c, compressed33, n, out_xy, ok.data()));
    for (size_t i = 0; i < n; i++) out_ok[i] = ok[i];
    return BP_OK;
}

// ---- verifier front end: test hooks (include/arkbp.h) ------------------------------------------------------------------------
int bp_debug_vfe_schedule_replay(const uint8_t state203[203], int absorb_commitments, uint64_t m, uint32_t k, uint64_t n, const uint8_t* items, uint8_t* seeds_out,
                                 uint32_t* nblocks_out) {
    if (!state203 || !items || !seeds_out || k >= 32 || state203[200] >= host::Strobe::RATE || m > 65535) return BP_E_ARG;
    vfe::Schedule sc;
    if (!vfe::build_verifier_schedule(sc, state203[200], state203[201], absorb_commitments != 0, m, k, n)) { g_err = "vfe schedule: unsupported shape"; return BP_E_ARG; }
    uint64_t st[25];
    memcpy(st, state203, 200);
    vfe::run_schedule_cpu(sc, st, items, seeds_out, [](uint64_t* s) { host::keccakf((host::u64*)s); });
    if (nblocks_out) *nblocks_out = (uint32_t)sc.blocks.size();
    return BP_OK;
}
int bp_debug_vfe_schedule_replay_2phase(const uint8_t state203[203], int absorb_commitments, uint64_t m, uint32_t k, uint64_t n, const char* const* labels, size_t nlabels,
                                        const uint8_t* items, uint8_t* seeds_out, uint32_t* nblocks_out) {
    if (!state203 || !items || !seeds_out || (nlabels && !labels) || k >= 32 || state203[200] >= host::Strobe::RATE || m > 65535 || nlabels > 4096) return BP_E_ARG;
    std::vector<std::string> gl;
    for (size_t i = 0; i < nlabels; i++) { if (!labels[i]) return BP_E_ARG; gl.emplace_back(labels[i]); }
    vfe::Schedule sc;
    if (!vfe::build_verifier_schedule_2phase(sc, state203[200], state203[201], absorb_commitments != 0, m, k, n, gl)) { g_err = "vfe schedule: unsupported shape"; return BP_E_ARG; }
    uint64_t st[25];
    memcpy(st, state203, 200);
    vfe::run_schedule_cpu(sc, st, items, seeds_out, [](uint64_t* s) { host::keccakf((host::u64*)s); });
    if (nblocks_out) *nblocks_out = (uint32_t)sc.blocks.size();
    return BP_OK;
}
int bp_debug_vfe_challenges(bp_ctx* c, size_t count, const uint8_t* proofs, size_t proof_len, const uint64_t* commit_xy, size_t m, const uint8_t* states203,
                            int shared_state, int absorb_commitments, uint8_t* seeds_out, uint64_t* chal_out, uint32_t* status_out) {
    if (!c || !count || !proofs || !states203 || !seeds_out || !chal_out || !status_out || (m && !commit_xy)) return BP_E_ARG;
    if (proof_len < 539 || (proof_len - 539) % 66 || count > 65535 || m > 65535) return BP_E_ARG;
    const size_t k = (proof_len - 539) / 66;
    if (k >= 32) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nst = shared_state ? 1 : count;
    for (size_t i = 0; i < nst; i++) if (states203[203 * i + 200] != states203[200] || states203[203 * i + 201] != states203[201]) { g_err = "vfe: transcript positions differ"; return BP_E_ARG; }
    vfe::Schedule sc;
    if (!vfe::build_verifier_schedule(sc, states203[200], states203[201], absorb_commitments != 0, m, (uint32_t)k, (uint64_t)1 << k)) return BP_E_ARG;
    const std::vector<uint32_t> enc = sc.encode();
    vfe::Shape sh;
    sh.P = (uint32_t)count; sh.m = (uint32_t)m; sh.nV = absorb_commitments ? (uint32_t)m : 0u; sh.k = (uint32_t)k; sh.plen = (uint32_t)proof_len;
    sh.tail = (uint32_t)(6 + m + 5 + 2 * k); sh.nitems = sh.nV + 11 + 2 * (uint32_t)k + 3;
    const size_t nch = 6 + k;
    auto up256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_proofs = up256(count * proof_len), b_V = up256(count * m * 64), b_st = up256(nst * 200), b_sched = up256(enc.size() * 4);
    BPCHK(c->vfe_in.ensure(b_proofs + b_V + b_st + b_sched));
    BPCHK(c->vfe_msg.ensure((size_t)sh.nitems * vfe::ITEM_WORDS * count * 8));
    BPCHK(c->vfe_chal.ensure(count * nch * 32));
    BPCHK(c->vfe_ws.ensure(count * nch * 32 + count * nch * 32));
    BPCHK(c->vfe_small.ensure(4096));
    BPCHK(c->r_tail.ensure(count * sh.tail * 64));
    uint8_t* d_in = (uint8_t*)c->vfe_in.p;
    std::vector<uint8_t> states(nst * 200);
    for (size_t i = 0; i < nst; i++) memcpy(&states[200 * i], states203 + 203 * i, 200);
    HIPCHK(hipMemcpyAsync(d_in, proofs, count * proof_len, hipMemcpyHostToDevice, st));
    if (m) HIPCHK(hipMemcpyAsync(d_in + b_proofs, commit_xy, count * m * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_in + b_proofs + b_V, states.data(), nst * 200, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_in + b_proofs + b_V + b_st, enc.data(), enc.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->vfe_small.p, 0, 256, st));
    if (vfe::launch_points(c->curve, st, sh, d_in, (const u32*)(d_in + b_proofs), (uint64_t*)c->vfe_msg.p, c->r_tail.as<u32>(), c->vfe_small.as<u32>(), nullptr)) return BP_E_HIP;
    uint8_t* d_seeds = (uint8_t*)c->vfe_ws.p;
    u32* d_ark = c->vfe_ws.as<u32>() + count * nch * 8;
    if (vfe::launch_sponge(c->curve, st, sh, (const u32*)(d_in + b_proofs + b_V + b_st), (const uint64_t*)(d_in + b_proofs + b_V), shared_state ? 0u : 25u, (const uint64_t*)c->vfe_msg.p,
                           c->vfe_chal.as<u32>(), d_seeds)) return BP_E_HIP;
    if (c->curve == 0) hipLaunchKernelGGL(k_dbg_scalars_to_ark<Secq>, dim3((u32)((count * nch + 255) / 256)), dim3(256), 0, st, c->vfe_chal.as<u32>(), d_ark, (u32)(count * nch));
    else hipLaunchKernelGGL(k_dbg_scalars_to_ark<Zorro>, dim3((u32)((count * nch + 255) / 256)), dim3(256), 0, st, c->vfe_chal.as<u32>(), d_ark, (u32)(count * nch));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(seeds_out, d_seeds, count * nch * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(chal_out, d_ark, count * nch * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status_out, c->vfe_small.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
int bp_debug_verify_challenges(int curve, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                               const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, int use_x8, uint64_t* out, size_t* nchal) {
    if (!count || count > 8 || !scenarios || !params || !proofs || !proof_lens || !commit_xy || !ms || !publics || !npubs || !out || !nchal) return BP_E_ARG;
    return curve == 0 ? dbg_verify_challenges<Secq>(count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, use_x8, out, nchal)
                      : dbg_verify_challenges<Zorro>(count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, use_x8, out, nchal);
}
int bp_ctx_fold_stats(bp_ctx* c, uint64_t* deferred_first_folds, uint64_t* second_folds_from_tables) {
    if (!c) return BP_E_ARG;
    if (deferred_first_folds) *deferred_first_folds = c->folds_deferred;
    if (second_folds_from_tables) *second_folds_from_tables = c->folds_tab2;
    return BP_OK;
}
int bp_ctx_msm_pair_stats(bp_ctx* c, uint64_t* paired_passes, uint64_t* jobs_redone) {
    if (!c) return BP_E_ARG;
    if (paired_passes) *paired_passes = c->pair_passes;
    if (jobs_redone) *jobs_redone = c->pair_redone;
    return BP_OK;
}
int bp_ctx_direct_stats(bp_ctx* c, uint64_t* direct_msms, size_t* bases_per_vector) {
    if (!c) return BP_E_ARG;
    if (direct_msms) *direct_msms = c->dt_runs;
    if (bases_per_vector) *bases_per_vector = c->dt_cap;
    return BP_OK;
}
int bp_ctx_msm_stats(bp_ctx* c, uint64_t* fixed_base_runs, uint64_t* fixed_base_runs_sharded) {
    if (!c) return BP_E_ARG;
    if (fixed_base_runs) *fixed_base_runs = c->fb_runs;
    if (fixed_base_runs_sharded) *fixed_base_runs_sharded = c->fb_runs_sharded;
    return BP_OK;
}
int bp_ctx_vfe_stats(bp_ctx* c, uint64_t* device_batches, uint64_t* host_fallbacks) {
    if (!c) return BP_E_ARG;
    if (device_batches) *device_batches = c->vfe_batches;
    if (host_fallbacks) *host_fallbacks = c->vfe_fallbacks;
    return BP_OK;
}
int bp_ctx_vfe_class_stats(bp_ctx* c, uint64_t* class_calls, uint64_t* device_classes, uint64_t* device_instances, uint64_t* remainder_instances, uint64_t* flagged_replayed) {
    if (!c) return BP_E_ARG;
    if (class_calls) *class_calls = c->vcl_calls;
    if (device_classes) *device_classes = c->vcl_classes;
    if (device_instances) *device_instances = c->vcl_instances;
    if (remainder_instances) *remainder_instances = c->vcl_remainder;
    if (flagged_replayed) *flagged_replayed = c->vcl_flagged;
    return BP_OK;
}
int bp_debug_vfy_class_plan(size_t count, const uint64_t* keys, const uint8_t* eligible, uint64_t class_min, uint32_t max_classes, int32_t* class_of, uint32_t* nclasses) {
    if (!nclasses || (count && (!keys || !class_of))) return BP_E_ARG;
    vfy_class_plan(count, keys, eligible, class_min, max_classes, class_of, nclasses);
    return BP_OK;
}

int bp_ctx_set_profiling(bp_ctx* c, int enabled) { if (!c) return BP_E_ARG; c->profiling = enabled != 0; return BP_OK; }
int bp_ctx_kernel_time(bp_ctx* c, int which, double* ms_total, uint64_t* launches) {
    if (!c || which < 0 || which >= BP_K_COUNT) return BP_E_ARG;
    collect_timers(c);
    if (ms_total) *ms_total = c->timers[which].ms;
    if (launches) *launches = c->timers[which].launches;
    return BP_OK;
}
int bp_ctx_reset_profiling(bp_ctx* c) {
    if (!c) return BP_E_ARG;
    collect_timers(c);
    for (int k = 0; k < BP_K_COUNT; k++) { c->timers[k].ms = 0; c->timers[k].launches = 0; }
    return BP_OK;
}

int bp_debug_exp_iter(bp_ctx* c, const uint64_t x[4], size_t n, uint64_t* out) {
    if (!c || !x || (n && !out) || n >= ((size_t)1 << 31)) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_exp_iter<Secq>(c, x, n, out) : dbg_exp_iter<Zorro>(c, x, n, out);
}
int bp_debug_inner_product(bp_ctx* c, const uint64_t* a, const uint64_t* b, size_t n, uint64_t out[4]) {
    if (!c || !a || !b || !out || !n || n >= ((size_t)1 << 30)) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? dbg_inner_product<Secq>(c, a, b, n, out) : dbg_inner_product<Zorro>(c, a, b, n, out);
}
int bp_debug_field_op(bp_ctx* c, int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    if (!c || !a || !b || !out || field < 0 || field > 3) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    BPCHK(c->io_pts.ensure(n * 32)); BPCHK(c->io_scal.ensure(n * 32)); BPCHK(c->io_out.ensure(n * 32));
    HIPCHK(hipMemcpyAsync(c->io_pts.p, a, n * 32, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->io_scal.p, b, n * 32, hipMemcpyHostToDevice, c->stream));
    const u32 gb = (u32)((n + 63) / 64);
    const u32 *pa = c->io_pts.as<u32>(), *pb = c->io_scal.as<u32>();
    u32* po = c->io_out.as<u32>();
    switch (field) {
        case 0: hipLaunchKernelGGL(k_dbg_field<SecqFq>, dim3(gb), dim3(64), 0, c->stream, op, pa, pb, po, (u32)n); break;
        case 1: hipLaunchKernelGGL(k_dbg_field<SecqFr>, dim3(gb), dim3(64), 0, c->stream, op, pa, pb, po, (u32)n); break;
        case 2: hipLaunchKernelGGL(k_dbg_field<ZorroFq>, dim3(gb), dim3(64), 0, c->stream, op, pa, pb, po, (u32)n); break;
        default: hipLaunchKernelGGL(k_dbg_field<ZorroFr>, dim3(gb), dim3(64), 0, c->stream, op, pa, pb, po, (u32)n); break;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, po, n * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
int bp_debug_point_op(bp_ctx* c, int op, const uint64_t* p, const uint64_t* q, const uint64_t* k, uint64_t* out, size_t n) {
    if (!c || !p || !q || !k || !out) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    BPCHK(c->io_pts.ensure(n * 128)); BPCHK(c->io_scal.ensure(n * 32)); BPCHK(c->io_out.ensure(n * 64));
    u32* dp = c->io_pts.as<u32>();
    u32* dq = dp + n * 16;
    HIPCHK(hipMemcpyAsync(dp, p, n * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dq, q, n * 64, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->io_scal.p, k, n * 32, hipMemcpyHostToDevice, c->stream));
    const u32 gb = (u32)((n + 63) / 64);
    if (c->curve == 0) hipLaunchKernelGGL(k_dbg_point<Secq>, dim3(gb), dim3(64), 0, c->stream, op, dp, dq, c->io_scal.as<u32>(), c->io_out.as<u32>(), (u32)n);
    else hipLaunchKernelGGL(k_dbg_point<Zorro>, dim3(gb), dim3(64), 0, c->stream, op, dp, dq, c->io_scal.as<u32>(), c->io_out.as<u32>(), (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->io_out.p, n * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
/* raw limbs in, raw limbs out (csrc/dbg_raw.cuh lists the ops and the layouts) */
int bp_debug_field_raw(bp_ctx* c, int field, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (!c || !in || !out || field < 0 || field > 3 || op < 0 || op >= RAW_F_COUNT || !n || n > ((size_t)1 << 24)) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    BPCHK(c->io_pts.ensure(n * RAW_F_IN * 4)); BPCHK(c->io_out.ensure(n * RAW_F_OUT * 4));
    HIPCHK(hipMemcpyAsync(c->io_pts.p, in, n * RAW_F_IN * 4, hipMemcpyHostToDevice, c->stream));
    const u32* pi = c->io_pts.as<u32>();
    u32* po = c->io_out.as<u32>();
    dbg_raw_launch_field(c->stream, field, op, pi, po, (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, po, n * RAW_F_OUT * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}
int bp_debug_point_raw(bp_ctx* c, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (!c || !in || !out || op < 0 || op >= RAW_P_COUNT || !n || n > ((size_t)1 << 22)) return BP_E_ARG;
    HIPCHK(hipSetDevice(c->device));
    const size_t lanes = op < RAW_P_QADD ? 1 : 4, obytes = n * lanes * RAW_P_OUT * 4;
    BPCHK(c->io_pts.ensure(n * RAW_P_IN * 4)); BPCHK(c->io_out.ensure(obytes));
    HIPCHK(hipMemcpyAsync(c->io_pts.p, in, n * RAW_P_IN * 4, hipMemcpyHostToDevice, c->stream));
    const u32* pi = c->io_pts.as<u32>();
    u32* po = c->io_out.as<u32>();
    dbg_raw_launch_point(c->stream, c->curve, op, pi, po, (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, po, obytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}

}  // extern "C"
