// batch_verify (src/r1cs/verifier.rs:604-691) on the host-replay route, as steps over one job; Verifier::verify (:559-600) is a batch
// of one with alpha = 1.  Included by r1cs_host.inc; verify_each.inc shares the front steps (vfy_parse .. vfy_resolve_templates).
//
// Pipeline.  Decode: framing on the host, every compressed point of the batch decompressed on the GPU, one block ahead.  The
// instances go through in blocks of VFY_BLOCK: the host threads replay the transcripts of a block (commitments, proof points,
// the instance's randomized constraints, challenges; verify_prepare) and stage parameter blocks, coefficient tables and tail
// scalars / points in pinned memory while the GPU evaluates the previous block (k_vfy_batch: flattened constraints from the
// circuit template, the 2N g/h scalars of every proof, alpha-weighted accumulation).  Instances are grouped by the template their
// recording canonicalises to — single-phase and randomized statements alike; one launch per (template, block).  The alpha-scaling
// of the tails and the canonical forms are GPU work; the host keeps only the two head scalars.  One MSM at the end (vfy_mega_check).
//
// The orderings the steps keep, each stated where it is enforced:
//   vfy_block_open       the waits on a staging half's two events come before vfy_stage_ensure, which may reallocate the half; the
//                        decode of the next block is enqueued before this block's replay starts (one block ahead);
//   vfy_stage_one        a recording is released in the pool thread that allocated it;
//   vfy_block_templates  eviction from the template cache once per block, before the block resolves its templates.

struct VfyMark {   // ARKBP_VFY_TRACE: the time since the previous mark, on stderr
    const char* tag; double t_last;
    void operator()(const char* what) {
        static const bool on = getenv("ARKBP_VFY_TRACE") != nullptr;
        if (on) { double t = now_s(); fprintf(stderr, "[%s] %-28s %8.3f ms\n", tag, what, (t - t_last) * 1e3); t_last = t; }
    }
};

// One instance after its replay: the recorded verifier, the proof, what verify_prepare made of them, and its circuit template
template <class C> struct VfyReplayed {
    VfyInstance<C> inst; host::ProofData pf; VerifyPrep<C> vp; int rc = BP_OK;
    const VTemplate<C>* tm = nullptr; std::shared_ptr<void> keep; char own_tab = 0;   // vfy_resolve_templates
};

// ---- front steps, shared with verify_each_core ---------------------------------------------------------------------------------------
// Pending wire commitments first (pst[k]: BP_E_FORMAT for a rejected encoding), then the framing of every proof on the pool (rcs[k])
template <class C>
static int vfy_parse(bp_ctx* ctx, const VfyProvider<C>& prov, size_t count, const uint8_t* proofs, const size_t* poff, std::vector<int>& pst,
                     std::vector<host::LazyProof>& lps, std::vector<int>& rcs) {
    pst.assign(count, BP_OK); rcs.assign(count, BP_OK); lps.resize(count);
    if (prov.prologue) BPCHK(prov.prologue(nullptr, count, pst.data()));
    pool_range(ctx, 0, count, [&](size_t k) { rcs[k] = host::proof_parse_lazy<C>(lps[k], proofs + poff[k], poff[k + 1] - poff[k]); });
    return BP_OK;
}
// The compressed points of instances idx[0 .. n) (idx null: instances 0 .. n), in that order: where each instance's points start ...
static std::vector<size_t> vfy_xoff(const std::vector<host::LazyProof>& lps, const size_t* idx, size_t n) {
    std::vector<size_t> xoff(n + 1, 0);
    for (size_t j = 0; j < n; j++) xoff[j + 1] = xoff[j] + lps[idx ? idx[j] : j].xs.size();
    return xoff;
}
// ... and their x words and flag words gathered into the caller's arrays of xoff[n] entries
static void vfy_gather(bp_ctx* ctx, const std::vector<host::LazyProof>& lps, const size_t* idx, size_t n, const std::vector<size_t>& xoff, F4* all_x, u32* all_f) {
    pool_range(ctx, 0, n, [&](size_t j) { const host::LazyProof& lp = lps[idx ? idx[j] : j]; std::copy(lp.xs.begin(), lp.xs.end(), all_x + xoff[j]); std::copy(lp.flags.begin(), lp.flags.end(), all_f + xoff[j]); });
}
// an x that is not on the curve is a FormatError of its instance
static bool vfy_points_ok(const u32* all_ok, size_t x0, size_t x1) { for (size_t j = x0; j < x1; j++) if (!all_ok[j]) return false; return true; }
// the proof's points in place, the instance's recording at hand ...
template <class C> static void vfy_replay_fetch(const VfyProvider<C>& prov, size_t k, const host::LazyProof& lp, const A4* pts, VfyReplayed<C>& r) {
    host::proof_finish_lazy(r.pf, lp, pts);
    r.rc = prov.get(k, r.inst);
}
// ... and the replay of its own transcript
template <class C> static int vfy_replay_one(bp_ctx* ctx, const VfyProvider<C>& prov, size_t k, const host::LazyProof& lp, const A4* pts, VfyReplayed<C>& r) {
    vfy_replay_fetch<C>(prov, k, lp, pts, r);
    if (!r.rc) r.rc = verify_prepare<C>(*r.inst.cs, r.pf, ctx->gens_cap, r.vp);
    return r.rc;
}
// Templates of the replayed instances at(0) .. at(n - 1): look up by structure digest; a miss records the matrices from that instance
// (upload + sync, once per gadget).  Bounded cache: the trim happens HERE, before the lookups, and only takes entries none of these
// instances resolves to (the bound is soft: more than 64 new shapes grow it).  uniform (optional): consecutive instances of one gadget
// with one table share the previous lookup; cleared when the instances did not all resolve like the first.
template <class C, class At> static int vfy_resolve_templates(bp_ctx* ctx, size_t n, At at, const char* who, bool* uniform) {
    if (n && ctx->templates.size() >= VFY_TEMPLATE_CACHE) {
        std::set<std::string> used;
        for (size_t p = 0; p < n; p++) used.insert(vfy_template_key(at(p).vp.digest));
        BPCHK(vfy_templates_trim(ctx, used));
    }
    for (size_t p = 0; p < n; p++) {
        VfyReplayed<C>& r = at(p);
        const VerifyPrep<C>& vp = r.vp;
        if (uniform && p > 0) {
            const VfyReplayed<C>& q = at(p - 1);
            if (vp.digest == q.vp.digest && vp.coef_ptr == q.vp.coef_ptr && vp.n == q.vp.n && vp.n1 == q.vp.n1) { r.tm = q.tm; r.keep = q.keep; r.own_tab = q.own_tab; continue; }
            *uniform = false;
        }
        BPCHK(vfy_template_get<C>(ctx, vp.digest, r.inst.cs, vp.n, vp.n1, vp.nq, vp.ncoef, who, r.keep, r.tm));
        r.own_tab = vfy_own_table<C>(*r.tm, vp);
    }
    return BP_OK;
}

// ---- the job: what lives across the block loop ------------------------------------------------------------------------------------------
template <class C> struct VfyHostJob {
    bp_ctx* ctx; const VfyProvider<C>& prov; size_t count; const uint8_t* proofs; const size_t* poff; const F4* alphas;
    int* inst_status;   // optional (bp_r1cs_batch_verify_locate): a status for EVERY instance that fails before the mega-check
    VfyMark mark;
    std::vector<host::LazyProof> lps; std::vector<int> rcs;   // framing
    std::vector<size_t> xoff, toff;                            // first compressed point / first tail term of each instance
    // decode arena, pinned and on the device: x words, points, flag words, ok words of every compressed point of the batch
    F4* all_x = nullptr; A4* all_pts = nullptr; u32 *all_f = nullptr, *all_ok = nullptr, *d_x = nullptr, *d_pts = nullptr, *d_f = nullptr, *d_ok = nullptr;
    size_t decoded_upto = 0;   // instances [0, decoded_upto) have their decode enqueued on the aux stream
    // layout of the mega-check MSM: [B, B_blinding | G[..maxN] | H[..maxN] | tails of instance 0, 1, ...]
    size_t maxN = 1, Ttot = 0; bool doomed = false;
    u32 *sc = nullptr, *acc_g = nullptr, *acc_h = nullptr, *d_tail_sc = nullptr, *d_alpha = nullptr, *d_toff = nullptr;
    F4 sB = host::Fld<typename C::Fr>::zero(), sBb = host::Fld<typename C::Fr>::zero();   // the two head scalars
    size_t nslots = 0;          // (wc + delta) slots in r_small: one per launched group
    double host_busy = 0;
    uint64_t dry_sum = 0xcbf29ce484222325ULL;   // host-only ctx: checksum of everything staged
};
// One block of the loop.  Staging half: [parameter blocks (block order) | tail scalars | tail points]; aux half: [perm | coefficient tables]
template <class C> struct VfyHostBlock {
    size_t lo = 0, hi = 0, nb = 0, t_lo = 0, bytes_pb = 0, bytes_ts = 0, bytes_tp = 0, bytes_perm = 0; int half = 0;
    F4 *st_pb = nullptr, *st_ts = nullptr; A4* st_tp = nullptr;
    std::vector<VfyReplayed<C>> rep; std::vector<F4> part_sB, part_sBb;
    bool uniform = true;   // every instance resolved like the first (the common case: one gadget, shared values)
};

// ---- decode: the square roots of all compressed points on the GPU, on a second stream, block by block -------------------------------
template <class C> static int vfy_decode_arena(VfyHostJob<C>& J) {
    bp_ctx* ctx = J.ctx;
    const size_t xtot = J.xoff[J.count], need = xtot * (32 + 4 + 64 + 4) + 64;
    BPCHK(pinned_ensure(ctx->h_dec, ctx->h_dec_cap, need, need >> 2));
    if (!ctx->aux_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->aux_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) if (!ctx->dec_ev[i]) HIPCHK(hipEventCreateWithFlags(&ctx->dec_ev[i], hipEventDisableTiming));
    BPCHK(ctx->v_dec.ensure(need));
    J.all_x = (F4*)ctx->h_dec; J.all_pts = (A4*)((char*)ctx->h_dec + xtot * 32); J.all_f = (u32*)((char*)ctx->h_dec + xtot * 96); J.all_ok = J.all_f + xtot;
    J.d_x = ctx->v_dec.as<u32>(); J.d_pts = J.d_x + xtot * 8; J.d_f = J.d_pts + xtot * 16; J.d_ok = J.d_f + xtot;
    return BP_OK;
}
// enqueue the decode of instances [decoded_upto, k_hi); event `ev` fires when their points are in host memory
template <class C> static int vfy_decode_issue(VfyHostJob<C>& J, size_t k_hi, int ev) {
    bp_ctx* ctx = J.ctx;
    const size_t x0 = J.xoff[J.decoded_upto], x1 = J.xoff[k_hi], cnt = x1 - x0;
    if (cnt && ctx->host_only) {
        // dry run without a device: the square roots on the host pool (what k_points_decompress computes)
        pool_range(ctx, x0, x1, [&](size_t j) {
            A4 pt{}; bool good = true;
            const u32 fl = J.all_f[j];
            if (!(fl & 0x40)) good = host::Grp<C>::from_x(pt, J.all_x[j], (fl & 0x80) != 0);
            J.all_pts[j] = good ? pt : A4{}; J.all_ok[j] = good ? 1u : 0u;
        });
    } else if (cnt) {
        hipStream_t as = ctx->aux_stream;
        HIPCHK(hipMemcpyAsync(J.d_x + x0 * 8, J.all_x + x0, cnt * 32, hipMemcpyHostToDevice, as));
        HIPCHK(hipMemcpyAsync(J.d_f + x0, J.all_f + x0, cnt * 4, hipMemcpyHostToDevice, as));
        hipLaunchKernelGGL(k_points_decompress<C>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, as, J.d_x + x0 * 8, J.d_f + x0, J.d_pts + x0 * 16, J.d_ok + x0, (u32)cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(J.all_pts + x0, J.d_pts + x0 * 16, cnt * 64, hipMemcpyDeviceToHost, as));
        HIPCHK(hipMemcpyAsync(J.all_ok + x0, J.d_ok + x0, cnt * 4, hipMemcpyDeviceToHost, as));
    }
    HIPCHK(hipEventRecord(ctx->dec_ev[ev], ctx->aux_stream));
    J.decoded_upto = k_hi;
    return BP_OK;
}
// x not on the curve -> FormatError, first in instance order
template <class C> static int vfy_decode_check(const VfyHostJob<C>& J, size_t k_lo, size_t k_hi) {
    return vfy_points_ok(J.all_ok, J.xoff[k_lo], J.xoff[k_hi]) ? BP_OK : BP_E_FORMAT;
}

// ---- layout ---------------------------------------------------------------------------------------------------------------------------
// A valid proof carries lg N points in L_vec (checked against the recording in verify_prepare), so the proofs themselves size the
// layout.  A proof whose claim cannot hold on this ctx (L/R lengths differ, k >= 32, 2^k above the installed generators) dooms the
// batch: the instances are then replayed without any GPU work, only to report the reference's first error in instance order.
static bool vfy_claim_bad(size_t kk, size_t gens_cap) { return kk == (size_t)-1 || kk >= 32 || ((size_t)1 << kk) > gens_cap; }
template <class C> static void vfy_layout(VfyHostJob<C>& J) {
    J.toff.assign(J.count + 1, 0);
    for (size_t k = 0; k < J.count; k++) {
        const size_t kk = J.lps[k].k;
        if (vfy_claim_bad(kk, J.ctx->gens_cap)) { J.doomed = true; J.toff[k + 1] = J.toff[k]; continue; }
        J.maxN = std::max(J.maxN, (size_t)1 << kk);
        J.toff[k + 1] = J.toff[k] + 6 + J.prov.m_of(k) + 5 + 2 * kk;
    }
    J.Ttot = J.toff[J.count];
}
// the resident buffers of that layout, the accumulators cleared, the weights and the tail offsets on the device
template <class C> static int vfy_reserve(VfyHostJob<C>& J) {
    bp_ctx* ctx = J.ctx;
    hipStream_t st = ctx->stream;
    const size_t count = J.count, maxN = J.maxN;
    BPCHK(ctx->r_g.ensure(vfy_rg_len(maxN, J.Ttot) * 32));   // (the r_g layout: vfy_dev_plan.hpp)
    BPCHK(ctx->r_tail.ensure(std::max<size_t>(J.Ttot, 1) * 64));
    BPCHK(ctx->r_small.ensure((count + 8) * 32));               // one (wc + delta) slot per launched group: at most one per instance
    BPCHK(ctx->v_alpha.ensure(count * 32 + (count + 1) * 4));
    J.sc = ctx->r_g.as<u32>(); J.acc_g = J.sc + VFY_RG_G * 8; J.acc_h = J.sc + vfy_rg_h(maxN) * 8; J.d_tail_sc = J.sc + vfy_rg_tails(maxN) * 8;
    J.d_alpha = ctx->v_alpha.as<u32>(); J.d_toff = J.d_alpha + count * 8;
    HIPCHK(hipMemsetAsync(J.sc, 0, vfy_rg_tails(maxN) * 32, st));
    BPCHK(upload_scalars<C>(ctx, J.d_alpha, J.alphas, count));
    std::vector<u32> toff32(J.toff.begin(), J.toff.end());
    HIPCHK(hipMemcpyAsync(J.d_toff, toff32.data(), (count + 1) * 4, hipMemcpyHostToDevice, st));
    return BP_OK;
}

// ---- one block ------------------------------------------------------------------------------------------------------------------------
// Opens block [lo, lo + VFY_BLOCK): its points in host memory (frc: one of them is not on the curve), the next block's decode enqueued
// beside this block's replay, its staging half free and large enough.
template <class C> static int vfy_block_open(VfyHostJob<C>& J, VfyHostBlock<C>& B, size_t lo, int& frc) {
    bp_ctx* ctx = J.ctx;
    const size_t blk = lo / VFY_BLOCK;
    B.lo = lo; B.hi = std::min(J.count, lo + VFY_BLOCK); B.nb = B.hi - lo; B.half = (int)(blk & 1);
    if (B.hi > J.decoded_upto) BPCHK(vfy_decode_issue<C>(J, B.hi, B.half));   // (only when block 0 was shorter than expected: not reached)
    if (blk > 0) {
        HIPCHK(event_wait(ctx, ctx->dec_ev[B.half]));                          // this block's points are in host memory
        if ((frc = vfy_decode_check<C>(J, lo, B.hi))) return BP_OK;
    }
    if (J.decoded_upto < J.count) BPCHK(vfy_decode_issue<C>(J, std::min(J.count, J.decoded_upto + VFY_BLOCK), B.half ^ 1));   // one block ahead
    B.t_lo = J.toff[lo];
    const size_t nt = J.toff[B.hi] - B.t_lo;
    B.bytes_pb = B.nb * VFY_PB_SCALARS * 32; B.bytes_ts = nt * 32; B.bytes_tp = nt * 64; B.bytes_perm = (B.nb * 4 + 31) / 32 * 32;
    if (blk >= 2 && ctx->vstage_ev[B.half]) HIPCHK(event_wait(ctx, ctx->vstage_ev[B.half]));   // the copies out of this half (two blocks ago) are done
    if (blk >= 2 && ctx->vtail_ev[B.half]) HIPCHK(event_wait(ctx, ctx->vtail_ev[B.half]));
    BPCHK(vfy_stage_ensure(ctx, B.half, B.bytes_pb + B.bytes_ts + B.bytes_tp));                  // (may reallocate: only after those copies)
    B.st_pb = (F4*)ctx->h_vstage[B.half];
    B.st_ts = (F4*)((char*)ctx->h_vstage[B.half] + B.bytes_pb);
    B.st_tp = (A4*)((char*)ctx->h_vstage[B.half] + B.bytes_pb + B.bytes_ts);
    B.rep.resize(B.nb); B.part_sB.resize(B.nb); B.part_sBb.resize(B.nb);
    return BP_OK;
}
// The replay of member p and its staging: parameter block, tails, part sums.  chal: the proof's challenges from the lockstep replay
// (inv_acc_y: its share of the group's one inversion), or nullptr: its own transcript.
template <class C> static void vfy_stage_one(VfyHostJob<C>& J, VfyHostBlock<C>& B, size_t p, const F4* chal, const F4* inv_acc_y) {
    typedef host::Fld<typename C::Fr> S;
    bp_ctx* ctx = J.ctx;
    const size_t k = B.lo + p;
    VfyReplayed<C>& r = B.rep[p];
    if (r.rc) return;
    if (chal) { PrecompTr T{chal, inv_acc_y}; r.rc = verify_prepare_t<C>(*r.inst.cs, r.pf, ctx->gens_cap, r.vp, T); }
    else r.rc = verify_prepare<C>(*r.inst.cs, r.pf, ctx->gens_cap, r.vp);
    if (r.rc) return;
    const VerifyPrep<C>& vp = r.vp;
    if (vp.tail_scalars.size() != J.toff[k + 1] - J.toff[k]) { r.rc = BP_E_VERIFICATION; return; }
    const F4& alpha = J.alphas[k];
    F4* b = B.st_pb + p * VFY_PB_SCALARS;
    for (u32 j = 0; j < VFY_PB_SCALARS; j++) b[j] = S::zero();
    for (int j = 0; j < 32; j++) { b[j] = vp.ztab[j]; b[32 + j] = vp.ypw[32 + j]; }
    b[64] = vp.allinv; b[65] = vp.x; b[66] = vp.a; b[67] = vp.b; b[68] = vp.u; b[69] = alpha; b[70] = S::mul(alpha, vp.coefD); b[71] = vp.rx;
    for (size_t j = 0; j < vp.k; j++) b[72 + j] = vp.u_sq[j];
    if (!vp.tail_scalars.empty()) {
        memcpy(B.st_ts + (J.toff[k] - B.t_lo), vp.tail_scalars.data(), vp.tail_scalars.size() * 32);
        memcpy(B.st_tp + (J.toff[k] - B.t_lo), vp.tail_points.data(), vp.tail_points.size() * 64);
    }
    B.part_sB[p] = S::mul(alpha, vp.sB); B.part_sBb[p] = S::mul(alpha, vp.sBb);
    // the recording is only needed again if its template does not exist yet (the map is not modified during the replay):
    // release it here, in the thread that allocated it
    if (r.inst.owned_cs && ctx->templates.count(vfy_template_key(vp.digest))) { r.inst.owned_cs.reset(); r.inst.owned_tr.reset(); r.inst.cs = nullptr; r.inst.released = true; }
    std::vector<F4>().swap(r.vp.tail_scalars); std::vector<A4>().swap(r.vp.tail_points);
    r.pf = host::ProofData();
}
// Members [p0, p0 + cnt), cnt <= 8, in one pool thread: their transcripts take the commitments in lockstep where the provider can do
// that (AVX-512 Keccak x8), and a full group of single-phase proofs the rest of the replay too (replay_challenges_x8)
template <class C> static void vfy_replay_group(VfyHostJob<C>& J, VfyHostBlock<C>& B, size_t p0, size_t cnt) {
    typedef host::Fld<typename C::Fr> S;
    if (J.prov.head8) {
        std::unique_ptr<host::Transcript> heads[8];
        J.prov.head8(B.lo + p0, cnt, heads);
        for (size_t j = 0; j < cnt; j++) B.rep[p0 + j].inst.owned_tr = std::move(heads[j]);
    }
    for (size_t j = 0; j < cnt; j++) { const size_t k = B.lo + p0 + j; vfy_replay_fetch<C>(J.prov, k, J.lps[k], J.all_pts + J.xoff[k], B.rep[p0 + j]); }
#if defined(__x86_64__)
    static const bool no_x8 = getenv("ARKBP_VFY_NOX8") != nullptr;   // A/B switch
    if (cnt == 8 && !no_x8 && host::cpu_has_avx512()) {
        // the eight transcripts in lockstep through the rest of the replay; the arithmetic per proof after
        host::ConstraintSystem<C>* csp[8];
        const host::ProofData* pfp[8];
        bool ok = true;
        for (size_t j = 0; j < 8; j++) { const VfyReplayed<C>& r = B.rep[p0 + j]; if (r.rc || !r.inst.cs) { ok = false; break; } csp[j] = r.inst.cs; pfp[j] = &r.pf; }
        std::vector<F4> chal[8];
        if (ok && replay_challenges_x8<C>(csp, pfp, chal)) {
            // the eight proofs' inversions as one (every challenge is known: y = chal[0], u_i = chal[5 + i])
            F4 prod[8], pre[8], both[8];
            F4 run = S::one();
            for (size_t j = 0; j < 8; j++) {
                const size_t kk = chal[j].size() - 6;
                F4 acc = S::one();
                for (size_t i = 0; i < kk; i++) if (!chal[j][5 + i].is_zero()) acc = S::mul(acc, chal[j][5 + i]);
                prod[j] = chal[j][0].is_zero() ? acc : S::mul(acc, chal[j][0]);
                pre[j] = run; run = S::mul(run, prod[j]);          // (never zero: products of non-zero scalars)
            }
            F4 inv = S::inv(run);
            for (size_t j = 8; j-- > 0;) { both[j] = S::mul(inv, pre[j]); inv = S::mul(inv, prod[j]); }
            for (size_t j = 0; j < 8; j++) vfy_stage_one<C>(J, B, p0 + j, chal[j].data(), &both[j]);
            return;
        }
    }
#endif
    for (size_t j = 0; j < cnt; j++) vfy_stage_one<C>(J, B, p0 + j, nullptr, nullptr);
}
template <class C> static void vfy_replay_block(VfyHostJob<C>& J, VfyHostBlock<C>& B) {
    const double th0 = now_s();
    pool_range(J.ctx, 0, (B.nb + 7) / 8, [&](size_t g) { vfy_replay_group<C>(J, B, g * 8, std::min<size_t>(8, B.nb - g * 8)); });
    J.host_busy += now_s() - th0;
    J.mark("  block: replay");
}
// host-only ctx: what the host staged for this block, folded into the job's checksum (compared across thread counts / replay modes)
template <class C> static void vfy_dry_fold(VfyHostJob<C>& J, const VfyHostBlock<C>& B) {
    for (size_t p = 0; p < B.nb; p++) if (B.rep[p].rc) return;
    uint64_t s = J.dry_sum;
    auto fold = [&s](const void* p, size_t nbytes) { const uint64_t* w = (const uint64_t*)p; for (size_t i = 0; i < nbytes / 8; i++) { s = (s ^ w[i]) * 0x100000001b3ULL; s ^= s >> 31; } };
    fold(B.st_pb, B.bytes_pb); fold(B.st_ts, B.bytes_ts); fold(B.st_tp, B.bytes_tp); fold(B.part_sB.data(), B.nb * 32); fold(B.part_sBb.data(), B.nb * 32);
    J.dry_sum = s;
}
// The block's first error in instance order (`?` at :619; with inst_status every member's own status), or its part sums into sB, sBb
template <class C> static int vfy_block_settle(VfyHostJob<C>& J, const VfyHostBlock<C>& B) {
    typedef host::Fld<typename C::Fr> S;
    for (size_t p = 0; p < B.nb; p++) if (B.rep[p].rc) {
        if (B.rep[p].vp.err) g_err = B.rep[p].vp.err;
        if (J.inst_status) for (size_t q = 0; q < B.nb; q++) J.inst_status[B.lo + q] = B.rep[q].rc;
        return B.rep[p].rc;
    }
    for (size_t p = 0; p < B.nb; p++) { J.sB = S::add(J.sB, B.part_sB[p]); J.sBb = S::add(J.sBb, B.part_sBb[p]); }
    return BP_OK;
}
// The replay workers released the recordings of instances whose template was cached at that moment, so nothing this block refers to
// may leave the cache before its lookups are through: vfy_resolve_templates trims once, before them, and never an entry the block
// uses.  (A miss therefore means the template was not cached during the replay either, and the worker kept that instance's recording:
// inst.cs is null only for a template that is found.)
template <class C> static int vfy_block_templates(VfyHostJob<C>& J, VfyHostBlock<C>& B) {
    BPCHK((vfy_resolve_templates<C>(J.ctx, B.nb, [&B](size_t p) -> VfyReplayed<C>& { return B.rep[p]; }, "batch_verify", &B.uniform)));
    J.mark("  block: templates");
    return BP_OK;
}
// Groups — same template, same kind of coefficient table; instance order inside a group — and everything the block enqueues: parameter
// blocks, launch order and own tables up on the main stream, their import, one k_vfy_tables / k_vfy_batch chain per group, the tails
// up on the aux stream, the two events that free the staging half
template <class C> static int vfy_block_launch(VfyHostJob<C>& J, VfyHostBlock<C>& B) {
    typedef typename C::Fr FrP;
    bp_ctx* ctx = J.ctx;
    hipStream_t st = ctx->stream;
    const size_t nb = B.nb;
    const std::vector<VfyReplayed<C>>& rep = B.rep;
    auto same = [&rep](u32 x, u32 y) { return rep[x].tm == rep[y].tm && rep[x].own_tab == rep[y].own_tab; };
    std::vector<u32> order(nb);
    for (size_t p = 0; p < nb; p++) order[p] = (u32)p;
    if (!B.uniform) std::stable_sort(order.begin(), order.end(), [&rep](u32 x, u32 y) { return rep[x].tm != rep[y].tm ? std::less<const void*>()(rep[x].tm, rep[y].tm) : rep[x].own_tab < rep[y].own_tab; });
    size_t coef_scalars = 0;
    for (size_t p = 0; p < nb; p++) if (rep[p].own_tab) coef_scalars += rep[p].tm->ncoef;
    BPCHK(vfy_aux_ensure(ctx, B.half, B.bytes_perm + coef_scalars * 32));
    u32* st_perm = (u32*)ctx->h_vaux[B.half];
    F4* st_coef = (F4*)((char*)st_perm + B.bytes_perm);
    memcpy(st_perm, order.data(), nb * 4);
    size_t at = 0;
    for (size_t j = 0; j < nb; j++) { const VfyReplayed<C>& r = rep[order[j]]; if (r.own_tab) { memcpy(st_coef + at, r.vp.coef_ptr, r.tm->ncoef * 32); at += r.tm->ncoef; } }
    BPCHK(ctx->v_params.ensure(B.bytes_pb + B.bytes_perm + coef_scalars * 32 + 64));
    u32* d_pb = ctx->v_params.as<u32>();
    u32* d_perm = d_pb + nb * VFY_PB_WORDS;
    u32* d_coef = d_perm + B.bytes_perm / 4;
    HIPCHK(hipMemcpyAsync(d_pb, B.st_pb, B.bytes_pb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_perm, st_perm, B.bytes_perm + coef_scalars * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((nb * VFY_PB_SCALARS + 255) / 256)), dim3(256), 0, st, d_pb, d_pb, (u32)(nb * VFY_PB_SCALARS));
    if (coef_scalars) hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((coef_scalars + 255) / 256)), dim3(256), 0, st, d_coef, d_coef, (u32)coef_scalars);
    size_t coef_at = 0;
    for (size_t j0 = 0, j1; j0 < nb; j0 = j1) {
        for (j1 = j0 + 1; j1 < nb && same(order[j1], order[j0]);) j1++;
        const VfyReplayed<C>& r = rep[order[j0]];
        BPCHK(verify_launch_template_group<C>(ctx, *r.tm, d_pb, d_perm + j0, r.own_tab ? d_coef + coef_at * 8 : nullptr, j1 - j0, r.vp.N, r.vp.k, J.acc_g, J.acc_h,
                                              ctx->r_small.as<u32>() + J.nslots * 8));
        if (r.own_tab) coef_at += (j1 - j0) * r.tm->ncoef;
        J.nslots++;
    }
    // the block's tails (96 B per tail term: 14.5 MB per block of cfg4) go up on the second stream: on the main stream the copy
    // would sit behind k_vfy_batch and lengthen the GPU's chain per block by ~0.6 ms; nothing reads them before the drain
    HIPCHK(hipMemcpyAsync(J.d_tail_sc + B.t_lo * 8, B.st_ts, B.bytes_ts, hipMemcpyHostToDevice, ctx->aux_stream));
    HIPCHK(hipMemcpyAsync(ctx->r_tail.as<u32>() + B.t_lo * 16, B.st_tp, B.bytes_tp, hipMemcpyHostToDevice, ctx->aux_stream));
    if (!ctx->vtail_ev[B.half]) HIPCHK(hipEventCreateWithFlags(&ctx->vtail_ev[B.half], hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->vtail_ev[B.half], ctx->aux_stream));
    HIPCHK(hipEventRecord(ctx->vstage_ev[B.half], st));
    J.mark("  block: launches");
    return BP_OK;
}
// recordings that were kept for a template build: rare, but then there may be hundreds (a new gadget's first block)
template <class C> static void vfy_block_release(VfyHostJob<C>& J, VfyHostBlock<C>& B) {
    size_t kept = 0;
    for (size_t p = 0; p < B.nb; p++) kept += B.rep[p].inst.owned_cs ? 1 : 0;
    if (kept > 8) pool_range(J.ctx, 0, B.nb, [&B](size_t p) { B.rep[p].inst.owned_cs.reset(); B.rep[p].inst.owned_tr.reset(); });
    J.mark("  block: release");
}

// ---- the failure exits ------------------------------------------------------------------------------------------------------------------
// the statuses' first error in instance order; emsg (optional): its text for g_err, for the instances from `from` on
static int vfy_first_of(const std::vector<int>& erc, const std::vector<const char*>& emsg, size_t from) {
    for (size_t k = 0; k < erc.size(); k++) if (erc[k]) { if (k >= from && emsg[k]) g_err = emsg[k]; return erc[k]; }
    return BP_OK;
}
// inst_status: instances [from, count) each on their own — framing, its points, its replay — with no GPU work but the decode
template <class C> static int vfy_report_each(VfyHostJob<C>& J, size_t from) {
    bp_ctx* ctx = J.ctx;
    const size_t count = J.count;
    if (J.decoded_upto < count) BPCHK(vfy_decode_issue<C>(J, count, 0));
    HIPCHK(hipStreamSynchronize(ctx->aux_stream));
    std::vector<int> erc(J.inst_status, J.inst_status + count);
    std::vector<const char*> emsg(count, nullptr);
    pool_range(ctx, from, count, [&](size_t k) {
        erc[k] = J.rcs[k] ? J.rcs[k] : vfy_decode_check<C>(J, k, k + 1);
        if (erc[k]) return;
        VfyReplayed<C> r;
        erc[k] = vfy_replay_one<C>(ctx, J.prov, k, J.lps[k], J.all_pts + J.xoff[k], r); emsg[k] = r.vp.err;
        if (!erc[k] && vfy_claim_bad(J.lps[k].k, ctx->gens_cap)) erc[k] = BP_E_VERIFICATION;   // (not reached: a doomed instance fails its own replay)
    });
    std::copy(erc.begin() + from, erc.end(), J.inst_status + from);
    return vfy_first_of(erc, emsg, from);
}
// The call's error without inst_status.  Precedence, as in the reference: it decodes EVERY proof before batch_verify runs, so every
// FormatError (framing, an x off the curve) comes before any error of the replay, and a malformed LATER proof wins over an earlier
// instance's VerificationError; within one kind the first in instance order.  Framing errors returned before the first block; the
// blocks stop at the first failing one, so what is left to look at here are the points of the blocks after it.
template <class C> static int vfy_first_error(VfyHostJob<C>& J, int first_err) {
    bp_ctx* ctx = J.ctx;
    if (first_err == BP_E_FORMAT) { (void)hipStreamSynchronize(ctx->aux_stream); return first_err; }
    if (J.decoded_upto < J.count) BPCHK(vfy_decode_issue<C>(J, J.count, 0));
    HIPCHK(hipStreamSynchronize(ctx->aux_stream));
    return vfy_decode_check<C>(J, 0, J.count) ? BP_E_FORMAT : first_err;
}
// a doomed batch without inst_status: every instance replayed, no GPU work, the first error in instance order
template <class C> static int vfy_doomed_error(VfyHostJob<C>& J) {
    std::vector<int> erc(J.count, BP_OK);
    std::vector<const char*> emsg(J.count, nullptr);
    pool_range(J.ctx, 0, J.count, [&](size_t k) { VfyReplayed<C> r; erc[k] = vfy_replay_one<C>(J.ctx, J.prov, k, J.lps[k], J.all_pts + J.xoff[k], r); emsg[k] = r.vp.err; });
    const int rc = vfy_first_of(erc, emsg, 0);
    return rc ? rc : BP_E_VERIFICATION;   // (not reached: a doomed instance fails its own replay)
}

// ---- the host path's own drain before the mega-check ------------------------------------------------------------------------------
// tails: alpha-scaling + canonical form on the GPU; points to the resident layout; accumulators to canonical integers; the groups'
// deltas back and into sB
template <class C> static int vfy_host_drain(VfyHostJob<C>& J) {
    typedef typename C::Fr FrP;
    bp_ctx* ctx = J.ctx;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx_aux_stream_wait(ctx));   // every block's tails have arrived (the main stream's kernels below read them)
    if (J.Ttot) {
        hipLaunchKernelGGL(k_vfy_tail_scale<FrP>, dim3((u32)((J.Ttot + 255) / 256)), dim3(256), 0, st, J.d_tail_sc, J.d_alpha, J.d_toff, (u32)J.count, (u32)J.Ttot);
        BPCHK(bp_points_import(ctx, ctx->r_tail.p, ctx->r_tail.p, J.Ttot));
    }
    hipLaunchKernelGGL(k_scalars_to_canon<FrP>, dim3((u32)((2 * J.maxN + 255) / 256)), dim3(256), 0, st, J.sc + 2 * 8, (u32)(2 * J.maxN));
    std::vector<F4> deltas(std::max<size_t>(J.nslots, 1));
    if (J.nslots) HIPCHK(hipMemcpyAsync(deltas.data(), ctx->r_small.p, J.nslots * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    for (size_t j = 0; j < J.nslots; j++) J.sB = host::Fld<FrP>::add(J.sB, deltas[j]);   // sum_p alpha_p * r_p * x_p^2 * (wc_p + delta_p) of the groups
    return BP_OK;
}

// inst_status (count ints, optional; bp_r1cs_batch_verify_locate): the call then does not stop at the first instance that fails
// before the mega-check (framing, decompression, verify_prepare).  EVERY such instance of the batch gets its own status — what a
// batch of that instance alone returns — the others stay BP_OK, and the call returns the first of them in instance order without
// a mega-check verdict.  When no instance fails that way the statuses are all BP_OK and the return value is the mega-check's.
//
// checked (optional): set when the call reached its mega-check, i.e. no instance failed before it.
template <class C>
static int batch_verify_host(bp_ctx* ctx, size_t count, const VfyProvider<C>& prov, const uint8_t* proofs, const size_t* poff /* count + 1 */, const F4* alphas,
                             double* timing, uint64_t* point_out, int* inst_status, bool* checked) {
    const double t_entry = now_s();
    if (checked) *checked = false;
    if (point_out) memset(point_out, 0, 64);   // every early exit leaves a defined (identity) check point
    if (inst_status) std::fill(inst_status, inst_status + count, BP_OK);
    VfyHostJob<C> J{ctx, prov, count, proofs, poff, alphas, inst_status, VfyMark{"vfy", t_entry}};
    host_pool_ensure(ctx, count);
    std::vector<int> pst;
    BPCHK(vfy_parse<C>(ctx, prov, count, proofs, poff, pst, J.lps, J.rcs));
    for (size_t k = 0; k < count; k++) if (pst[k]) {   // a rejected encoding is reported before anything the proof bytes would give
        if (inst_status) std::copy(pst.begin(), pst.end(), inst_status);
        g_err = "batch_verify: a commitment's encoding was rejected";
        return pst[k];
    }
    for (size_t k = 0; k < count; k++) if (J.rcs[k]) {
        if (!inst_status) return J.rcs[k];
        J.lps[k].xs.clear(); J.lps[k].flags.clear(); J.lps[k].k = (size_t)-1;   // no points of its own; it dooms the batch below
    }
    J.xoff = vfy_xoff(J.lps, nullptr, count);
    BPCHK(vfy_decode_arena<C>(J));
    vfy_gather(ctx, J.lps, nullptr, count, J.xoff, J.all_x, J.all_f);
    J.mark("parse + gather x");
    vfy_layout<C>(J);
    const size_t first_hi = J.doomed ? count : std::min(count, VFY_BLOCK);   // a doomed batch has no blocks: all of it at once
    BPCHK(vfy_decode_issue<C>(J, first_hi, 0));
    HIPCHK(event_wait(ctx, ctx->dec_ev[0]));
    const int frc0 = vfy_decode_check<C>(J, 0, first_hi);
    if (frc0 && !inst_status) return frc0;
    J.mark("gpu decompress (first block)");
    if (timing) timing[4] = now_s() - t_entry;
    if (inst_status && (J.doomed || frc0)) return vfy_report_each<C>(J, 0);
    if (J.doomed) return vfy_doomed_error<C>(J);
    BPCHK(vfy_reserve<C>(J));
    J.mark("layout + alphas");
    int first_err = BP_OK;
    size_t err_from = 0;   // inst_status: the instances from here on have no status yet when first_err stops the blocks
    for (size_t lo = 0; lo < count && !first_err; lo += VFY_BLOCK) {
        VfyHostBlock<C> B;
        BPCHK(vfy_block_open<C>(J, B, lo, first_err));
        if (first_err) { err_from = lo; break; }
        vfy_replay_block<C>(J, B);
        if (ctx->host_only) vfy_dry_fold<C>(J, B);
        if ((first_err = vfy_block_settle<C>(J, B))) { err_from = B.hi; break; }
        BPCHK(vfy_block_templates<C>(J, B));
        BPCHK(vfy_block_launch<C>(J, B));
        vfy_block_release<C>(J, B);
    }
    if (first_err) {
        (void)hipStreamSynchronize(ctx->stream);
        return inst_status ? vfy_report_each<C>(J, err_from) : vfy_first_error<C>(J, first_err);   // (the blocks before err_from passed their replay)
    }
    if (checked) *checked = true;
    if (ctx->host_only) {   // dry run: no mega-check; the checksum of everything the host staged comes back in the check point's words
        if (point_out) { memset(point_out, 0, 64); point_out[0] = J.dry_sum; point_out[1] = count; point_out[2] = J.nslots; }
        if (timing) { timing[0] = now_s() - t_entry; timing[1] = J.host_busy; }
        return BP_OK;
    }
    const double t_drain = now_s();
    BPCHK(vfy_host_drain<C>(J));
    J.mark("pipeline (replay | k_vfy_batch)");
    const double t_msm = now_s();
    J4 r;
    BPCHK(vfy_mega_check<C>(ctx, J.maxN, J.Ttot, J.sB, J.sBb, r));
    if (point_out) aff_out<C>(point_out, host::Grp<C>::to_aff(r));
    J.mark("mega-check msm");
    const double t_end = now_s();
    if (timing) { timing[0] = t_end - t_entry; timing[1] = J.host_busy; timing[2] = t_msm - t_drain; timing[3] = t_end - t_msm; }
    if (ctx->profiling) collect_timers(ctx);
    return host::Grp<C>::is_inf(r) ? BP_OK : BP_E_VERIFICATION;  // `mega_check.is_zero()` (verifier.rs:595)
}
