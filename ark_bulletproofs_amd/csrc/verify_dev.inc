// batch_verify with the per-proof front end on the GPU, as steps over VfyDevJob: one class of like-instances of one recording
// (included by r1cs_host.inc).  The host does NOT replay transcripts: it stages the proofs' bytes, the commitments and the transcript
// states in pinned memory and enqueues k_vfe_points -> k_vfe_sponge -> k_vfe_consts / k_vfe_wv / k_vfe_sum2 (vfe.hip) -> per block of
// 512: k_vfy_tables, k_vfy_batch -> the mega-check MSM on the ctx's stream; one wait at the end.  The challenges are derived on the
// device (Keccak-f / STROBE schedule / ChaCha20 / Fr::rand), the decompressed points never leave it.  batch_verify_device runs ONE
// job that is the whole batch, batch_verify_classes several, which share the g / h accumulators, the tail array, the wait and the
// MSM.  Every size, offset and shape rule is vfy_dev_plan.hpp's.  The steps (vfy_dev_run is all but the first):
//   vfy_dev_admit    shape, state, (two-phase) vfy_dev_rehearse, template, vfy_dev_class_consts / vfy_dev_sched2; may wait for an upload
//   vfy_dev_place    where each job lives (the header);  vfy_dev_reserve: every buffer at its final size, the zeroing
//   vfy_dev_launch   per job: vfy_dev_stage -> vfy_dev_front -> vfy_dev_blocks_single / vfy_dev_blocks_two
//   vfy_dev_finish   ONE wait, the head scalars, ONE MSM;  vfy_dev_flagged: the instances the kernels flagged
// Every way out that is not "done" leaves the batch to the host replay — of the flagged instances alone where the kernels named them
// (vfy_replay_flagged) —, which reports the reference's error in instance order.  The exits and what each counts:
//   vfy_dev_admit         route off, no recording, empty class; two-phase without BP_TUNE_VFY_DEVICE = 2; a recording with own
//                         constraints; any VfyDevDecline; vfy_dev_state_ok; fewer generators than N                  nothing
//   vfy_dev_rehearse      each wire commitment of instance 0 that reaches the host                                   cw_host
//                         ... one of them, or A_I1 / A_O1 / S1, rejected                                             vfe_fallbacks
//                         callbacks that fail or record what the device cannot take; VFY_DEV_N; VFY_DEV_TABLES       nothing
//   vfy_dev_class_consts, vfy_dev_sched2    no schedule for this shape                                               nothing
//   vfy_dev_blocks_two    a kernel raised a status bit                                                               vfe_fallbacks
//                         challenges that are not instance 0's; a callback that records another structure            nothing
//   vfy_dev_finish        flagged: a kernel raised a status bit    vfe_fallbacks (classes: + vcl_calls, vcl_remainder, vcl_flagged)
//   done                  batch_verify_device: vfe_batches; batch_verify_classes: vcl_calls, vcl_remainder, vcl_classes,
//                         vcl_instances; both: cw_front_end by count * m of a wire job
template <class C> struct VfeClassDev {
    std::weak_ptr<const host::FrozenRecording> base;
    DevBuf sched, voff, vq, vc, coefs, iota;
    bool coefs_up = false;       // coefs holds this class's coefficient table (uploaded by the first batch that needs it)
    std::string tkey;            // structure digest of the template this class evaluates with
    ~VfeClassDev() { sched.release(); voff.release(); vq.release(); vc.release(); coefs.release(); iota.release(); }
};
// Two-phase batches (BP_TUNE_VFY_DEVICE = 2): what the reference instance's live randomized phase recorded.  Every other instance's
// callbacks must reproduce it with their own challenges: same labels, multipliers, constraint offsets and term variables, a +-1 where
// it has +-1, one value per coefficient id.  The coefficient ids are the canonical numbering of the whole recording (CanonState):
// [0, nbase) the shared phase-1 values, then the phase-2 ones.
template <class C> struct Vfe2Ref {
    std::vector<std::string> labels;     // gadget challenges in drawing order
    std::vector<F4> chal0;               // instance 0's, from its live transcript
    size_t n = 0, n1 = 0, nbase = 0, ncoef = 0;
    std::vector<size_t> off;             // the phase-2 part: constraint offsets (cs_off)
    std::vector<host::Var> vars;         // its terms' variables
    std::vector<u32> cid;                // its terms' coefficient ids
    std::vector<F4> base_coefs;          // ids [0, nbase)
};
// An event on the ctx's stream, polled with sleeps (HIP's own synchronisation busy-waits on this stack; see event_wait)
static hipError_t vfe_poll(bp_ctx* ctx, hipEvent_t ev) {
    wait_thread_setup();
    const long ns = 1000L * (ctx->tune_wait_sleep ? (long)ctx->tune_wait_sleep : 100L);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        struct timespec ts = {0, ns};
        nanosleep(&ts, nullptr);
    }
}
struct VfyDrain { bp_ctx* c; bool armed; ~VfyDrain() { if (armed) (void)hipStreamSynchronize(c->stream); } };   // the stream reads pinned memory of this call: a decline waits for it first
// Pinned memory the stream may still be reading: wait before it is freed.  cap >= least keeps it; else `alloc` bytes (the site's rule).
static int vfy_pinned_grow(bp_ctx* ctx, void*& p, size_t& cap, size_t least, size_t alloc) {
    if (cap >= least) return BP_OK;
    if (p) { HIPCHK(ctx_stream_wait(ctx)); HIPCHK(hipHostFree(p)); }
    p = nullptr; cap = 0;
    HIPCHK(hipHostMalloc(&p, alloc));
    cap = alloc;
    return BP_OK;
}
template <class C> struct VfyDevJob {
    typedef host::ConstraintSystem<C> CS;
    // the class: member j is instance idx[j] of the call's proofs / poff / alphas (idx null: j itself); db's accessors take j
    size_t count = 0;
    VfyDevBatch<C> db;
    const uint32_t* idx = nullptr;
    size_t at(size_t j) const { return idx ? idx[j] : j; }
    // shape and constants (vfy_dev_admit)
    VfyDevShape sh;
    bool two = false, own_coefs = false;
    size_t n = 0;
    const host::Strobe* s0 = nullptr;
    double t_entry = 0;
    CS like;
    host::CanonState scratch;
    host::Digest dg;
    Vfe2Ref<C> ref;
    std::vector<u32> v2off, v2q, v2cid;   // two-phase: the terms on commitments by commitment (CSR), coefficient ids
    std::shared_ptr<void> tkeep, ckeep;   // the template and the class constants stay alive until the call's wait
    const VTemplate<C>& tmpl() const { return *(const VTemplate<C>*)tkeep.get(); }
    const u32 *d_sched = nullptr, *d_voff = nullptr, *d_vq = nullptr, *d_vc = nullptr, *d_iota = nullptr;
    VfyDevPlace pl;                       // placement (vfy_dev_place)
};
static bool vfy_device_on(const bp_ctx* ctx) {
    static const bool off = getenv("ARKBP_VFY_HOST") != nullptr;   // A/B switch: the host replay for every batch
    return !off && !ctx->host_only && ctx->tune_vfy_device && ctx->shard_world <= 1;
}
// Terms on committed variables by commitment (CSR over j; constraint order inside a commitment): per term its constraint and a payload
template <class P, class F>
static void vfy_dev_csr(const std::vector<host::VTerm>& vts, size_t m, std::vector<u32>& off, std::vector<u32>& q, std::vector<P>& pay, F payload) {
    off.assign(m + 1, 0); q.resize(vts.size()); pay.resize(vts.size());
    for (const auto& v : vts) off[v.j + 1]++;
    for (size_t j = 0; j < m; j++) off[j + 1] += off[j];
    std::vector<u32> cur(off.begin(), off.end() - 1);
    for (const auto& v : vts) { const u32 at = cur[v.j]++; q[at] = v.q; pay[at] = payload(v); }
}
static const std::vector<u32>& vfy_dev_iota() {   // a block's launch order when every instance is in it: 0 .. VFY_BLOCK
    static const std::vector<u32> iota = [] { std::vector<u32> v(VFY_BLOCK); for (size_t i = 0; i < VFY_BLOCK; i++) v[i] = (u32)i; return v; }();
    return iota;
}
// the circuit template of `rec` (constraint matrices on the GPU, keyed by structure): looked up, or built (upload + sync)
template <class C> static int vfy_dev_template(bp_ctx* ctx, VfyDevJob<C>& J, const host::ConstraintSystem<C>& rec, const host::CanonState& cst) {
    J.dg = cst.digest(rec.n1, J.n, rec.num_constraints());
    // a miss with a full cache: the one template this batch needs is the one that is missing, so everything leaves
    if (ctx->templates.size() >= VFY_TEMPLATE_CACHE && !ctx->templates.count(vfy_template_key(J.dg))) BPCHK(vfy_templates_trim(ctx, {}));
    const VTemplate<C>* T;
    return vfy_template_get<C>(ctx, J.dg, &rec, J.n, rec.n1, rec.num_constraints(), cst.coefs.size(), "batch_verify", J.tkeep, T);
}
// instance 0's transcript through S1 (verifier.rs:403-415): a copy of its state, its commitments, the proof's first three points
template <class C> static bool vfy_dev_transcript0(bp_ctx* ctx, const VfyDevJob<C>& J, const uint8_t* proof0, host::Transcript& t0) {
    const VfyDevBatch<C>& db = J.db;
    t0.s = *J.s0;
    if (db.absorb_commitments) for (size_t j = 0; j < J.sh.m; j++) {
        A4 v;
        if (!J.sh.wire) memcpy(&v, db.commit_xy(0) + 8 * j, 64);
        else {   // instance 0's own m roots on the host: the rehearsal needs them in affine form (m per batch, not m x count)
            ctx->cw_host++;
            if (!host::Grp<C>::deser_compressed(v, db.commit_wire(0) + 33 * j)) return false;   // the prologue names the instance
        }
        host::TP<C>::append_point(t0, "V", v);
    }
    t0.append_u64("m", J.sh.m);
    static const char* const lab3[3] = {"A_I1", "A_O1", "S1"};
    for (int j = 0; j < 3; j++) {
        A4 p;
        if (!host::Grp<C>::deser_compressed(p, proof0 + 33 * j) || !host::TP<C>::validate_and_append_point(t0, lab3[j], p)) return false;
    }
    return true;
}
// What r0's randomized phase recorded, as J.ref and the CSR of its terms on commitments: coefficient ids from the canonical walk over
// both parts (the numbering canonical() and build_template produce).  false: ids or commitments out of range.
template <class C> static bool vfy_dev_ref_ids(VfyDevJob<C>& J, const host::ConstraintSystem<C>& r0) {
    typedef host::Fld<typename C::Fr> S;
    const host::ConstraintSystem<C>& src = *J.db.src;
    Vfe2Ref<C>& ref = J.ref;
    const F4 one = S::one(), mone = S::neg(S::one());
    ref.n = J.n; ref.n1 = r0.n1;
    ref.off = r0.cs_off;
    host::CanonState cw;
    std::vector<host::VTerm> vts;   // (j, q, c.v[0] = id)
    auto vsink = [&](size_t q, const host::Term& t, u32 cid) { if (t.v.k == host::VK_COMMITTED) { host::VTerm v{t.v.i, (u32)q, F4{}}; v.c.v[0] = cid; vts.push_back(v); } };
    cw.walk(src.base->terms.data(), src.base->off.data(), src.base->nq(), 0, one, mone, vsink);
    ref.nbase = cw.coefs.size(); ref.base_coefs = cw.coefs;
    cw.walk(r0.cs_terms.data(), r0.cs_off.data(), r0.cs_off.size() - 1, r0.base_nq(), one, mone, [&](size_t q, const host::Term& t, u32 cid) {
        ref.vars.push_back(t.v); ref.cid.push_back(cid); vsink(q, t, cid);
    });
    ref.ncoef = cw.coefs.size();
    for (u32 c : ref.cid) if (!(c & (host::CID_ONE | host::CID_MONE)) && c >= (1u << 30)) return false;
    for (const auto& v : vts) if (v.j >= J.sh.m) return false;
    vfy_dev_csr(vts, J.sh.m, J.v2off, J.v2q, J.v2cid, [](const host::VTerm& v) { return (u32)v.c.v[0]; });
    return true;
}
// Two-phase: the reference instance.  Instance 0's randomized phase for real, on a copy of its transcript; fills J.ref, J.n, the
// shape's N / G / ncoef and the template.  r0 is left as it was found.
template <class C> static int vfy_dev_rehearse(bp_ctx* ctx, VfyDevJob<C>& J, const uint8_t* proofs, const size_t* poff, bool& ok) {
    typedef host::ConstraintSystem<C> CS;
    ok = false;
    host::Transcript t0;
    if (!vfy_dev_transcript0<C>(ctx, J, proofs + poff[J.at(0)], t0)) { ctx->vfe_fallbacks++; return BP_OK; }   // something the reference rejects: the host replay reports it
    CS* r0 = J.db.cs_of ? J.db.cs_of(0) : &J.like;
    typename CS::RandSnap snap0;
    r0->snapshot(snap0);
    host::Transcript* tr_save = r0->tr;
    std::vector<std::pair<std::string, F4>> log;
    r0->tr = &t0; r0->chal_log = &log;
    const int rrc = r0->run_randomized();
    r0->chal_log = nullptr; r0->tr = tr_save;
    ok = !rrc && r0->cs_off.size() >= 1 && r0->n1 == J.db.src->base->num_vars && log.size() <= 4096;
    if (ok) {
        J.n = r0->num_vars;
        ok = !vfy_dev_set_N(J.sh, host::next_pow2(J.n)) && ctx->gens_cap >= J.sh.N;
    }
    int trc = BP_OK;
    if (ok) {
        for (auto& e : log) { J.ref.labels.push_back(e.first); J.ref.chal0.push_back(e.second); }
        ok = vfy_dev_ref_ids<C>(J, *r0);
        if (ok) trc = vfy_dev_template<C>(ctx, J, *r0, r0->canonical(J.scratch, nullptr));
    }
    r0->restore(snap0);
    if (trc) return trc;
    if (ok) ok = !vfy_dev_set_tables(J.sh, J.ref.labels.size(), J.ref.ncoef);   // (stated in include/arkbp.h)
    return BP_OK;
}
// Single phase: the class's device-side constants — schedule, terms on commitments, iota —, cached by (recording, m, k, transcript
// position) and uploaded once; the coefficient table where this batch's public constants are not the template's.
template <class C> static int vfy_dev_class_consts(bp_ctx* ctx, VfyDevJob<C>& J, bool& ok) {
    ok = false;
    const VfyDevBatch<C>& db = J.db;
    const host::ConstraintSystem<C>& src = *db.src;
    const VfyDevShape& sh = J.sh;
    hipStream_t st = ctx->stream;
    const std::string tkey((const char*)&J.dg, sizeof J.dg);
    char ckeyb[96];
    snprintf(ckeyb, sizeof ckeyb, "%p/%zu/%zu/%u/%u/%d", (const void*)src.base.get(), sh.m, sh.k, (unsigned)J.s0->pos, (unsigned)J.s0->pos_begin, (int)db.absorb_commitments);
    const std::string ckey(ckeyb);
    auto cit = ctx->vfe_classes.find(ckey);
    if (cit != ctx->vfe_classes.end()) {
        VfeClassDev<C>* c = (VfeClassDev<C>*)cit->second.get();
        if (c->base.lock().get() == src.base.get() && c->tkey == tkey) J.ckeep = cit->second;   // (same recording still alive, same template)
        else ctx->vfe_classes.erase(cit);
    }
    if (!J.ckeep) {
        if (ctx->vfe_classes.size() >= 16) { HIPCHK(ctx_stream_wait(ctx)); ctx->vfe_classes.clear(); }
        VfeClassDev<C>* c = new VfeClassDev<C>();
        J.ckeep.reset(c, [](void* q) { delete (VfeClassDev<C>*)q; });
        c->base = src.base; c->tkey = tkey;
        vfe::Schedule sched;
        if (!vfe::build_verifier_schedule(sched, J.s0->pos, J.s0->pos_begin, db.absorb_commitments, sh.m, (uint32_t)sh.k, sh.N)) return BP_OK;
        const std::vector<uint32_t> enc = sched.encode();
        std::vector<u32> voff, vq;
        std::vector<F4> vc;
        vfy_dev_csr(src.base->vterms, sh.m, voff, vq, vc, [](const host::VTerm& v) { return v.c; });
        const std::vector<u32>& iota = vfy_dev_iota();
        BPCHK(c->sched.ensure(enc.size() * 4)); BPCHK(c->voff.ensure(voff.size() * 4)); BPCHK(c->vq.ensure(std::max<size_t>(vq.size(), 1) * 4));
        BPCHK(c->vc.ensure(std::max<size_t>(vc.size(), 1) * 32)); BPCHK(c->iota.ensure(iota.size() * 4));
        HIPCHK(hipMemcpyAsync(c->sched.p, enc.data(), enc.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->voff.p, voff.data(), voff.size() * 4, hipMemcpyHostToDevice, st));
        if (!vq.empty()) HIPCHK(hipMemcpyAsync(c->vq.p, vq.data(), vq.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->iota.p, iota.data(), iota.size() * 4, hipMemcpyHostToDevice, st));
        if (!vc.empty()) BPCHK(upload_scalars<C>(ctx, (u32*)c->vc.p, vc.data(), vc.size()));
        HIPCHK(ctx_stream_wait(ctx));   // (the host arrays above are locals)
        ctx->vfe_classes[ckey] = J.ckeep;
    }
    VfeClassDev<C>& cls = *(VfeClassDev<C>*)J.ckeep.get();
    // the coefficient table is decided per batch: the template may have been evicted and rebuilt since, from an instance of the
    // same structure with other public constants
    const VTemplate<C>& T = J.tmpl();
    const host::CanonState& cst = J.like.canonical(J.scratch, nullptr);
    J.own_coefs = T.ncoef && memcmp(T.coefs_host.data(), cst.coefs.data(), T.ncoef * 32) != 0;
    if (J.own_coefs && !cls.coefs_up) {
        BPCHK(cls.coefs.ensure(T.ncoef * 32)); BPCHK(upload_scalars<C>(ctx, (u32*)cls.coefs.p, cst.coefs.data(), T.ncoef));
        HIPCHK(ctx_stream_wait(ctx));
        cls.coefs_up = true;
    }
    J.d_sched = (u32*)cls.sched.p; J.d_voff = (u32*)cls.voff.p; J.d_vq = (u32*)cls.vq.p; J.d_vc = (u32*)cls.vc.p; J.d_iota = (u32*)cls.iota.p;
    ok = true;
    return BP_OK;
}
// Two-phase: this batch's schedule (its gadget labels are in it), the iota behind it, and the CSR with coefficient ids, uploaded per batch
template <class C> static int vfy_dev_sched2(bp_ctx* ctx, VfyDevJob<C>& J, bool& ok) {
    ok = false;
    hipStream_t st = ctx->stream;
    vfe::Schedule sched;
    if (!vfe::build_verifier_schedule_2phase(sched, J.s0->pos, J.s0->pos_begin, J.db.absorb_commitments, J.sh.m, (uint32_t)J.sh.k, J.sh.N, J.ref.labels)) return BP_OK;
    const std::vector<uint32_t> enc2 = sched.encode();
    const std::vector<u32>& iota = vfy_dev_iota();
    BPCHK(ctx->vfe2_sched.ensure(enc2.size() * 4 + iota.size() * 4)); BPCHK(ctx->vfe2_voff.ensure(J.v2off.size() * 4));
    BPCHK(ctx->vfe2_vq.ensure(std::max<size_t>(J.v2q.size(), 1) * 4)); BPCHK(ctx->vfe2_vcid.ensure(std::max<size_t>(J.v2cid.size(), 1) * 4));
    HIPCHK(hipMemcpyAsync(ctx->vfe2_sched.p, enc2.data(), enc2.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->vfe2_sched.as<u32>() + enc2.size(), iota.data(), iota.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->vfe2_voff.p, J.v2off.data(), J.v2off.size() * 4, hipMemcpyHostToDevice, st));
    if (!J.v2q.empty()) {
        HIPCHK(hipMemcpyAsync(ctx->vfe2_vq.p, J.v2q.data(), J.v2q.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->vfe2_vcid.p, J.v2cid.data(), J.v2cid.size() * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx_stream_wait(ctx));   // (enc2 is a local)
    J.d_sched = ctx->vfe2_sched.as<u32>(); J.d_iota = J.d_sched + enc2.size(); J.d_voff = ctx->vfe2_voff.as<u32>(); J.d_vq = ctx->vfe2_vq.as<u32>(); J.d_vc = ctx->vfe2_vcid.as<u32>();
    ok = true;
    return BP_OK;
}
// what the provider's accessors must give beyond the shape: proofs of one length, terms on commitments that exist, one form of
// commitment, every transcript present and at instance 0's position
template <class C> static bool vfy_dev_state_ok(VfyDevJob<C>& J, const size_t* poff) {
    const VfyDevBatch<C>& db = J.db;
    for (size_t i = 0; i < J.count; i++) if (poff[J.at(i) + 1] - poff[J.at(i)] != J.sh.plen) return false;
    for (const auto& vt : db.src->base->vterms) if (vt.j >= db.m) return false;           // (a weaker statement than the recorded one: BP_E_ARG there)
    if (db.commit_wire && db.commit_xy) return false;
    const host::Strobe* s0 = J.s0 = db.state_of(0);
    if (!s0) return false;
    if (!db.shared_state) for (size_t i = 1; i < J.count; i++) { const host::Strobe* si = db.state_of(i); if (!si || si->pos != s0->pos || si->pos_begin != s0->pos_begin) return false; }
    return true;
}
template <class C>
static int vfy_dev_admit(bp_ctx* ctx, VfyDevJob<C>& J, const uint8_t* proofs, const size_t* poff, bool& ok) {
    ok = false;
    const VfyDevBatch<C>& db = J.db;
    if (!vfy_device_on(ctx) || !db.src || !J.count) return BP_OK;
    const host::ConstraintSystem<C>& src = *db.src;
    J.two = !src.deferred.empty();   // randomized constraints: the device derives every challenge, the host runs the callbacks
    if (J.two && ctx->tune_vfy_device < 2) return BP_OK;
    if (!src.base || src.cs_off.size() != 1 || src.phase2 || src.num_vars != src.base->num_vars) return BP_OK;
    if (vfy_dev_shape(J.sh, poff[J.at(0) + 1] - poff[J.at(0)], J.count, db.m, db.absorb_commitments, (bool)db.commit_wire, db.shared_state)) return BP_OK;
    if (!vfy_dev_state_ok<C>(J, poff)) return BP_OK;
    J.t_entry = now_s();
    J.like.init_like(src);
    J.n = src.num_vars;
    if (!J.two) {
        J.like.n1 = J.like.num_vars;   // single phase: every multiplier is a phase-1 multiplier (run_randomized with nothing deferred)
        if (vfy_dev_set_N(J.sh, host::next_pow2(J.n)) || ctx->gens_cap < J.sh.N) return BP_OK;   // (VerificationError / InvalidGeneratorsLength: the host path's to report)
        BPCHK(vfy_dev_template<C>(ctx, J, J.like, J.like.canonical(J.scratch, nullptr)));
        return vfy_dev_class_consts<C>(ctx, J, ok);
    }
    BPCHK(vfy_dev_rehearse<C>(ctx, J, proofs, poff, ok));
    if (!ok) return BP_OK;
    return vfy_dev_sched2<C>(ctx, J, ok);
}
// every buffer of the call at its final size BEFORE the first launch (a later ensure() could move one under a running kernel), the
// accumulators, the status word and the per-proof flags zeroed
template <class C> static int vfy_dev_reserve(bp_ctx* ctx, const VfyDevTotals& tot) {
    hipStream_t st = ctx->stream;
    const VfyDevSizes z = vfy_dev_sizes(tot, VFY_PB_WORDS);
    BPCHK(vfy_pinned_grow(ctx, ctx->h_vfe, ctx->h_vfe_cap, z.stage + VFY_SMALL_BYTES, z.stage + z.stage / 8 + VFY_SMALL_BYTES));
    BPCHK(ctx->vfe_in.ensure(z.in)); BPCHK(ctx->vfe_msg.ensure(z.msg)); BPCHK(ctx->vfe_chal.ensure(z.chal)); BPCHK(ctx->vfe_ws.ensure(z.ws));
    BPCHK(ctx->vfe_small.ensure(z.small)); BPCHK(ctx->vfe_flags.ensure(z.flags));
    BPCHK(ctx->r_g.ensure(z.r_g)); BPCHK(ctx->r_tail.ensure(z.r_tail)); BPCHK(ctx->r_small.ensure(z.r_small));
    BPCHK(ctx->v_alpha.ensure(z.alpha)); BPCHK(ctx->v_params.ensure(z.params));
    if (!ctx->sync_ev) HIPCHK(hipEventCreateWithFlags(&ctx->sync_ev, hipEventDisableTiming));
    HIPCHK(hipMemsetAsync(ctx->r_g.p, 0, z.z_rg, st));
    HIPCHK(hipMemsetAsync(ctx->vfe_small.p, 0, z.z_small, st));
    HIPCHK(hipMemsetAsync(ctx->vfe_flags.p, 0, z.z_flags, st));
    return BP_OK;
}
// The addresses of a job in the call's buffers (J null: of the call, as a job at place zero would have them).  Every job accumulates
// into the front of the call's g / h accumulators; its tails: scalars behind the accumulators, points in r_tail.
struct VfyDevPtrs {
    u32 *sc, *acc_g, *acc_h, *tail_sc, *tail_pts, *alpha, *pb, *status, *sums, *flags, *slots, *chal, *ws, *coef;
    uint64_t* msg;
    uint8_t *in, *hs, *h_small;   // hs, h_small are pinned: the job's staging, the call's small results
};
template <class C> static VfyDevPtrs vfy_dev_ptrs(bp_ctx* ctx, const VfyDevTotals& tot, const VfyDevJob<C>* J) {
    const VfyDevPlace pl = J ? J->pl : VfyDevPlace();
    VfyDevPtrs P;
    P.sc = ctx->r_g.as<u32>(); P.acc_g = P.sc + VFY_RG_G * 8; P.acc_h = P.sc + vfy_rg_h(tot.Nmax) * 8; P.tail_sc = P.sc + (vfy_rg_tails(tot.Nmax) + pl.tail) * 8;
    P.tail_pts = ctx->r_tail.as<u32>() + pl.tail * 16;
    P.alpha = ctx->v_alpha.as<u32>() + pl.inst * 8; P.pb = ctx->v_params.as<u32>() + pl.inst * VFY_PB_WORDS; P.flags = ctx->vfe_flags.as<u32>() + pl.inst;
    P.status = ctx->vfe_small.as<u32>(); P.sums = P.status + VFY_DS_SUMS + VFY_DS_JOB * pl.cls;
    P.slots = ctx->r_small.as<u32>() + pl.blk * 8;
    P.msg = (uint64_t*)ctx->vfe_msg.p + pl.msg; P.chal = ctx->vfe_chal.as<u32>() + pl.chal * 8; P.ws = ctx->vfe_ws.as<u32>() + pl.ws * 8;
    P.coef = ctx->vfe2_coef.as<u32>();
    P.in = (uint8_t*)ctx->vfe_in.p + pl.in; P.hs = (uint8_t*)ctx->h_vfe + pl.in; P.h_small = (uint8_t*)ctx->h_vfe + ctx->h_vfe_cap - VFY_SMALL_BYTES;
    return P;
}
static vfe::Shape vfy_dev_kernel_shape(const VfyDevShape& s) {
    vfe::Shape sh;
    sh.P = (uint32_t)s.count; sh.m = (uint32_t)s.m; sh.nV = (uint32_t)s.nV; sh.k = (uint32_t)s.k; sh.plen = (uint32_t)s.plen; sh.tail = (uint32_t)s.tail;
    sh.nitems = (uint32_t)s.nitems; sh.G = (uint32_t)s.G; sh.vwire = s.wire ? 1u : 0u;
    return sh;
}
// the job's part of the pinned area filled by the pool, ONE copy up, the weights into resident form
template <class C>
static int vfy_dev_stage(bp_ctx* ctx, const VfyDevJob<C>& J, const VfyDevPtrs& P, const uint8_t* proofs, const size_t* poff, const F4* alphas, double* timing) {
    const VfyDevBatch<C>& db = J.db;
    const VfyDevShape& s = J.sh;
    const size_t count = s.count, plen = s.plen, vrow = s.m * s.vbytes, chunk = 64;
    uint8_t* hs = P.hs;
    pool_range(ctx, 0, (count + chunk - 1) / chunk, [&](size_t c) {
        const size_t lo = c * chunk, hi = std::min(count, lo + chunk);
        if (!J.idx) memcpy(hs + lo * plen, proofs + poff[lo], (hi - lo) * plen);
        for (size_t i = lo; i < hi; i++) {
            if (J.idx) { memcpy(hs + i * plen, proofs + poff[J.idx[i]], plen); memcpy(hs + s.o_alpha() + i * 32, alphas + J.idx[i], 32); }
            if (vrow) memcpy(hs + s.o_V() + i * vrow, s.wire ? (const void*)db.commit_wire(i) : (const void*)db.commit_xy(i), vrow);
            if (!db.shared_state) memcpy(hs + s.o_st() + i * 200, db.state_of(i)->st.b, 200);
        }
    });
    if (db.shared_state) memcpy(hs + s.o_st(), J.s0->st.b, 200);
    if (!J.idx) memcpy(hs + s.o_alpha(), alphas, count * 32);
    if (timing) timing[4] = now_s() - J.t_entry;
    HIPCHK(hipMemcpyAsync(P.in, hs, s.b_in, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_scalars_import<typename C::Fr>, dim3((u32)((count + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)(P.in + s.o_alpha()), P.alpha, (u32)count);
    return BP_OK;
}
// k_vfe_points, then k_vfe_sponge (two-phase: the gadget challenges once more as ark words, for the host)
template <class C> static int vfy_dev_front(bp_ctx* ctx, const VfyDevJob<C>& J, const VfyDevPtrs& P, const vfe::Shape& sh) {
    hipStream_t st = ctx->stream;
    {
        ScopedK tk(ctx, BP_K_VFE_POINTS);
        if (vfe::launch_points(C::ID, st, sh, P.in, (const u32*)(P.in + J.sh.o_V()), P.msg, P.tail_pts, P.status, P.flags)) { g_err = "k_vfe_points: launch failed"; return BP_E_HIP; }
    }
    ScopedK tk(ctx, BP_K_VFE_SPONGE);
    if (vfe::launch_sponge(C::ID, st, sh, J.d_sched, (const uint64_t*)(P.in + J.sh.o_st()), J.db.shared_state ? 0u : 25u, P.msg, P.chal, nullptr,
                           J.two ? ctx->vfe2_gch.as<u32>() : nullptr)) { g_err = "k_vfe_sponge: launch failed"; return BP_E_HIP; }
    return BP_OK;
}
// single phase: k_vfe_consts / k_vfe_wv / k_vfe_sum2 for the whole job, then k_vfy_tables / k_vfy_batch per block
template <class C> static int vfy_dev_blocks_single(bp_ctx* ctx, const VfyDevJob<C>& J, const VfyDevPtrs& P, const vfe::Shape& sh) {
    ScopedK tk(ctx, BP_K_VFE_PREPARE);
    if (vfe::launch_prepare(C::ID, ctx->stream, sh, P.in, P.chal, P.alpha, J.d_voff, J.d_vq, J.d_vc, P.pb, P.tail_sc, P.ws, P.sums)) { g_err = "k_vfe_consts: launch failed"; return BP_E_HIP; }
    VfeClassDev<C>& cls = *(VfeClassDev<C>*)J.ckeep.get();
    for (size_t blk = 0; blk < J.sh.nblocks; blk++) {
        const size_t lo = blk * VFY_BLOCK, nb = std::min(J.count, lo + VFY_BLOCK) - lo;
        BPCHK(verify_launch_template_group<C>(ctx, J.tmpl(), P.pb + lo * VFY_PB_WORDS, J.d_iota, J.own_coefs ? (u32*)cls.coefs.p : nullptr, nb, J.sh.N, J.sh.k,
                                              P.acc_g, P.acc_h, P.slots + blk * 8, true));
    }
    return BP_OK;
}
// Instance i's callbacks with the device's challenges gch[0 .. G), on its own recorder (db.cs_of) or a like-instance made for the
// purpose.  Whether it reproduced the reference structure (J.ref) and filled its table row tab[0 .. ncoef).
template <class C> static bool vfy_dev_replay_callbacks(const VfyDevJob<C>& J, size_t i, const F4* gch, F4* tab) {
    typedef host::ConstraintSystem<C> CS;
    typedef host::Fld<typename C::Fr> S;
    const Vfe2Ref<C>& ref = J.ref;
    const F4 one = S::one(), mone = S::neg(S::one());
    std::unique_ptr<CS> tmp;
    CS* ci;
    typename CS::RandSnap snap;
    if (J.db.cs_of) { ci = J.db.cs_of(i); ci->snapshot(snap); }
    else { tmp.reset(new CS()); tmp->init_like(*J.db.src); ci = tmp.get(); }
    host::Transcript sink;   // ("r1cs-2phase" is appended here: the device's sponge has absorbed it already)
    memset(&sink.s, 0, sizeof sink.s);
    host::Transcript* tr_save = ci->tr;
    ci->tr = &sink;
    ci->preset = gch; ci->preset_labels = &ref.labels; ci->preset_at = 0; ci->preset_bad = false;
    const int rc = ci->run_randomized();
    bool ok = !rc && !ci->preset_bad && ci->preset_at == J.sh.G && ci->num_vars == ref.n && ci->n1 == ref.n1 && ci->cs_off == ref.off &&
              ci->cs_terms.size() == ref.vars.size();
    if (ok) {
        std::vector<char> set(J.sh.ncoef - ref.nbase, 0);
        for (size_t j = 0; j < ref.nbase; j++) tab[j] = ref.base_coefs[j];
        for (size_t t = 0; ok && t < ref.vars.size(); t++) {
            const host::Term& tm = ci->cs_terms[t];
            const u32 cid = ref.cid[t];
            if (tm.v.k != ref.vars[t].k || tm.v.i != ref.vars[t].i) ok = false;
            else if (cid & host::CID_ONE) ok = tm.c == one;
            else if (cid & host::CID_MONE) ok = tm.c == mone;
            else if (cid < ref.nbase) ok = tm.c == tab[cid];
            else if (!set[cid - ref.nbase]) { tab[cid] = tm.c; set[cid - ref.nbase] = 1; }
            else ok = tm.c == tab[cid];
        }
        for (size_t j = 0; ok && j < set.size(); j++) ok = set[j] != 0;
    }
    ci->tr = tr_save;
    if (J.db.cs_of) ci->restore(snap);
    return ok;
}
// Two-phase: the gadget challenges (and the kernels' reject bits) come back while k_vfe_consts runs; the host then runs every
// instance's callbacks with its challenges, block by block, each block's table upload, k_vfe_wv_tab and launches behind its tables.
template <class C> static int vfy_dev_blocks_two(bp_ctx* ctx, const VfyDevJob<C>& J, const VfyDevPtrs& P, const vfe::Shape& sh, bool& ok) {
    hipStream_t st = ctx->stream;
    const size_t G = J.sh.G, ncoef = J.sh.ncoef;
    F4 *h_gch = (F4*)ctx->h_vfe2, *h_tab = h_gch + J.sh.gch();
    if (G) HIPCHK(hipMemcpyAsync(h_gch, ctx->vfe2_gch.p, J.sh.gch() * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P.h_small + VFY_HS_STATUS, P.status, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(ctx->sync_ev, st));
    {
        ScopedK tk(ctx, BP_K_VFE_PREPARE);
        if (vfe::launch_consts(C::ID, st, sh, P.in, P.chal, P.alpha, P.pb, P.tail_sc, P.ws, P.sums)) { g_err = "k_vfe_consts: launch failed"; return BP_E_HIP; }
    }
    HIPCHK(vfe_poll(ctx, ctx->sync_ev));
    u32 status0; memcpy(&status0, P.h_small + VFY_HS_STATUS, 4);
    if (status0) { ctx->vfe_fallbacks++; return BP_OK; }
    for (size_t g = 0; g < G; g++) if (h_gch[g] != J.ref.chal0[g]) return BP_OK;   // (the device's transcript is not instance 0's: never expected)
    for (size_t blk = 0; blk < J.sh.nblocks; blk++) {
        const size_t lo = blk * VFY_BLOCK, nb = std::min(J.count, lo + VFY_BLOCK) - lo;
        std::atomic<bool> bad{false};
        pool_range(ctx, lo, lo + nb, [&](size_t i) {
            if (!bad.load(std::memory_order_relaxed) && !vfy_dev_replay_callbacks<C>(J, i, h_gch + i * G, h_tab + i * ncoef)) bad.store(true, std::memory_order_relaxed);
        });
        if (bad.load()) return BP_OK;   // a callback that records another structure (or draws other challenges): the host replay decides
        u32* d_tab = P.coef + lo * ncoef * 8;
        if (ncoef) {
            HIPCHK(hipMemcpyAsync(d_tab, h_tab + lo * ncoef, nb * ncoef * 32, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_scalars_import<typename C::Fr>, dim3((u32)((nb * ncoef + 255) / 256)), dim3(256), 0, st, d_tab, d_tab, (u32)(nb * ncoef));
        }
        {
            ScopedK tk(ctx, BP_K_VFE_PREPARE);
            if (vfe::launch_wv_tab(C::ID, st, sh, (uint32_t)lo, (uint32_t)nb, P.pb, J.d_voff, J.d_vq, J.d_vc, d_tab, (uint32_t)(ncoef * 8), P.tail_sc)) {
                g_err = "k_vfe_wv_tab: launch failed"; return BP_E_HIP;
            }
        }
        BPCHK(verify_launch_template_group<C>(ctx, J.tmpl(), P.pb + lo * VFY_PB_WORDS, J.d_iota, ncoef ? d_tab : nullptr, nb, J.sh.N, J.sh.k,
                                              P.acc_g, P.acc_h, P.slots + blk * 8, false));
    }
    ok = true;
    return BP_OK;
}
// staging and the launch chain of one job.  ok stays false when a two-phase batch declines on the way (its kernels flagged something,
// a callback recorded another structure).  Two-phase: the pinned [gadget challenges | coefficient tables] (ark words, host form) and
// their device copies are sized here, before anything of the job is enqueued.
template <class C>
static int vfy_dev_launch(bp_ctx* ctx, VfyDevJob<C>& J, const VfyDevTotals& tot, const uint8_t* proofs, const size_t* poff, const F4* alphas, double* timing, bool& ok) {
    ok = false;
    const size_t b_gch = J.sh.gch() * 32, b_tab = J.sh.tab() * 32;
    if (J.two) {
        BPCHK(vfy_pinned_grow(ctx, ctx->h_vfe2, ctx->h_vfe2_cap, b_gch + b_tab + 64, b_gch + b_tab + (b_gch + b_tab) / 8 + 64));
        BPCHK(ctx->vfe2_gch.ensure(std::max<size_t>(b_gch, 32))); BPCHK(ctx->vfe2_coef.ensure(std::max<size_t>(b_tab, 32)));
    }
    const VfyDevPtrs P = vfy_dev_ptrs<C>(ctx, tot, &J);
    const vfe::Shape sh = vfy_dev_kernel_shape(J.sh);
    BPCHK(vfy_dev_stage<C>(ctx, J, P, proofs, poff, alphas, timing));
    BPCHK(vfy_dev_front<C>(ctx, J, P, sh));
    if (J.two) return vfy_dev_blocks_two<C>(ctx, J, P, sh, ok);
    BPCHK(vfy_dev_blocks_single<C>(ctx, J, P, sh));
    ok = true;
    return BP_OK;
}
// The mega-check of the host replay and of the device front end alike: the two head scalars up, then ONE MSM over
// [B, B_blinding | G[0..Nmax) | H[0..Nmax) | tails] with the scalars resident in r_g (accumulators and tails in canonical form by now)
template <class C> static int vfy_mega_check(bp_ctx* ctx, size_t Nmax, size_t Ttot, const F4& sB, const F4& sBb, J4& r) {
    u32* sc = ctx->r_g.as<u32>();
    uint64_t head[8];
    canon_words<typename C::Fr>(head, sB); canon_words<typename C::Fr>(head + 4, sBb);
    HIPCHK(hipMemcpyAsync(sc, head, 64, hipMemcpyHostToDevice, ctx->stream));
    BaseSegs sg; memset(&sg, 0, sizeof sg);
    sg.nseg = 4;
    sg.ptr[0] = ctx->d_pc.as<u32>(); sg.ptr[1] = ctx->d_G.as<u32>(); sg.ptr[2] = ctx->d_H.as<u32>(); sg.ptr[3] = ctx->r_tail.as<u32>();
    sg.start[0] = 0; sg.start[1] = (u32)VFY_RG_G; sg.start[2] = (u32)vfy_rg_h(Nmax); sg.start[3] = (u32)vfy_rg_tails(Nmax); sg.start[4] = (u32)vfy_rg_len(Nmax, Ttot);
    return msm_run<C>(ctx, sg, sc, vfy_rg_len(Nmax, Ttot), 0, r);
}
// After the last job: the accumulators to canonical integers, ONE copy back, ONE polled wait, the head scalars summed on the host,
// the mega-check over every job's tails.  flagged: a kernel raised a reject bit (no MSM then; the per-instance flag words are in
// pinned memory, vfy_dev_flagged reads them).
template <class C>
static int vfy_dev_finish(bp_ctx* ctx, VfyDevJob<C>* const* jobs, size_t nj, const VfyDevTotals& tot, VfyDrain& drain, double* timing, J4& r, bool& flagged) {
    typedef host::Fld<typename C::Fr> S;
    hipStream_t st = ctx->stream;
    flagged = false;
    const VfyDevPtrs P = vfy_dev_ptrs<C>(ctx, tot, (const VfyDevJob<C>*)nullptr);
    hipLaunchKernelGGL(k_scalars_to_canon<typename C::Fr>, dim3((u32)((2 * tot.Nmax + 255) / 256)), dim3(256), 0, st, P.acc_g, (u32)(2 * tot.Nmax));
    HIPCHK(hipMemcpyAsync(P.h_small, P.slots, tot.blocks * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P.h_small + VFY_HS_SUMS, P.sums, nj * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(P.h_small + VFY_HS_STATUS, P.status, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync((uint8_t*)ctx->h_vfe + vfy_dev_flags_at(tot), P.flags, tot.inst * 4, hipMemcpyDeviceToHost, st));
    const double t_drain = now_s();
    // ONE wait per call, ~10 ms long: poll and sleep (HIP's own synchronisation calls busy-wait on this stack: a core per batch in
    // flight for nothing; see event_wait)
    HIPCHK(hipEventRecord(ctx->sync_ev, st));
    HIPCHK(vfe_poll(ctx, ctx->sync_ev));
    drain.armed = false;
    HIPCHK(hipGetLastError());
    u32 status; memcpy(&status, P.h_small + VFY_HS_STATUS, 4);
    if (status) { flagged = true; return BP_OK; }   // something the reference rejects: the host replay decides which error, in instance order
    F4 sB = S::zero(), sBb = S::zero();
    for (size_t c = 0; c < nj; c++) { F4 a, b; memcpy(a.v, P.h_small + VFY_HS_SUMS + c * 64, 32); memcpy(b.v, P.h_small + VFY_HS_SUMS + c * 64 + 32, 32); sB = S::add(sB, a); sBb = S::add(sBb, b); }
    for (size_t j = 0; j < tot.blocks; j++) { F4 d; memcpy(d.v, P.h_small + j * 32, 32); sB = S::add(sB, d); }
    const double t_msm = now_s();
    BPCHK(vfy_mega_check<C>(ctx, tot.Nmax, tot.tail, sB, sBb, r));
    const double t_end = now_s(), t_entry = jobs[0]->t_entry;
    if (timing) { timing[0] = t_end - t_entry; timing[1] = 0; timing[2] = t_msm - t_drain; timing[3] = t_end - t_msm; }
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}
// the instances the kernels flagged (after a flagged vfy_dev_finish), as instance numbers of the call, ascending
template <class C> static void vfy_dev_flagged(bp_ctx* ctx, VfyDevJob<C>* const* jobs, size_t nj, const VfyDevTotals& tot, std::vector<uint32_t>& out) {
    const u32* fl = (const u32*)((const uint8_t*)ctx->h_vfe + vfy_dev_flags_at(tot));
    for (size_t c = 0; c < nj; c++) for (size_t j = 0; j < jobs[c]->count; j++) if (fl[jobs[c]->pl.inst + j]) out.push_back((uint32_t)jobs[c]->at(j));
    std::sort(out.begin(), out.end());
}
// The admitted jobs of one call, nj <= BP_VFY_MAX_CLASSES, through place, reserve, launch, finish.  DECLINED: a job declined on the
// way; FLAGGED: the kernels raised reject bits, on which instances is in `flagged` (optional); DONE: r is the call's check point.
enum VfyDevRun { VFY_RUN_DECLINED, VFY_RUN_FLAGGED, VFY_RUN_DONE };
template <class C>
static int vfy_dev_run(bp_ctx* ctx, VfyDevJob<C>* const* jobs, size_t nj, const uint8_t* proofs, const size_t* poff, const F4* alphas, double* timing, J4& r,
                       std::vector<uint32_t>* flagged, VfyDevRun& out) {
    out = VFY_RUN_DECLINED;
    if (!nj || nj > BP_VFY_MAX_CLASSES) { g_err = "batch_verify: device jobs of one call"; return BP_E_ARG; }
    VfyDevShape shapes[BP_VFY_MAX_CLASSES];
    VfyDevPlace places[BP_VFY_MAX_CLASSES];
    VfyDevTotals tot;
    for (size_t c = 0; c < nj; c++) shapes[c] = jobs[c]->sh;
    vfy_dev_place(shapes, nj, places, tot);
    for (size_t c = 0; c < nj; c++) jobs[c]->pl = places[c];
    VfyDrain drain{ctx, true};
    BPCHK(vfy_dev_reserve<C>(ctx, tot));
    for (size_t c = 0; c < nj; c++) {
        bool ok = false;
        BPCHK(vfy_dev_launch<C>(ctx, *jobs[c], tot, proofs, poff, alphas, nj == 1 ? timing : nullptr, ok));
        if (!ok) return BP_OK;   // (single-phase jobs do not decline on the way)
    }
    bool bad = false;
    BPCHK(vfy_dev_finish<C>(ctx, jobs, nj, tot, drain, timing, r, bad));
    if (bad && flagged) vfy_dev_flagged<C>(ctx, jobs, nj, tot, *flagged);
    out = bad ? VFY_RUN_FLAGGED : VFY_RUN_DONE;
    return BP_OK;
}
// The whole batch as one job.  flagged (optional): the instances the kernels flagged when the batch is declined for that reason.
template <class C>
static int batch_verify_device(bp_ctx* ctx, size_t count, const VfyDevBatch<C>& db, const uint8_t* proofs, const size_t* poff, const F4* alphas, double* timing,
                               uint64_t* point_out, bool& handled, std::vector<uint32_t>* flagged = nullptr) {
    handled = false;
    VfyDevJob<C> J;
    J.count = count; J.db = db;
    bool ok = false;
    BPCHK(vfy_dev_admit<C>(ctx, J, proofs, poff, ok));
    if (!ok) return BP_OK;
    VfyDevJob<C>* jobs[1] = {&J};
    J4 r;
    VfyDevRun ran;
    BPCHK(vfy_dev_run<C>(ctx, jobs, 1, proofs, poff, alphas, timing, r, flagged, ran));
    if (ran == VFY_RUN_FLAGGED) ctx->vfe_fallbacks++;
    if (ran != VFY_RUN_DONE) return BP_OK;
    if (point_out) aff_out<C>(point_out, host::Grp<C>::to_aff(r));
    ctx->vfe_batches++;
    if (J.sh.wire) ctx->cw_front_end += count * J.sh.m;
    handled = true;
    return host::Grp<C>::is_inf(r) ? BP_OK : BP_E_VERIFICATION;
}
