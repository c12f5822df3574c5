// Included by arkbp.hip after r1cs_host.inc.  bp_prover_prove_batch: many statements in one call, the inner-product arguments of
// like-sized small statements in LOCKSTEP groups (small_batch.cuh).
//
// Every instance runs r1cs_prove up to its inner-product argument (commitments, randomized phase, flatten, t(x), evaluations — on the
// ctx's single-proof workspaces, one instance after the other, as bp_prover_prove would).  An instance whose argument runs over the
// direct window tables then hands a, b and its factor vectors to the open group of its padded size N (IpaDefer) instead of running
// lg N rounds of its own.  A group runs when it is full, when an instance of another size needs the arena, or at the end of the
// call: per round ONE upload of the descriptors and challenges, k_dt_round_multi, k_dt_accum_multi (+ k_dt_finish), ONE copy back and
// ONE host wait for every proof of the group; the transcript steps of all proofs run on the ctx's host pool.  L, R, a and b are the
// values the single-proof schedule computes, so every byte of every proof is.

static constexpr size_t PB_ARENA_BUDGET = (size_t)256 << 20;   // device bytes of one group's arena (BP_TUNE_PROVE_BATCH = 0)
static constexpr size_t PB_GROUP_MAX = 16384;                   // (2 x B table sums per launch: grid.y stays below 65536)

static size_t pb_align(size_t x) { return (x + 255) & ~(size_t)255; }
static size_t pb_lg(size_t x) { size_t k = 0; while (((size_t)1 << k) < x) k++; return k; }
// bytes of a serialised proof with `lg` rounds (host_proto.hpp::proof_to_bytes: 11 points, 3 scalars, two length-prefixed vectors, a, b)
static size_t pb_proof_len(size_t lg) { return 11 * 33 + 3 * 32 + 2 * (8 + 33 * lg) + 2 * 32; }

// arena layout of a group of `cap` proofs of padded size N
struct PbLayout {
    size_t N = 0, cap = 0, gf = 0, nblk = 0;
    size_t per_vec = 0, o_b = 0, o_a2 = 0, o_b2 = 0, o_cG = 0, o_cH = 0, o_sL = 0, o_sR = 0, o_part = 0;   // one proof's vectors
    size_t vec_end = 0, cnt_off = 0, desc_off = 0, jobs_off = 0, acc_off = 0, res_off = 0, ab_off = 0, total = 0;   // the arena
    size_t stage_bytes = 0, stage_res = 0, stage_ab = 0;   // the pinned staging: [descriptors | jobs], results, a / b
    void make(size_t N_, size_t cap_) {
        N = N_; cap = cap_;
        gf = (N + 255) / 256;
        const size_t units = (N + 1) * DT_UNITS_PER_TERM;   // a round's table sums: N / 2 of G, N / 2 of H, c * w of B
        nblk = std::max<size_t>(1, (units + 63) / 64);
        if (nblk * 2 * cap > 256) nblk = std::max<size_t>(1, std::min<size_t>(1024, (units + 127) / 128));
        o_b = pb_align(N * 32); o_a2 = o_b + pb_align(N * 32); o_b2 = o_a2 + pb_align(N * 16); o_cG = o_b2 + pb_align(N * 16);
        o_cH = o_cG + pb_align(N * 32); o_sL = o_cH + pb_align(N * 32); o_sR = o_sL + pb_align((2 * N + 2) * 32);
        o_part = o_sR + pb_align((2 * N + 2) * 32); per_vec = o_part + pb_align((gf + 1) * 64);
        vec_end = per_vec * cap;
        cnt_off = vec_end; desc_off = cnt_off + pb_align(cap * 64);   // (counters: 64 bytes = 16 words per proof, DtRoundGeom)
        jobs_off = desc_off + cap * sizeof(DtRoundDesc);
        acc_off = pb_align(jobs_off + 2 * cap * sizeof(DtJob));
        res_off = acc_off + pb_align(2 * cap * nblk * 96);
        ab_off = res_off + pb_align(2 * cap * 96);
        total = ab_off + pb_align(cap * 64);
        stage_res = pb_align(cap * sizeof(DtRoundDesc) + 2 * cap * sizeof(DtJob));
        stage_ab = stage_res + pb_align(2 * cap * 96);
        stage_bytes = stage_ab + pb_align(cap * 64);
    }
    static size_t per_proof(size_t N) { PbLayout l; l.make(N, 1); return l.total; }
};

template <class C> struct PbMember {
    size_t k;                 // instance index in the call
    host::Transcript* tr;
    host::ProofData* pf;
    F4 w;
};
template <class C> struct PbGroup {
    PbLayout lay;
    std::vector<PbMember<C>> mem;
    bool open = false;
};

// Montgomery's trick over a chunk: affine forms of `count` Jacobian points with one field inversion (the identity stays (0, 0))
template <class C> static void pb_to_aff(const J4* in, size_t count, A4* out) {
    typedef host::Grp<C> G;
    typedef host::Fld<typename C::Fq> F;
    std::vector<F4> pref(count);
    F4 run = F::one();
    for (size_t i = 0; i < count; i++) { pref[i] = run; if (!G::is_inf(in[i])) run = F::mul(run, in[i].Z); }
    F4 inv = F::inv(run);
    for (size_t i = count; i-- > 0;) {
        if (G::is_inf(in[i])) { out[i] = G::aff_inf(); continue; }
        const F4 zi = F::mul(inv, pref[i]), zi2 = F::sqr(zi);
        inv = F::mul(inv, in[i].Z);
        out[i] = A4{F::mul(in[i].X, zi2), F::mul(in[i].Y, F::mul(zi2, zi))};
    }
}
template <class S> static void pb_inv_many(const F4* in, size_t count, F4* out) {   // (challenges are never zero)
    std::vector<F4> pref(count);
    F4 run = S::one();
    for (size_t i = 0; i < count; i++) { pref[i] = run; run = S::mul(run, in[i]); }
    F4 inv = S::inv(run);
    for (size_t i = count; i-- > 0;) { out[i] = S::mul(inv, pref[i]); inv = S::mul(inv, in[i]); }
}

// the lg N rounds of every member's inner-product argument, then a and b.  On success the members' proofs are complete.
template <class C> static int pb_run_group(bp_ctx* ctx, PbGroup<C>& g) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    typedef host::TP<C> TP;
    const PbLayout& L = g.lay;
    const size_t B = g.mem.size(), N = L.N, lg = pb_lg(N);
    hipStream_t st = ctx->stream;
    char* ar = (char*)ctx->pb_arena.p;
    char* hs = (char*)ctx->h_pb;
    DtRoundDesc* hd = (DtRoundDesc*)hs;
    DtJob* hj = (DtJob*)(hs + B * sizeof(DtRoundDesc));
    const DtRoundDesc* d_desc = (const DtRoundDesc*)(ar + L.desc_off);
    const DtJob* d_jobs = (const DtJob*)(ar + L.desc_off + B * sizeof(DtRoundDesc));
    u32* d_acc = (u32*)(ar + L.acc_off);
    u32* d_res = (u32*)(ar + L.res_off);
    u32* d_ab = (u32*)(ar + L.ab_off);
    auto vec = [&](size_t j, size_t off) { return (u32*)(ar + j * L.per_vec + off); };
    // every member's vectors at the same offsets of its slice; the current / other buffer pair of a and b swap for all at once
    DtRoundGeom geo;
    geo.arena = ar; geo.counters = (u32*)(ar + L.cnt_off); geo.per_proof = L.per_vec;
    geo.a_in = 0; geo.b_in = (u32)L.o_b; geo.a_out = (u32)L.o_a2; geo.b_out = (u32)L.o_b2;
    geo.cG = (u32)L.o_cG; geo.cH = (u32)L.o_cH; geo.sL = (u32)L.o_sL; geo.sR = (u32)L.o_sR; geo.partials = (u32)L.o_part;
    std::vector<F4> u(B, S::zero()), ui(B, S::zero());
    std::vector<J4> pts(2 * B);
    std::vector<A4> aff(2 * B);
    // the per-proof ticket counters start every group at zero (an aborted launch of an earlier call cannot leave one behind)
    HIPCHK(hipMemsetAsync(ar + L.cnt_off, 0, B * 64, st));
    if (!ctx->pool && B > 1) ctx->pool.reset(new host::HostPool(std::max(1u, ctx->tune_host_threads ? (unsigned)ctx->tune_host_threads : host::host_pool_threads()) - 1));
    const size_t chunk = 64, nchunks = (B + chunk - 1) / chunk;
    auto on_pool = [&](const std::function<void(size_t)>& fn) {
        if (!ctx->pool || nchunks == 1) { for (size_t c = 0; c < nchunks; c++) fn(c); return; }
        ctx->pool->run(0, nchunks, fn);
    };
    auto fill_desc = [&](size_t j, bool fold) {
        DtRoundDesc& d = hd[j];
        if (fold) { memcpy(d.u, u[j].v, 32); memcpy(d.ui, ui[j].v, 32); } else { memset(d.u, 0, 32); memset(d.ui, 0, 32); }
        memcpy(d.qw, g.mem[j].w.v, 32);
    };
    const double t_begin = now_s();
    for (size_t r = 0; r < lg; r++) {
        const size_t n = N >> (r + 1);
        const bool fold = r > 0;
        for (size_t j = 0; j < B; j++) {
            fill_desc(j, fold);
            for (int o = 0; o < 2; o++) {   // L and R: the same runs as ipa_round_lr's direct path
                DtJob& jb = hj[2 * j + o];
                memset(&jb, 0, sizeof jb);
                const u32* sc = vec(j, o ? L.o_sR : L.o_sL);
                jb.nseg = 3; jb.terms = (u32)(N + 1);
                jb.seg[0] = DtSeg{sc, dt_base_G(ctx, 0), (u32)(N / 2), 0, (u32)n, o == 0 ? 1u : 0u};
                jb.seg[1] = DtSeg{sc + N * 8, dt_base_H(ctx, 0), (u32)(N / 2), 0, (u32)n, o == 0 ? 0u : 1u};
                jb.seg[2] = DtSeg{sc + (2 * N + 1) * 8, dt_base_pc(0), 1, 0, 0, 0};
            }
        }
        HIPCHK(hipMemcpyAsync(ar + L.desc_off, hs, B * sizeof(DtRoundDesc) + 2 * B * sizeof(DtJob), hipMemcpyHostToDevice, st));
        {
            ScopedK tk(ctx, BP_K_IPA_SCALARS);
            hipLaunchKernelGGL(k_dt_round_multi<C>, dim3((u32)L.gf, (u32)B), dim3(256), 0, st, d_desc, geo, (u32)n, (u32)N, fold ? 1 : 0);
        }
        if (fold) { std::swap(geo.a_in, geo.a_out); std::swap(geo.b_in, geo.b_out); }
        {
            ScopedK tk(ctx, BP_K_MSM_ACCUM);
            hipLaunchKernelGGL(k_dt_accum_multi<C>, dim3((u32)L.nblk, (u32)(2 * B)), dim3(256), 0, st, ctx->dt_tab.as<u32>(), d_jobs, L.nblk == 1 ? d_res : d_acc);
            if (L.nblk > 1) hipLaunchKernelGGL(k_dt_finish<C>, dim3((u32)(2 * B)), dim3(256), 0, st, (const u32*)d_acc, (u32)L.nblk, d_res);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs + L.stage_res, d_res, 2 * B * 96, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        ctx->dt_runs += 2 * B;
        const u64* res = (const u64*)(hs + L.stage_res);
        on_pool([&](size_t c) {
            const size_t lo = c * chunk, hi = std::min(B, lo + chunk);
            for (size_t i = 2 * lo; i < 2 * hi; i++) { const u64* P = res + 12 * i; memcpy(pts[i].X.v, P, 32); memcpy(pts[i].Y.v, P + 4, 32); memcpy(pts[i].Z.v, P + 8, 32); }
            pb_to_aff<C>(pts.data() + 2 * lo, 2 * (hi - lo), aff.data() + 2 * lo);
            for (size_t j = lo; j < hi; j++) {
                host::ProofData& pf = *g.mem[j].pf;
                pf.L_vec[r] = aff[2 * j]; pf.R_vec[r] = aff[2 * j + 1];
                host::Transcript& tr = *g.mem[j].tr;
                TP::append_point(tr, "L", aff[2 * j]); TP::append_point(tr, "R", aff[2 * j + 1]);
                u[j] = TP::challenge_scalar(tr, "u");
            }
            pb_inv_many<S>(u.data() + lo, hi - lo, ui.data() + lo);
        });
    }
    // a[0], b[0] after the last challenge's fold
    for (size_t j = 0; j < B; j++) fill_desc(j, true);
    HIPCHK(hipMemcpyAsync(ar + L.desc_off, hs, B * sizeof(DtRoundDesc), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_dt_ab_final_multi<C>, dim3((u32)((B + 63) / 64)), dim3(64), 0, st, d_desc, geo, (u32)B, d_ab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hs + L.stage_ab, d_ab, B * 64, hipMemcpyDeviceToHost, st));
    // secret hygiene (prover.rs:805-812): the group's witness-derived vectors, one operation for all of them
    HIPCHK(hipMemsetAsync(ar, 0, L.vec_end, st));
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    const u64* ab = (const u64*)(hs + L.stage_ab);
    for (size_t j = 0; j < B; j++) { memcpy(g.mem[j].pf->a.v, ab + 8 * j, 32); memcpy(g.mem[j].pf->b.v, ab + 8 * j + 4, 32); }
    ctx->pb_groups++;
    ctx->pb_lockstep += B;
    ctx->pb_ipa_s += now_s() - t_begin;
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}

template <class C>
static int cs_prove_batch(bp_ctx* c, size_t count, bp_cs* const* hs, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens, int* status, double* timing) {
    const double t_begin = now_s();
    c->pb_ipa_s = 0;
    std::vector<int> st(count, BP_OK);
    std::vector<host::ProofData> pfs(count);
    std::vector<char> grouped(count, 0);
    StageTimes tm;
    // 1. TranscriptRng heads: same-shaped statements eight at a time in lockstep (prove_precompute_batch)
    {
        std::vector<bp_cs*> need;
        for (size_t k = 0; k < count; k++) if (!(C::ID == 0 ? (void*)hs[k]->pre0.rng.get() : (void*)hs[k]->pre1.rng.get())) need.push_back(hs[k]);
        std::stable_sort(need.begin(), need.end(), [](bp_cs* a, bp_cs* b) {
            const auto &x = *a->cs<C>(), &y = *b->cs<C>();
            return std::make_pair(x.a_L.size(), x.v.size()) < std::make_pair(y.a_L.size(), y.v.size());
        });
        const double t0 = now_s();
        if (!need.empty()) BPCHK(cs_precompute_batch<C>(need.data(), need.size()));
        tm.rng += now_s() - t0;
    }
    // 2. every instance up to its inner-product argument; lockstep-ready ones join the open group of their size
    const size_t cap_knob = c->tune_prove_batch ? std::min(c->tune_prove_batch, PB_GROUP_MAX) : 0;
    PbGroup<C> grp;
    auto flush = [&]() {
        if (!grp.open) return;
        const int rc = grp.mem.empty() ? BP_OK : pb_run_group<C>(c, grp);
        for (auto& m : grp.mem) { if (rc) st[m.k] = rc; }
        grp.mem.clear(); grp.open = false;
    };
    std::vector<size_t> order(count);
    for (size_t k = 0; k < count; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return hs[a]->cs<C>()->a_L.size() < hs[b]->cs<C>()->a_L.size(); });
    for (size_t oi = 0; oi < count; oi++) {
        const size_t k = order[oi];
        bp_cs* s = hs[k];
        auto* pre = C::ID == 0 ? (ProvePre<C>*)&s->pre0 : (ProvePre<C>*)&s->pre1;
        if (!s->csc_tried) {
            s->csc.reset(new HostCsc());
            if (!build_host_csc<C>(*s->cs<C>(), *s->csc)) s->csc.reset();
            s->csc_tried = true;
        }
        IpaDefer defer;
        defer.take = [&](size_t N, IpaDeferSlot& slot) -> bool {
            if (grp.open && (grp.lay.N != N || grp.mem.size() >= grp.lay.cap)) flush();
            if (!grp.open) {
                size_t cap = cap_knob ? cap_knob : std::max<size_t>(1, std::min(PB_GROUP_MAX, PB_ARENA_BUDGET / PbLayout::per_proof(N)));
                cap = std::max<size_t>(1, std::min(cap, count - oi));
                grp.lay.make(N, cap);
                if (c->pb_arena.ensure(grp.lay.total)) return false;
                if (c->h_pb_cap < grp.lay.stage_bytes) {
                    if (c->h_pb) (void)hipHostFree(c->h_pb);
                    c->h_pb = nullptr; c->h_pb_cap = 0;
                    if (hipHostMalloc(&c->h_pb, grp.lay.stage_bytes) != hipSuccess) { c->h_pb = nullptr; return false; }
                    c->h_pb_cap = grp.lay.stage_bytes;
                }
                grp.open = true;
            }
            const size_t j = grp.mem.size();
            char* base = (char*)c->pb_arena.p + j * grp.lay.per_vec;
            slot.a = (u32*)base; slot.b = (u32*)(base + grp.lay.o_b); slot.cG = (u32*)(base + grp.lay.o_cG); slot.cH = (u32*)(base + grp.lay.o_cH);
            return true;
        };
        s->consumed = true; s->running = true;
        const int rc = r1cs_prove<C>(c, *s->cs<C>(), s->rng32, pfs[k], tm, pre, s->csc.get(), &defer);
        s->running = false;
        if (defer.taken) {
            grp.mem.push_back(PbMember<C>{k, s->cs<C>()->tr, &pfs[k], defer.w});
            pfs[k].L_vec.resize(pb_lg(defer.N)); pfs[k].R_vec.resize(pb_lg(defer.N));
            grouped[k] = 1;
            if (rc) st[k] = rc;   // (a device error after the hand-over: the group's result for this instance is dropped)
        } else {
            st[k] = rc;
            if (!rc) c->pb_single++;
        }
    }
    flush();
    // 3. serialisation, per-instance status
    int first = BP_OK;
    for (size_t k = 0; k < count; k++) {
        proof_lens[k] = 0;
        if (!st[k]) {
            std::vector<host::u8> bytes = host::proof_to_bytes<C>(pfs[k]);
            if (bytes.size() > proof_stride) st[k] = BP_E_ARG;   // (cannot happen: the stride was checked against the generators)
            else { memcpy(proofs_out + k * proof_stride, bytes.data(), bytes.size()); proof_lens[k] = bytes.size(); }
        }
        if (status) status[k] = st[k];
        if (st[k] && first == BP_OK) first = st[k];
    }
    if (timing) {
        timing[0] = now_s() - t_begin; timing[1] = c->pb_ipa_s; timing[2] = tm.rng; timing[3] = tm.upload; timing[4] = tm.commit_msm; timing[5] = tm.flatten;
        timing[6] = tm.poly; timing[7] = tm.ipa;
    }
    return first;
}

int bp_prover_prove_batch(bp_ctx* c, size_t count, bp_cs* const* provers, const uint8_t* rng_bytes, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens,
                          int* status, double* timing) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!provers || !proofs_out || !proof_lens) return BP_E_ARG;
    // up-front checks: nothing is consumed unless every instance passes
    for (size_t k = 0; k < count; k++) {
        bp_cs* h = provers[k];
        if (!h || !h->proving || h->curve != c->curve || !cs_live(h) || h->running) { g_err = "prove_batch: every instance needs a live prover of the ctx's curve"; return BP_E_ARG; }
        if (rng_bytes) {
            if (h->have_rng && (h->pre0.rng || h->pre1.rng) && memcmp(h->rng32, rng_bytes + 32 * k, 32)) { g_err = "prove_batch: rng bytes differ from the precomputed ones"; return BP_E_ARG; }
        } else if (!h->have_rng) { g_err = "prove_batch: the external rng bytes are missing"; return BP_E_ARG; }
    }
    {
        std::vector<const void*> hv(provers, provers + count), tv(count);
        for (size_t k = 0; k < count; k++) tv[k] = provers[k]->tr;
        std::sort(hv.begin(), hv.end()); std::sort(tv.begin(), tv.end());
        if (std::adjacent_find(hv.begin(), hv.end()) != hv.end()) { g_err = "prove_batch: a prover appears twice (prove takes self)"; return BP_E_ARG; }
        if (std::adjacent_find(tv.begin(), tv.end()) != tv.end()) { g_err = "prove_batch: two provers borrow one transcript"; return BP_E_ARG; }
    }
    if (!c->gens_cap) { g_err = "prove_batch: generators not installed (bp_gens_derive / bp_gens_upload / bp_gens_share)"; return BP_E_GENS_LENGTH; }
    if (proof_stride < pb_proof_len(pb_lg(c->gens_cap))) { g_err = "prove_batch: proof_stride is shorter than a proof with lg(gens capacity) rounds"; return BP_E_ARG; }
    if (c->host_only) { g_err = "prove_batch: a host-only ctx has no device to prove on"; return BP_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(c->device));
    for (size_t k = 0; k < count; k++) if (rng_bytes) { memcpy(provers[k]->rng32, rng_bytes + 32 * k, 32); provers[k]->have_rng = true; }
    return c->curve == 0 ? cs_prove_batch<Secq>(c, count, provers, proofs_out, proof_stride, proof_lens, status, timing)
                         : cs_prove_batch<Zorro>(c, count, provers, proofs_out, proof_stride, proof_lens, status, timing);
}

template <class C> static int prover_commit_batch_t(bp_ctx* ctx, size_t count, bp_cs* const* hs, const size_t* m_each, const uint64_t* v, const uint64_t* blind,
                                                    uint64_t* V_xy, bp_var* vars) {
    size_t total = 0;
    for (size_t k = 0; k < count; k++) total += m_each[k];
    host::PedersenGens<C> pc = host::PedersenGens<C>::make_default();
    pedersen_attach<C>(ctx, pc);
    std::vector<A4> pts(total);
    BPCHK(pc.commit_many((const F4*)v, (const F4*)blind, total, pts.data()));   // every commitment of the batch: one launch, one inversion
    size_t i = 0;
    for (size_t k = 0; k < count; k++) {
        host::ConstraintSystem<C>& cs = *hs[k]->cs<C>();
        for (size_t e = 0; e < m_each[k]; e++, i++) {   // Prover::commit (prover.rs:327-341), in order
            const u32 idx = (u32)cs.v.size();
            F4 a, b; memcpy(a.v, v + 4 * i, 32); memcpy(b.v, blind + 4 * i, 32);
            cs.v.push_back(a); cs.v_blinding.push_back(b);
            host::TP<C>::append_point(*cs.tr, "V", pts[i]);
            hs[k]->commitments.push_back(pts[i]);
            if (V_xy) memcpy(V_xy + 8 * i, &pts[i], 64);
            if (vars) { vars[i].kind = BP_VAR_COMMITTED; vars[i].index = idx; }
        }
    }
    return BP_OK;
}
int bp_prover_commit_batch(bp_ctx* c, size_t count, bp_cs* const* provers, const size_t* m_each, const uint64_t* v, const uint64_t* v_blinding, uint64_t* V_xy_out,
                           bp_var* vars_out) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!provers || !m_each) return BP_E_ARG;
    size_t total = 0;
    for (size_t k = 0; k < count; k++) {
        bp_cs* h = provers[k];
        if (!cs_live(h) || !h->proving || h->curve != c->curve) { g_err = "prover_commit_batch: every instance needs a live prover of the ctx's curve"; return BP_E_ARG; }
        if (CS_DISPATCH(h, h->cs0->phase2, h->cs1->phase2)) return BP_E_ARG;
        total += m_each[k];
    }
    if (total && (!v || !v_blinding)) return BP_E_ARG;
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? prover_commit_batch_t<Secq>(c, count, provers, m_each, v, v_blinding, V_xy_out, vars_out)
                         : prover_commit_batch_t<Zorro>(c, count, provers, m_each, v, v_blinding, V_xy_out, vars_out);
}
int bp_ctx_prove_batch_stats(bp_ctx* c, uint64_t* lockstep_instances, uint64_t* single_instances, uint64_t* groups) {
    if (!c) return BP_E_ARG;
    if (lockstep_instances) *lockstep_instances = c->pb_lockstep;
    if (single_instances) *single_instances = c->pb_single;
    if (groups) *groups = c->pb_groups;
    return BP_OK;
}
