// bp_verifier_verify_batch / bp_r1cs_verify_each_scenarios: `Verifier::verify` (src/r1cs/verifier.rs:549-600) for many instances in
// one call, a verdict for each (see "Verification of many proofs with a verdict for EACH" in include/arkbp.h).
//
// Host side.  Framing of every proof (proof_parse_lazy) on the pool; the proof's own claim (lg N = length of L_vec) routes it: padded
// sizes the direct window tables reach take the GROUPED path, everything else the single-instance route (batch_verify_core with one
// instance, weight 1 — what bp_verifier_verify runs), inside the same call.  Grouped instances: one launch decompresses all their
// points (one wait per call), the pool replays the transcripts (verify_prepare: the same function the single route runs, so an
// instance's status is the same either way), an instance that fails keeps its own status and leaves the launches.  The survivors
// are grouped by (circuit template, kind of coefficient table) — equal templates have equal padded sizes — and cut at the group cap.
//
// Device side of a group of P proofs of padded size N (ve_run_group): ONE copy up from a pinned staging half, then on the ctx's stream
//   k_scalars_import (parameter blocks, coefficient tables, tail scalars) -> k_scalars_to_canon (tail scalars) -> points import ->
//   k_vfy_tables -> k_vfy_batch (one chunk per proof, alpha = 1: rows g_p, h_p and the (wc + delta) partials per proof) ->
//   k_ve_heads (head scalars + DtJobs) -> k_dt_accum_multi (+ k_dt_finish) -> k_ve_tail -> k_ve_check -> one copy back
// and ONE host wait (BP_VERIFY_EACH_WAITS_PER_GROUP), whatever P and N.
// Memory per proof in the 256 MB arena: 3.3 KB parameter block, its coefficient table (own values only), 96 B per tail term, the
// k_vfy_tables stride (48 B per entry), the two rows (2 * N * 32 B), 32 B per block of 256 elements, 64 + 64 B heads, one DtJob,
// 96 B per workgroup of its table sum, 3 * 96 B points and a flag.
static constexpr size_t VE_ARENA_BUDGET = (size_t)256 << 20, VE_GROUP_MAX = 4096;
static inline size_t ve_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct VeLayout {
    // staged inputs, in the order of the pinned half (one copy): [parameter blocks | coefficient tables | tail scalars] are ark words
    // that one import launch converts in place
    size_t o_pb = 0, o_coef = 0, o_tsc = 0, o_hin = 0, o_tpt = 0, o_toff = 0, o_perm = 0, stage_bytes = 0;
    // device only
    size_t o_tab = 0, o_g = 0, o_h = 0, o_dpart = 0, o_heads = 0, o_jobs = 0, o_acc = 0, o_fixed = 0, o_tsum = 0, o_res = 0, res_bytes = 0, total = 0;
    size_t nblk = 0, nblk_dt = 0, tab_stride = 0;
    void make(size_t P, size_t N, size_t kk, size_t q, size_t ncoef_own, size_t T) {
        const u32 LOB = (u32)((kk + 1) / 2), nlo = 1u << LOB, nhi = 1u << (kk - LOB), nzhi = (u32)((q + 1) >> 8) + 1;
        nblk = (N + 255) / 256;
        nblk_dt = pf_nblk(2 + 2 * N, P);
        tab_stride = vfy_tab_stride(nlo, nhi, nzhi);
        size_t at = 0;
        o_pb = at; at += P * VFY_PB_SCALARS * 32;
        o_coef = at; at += P * ncoef_own * 32;
        o_tsc = at; at += T * 32;
        o_hin = at; at += P * 64;
        at = ve_align(at); o_tpt = at; at += T * 64;
        at = ve_align(at); o_toff = at; at += (P + 1) * 4;
        at = ve_align(at); o_perm = at; at += P * 4;
        stage_bytes = at;
        at = ve_align(at); o_tab = at; at += P * tab_stride * VT_W * 4;
        at = ve_align(at); o_g = at; at += P * N * 32;
        at = ve_align(at); o_h = at; at += P * N * 32;
        at = ve_align(at); o_dpart = at; at += P * nblk * 32;
        at = ve_align(at); o_heads = at; at += P * 64;
        at = ve_align(at); o_jobs = at; at += P * sizeof(DtJob);
        at = ve_align(at); o_acc = at; at += P * nblk_dt * 96;
        at = ve_align(at); o_fixed = at; at += P * 96;
        at = ve_align(at); o_tsum = at; at += P * 96;
        at = ve_align(at); o_res = at; res_bytes = ve_align(P * 4) + P * 96; at += res_bytes;   // [flags | check points]
        total = at;
    }
    // upper bound of what one proof adds to a group (the group cap divides the budget by it)
    static size_t per_proof(size_t N, size_t kk, size_t q, size_t ncoef_own, size_t tmax) {
        VeLayout l;
        l.make(1, N, kk, q, ncoef_own, tmax);   // (a lone proof's table sum has the most workgroups per job, and its layout all the alignment gaps)
        return l.total;
    }
};

template <class C> struct VeRep : VfyReplayed<C> { size_t k = 0, kk = 0; };   // + instance index in the call; lg N as the proof claims it

// One group: P proofs of one template.  flags_out[j] = 1 iff member j's check is the identity; pts_out (may be null): the checks.
template <class C>
static int ve_run_group(bp_ctx* ctx, const VTemplate<C>& t, bool own, VeRep<C>* const* mem, size_t P, int half, u32* flags_out, J4* pts_out, double& wait_s) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    hipStream_t st = ctx->stream;
    const size_t N = mem[0]->vp.N, kk = mem[0]->vp.k;
    size_t T = 0, tmax = 0;
    for (size_t j = 0; j < P; j++) { T += mem[j]->vp.tail_scalars.size(); tmax = std::max(tmax, mem[j]->vp.tail_scalars.size()); }
    if (T >= ((size_t)1 << 31) || P * N >= ((size_t)1 << 31)) { g_err = "verify_batch: group too large"; return BP_E_ARG; }
    VeLayout L;
    L.make(P, N, kk, t.q, own ? t.ncoef : 0, T);
    BPCHK(ctx->ve_arena.ensure(L.total));
    BPCHK(vfy_stage_ensure(ctx, half, L.stage_bytes));
    BPCHK(vfy_aux_ensure(ctx, half, L.res_bytes));
    char* hs = (char*)ctx->h_vstage[half];
    char* d = (char*)ctx->ve_arena.p;
    {
        F4* pb = (F4*)(hs + L.o_pb);
        F4* coef = (F4*)(hs + L.o_coef);
        F4* tsc = (F4*)(hs + L.o_tsc);
        F4* hin = (F4*)(hs + L.o_hin);
        A4* tpt = (A4*)(hs + L.o_tpt);
        u32* toff = (u32*)(hs + L.o_toff);
        u32* perm = (u32*)(hs + L.o_perm);
        memset(hs, 0, L.stage_bytes);
        size_t at = 0;
        for (size_t j = 0; j < P; j++) {
            const VerifyPrep<C>& vp = mem[j]->vp;
            F4* b = pb + j * VFY_PB_SCALARS;   // the parameter block of batch_verify_core with weight 1
            for (int i = 0; i < 32; i++) { b[i] = vp.ztab[i]; b[32 + i] = vp.ypw[32 + i]; }
            b[64] = vp.allinv; b[65] = vp.x; b[66] = vp.a; b[67] = vp.b; b[68] = vp.u; b[69] = S::one(); b[70] = vp.coefD; b[71] = vp.rx;
            for (size_t i = 0; i < vp.k; i++) b[72 + i] = vp.u_sq[i];
            if (own) memcpy(coef + j * t.ncoef, vp.coef_ptr, t.ncoef * 32);
            toff[j] = (u32)at;
            if (!vp.tail_scalars.empty()) {
                memcpy(tsc + at, vp.tail_scalars.data(), vp.tail_scalars.size() * 32);
                memcpy(tpt + at, vp.tail_points.data(), vp.tail_points.size() * 64);
            }
            at += vp.tail_scalars.size();
            hin[2 * j] = vp.sB; hin[2 * j + 1] = vp.sBb;
            perm[j] = (u32)j;
        }
        toff[P] = (u32)at;
    }
    HIPCHK(hipMemcpyAsync(d, hs, L.stage_bytes, hipMemcpyHostToDevice, st));
    u32* d_pb = (u32*)(d + L.o_pb);
    u32* d_coef = (u32*)(d + L.o_coef);
    u32* d_tsc = (u32*)(d + L.o_tsc);
    u32* d_tpt = (u32*)(d + L.o_tpt);
    u32* d_toff = (u32*)(d + L.o_toff);
    u32* d_perm = (u32*)(d + L.o_perm);
    u32* d_tab = (u32*)(d + L.o_tab);
    u32* d_g = (u32*)(d + L.o_g);
    u32* d_h = (u32*)(d + L.o_h);
    u32* d_dpart = (u32*)(d + L.o_dpart);
    u32* d_heads = (u32*)(d + L.o_heads);
    DtJob* d_jobs = (DtJob*)(d + L.o_jobs);
    u32* d_acc = (u32*)(d + L.o_acc);
    u32* d_fixed = (u32*)(d + L.o_fixed);
    u32* d_tsum = (u32*)(d + L.o_tsum);
    u32* d_flags = (u32*)(d + L.o_res);
    u32* d_check = (u32*)(d + L.o_res + ve_align(P * 4));
    const size_t nimp = P * VFY_PB_SCALARS + (own ? P * t.ncoef : 0) + T;
    hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((nimp + 255) / 256)), dim3(256), 0, st, d_pb, d_pb, (u32)nimp);
    if (T) {
        hipLaunchKernelGGL(k_scalars_to_canon<FrP>, dim3((u32)((T + 255) / 256)), dim3(256), 0, st, d_tsc, (u32)T);
        BPCHK(bp_points_import(ctx, d_tpt, d_tpt, T));
    }
    const u32 LOB = (u32)((kk + 1) / 2), nlo = 1u << LOB, nhi = 1u << (kk - LOB), nzhi = (u32)((t.q + 1) >> 8) + 1;
    {
        ScopedK tk(ctx, BP_K_VFY_TABLES);
        hipLaunchKernelGGL(k_vfy_tables<C>, dim3((std::max(std::max(nlo, nhi), std::max(256u, nzhi)) + 255) / 256, (u32)P), dim3(256), 0, st, d_pb, d_perm, (u32)P, (u32)kk,
                           LOB, nzhi, d_tab);
    }
    {
        ScopedK tk(ctx, BP_K_VFY_SCALARS);   // one chunk per proof: nothing is summed over proofs
        hipLaunchKernelGGL(k_vfy_batch<C>, dim3((u32)L.nblk, (u32)P), dim3(256), 0, st, t.dev, d_pb, d_perm, own ? d_coef : nullptr, own ? (u32)(t.ncoef * 8) : 0u, (u32)P, 1u,
                           (u32)t.n, (u32)t.n1, (u32)N, (u32)kk, d_g, d_h, d_dpart, d_tab, LOB, nzhi);
    }
    hipLaunchKernelGGL(k_ve_heads<C>, dim3((u32)((P + 63) / 64)), dim3(64), 0, st, (const u32*)(d + L.o_hin), d_dpart, (u32)L.nblk, (u32)P, (u32)N, dt_base_G(ctx, 0),
                       dt_base_H(ctx, 0), d_g, d_h, d_heads, d_jobs);
    BPCHK(pf_accum<C>(ctx, d_jobs, P, L.nblk_dt, d_acc, d_fixed));
    {
        ScopedK tk(ctx, BP_K_VE_TAIL);
        hipLaunchKernelGGL(k_ve_tail<C>, dim3((u32)P), dim3(256), 0, st, d_tpt, d_tsc, d_toff, (u32)tmax, d_tsum);
    }
    hipLaunchKernelGGL(k_ve_check<C>, dim3((u32)((P + 63) / 64)), dim3(64), 0, st, d_fixed, d_tsum, (u32)P, d_check, d_flags);
    HIPCHK(hipGetLastError());
    char* hr = (char*)ctx->h_vaux[half];
    HIPCHK(hipMemcpyAsync(hr, d_flags, pts_out ? L.res_bytes : P * 4, hipMemcpyDeviceToHost, st));
    const double tw = now_s();
    HIPCHK(ctx_stream_wait(ctx));
    wait_s += now_s() - tw;
    ctx->ve_waits++;
    memcpy(flags_out, hr, P * 4);
    if (pts_out) pf_points_in(hr + ve_align(P * 4), P, pts_out);
    ctx->ve_groups++;
    return BP_OK;
}

template <class C>
static int verify_each_core(bp_ctx* ctx, size_t count, const VfyProvider<C>& prov, const uint8_t* proofs, const size_t* poff /* count + 1 */, int* status,
                            uint64_t* points, double* timing) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    const double t_entry = now_s();
    VfyMark mark{"vfy-each", t_entry};
    if (points) memset(points, 0, count * 64);
    std::vector<int> stv(count, BP_OK);
    host_pool_ensure(ctx, count);
    // 0. pending wire commitments: decoded and committed first; an instance with a rejected encoding is left out with BP_E_FORMAT
    // 1. framing; the proof's claim decides the route
    std::vector<host::LazyProof> lps;
    std::vector<int> pst, prc;
    BPCHK(vfy_parse<C>(ctx, prov, count, proofs, poff, pst, lps, prc));
    const size_t reach_max = ctx->shard_world <= 1 && ctx->tune_direct_max >= 2 ? std::min(ctx->gens_cap, ctx->tune_direct_max) : 0;
    auto claim = [&](size_t k) -> size_t {   // the padded size the proof claims, 0 when it cannot take the grouped path
        const size_t kk = lps[k].k;
        if (prc[k] || kk == (size_t)-1 || kk == 0 || kk >= 32 || ((size_t)1 << kk) > reach_max) return 0;
        return (size_t)1 << kk;
    };
    size_t want = 0, reach = 0;
    for (size_t k = 0; k < count; k++) want = std::max(want, claim(k));
    if (want) {   // the tables are built when the first candidate appears, as for proving
        bool ready = false;
        BPCHK(dt_ensure<C>(ctx, want, ready));
        if (ready) reach = std::min(ctx->dt_cap, reach_max);
    }
    std::vector<size_t> gl, sl;
    for (size_t k = 0; k < count; k++) {
        if (pst[k]) { stv[k] = pst[k]; continue; }
        const size_t Nk = claim(k);
        if (Nk && Nk <= reach) gl.push_back(k); else sl.push_back(k);
    }
    const size_t ng = gl.size();
    ctx->ve_grouped += ng;
    mark("parse + route");
    // 2. the grouped instances' points: one decompression launch, one wait
    const std::vector<size_t> xoff = vfy_xoff(lps, gl.data(), ng);
    std::vector<F4> all_x(xoff[ng]);
    std::vector<u32> all_f(xoff[ng]), all_ok;
    std::vector<A4> all_pts;
    vfy_gather(ctx, lps, gl.data(), ng, xoff, all_x.data(), all_f.data());
    BPCHK(decompress_points<C>(ctx, all_x.data(), all_f.data(), xoff[ng], all_pts, all_ok));
    const double t_dec = now_s();
    mark("gpu decompress");
    // 3. replay on the pool: every instance keeps its own status
    std::vector<VeRep<C>> rep(ng);
    pool_range(ctx, 0, ng, [&](size_t j) {
        VeRep<C>& r = rep[j];
        r.k = gl[j]; r.kk = lps[r.k].k;
        if (!vfy_points_ok(all_ok.data(), xoff[j], xoff[j + 1])) { r.rc = BP_E_FORMAT; return; }
        if (vfy_replay_one<C>(ctx, prov, r.k, lps[r.k], all_pts.data() + xoff[j], r)) return;
        if (r.vp.tail_scalars.size() != 6 + prov.m_of(r.k) + 5 + 2 * r.kk || r.vp.N != ((size_t)1 << r.kk) || r.vp.k != r.kk) { r.rc = BP_E_VERIFICATION; return; }
        r.pf = host::ProofData();
    });
    const double t_rep = now_s();
    mark("replay");
    std::vector<VeRep<C>*> live;
    for (size_t j = 0; j < ng; j++) {
        if (rep[j].rc) { stv[rep[j].k] = rep[j].rc; if (rep[j].vp.err) g_err = rep[j].vp.err; continue; }   // (left out of the launches)
        live.push_back(&rep[j]);
    }
    // 4. templates: by structure digest; a miss records the matrices from this instance (upload + sync, once per gadget)
    // (bounded cache: only entries no instance of this call resolves to leave it)
    BPCHK((vfy_resolve_templates<C>(ctx, live.size(), [&live](size_t j) -> VfyReplayed<C>& { return *live[j]; }, "verify_batch", nullptr)));
    {   // one kind of coefficient table per template: when any instance carries values of its own (public constants, the challenges of
        // randomized constraints), every instance of the template ships its table — the template's creator among them — so that the
        // groups do not depend on which instance happened to build the template
        std::set<const void*> mixed;
        for (auto* r : live) if (r->own_tab) mixed.insert(r->tm);
        for (auto* r : live) if (mixed.count(r->tm)) r->own_tab = true;
    }
    mark("templates");
    // 5. groups: same template, same kind of coefficient table; instance order inside a group; cut at the cap
    std::stable_sort(live.begin(), live.end(), [](const VeRep<C>* x, const VeRep<C>* y) {
        return x->tm != y->tm ? std::less<const void*>()(x->tm, y->tm) : x->own_tab < y->own_tab;
    });
    const size_t cap_knob = ctx->tune_verify_each ? std::min(ctx->tune_verify_each, VE_GROUP_MAX) : VE_GROUP_MAX;
    double wait_s = 0;
    std::vector<u32> flags;
    std::vector<J4> jpts;
    std::vector<A4> apts;
    int ngroups = 0;
    for (size_t j0 = 0; j0 < live.size();) {
        size_t j1 = j0 + 1, tmax = live[j0]->vp.tail_scalars.size();
        while (j1 < live.size() && live[j1]->tm == live[j0]->tm && live[j1]->own_tab == live[j0]->own_tab) { tmax = std::max(tmax, live[j1]->vp.tail_scalars.size()); j1++; }
        const VTemplate<C>& t = *live[j0]->tm;
        const bool own = live[j0]->own_tab;
        const size_t cap = std::max<size_t>(1, std::min(cap_knob, VE_ARENA_BUDGET / VeLayout::per_proof(live[j0]->vp.N, live[j0]->vp.k, t.q, own ? t.ncoef : 0, tmax)));
        for (size_t lo = j0; lo < j1; lo += cap) {
            const size_t P = std::min(cap, j1 - lo);
            flags.assign(P, 0);
            if (points) jpts.resize(P);
            BPCHK(ve_run_group<C>(ctx, t, own, live.data() + lo, P, ngroups & 1, flags.data(), points ? jpts.data() : nullptr, wait_s));
            ngroups++;
            if (points) { apts.resize(P); to_aff_many<C>(jpts.data(), P, apts.data()); }   // one inversion for the group's points
            for (size_t j = 0; j < P; j++) {
                const size_t k = live[lo + j]->k;
                stv[k] = flags[j] ? BP_OK : BP_E_VERIFICATION;
                if (points && !flags[j]) aff_out<C>(points + 8 * k, apts[j]);
            }
        }
        j0 = j1;
    }
    if (ctx->profiling && ngroups) collect_timers(ctx);
    rep.clear();
    mark("groups");
    // 6. everything else: the single-instance route, in instance order
    const double t_single = now_s();
    for (size_t k : sl) {
        const uint32_t self = (uint32_t)k;
        VfyProvider<C> one;
        provider_subset<C>(prov, &self, one);
        one.dev_batch = nullptr;   // (one instance: the host replay)
        const F4 alpha = S::one();
        const size_t po[2] = {0, poff[k + 1] - poff[k]};
        stv[k] = batch_verify_core<C>(ctx, 1, one, proofs + poff[k], po, &alpha, nullptr, points ? points + 8 * k : nullptr);
        ctx->ve_single++;
    }
    mark("single route");
    int first = BP_OK;
    for (size_t k = 0; k < count; k++) { status[k] = stv[k]; if (stv[k] && first == BP_OK) first = stv[k]; }
    if (timing) { const double t_end = now_s(); timing[0] = t_end - t_entry; timing[1] = t_rep - t_dec; timing[2] = wait_s; timing[3] = t_end - t_single; timing[4] = t_dec - t_entry; }
    return first;
}

template <class C>
static int cs_verify_each(bp_ctx* c, size_t count, bp_cs* const* vs, const uint8_t* proofs, const size_t* proof_lens, int* status, uint64_t* points, double* timing) {
    const std::vector<size_t> poff = prefix_offsets(proof_lens, count);
    VfyProvider<C> prov;
    cs_provider<C>(c, count, CsView{vs, nullptr}, prov);
    prov.dev_batch = nullptr;   // (the device front end gives one verdict for a batch, not one per instance)
    VerifyingScope scope(vs, count);
    return verify_each_core<C>(c, count, prov, proofs, poff.data(), status, points, timing);
}
// scenario statements: the statement sources, the per-instance recorders and the lockstep transcript heads are batch_verify_scenarios'
// own; only the core differs
template <class C>
static int scenarios_verify_each(bp_ctx* c, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                 const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, int* status, uint64_t* points, double* timing) {
    const VfyCoreFn<C> core = [&](const VfyProvider<C>& prov, const size_t* poff, const F4*) {
        return verify_each_core<C>(c, count, prov, proofs, poff, status, points, timing);
    };
    return batch_verify_scenarios<C>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, nullptr, nullptr, 0, nullptr, &core);
}

int bp_verifier_verify_batch(bp_ctx* c, size_t count, bp_cs* const* verifiers, const uint8_t* proofs, const size_t* proof_lens, int* status, uint64_t* check_points_xy,
                             double* timing) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!verifiers || !proofs || !proof_lens || !status) return BP_E_ARG;
    BPCHK(verifiers_check("verify_batch", c, count, verifiers));
    if (!c->gens_cap) { g_err = "verify_batch: generators not installed"; return BP_E_GENS_LENGTH; }
    if (c->host_only) { g_err = "verify_batch: a host-only ctx has no device to verify on"; return BP_E_NO_DEVICE; }
    BPCHK(wire_check_states("verify_batch", count, verifiers));
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? cs_verify_each<Secq>(c, count, verifiers, proofs, proof_lens, status, check_points_xy, timing)
                         : cs_verify_each<Zorro>(c, count, verifiers, proofs, proof_lens, status, check_points_xy, timing);
}

int bp_r1cs_verify_each_scenarios(bp_ctx* c, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                  const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, int* status, uint64_t* check_points_xy,
                                  double* timing) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!scenarios || !params || !proofs || !proof_lens || !ms || !npubs || !status) return BP_E_ARG;
    size_t tm = 0, tp = 0;
    for (size_t k = 0; k < count; k++) { tm += ms[k]; tp += npubs[k]; }
    if ((tm && !commit_xy) || (tp && !publics)) return BP_E_ARG;
    if (!c->gens_cap) { g_err = "verify_each: generators not installed"; return BP_E_GENS_LENGTH; }
    if (c->host_only) { g_err = "verify_each: a host-only ctx has no device to verify on"; return BP_E_NO_DEVICE; }
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? scenarios_verify_each<Secq>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, status, check_points_xy, timing)
                         : scenarios_verify_each<Zorro>(c, count, scenarios, params, proofs, proof_lens, commit_xy, ms, publics, npubs, status, check_points_xy, timing);
}

int bp_ctx_verify_each_stats(bp_ctx* c, uint64_t* grouped_instances, uint64_t* single_instances, uint64_t* groups, uint64_t* host_waits) {
    if (!c) return BP_E_ARG;
    if (grouped_instances) *grouped_instances = c->ve_grouped;
    if (single_instances) *single_instances = c->ve_single;
    if (groups) *groups = c->ve_groups;
    if (host_waits) *host_waits = c->ve_waits;
    return BP_OK;
}

// ---- test hooks ---------------------------------------------------------------------------------------------------------------------
template <class C>
static int msm_each_entry(bp_ctx* ctx, size_t count, const size_t* offsets, const uint64_t* bases_xy, const uint64_t* scalars, int canonical, uint64_t* out_xy) {
    typedef typename C::Fr FrP;
    hipStream_t st = ctx->stream;
    const size_t o0 = offsets[0], n = offsets[count] - o0;
    size_t tmax = 0;
    std::vector<u32> toff(count + 1);
    for (size_t j = 0; j <= count; j++) toff[j] = (u32)(offsets[j] - o0);
    for (size_t j = 0; j < count; j++) tmax = std::max(tmax, offsets[j + 1] - offsets[j]);
    const size_t o_pts = 0, o_sc = ve_align(n * 64), o_toff = ve_align(o_sc + n * 32), o_out = ve_align(o_toff + (count + 1) * 4), total = o_out + count * 96;
    BPCHK(ctx->ve_arena.ensure(total));
    char* d = (char*)ctx->ve_arena.p;
    if (n) {
        HIPCHK(hipMemcpyAsync(d + o_pts, bases_xy + 8 * o0, n * 64, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d + o_sc, scalars + 4 * o0, n * 32, hipMemcpyHostToDevice, st));
        BPCHK(bp_points_import(ctx, d + o_pts, d + o_pts, n));
        if (!canonical) {
            hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (const u32*)(d + o_sc), (u32*)(d + o_sc), (u32)n);
            hipLaunchKernelGGL(k_scalars_to_canon<FrP>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (u32*)(d + o_sc), (u32)n);
        }
    }
    HIPCHK(hipMemcpyAsync(d + o_toff, toff.data(), (count + 1) * 4, hipMemcpyHostToDevice, st));
    {
        ScopedK tk(ctx, BP_K_VE_TAIL);
        hipLaunchKernelGGL(k_ve_tail<C>, dim3((u32)count), dim3(256), 0, st, (const u32*)(d + o_pts), (const u32*)(d + o_sc), (const u32*)(d + o_toff), (u32)tmax, (u32*)(d + o_out));
    }
    HIPCHK(hipGetLastError());
    std::vector<u64> res(count * 12);
    HIPCHK(hipMemcpyAsync(res.data(), d + o_out, count * 96, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    std::vector<J4> jp(count);
    std::vector<A4> ap(count);
    pf_points_in(res.data(), count, jp.data());
    to_aff_many<C>(jp.data(), count, ap.data());
    for (size_t j = 0; j < count; j++) { memcpy(out_xy + 8 * j, ap[j].x.v, 32); memcpy(out_xy + 8 * j + 4, ap[j].y.v, 32); }
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}
int bp_debug_msm_each(bp_ctx* c, size_t count, const size_t* offsets, const uint64_t* bases_xy, const uint64_t* scalars, int scalars_canonical, uint64_t* out_xy) {
    if (!c) return BP_E_ARG;
    if (count == 0) return BP_OK;
    if (!offsets || !out_xy || count >= ((size_t)1 << 31)) return BP_E_ARG;
    for (size_t j = 0; j < count; j++) if (offsets[j + 1] < offsets[j]) { g_err = "bp_debug_msm_each: offsets must not decrease"; return BP_E_ARG; }
    const size_t n = offsets[count] - offsets[0];
    if (n >= ((size_t)1 << 31) || (n && (!bases_xy || !scalars))) return BP_E_ARG;
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_each_entry<Secq>(c, count, offsets, bases_xy, scalars, scalars_canonical, out_xy)
                         : msm_each_entry<Zorro>(c, count, offsets, bases_xy, scalars, scalars_canonical, out_xy);
}
int bp_debug_ve_plan(size_t count, const size_t* offsets, const uint64_t* scalars_canonical, size_t job, uint32_t* first, uint32_t* terms, uint8_t* digits, uint8_t* planes,
                     uint32_t* lanes, uint32_t* groups) {
    if (!offsets || job >= count || !first || !terms) return BP_E_ARG;
    std::vector<u32> toff(count + 1);
    for (size_t j = 0; j <= count; j++) { if (j && offsets[j] < offsets[j - 1]) return BP_E_ARG; toff[j] = (u32)(offsets[j] - offsets[0]); }
    const u32 t0 = ve_job_first(toff.data(), (u32)job), nt = ve_job_terms(toff.data(), (u32)job);
    *first = t0; *terms = nt;
    if (nt && (digits || planes) && !scalars_canonical) return BP_E_ARG;
    for (u32 t = 0; t < nt; t++) {
        const u32* k = (const u32*)(scalars_canonical + 4 * (size_t)(t0 + t));
        for (u32 w = 0; w < VE_WINDOWS; w++) {
            const u32 dg = ve_digit(k, w);
            if (digits) digits[(size_t)VE_WINDOWS * t + w] = (uint8_t)dg;
            if (planes) {
                u32 m = 0;
                for (u32 b = 0; b < VE_PLANES; b++) m |= ve_plane_bit(dg, b) << b;
                planes[(size_t)VE_WINDOWS * t + w] = (uint8_t)m;
            }
        }
    }
    for (u32 w = 0; w < VE_WINDOWS; w++) {
        if (lanes) { u32 l = 0; while (ve_window_of_lane(l) != w) l++; lanes[w] = l; }
        if (groups) groups[w] = ve_group_slot(ve_group_of_window(w));
    }
    return BP_OK;
}
