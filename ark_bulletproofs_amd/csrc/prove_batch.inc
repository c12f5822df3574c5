// Included by arkbp.hip after r1cs_host.inc.  bp_prover_prove_batch: many statements in one call, the inner-product arguments of
// like-sized small statements in LOCKSTEP groups (small_batch.cuh).
//
// FRONT GROUPS (BP_TUNE_PROVE_BATCH_FRONT = 1, pf_* below): an instance whose argument runs over the direct window tables and whose
// constraints can be indexed (HostCsc) runs EVERY stage group-wide.  Instances of equal phase-1 multiplier count n1 form a front group:
// one import launch and one k_dt_accum_multi launch give all A_I1 / A_O1 / S1, ONE host wait.  The randomized phases run on the calling
// thread; the survivors are re-partitioned by padded size N and every part goes on as a group of its own: the phase-2 TranscriptRng
// draws on the ctx's host pool, one import launch for the whole witness, the phase-2 commitments (ONE wait), then ztables / flatten /
// t(x) / the T commitments behind one another (ONE wait), l(x) / r(x) straight into the slots pb_run_group reads, and the lockstep
// rounds.  A member that stops qualifying after its randomized phase continues through r1cs_prove's resume entry.
//
// Every other instance runs r1cs_prove up to its inner-product argument (commitments, randomized phase, flatten, t(x), evaluations — on
// the ctx's single-proof workspaces, one instance after the other, as bp_prover_prove would; with the knob at 0 every instance does).
// An instance whose argument runs over the direct window tables then hands a, b and its factor vectors to the open group of its padded
// size N (IpaDefer) instead of running lg N rounds of its own.  A group runs when it is full, when an instance of another size needs the arena, or at the end of the
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
    // ... and what the front stages keep there: the witness a_L, a_R, a_O and the t(x) partials in room of their own; s_L in the a2 | b2
    // pair and s_R, w_L, w_R, w_O in the rounds' scalar vectors — those are first written by round 1 / round 0, after l(x), r(x) are out
    size_t o_waL = 0, o_waR = 0, o_waO = 0, o_wsL = 0, o_wsR = 0, o_wwL = 0, o_wwR = 0, o_wwO = 0, o_tp = 0;
    size_t ts_off = 0, bl_off = 0;   // the group's t(x) sums (6 x 32 bytes per proof) and blinding factors (8 x 32): inside the wiped range
    size_t bd_off = 0;               // ... and the expansion jobs of BP_BLINDING_EXPANDED members (2 x BlindDesc per proof: they hold the keys)
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
        o_part = o_sR + pb_align((2 * N + 2) * 32);
        o_waL = o_part + pb_align((gf + 1) * 64); o_waR = o_waL + pb_align(N * 32); o_waO = o_waR + pb_align(N * 32); o_tp = o_waO + pb_align(N * 32);
        per_vec = o_tp + pb_align(gf * 6 * 32);
        o_wsL = o_a2; o_wsR = o_sL; o_wwL = o_sL + N * 32; o_wwR = o_sL + 2 * N * 32; o_wwO = o_sL + 3 * N * 32;   // (a2 | b2: >= 32 N bytes, sL | sR: >= 128 N)
        ts_off = per_vec * cap; bl_off = ts_off + pb_align(cap * 192);
        bd_off = bl_off + cap * 256;
        vec_end = bd_off + pb_align(cap * 2 * sizeof(BlindDesc));
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

template <class S> static void pb_inv_many(const F4* in, size_t count, F4* out) {   // (challenges are never zero)
    std::vector<F4> pref(count);
    F4 run = S::one();
    for (size_t i = 0; i < count; i++) { pref[i] = run; run = S::mul(run, in[i]); }
    F4 inv = S::inv(run);
    for (size_t i = count; i-- > 0;) { out[i] = S::mul(inv, pref[i]); inv = S::mul(inv, in[i]); }
}

static void pb_pool_ensure(bp_ctx* ctx, size_t B) {
    host_pool_ensure(ctx, B);
}
static void pb_on_pool(bp_ctx* ctx, size_t count, const std::function<void(size_t)>& fn) {
    if (!ctx->pool || count <= 1) { for (size_t c = 0; c < count; c++) fn(c); return; }
    ctx->pool->run(0, count, fn);
}
// the lg N rounds of every member's inner-product argument, then a and b.  On success the members' proofs are complete.
template <class C> static int pb_run_group(bp_ctx* ctx, PbGroup<C>& g) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
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
    pb_pool_ensure(ctx, B);
    const size_t chunk = 64, nchunks = (B + chunk - 1) / chunk;
    auto on_pool = [&](const std::function<void(size_t)>& fn) { pb_on_pool(ctx, nchunks, fn); };
    auto fill_desc = [&](size_t j, bool fold) {
        DtRoundDesc& d = hd[j];
        if (fold) { memcpy(d.u, u[j].v, 32); memcpy(d.ui, ui[j].v, 32); } else { memset(d.u, 0, 32); memset(d.ui, 0, 32); }
        memcpy(d.qw, g.mem[j].w.v, 32);
    };
    const double t_begin = now_s();
    for (size_t r = 0; r < lg; r++) {
        const size_t n = N >> (r + 1);
        const bool fold = r > 0;
        const IpaPlan plan = ipa_plan({IPA_FROZEN, n, 0, N, 0, 0, 1});   // (ipa_round_lr's direct route, every member's vectors frozen at N)
        for (size_t j = 0; j < B; j++) {
            fill_desc(j, fold);
            ipa_direct_jobs(ctx, plan, n, vec(j, L.o_sL), vec(j, L.o_sR), hj + 2 * j);
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
            for (size_t i = 2 * lo; i < 2 * hi; i++) pts[i] = jac_from_words(res + 12 * i);
            to_aff_many<C>(pts.data() + 2 * lo, 2 * (hi - lo), aff.data() + 2 * lo);
            for (size_t j = lo; j < hi; j++) {
                host::ProofData& pf = *g.mem[j].pf;
                pf.L_vec[r] = aff[2 * j]; pf.R_vec[r] = aff[2 * j + 1];
                u[j] = host::prove_round_challenge<C>(*g.mem[j].tr, aff[2 * j], aff[2 * j + 1]);
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


// ---- front groups ----------------------------------------------------------------------------------------------------------------
static constexpr size_t PF_PHASE1_MAX = 16384;   // most members of a front group (3 table sums each: launches are split below 65536 rows)

template <class C> struct PfMember {
    size_t k = 0;                       // instance index in the call
    bp_cs* s = nullptr;
    host::ConstraintSystem<C>* cs = nullptr;
    ProvePre<C>* pre = nullptr;
    const HostCsc* csc = nullptr;
    std::unique_ptr<HostCsc> csc_late;  // two-phase statements: indexed after the randomized phase
    size_t n1 = 0, n = 0, N = 0;
    A4 c1[3];                           // A_I1, A_O1, S1
    F4 bl2[3], tb[5];                   // i_b2, o_b2, s_b2; the blinding factors of T_1, T_3 .. T_6
    F4 y, z;
    F4 kappa2 = F4{{0, 0, 0, 0}};       // BP_BLINDING_EXPANDED: phase 2's key
    std::vector<F4> wV;
    F4 w;
    bool csc_ok = true;
    std::unique_ptr<HostRowIndex> widx; // a guarded member's row index (bp_prover_set_check)
    std::shared_ptr<const HostRowIndex> widx_shared;   // ... or the one of the recording it shares
    const HostRowIndex* row() const { return widx_shared ? widx_shared.get() : widx.get(); }
    bool unsat = false;                 // ... and what the check found
    bp_witness_report report;
};

static int pf_stage_ensure(bp_ctx* c, size_t bytes) { return pinned_ensure(c->h_pf, c->h_pf_cap, bytes, bytes / 4 + 4096); }
static int pb_stage_ensure(bp_ctx* c, size_t bytes) {   // the rounds' staging (pb_run_group)
    if (pinned_ensure(c->h_pb, c->h_pb_cap, bytes, 0)) { c->h_pb = nullptr; c->h_pb_cap = 0; g_err = "prove_batch: pinned staging"; return BP_E_HIP; }
    return BP_OK;
}
// workgroups per table sum, as pb_run_group sizes a round's
static size_t pf_nblk(size_t maxterms, size_t njobs) {
    const size_t units = maxterms * DT_UNITS_PER_TERM;
    size_t nblk = std::max<size_t>(1, (units + 63) / 64);
    if (nblk * njobs > 256) nblk = std::max<size_t>(1, std::min<size_t>(1024, (units + 127) / 128));
    return nblk;
}
// njobs table sums: k_dt_accum_multi (+ k_dt_finish), results at d_res[job]
template <class C> static int pf_accum(bp_ctx* ctx, const DtJob* d_jobs, size_t njobs, size_t nblk, u32* d_acc, u32* d_res) {
    ScopedK tk(ctx, BP_K_MSM_ACCUM);
    for (size_t lo = 0; lo < njobs; lo += 32768) {
        const size_t cnt = std::min<size_t>(32768, njobs - lo);
        hipLaunchKernelGGL(k_dt_accum_multi<C>, dim3((u32)nblk, (u32)cnt), dim3(256), 0, ctx->stream, ctx->dt_tab.as<u32>(), d_jobs + lo,
                           nblk == 1 ? d_res + lo * 24 : d_acc + lo * nblk * 24);
        if (nblk > 1) hipLaunchKernelGGL(k_dt_finish<C>, dim3((u32)cnt), dim3(256), 0, ctx->stream, (const u32*)(d_acc + lo * nblk * 24), (u32)nblk, d_res + lo * 24);
    }
    HIPCHK(hipGetLastError());
    ctx->dt_runs += njobs;
    return BP_OK;
}
static void pf_points_in(const void* res, size_t count, J4* out) { for (size_t i = 0; i < count; i++) out[i] = jac_from_words((const u64*)res + 12 * i); }

// Phase 1 of a front group (equal n1): A_I1, A_O1, S1 of every member into its transcript
template <class C> static int pf_phase1(bp_ctx* ctx, std::vector<PfMember<C>>& mem, StageTimes& tm) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    const size_t B = mem.size(), n1 = mem[0].n1;
    const bool expanded = mem[0].pre->mode == BP_BLINDING_EXPANDED;   // (a front group holds members of ONE mode: cs_prove_batch)
    const size_t nv = expanded ? 3 : 5;                              // vectors that come through the staging
    hipStream_t st = ctx->stream;
    pb_pool_ensure(ctx, B);
    std::vector<J4> pts(3 * B);
    double t0 = now_s();
    if (n1 == 0) {   // no multipliers in this phase (a k-shuffle's phase 1): single Pedersen terms on the host's tables
        host::PedersenGens<C> pc; pc.B = ctx->pc_B; pc.B_blinding = ctx->pc_Bb;
        pb_on_pool(ctx, B, [&](size_t j) {
            const ProvePre<C>& pre = *mem[j].pre;
            pts[3 * j] = pc.commit_jac(S::zero(), pre.i_b1); pts[3 * j + 1] = pc.commit_jac(S::zero(), pre.o_b1); pts[3 * j + 2] = pc.commit_jac(S::zero(), pre.s_b1);
        });
    } else {
        const size_t vb = pb_align(n1 * 32), p1 = 5 * vb, bl_off = p1 * B;             // the arena, for this phase: [B x 5 vectors | blinding factors | expansion jobs]
        const size_t bd_off = bl_off + pb_align(B * 96), ar_end = bd_off + (expanded ? pb_align(B * sizeof(BlindDesc)) : 0);
        const size_t nblk = pf_nblk(2 * n1 + 1, 3 * B);
        const size_t s_bl = B * nv * n1 * 32, s_bd = s_bl + pb_align(B * 96), s_jobs = s_bd + (expanded ? pb_align(B * sizeof(BlindDesc)) : 0), s_res = s_jobs + pb_align(3 * B * sizeof(DtJob)), s_end = s_res + 3 * B * 96;
        const size_t a_acc = pb_align(3 * B * sizeof(DtJob)), a_res = a_acc + pb_align(3 * B * nblk * 96), a_end = a_res + 3 * B * 96;
        BPCHK(ctx->pb_arena.ensure(ar_end));
        BPCHK(ctx->pf_aux.ensure(a_end));
        BPCHK(pf_stage_ensure(ctx, s_end));
        char* hs = (char*)ctx->h_pf;
        char* ar = (char*)ctx->pb_arena.p;
        char* ax = (char*)ctx->pf_aux.p;
        DtJob* hj = (DtJob*)(hs + s_jobs);
        pb_on_pool(ctx, B, [&](size_t j) {
            const host::ConstraintSystem<C>& cs = *mem[j].cs;
            const ProvePre<C>& pre = *mem[j].pre;
            char* w = hs + j * nv * n1 * 32;
            const F4* src[5] = {cs.a_L.data(), cs.a_R.data(), cs.a_O.data(), pre.s_L.data(), pre.s_R.data()};
            for (size_t v = 0; v < nv; v++) memcpy(w + v * n1 * 32, src[v], n1 * 32);
            if (expanded) {
                BlindDesc& bd = ((BlindDesc*)(hs + s_bd))[j];
                memset(&bd, 0, sizeof bd);
                S::to_bytes((host::u8*)bd.key, pre.kappa1);
                bd.slot = (u32)j; bd.first = 0; bd.count = (u32)n1;
            }
            const F4 bl[3] = {pre.i_b1, pre.o_b1, pre.s_b1};
            memcpy(hs + s_bl + j * 96, bl, 96);
            const u32* base = (const u32*)(ar + j * p1);
            const u32* blp = (const u32*)(ar + bl_off + j * 96);
            const u32* xs[3] = {base, base + 2 * vb / 4, base + 3 * vb / 4};
            const u32* ys[3] = {base + vb / 4, nullptr, base + 4 * vb / 4};
            dt_commit_jobs<C>(ctx, hj + 3 * j, xs, ys, 0, n1, nullptr, blp);
        });
        tm.upload += now_s() - t0; t0 = now_s();
        PfGeom geo; memset(&geo, 0, sizeof geo);
        geo.arena = ar; geo.per_proof = p1; geo.aL = 0; geo.aR = (u32)vb; geo.aO = (u32)(2 * vb); geo.sL = (u32)(3 * vb); geo.sR = (u32)(4 * vb);
        hipLaunchKernelGGL(k_pf_import<FrP>, dim3((u32)((nv * n1 + 255) / 256), (u32)B), dim3(256), 0, st, (const u32*)hs, (const PfDesc*)nullptr, (u32)n1, (u32)nv, geo);
        if (expanded) {   // s_L, s_R of every member from its key: one launch for the group
            HIPCHK(hipMemcpyAsync(ar + bd_off, hs + s_bd, B * sizeof(BlindDesc), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_blind_expand_multi<FrP>, dim3((u32)((2 * n1 + 255) / 256), (u32)B), dim3(256), 0, st, (const BlindDesc*)(ar + bd_off), ar, (unsigned long long)p1, geo.sL, geo.sR);
            ctx->bx_scalars += 2 * n1 * B; ctx->bx_launches++;
        }
        HIPCHK(hipMemcpyAsync(ar + bl_off, hs + s_bl, B * 96, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ax, hs + s_jobs, 3 * B * sizeof(DtJob), hipMemcpyHostToDevice, st));
        BPCHK((pf_accum<C>(ctx, (const DtJob*)ax, 3 * B, nblk, (u32*)(ax + a_acc), (u32*)(ax + a_res))));
        HIPCHK(hipMemcpyAsync(hs + s_res, ax + a_res, 3 * B * 96, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemsetAsync(ar, 0, ar_end, st));   // secret hygiene: this phase's copy of the witness (and the keys)
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        ctx->pf_waits++;
        pf_points_in(hs + s_res, 3 * B, pts.data());
        memset(hs, 0, s_jobs);   // the staged witness, blinding factors and keys
    }
    const size_t chunk = 64, nchunks = (B + chunk - 1) / chunk;
    std::vector<A4> aff(3 * B);
    pb_on_pool(ctx, nchunks, [&](size_t c) {
        const size_t lo = c * chunk, hi = std::min(B, lo + chunk);
        to_aff_many<C>(pts.data() + 3 * lo, 3 * (hi - lo), aff.data() + 3 * lo);
        for (size_t j = lo; j < hi; j++) {
            for (int o = 0; o < 3; o++) mem[j].c1[o] = aff[3 * j + o];
            host::prove_append_phase<C>(*mem[j].cs->tr, 1, aff[3 * j], aff[3 * j + 1], aff[3 * j + 2]);
        }
    });
    tm.commit_msm += now_s() - t0;
    return BP_OK;
}

// A part of a front group after the randomized phases (equal padded size N): everything up to and including the lockstep rounds.
// Members whose constraints cannot be indexed after all come back in `leavers` (nothing of theirs was touched).
template <class C> static int pf_run_part_stages(bp_ctx* ctx, std::vector<PfMember<C>*>& part, size_t N, std::vector<host::ProofData>& pfs, StageTimes& tm,
                                                 std::vector<PfMember<C>*>& leavers, size_t& secret_stage_bytes) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    typedef host::Grp<C> G;
    typedef host::TP<C> TP;
    hipStream_t st = ctx->stream;
    pb_pool_ensure(ctx, part.size());
    double t0 = now_s();
    // the constraint index of the two-phase members
    pb_on_pool(ctx, part.size(), [&](size_t j) {
        PfMember<C>& m = *part[j];
        const HostCsc* have = m.cs->own_empty() && m.s->csc_shared ? m.s->csc_shared.get() : m.s->csc.get();
        if (m.s->check) {   // (a like-prover that recorded nothing itself: the recording's index, built once)
            if (m.cs->base && m.cs->own_empty()) m.widx_shared = host::shared_row_index<C>(*m.cs->base, m.cs->v.size(), WC_PIECE);
            if (!m.widx_shared) { m.widx.reset(new HostRowIndex()); if (!build_row_index<C>(*m.cs, WC_PIECE, *m.widx)) { m.csc_ok = false; return; } }   // (r1cs_prove reports it)
        }
        if (have && have->n == m.n && have->q == m.cs->num_constraints()) { m.csc = have; return; }
        m.csc_late.reset(new HostCsc());
        m.csc_ok = build_host_csc<C>(*m.cs, *m.csc_late);
        m.csc = m.csc_late.get();
    });
    {
        std::vector<PfMember<C>*> keep;
        for (auto* m : part) (m->csc_ok ? keep : leavers).push_back(m);
        part.swap(keep);
    }
    tm.flatten += now_s() - t0;
    const size_t B = part.size();
    if (!B) return BP_OK;
    PbLayout L; L.make(N, B);
    BPCHK(ctx->pb_arena.ensure(L.total));
    BPCHK(pb_stage_ensure(ctx, L.stage_bytes));
    // the aux buffer (32-bit words) and the pinned staging
    std::vector<PfDesc> descs(B);
    const bool expanded = part[0]->pre->mode == BP_BLINDING_EXPANDED;   // (all members alike: they come from one front group)
    const size_t nv = expanded ? 3 : 5;
    size_t nmax = 0, nzmax = 0, B2 = 0, in_words = 0, NG = 0;   // NG: guarded members (bp_prover_set_check); their flags lie behind the T results
    const size_t a_jobs2 = pb_align(B * sizeof(PfDesc));
    for (size_t j = 0; j < B; j++) if (part[j]->n > part[j]->n1) B2++;
    for (size_t j = 0; j < B; j++) if (part[j]->row()) NG++;
    const size_t a_jobsT = a_jobs2 + pb_align(3 * B2 * sizeof(DtJob)), a_data = a_jobsT + pb_align(5 * B * sizeof(DtJob));
    size_t at = a_data;
    std::map<const HostCsc*, size_t> first_of;   // like-provers of one recording point at ONE copy of its index and coefficient table
    std::vector<char> owns(B, 1);
    for (size_t j = 0; j < B; j++) {
        const PfMember<C>& m = *part[j];
        PfDesc& d = descs[j];
        memset(&d, 0, sizeof d);
        const size_t nnz = m.csc->ment.size(), nc = m.csc->coefs.size();
        d.n = (u32)m.n; d.n1 = (u32)m.n1; d.nzhi = (u32)((m.csc->q + 1) >> 8) + 1;
        d.in_off = in_words; in_words += nv * m.n * 8;
        nmax = std::max(nmax, m.n); nzmax = std::max<size_t>(nzmax, d.nzhi);
        const auto seen = first_of.find(m.csc);
        if (seen != first_of.end()) { const PfDesc& f = descs[seen->second]; d.moff = f.moff; d.ment = f.ment; d.mc = f.mc; d.coefs = f.coefs; owns[j] = 0; continue; }
        first_of[m.csc] = j;
        d.moff = (u32)(at / 4); at += pb_align((m.n + 1) * 4);
        d.ment = (u32)(at / 4); at += pb_align(std::max<size_t>(nnz, 1) * 4);
        d.mc = (u32)(at / 4); at += pb_align(std::max<size_t>(nnz, 1) * 4);
        d.coefs = (u32)(at / 4); at += pb_align(nc * 32);
    }
    const size_t a_u2 = at;                       // [B][96] scalars: z^(2^j) (32), y^(2^k) | y^-(2^k) (64)
    const size_t a_xu = a_u2 + B * 96 * 32;
    at = a_xu + pb_align(B * sizeof(PfXu));
    for (size_t j = 0; j < B; j++) {
        descs[j].ztab = (u32)((a_u2 + j * 96 * 32) / 4); descs[j].ypow = descs[j].ztab + 32 * 8;
        descs[j].Z = (u32)(at / 4); at += (256 + (size_t)descs[j].nzhi) * 32;
    }
    const size_t nblk2 = B2 ? pf_nblk(2 * (nmax - part[0]->n1) + 1, 3 * B2) : 1;
    const size_t a_acc2 = pb_align(at), a_res2 = a_acc2 + pb_align(3 * B2 * nblk2 * 96), a_resT = a_res2 + pb_align(3 * B2 * 96), a_flags = a_resT + 5 * B * 96, a_end = a_flags + NG * 16;
    if (a_end >= ((size_t)1 << 34)) { g_err = "prove_batch: a front group's tables exceed 16 GB"; return BP_E_ARG; }
    BPCHK(ctx->pf_aux.ensure(a_end));
    const size_t s_bl = in_words * 4, s_bd = s_bl + B * 256, s_u1 = s_bd + (expanded ? pb_align(B * 2 * sizeof(BlindDesc)) : 0), s_u2 = s_u1 + a_u2, s_xu = s_u2 + B * 96 * 32, s_res2 = s_xu + pb_align(B * sizeof(PfXu)),
                 s_ts = s_res2 + pb_align(3 * B2 * 96), s_resT = s_ts + pb_align(B * 192), s_end = s_resT + 5 * B * 96 + NG * 16;
    BPCHK(pf_stage_ensure(ctx, s_end));
    secret_stage_bytes = s_u1;   // the witness, the blinding factors and the keys, in front of everything public
    char* hs = (char*)ctx->h_pf;
    char* ar = (char*)ctx->pb_arena.p;
    char* ax = (char*)ctx->pf_aux.p;
    PfGeom geo; memset(&geo, 0, sizeof geo);
    geo.arena = ar; geo.per_proof = L.per_vec;
    geo.aL = (u32)L.o_waL; geo.aR = (u32)L.o_waR; geo.aO = (u32)L.o_waO; geo.sL = (u32)L.o_wsL; geo.sR = (u32)L.o_wsR;
    geo.wL = (u32)L.o_wwL; geo.wR = (u32)L.o_wwR; geo.wO = (u32)L.o_wwO; geo.tpart = (u32)L.o_tp;
    geo.a = 0; geo.b = (u32)L.o_b; geo.cG = (u32)L.o_cG; geo.cH = (u32)L.o_cH;
    geo.tsum = (u32*)(ar + L.ts_off);
    auto wit = [&](size_t j, size_t off) { return (const u32*)(ar + j * L.per_vec + off); };
    std::vector<size_t> job2_of(B, 0);
    { size_t q = 0; for (size_t j = 0; j < B; j++) if (part[j]->n > part[j]->n1) job2_of[j] = q++; }
    DtJob* hj2 = (DtJob*)(hs + s_u1 + a_jobs2);
    DtJob* hjT = (DtJob*)(hs + s_u1 + a_jobsT);
    // phase-2 blinding draws: the Keccak chain is sequential inside a proof and independent across proofs
    t0 = now_s();
    pb_on_pool(ctx, B, [&](size_t j) {
        PfMember<C>& m = *part[j];
        ProvePre<C>& pre = *m.pre;
        host::prove_draw_phase2<C>(*pre.rng, m.n > m.n1, expanded, m.n1, m.n, m.bl2, m.kappa2, pre.s_L, pre.s_R);
        host::prove_draw_t<C>(*pre.rng, m.tb);
    });
    tm.rng += now_s() - t0; t0 = now_s();
    // staging of the witness, the descriptors, the jobs of both commitment stages, the constraint index and its coefficients
    pb_on_pool(ctx, B, [&](size_t j) {
        PfMember<C>& m = *part[j];
        ProvePre<C>& pre = *m.pre;
        const size_t n = m.n, n1 = m.n1;
        const bool has2 = n > n1;
        char* w = hs + descs[j].in_off * 4;
        const F4* src[5] = {m.cs->a_L.data(), m.cs->a_R.data(), m.cs->a_O.data(), pre.s_L.data(), pre.s_R.data()};
        for (size_t v = 0; v < nv; v++) memcpy(w + v * n * 32, src[v], n * 32);
        if (expanded) {   // both phases' vectors again (phase 1's copy went with that phase's arena): two jobs, an empty phase has count 0
            BlindDesc* bd = (BlindDesc*)(hs + s_bd) + 2 * j;
            memset(bd, 0, 2 * sizeof(BlindDesc));
            S::to_bytes((host::u8*)bd[0].key, pre.kappa1); bd[0].slot = (u32)j; bd[0].first = 0; bd[0].count = (u32)n1;
            S::to_bytes((host::u8*)bd[1].key, m.kappa2); bd[1].slot = (u32)j; bd[1].first = (u32)n1; bd[1].count = (u32)(n - n1);
        }
        F4 bl[8] = {m.bl2[0], m.bl2[1], m.bl2[2], m.tb[0], m.tb[1], m.tb[2], m.tb[3], m.tb[4]};
        memcpy(hs + s_bl + j * 256, bl, 256);
        const u32* blp = (const u32*)(ar + L.bl_off + j * 256);
        if (has2) {
            const size_t n2 = n - n1;
            const u32* xs[3] = {wit(j, L.o_waL) + n1 * 8, wit(j, L.o_waO) + n1 * 8, wit(j, L.o_wsL) + n1 * 8};
            const u32* ys[3] = {wit(j, L.o_waR) + n1 * 8, nullptr, wit(j, L.o_wsR) + n1 * 8};
            dt_commit_jobs<C>(ctx, hj2 + 3 * job2_of[j], xs, ys, n1, n2, nullptr, blp);
        }
        dt_t_jobs<C>(hjT + 5 * j, geo.tsum + j * 6 * 8, nullptr, blp + 8 * 3);
        char* u1 = hs + s_u1;
        memcpy(u1 + j * sizeof(PfDesc), &descs[j], sizeof(PfDesc));
        const HostCsc& cc = *m.csc;
        if (!owns[j]) return;
        memcpy(u1 + (size_t)descs[j].moff * 4, cc.moff.data(), (n + 1) * 4);
        if (!cc.ment.empty()) { memcpy(u1 + (size_t)descs[j].ment * 4, cc.ment.data(), cc.ment.size() * 4); memcpy(u1 + (size_t)descs[j].mc * 4, cc.mc.data(), cc.mc.size() * 4); }
        F4* co = (F4*)(u1 + (size_t)descs[j].coefs * 4);
        for (size_t i = 0; i < cc.coefs.size(); i++) co[i] = to_resident<FrP>(cc.coefs[i]);
    });
    tm.upload += now_s() - t0; t0 = now_s();
    HIPCHK(hipMemcpyAsync(ax, hs + s_u1, a_u2, hipMemcpyHostToDevice, st));   // descriptors, jobs, constraint indices, coefficients: one copy
    HIPCHK(hipMemcpyAsync(ar + L.bl_off, hs + s_bl, B * 256, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_pf_import<FrP>, dim3((u32)((nv * nmax + 255) / 256), (u32)B), dim3(256), 0, st, (const u32*)hs, (const PfDesc*)ax, 0u, (u32)nv, geo);
    if (expanded) {
        size_t total = 0;
        for (size_t j = 0; j < B; j++) total += 2 * part[j]->n;
        HIPCHK(hipMemcpyAsync(ar + L.bd_off, hs + s_bd, B * 2 * sizeof(BlindDesc), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_blind_expand_multi<FrP>, dim3((u32)((2 * nmax + 255) / 256), (u32)(2 * B)), dim3(256), 0, st, (const BlindDesc*)(ar + L.bd_off), ar, (unsigned long long)L.per_vec, geo.sL, geo.sR);
        ctx->bx_scalars += total; ctx->bx_launches++;
    }
    HIPCHK(hipGetLastError());
    // the guard: gates and constraints of every guarded member over its arena slices, ONE launch sequence; no wait of its own
    WcRun<C> wc;
    std::vector<size_t> wc_member;
    for (size_t j = 0; j < B; j++) {
        if (!part[j]->row()) continue;
        WcItem<C> it; it.cs = part[j]->cs; it.idx = part[j]->row(); it.aL = wit(j, L.o_waL); it.aR = wit(j, L.o_waR); it.aO = wit(j, L.o_waO);
        wc.items.push_back(it); wc_member.push_back(j);
    }
    if (NG) { BPCHK(wc_enqueue<C>(ctx, wc, (u32*)(ax + a_flags))); BPCHK(wc_wipe_dev<C>(ctx, wc)); }
    std::vector<A4> aff2(3 * B2);
    if (B2) {
        BPCHK((pf_accum<C>(ctx, (const DtJob*)(ax + a_jobs2), 3 * B2, nblk2, (u32*)(ax + a_acc2), (u32*)(ax + a_res2))));
        HIPCHK(hipMemcpyAsync(hs + s_res2, ax + a_res2, 3 * B2 * 96, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        ctx->pf_waits++;
    }
    tm.commit_msm += now_s() - t0; t0 = now_s();
    // A_I2, A_O2, S2 -> y, z; the power tables; wV
    const size_t chunk = 64, nchunks = (B + chunk - 1) / chunk;
    std::vector<J4> pts2(3 * B2);
    if (B2) pf_points_in(hs + s_res2, 3 * B2, pts2.data());
    {   // (one inversion per chunk of the phase-2 members)
        const size_t nc2 = (B2 + chunk - 1) / chunk;
        pb_on_pool(ctx, nc2, [&](size_t c) { const size_t lo = c * chunk, hi = std::min(B2, lo + chunk); to_aff_many<C>(pts2.data() + 3 * lo, 3 * (hi - lo), aff2.data() + 3 * lo); });
    }
    pb_on_pool(ctx, B, [&](size_t j) {
        PfMember<C>& m = *part[j];
        host::Transcript& tr = *m.cs->tr;
        host::ProofData& pf = pfs[m.k];
        const bool has2 = m.n > m.n1;
        pf.A_I1 = m.c1[0]; pf.A_O1 = m.c1[1]; pf.S1 = m.c1[2];
        pf.A_I2 = has2 ? aff2[3 * job2_of[j]] : G::aff_inf(); pf.A_O2 = has2 ? aff2[3 * job2_of[j] + 1] : G::aff_inf(); pf.S2 = has2 ? aff2[3 * job2_of[j] + 2] : G::aff_inf();
        host::prove_append_phase<C>(tr, 2, pf.A_I2, pf.A_O2, pf.S2);
        m.y = TP::challenge_scalar(tr, "y"); m.z = TP::challenge_scalar(tr, "z");
        F4* u2 = (F4*)(hs + s_u2) + j * 96;
        F4 ztab[32], ypw[64];
        host::prove_pow_tables<C>(m.z, m.y, ztab, ypw);
        for (int i = 0; i < 32; i++) u2[i] = to_resident<FrP>(ztab[i]);
        for (int i = 0; i < 64; i++) u2[32 + i] = to_resident<FrP>(ypw[i]);
        host::prove_wv<C>(*m.csc, ztab, m.cs->v.size(), m.wV);
    });
    HIPCHK(hipMemcpyAsync(ax + a_u2, hs + s_u2, B * 96 * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_r1cs_ztables_multi<C>, dim3((u32)((std::max<size_t>(256, nzmax) + 255) / 256), (u32)B), dim3(256), 0, st, (u32*)ax, (const PfDesc*)ax);
    hipLaunchKernelGGL(k_r1cs_flatten_multi<C>, dim3((u32)((nmax + 255) / 256), (u32)B), dim3(256), 0, st, (const u32*)ax, (const PfDesc*)ax, geo);
    HIPCHK(hipGetLastError());
    tm.flatten += now_s() - t0; t0 = now_s();
    {
        const u32 gb = (u32)((nmax + 255) / 256);
        ScopedK tk(ctx, BP_K_R1CS_POLY);
        hipLaunchKernelGGL(k_r1cs_poly_t_multi<C>, dim3(gb, (u32)B), dim3(256), 0, st, (const u32*)ax, (const PfDesc*)ax, geo);
        if (gb > 1) hipLaunchKernelGGL(k_r1cs_sum_multi<C>, dim3((u32)B), dim3(256), 0, st, geo, gb);
    }
    HIPCHK(hipGetLastError());
    BPCHK((pf_accum<C>(ctx, (const DtJob*)(ax + a_jobsT), 5 * B, 1, (u32*)nullptr, (u32*)(ax + a_resT))));
    HIPCHK(hipMemcpyAsync(hs + s_ts, ar + L.ts_off, B * 192, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hs + s_resT, ax + a_resT, 5 * B * 96 + NG * 16, hipMemcpyDeviceToHost, st));   // (the guard's flags ride behind the T results)
    HIPCHK(ctx_stream_wait(ctx));
    HIPCHK(hipGetLastError());
    ctx->pf_waits++;
    // a member whose witness fails stays in the group to the end (no other member's launches change) and is refused by the caller
    wc_wipe_host<C>(ctx, wc);
    for (size_t g = 0; g < NG; g++) {
        const u32* f = (const u32*)(hs + s_resT + 5 * B * 96) + 4 * g;
        PfMember<C>& m = *part[wc_member[g]];
        if (wc_flags_bad(f)) { m.unsat = true; host::witness_report_from_flags<C>(*m.cs, f, m.report); }
    }
    // T appends, u, x, t_x, t_x_blinding, e_blinding, w
    std::vector<J4> ptsT(5 * B);
    std::vector<A4> affT(5 * B);
    pf_points_in(hs + s_resT, 5 * B, ptsT.data());
    PfXu* hxu = (PfXu*)(hs + s_xu);
    pb_on_pool(ctx, nchunks, [&](size_t c) {
        const size_t lo = c * chunk, hi = std::min(B, lo + chunk);
        to_aff_many<C>(ptsT.data() + 5 * lo, 5 * (hi - lo), affT.data() + 5 * lo);
        for (size_t j = lo; j < hi; j++) {
            PfMember<C>& m = *part[j];
            host::Transcript& tr = *m.cs->tr;
            host::ProofData& pf = pfs[m.k];
            const ProvePre<C>& pre = *m.pre;
            F4 tco[6];
            memcpy(tco, hs + s_ts + j * 192, 192);
            const A4* Tc = affT.data() + 5 * j;
            pf.T_1 = Tc[0]; pf.T_3 = Tc[1]; pf.T_4 = Tc[2]; pf.T_5 = Tc[3]; pf.T_6 = Tc[4];
            const F4 b1[3] = {pre.i_b1, pre.o_b1, pre.s_b1};
            F4 u, x;
            host::prove_t_tail<C>(tr, Tc, tco, m.tb, m.wV, m.cs->v_blinding, b1, m.bl2, u, x, pf.t_x, pf.t_x_blinding, pf.e_blinding, m.w);
            memcpy(hxu[j].x, x.v, 32); memcpy(hxu[j].u, u.v, 32);
            TP::innerproduct_domain_sep(tr, N);
            pf.L_vec.resize(pb_lg(N)); pf.R_vec.resize(pb_lg(N));
        }
    });
    HIPCHK(hipMemcpyAsync(ax + a_xu, hs + s_xu, B * sizeof(PfXu), hipMemcpyHostToDevice, st));
    {
        ScopedK tk(ctx, BP_K_R1CS_POLY);
        hipLaunchKernelGGL(k_r1cs_poly_eval_multi<C>, dim3((u32)((N + 255) / 256), (u32)B), dim3(256), 0, st, (const u32*)ax, (const PfDesc*)ax, (const PfXu*)(ax + a_xu), geo, (u32)N);
    }
    HIPCHK(hipGetLastError());
    tm.poly += now_s() - t0;
    PbGroup<C> g;
    g.lay = L; g.open = true;
    for (size_t j = 0; j < B; j++) g.mem.push_back(PbMember<C>{part[j]->k, part[j]->cs->tr, &pfs[part[j]->k], part[j]->w});
    BPCHK(pb_run_group<C>(ctx, g));
    ctx->pf_instances += B; ctx->pf_groups++;
    return BP_OK;
}
// ... and the secret hygiene of a part on EVERY way out: the host copies of the blinding vectors (r1cs_prove's closing wipe), the
// witness and blinding factors in the pinned staging, and — when a stage failed before the group's closing memset — the arena
template <class C> static int pf_run_part(bp_ctx* ctx, std::vector<PfMember<C>*>& part, size_t N, std::vector<host::ProofData>& pfs, StageTimes& tm,
                                          std::vector<PfMember<C>*>& leavers) {
    typedef host::Fld<typename C::Fr> S;
    size_t secret_stage_bytes = 0;
    const std::vector<PfMember<C>*> all = part;
    const int rc = pf_run_part_stages<C>(ctx, part, N, pfs, tm, leavers, secret_stage_bytes);
    for (auto* m : all) {
        if (std::find(leavers.begin(), leavers.end(), m) != leavers.end()) continue;   // (a leaver's vectors are r1cs_prove's to wipe)
        for (auto& x : m->pre->s_L) x = S::zero();
        for (auto& x : m->pre->s_R) x = S::zero();
        m->pre->kappa1 = S::zero(); m->kappa2 = S::zero();
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);   // (nothing reads the staging any more)
        if (ctx->pb_arena.p) (void)hipMemsetAsync(ctx->pb_arena.p, 0, ctx->pb_arena.cap, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
    if (ctx->h_pf && secret_stage_bytes) memset(ctx->h_pf, 0, std::min(secret_stage_bytes, ctx->h_pf_cap));
    return rc;
}

template <class C>
static int cs_prove_batch(bp_ctx* c, size_t count, bp_cs* const* hs, uint8_t* proofs_out, size_t proof_stride, size_t* proof_lens, int* status, double* timing) {
    const double t_begin = now_s();
    c->pb_ipa_s = 0;
    std::vector<int> st(count, BP_OK);
    std::vector<host::ProofData> pfs(count);
    std::vector<char> grouped(count, 0);
    StageTimes tm;
    std::vector<std::pair<uint64_t, bp_witness_report>> unsat;   // the instances the guard refuses (bp_ctx_last_unsatisfied)
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
    // (members of both blinding modes may arrive in one call; a front group holds one mode, so equal sizes are ordered by mode)
    auto mode_of = [&](size_t k) { return C::ID == 0 ? hs[k]->pre0.mode : hs[k]->pre1.mode; };
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return std::make_pair(hs[a]->cs<C>()->a_L.size(), mode_of(a)) < std::make_pair(hs[b]->cs<C>()->a_L.size(), mode_of(b));
    });
    // one instance through r1cs_prove (resume1: it left a front group after its randomized phase); `left`: instances still to come
    auto prove_single = [&](size_t k, size_t left, const A4* resume1) {
        bp_cs* s = hs[k];
        auto* pre = C::ID == 0 ? (ProvePre<C>*)&s->pre0 : (ProvePre<C>*)&s->pre1;
        const HostCsc* csc = cs_index<C>(s);
        IpaDefer defer;
        defer.take = [&](size_t N, IpaDeferSlot& slot) -> bool {
            if (grp.open && (grp.lay.N != N || grp.mem.size() >= grp.lay.cap)) flush();
            if (!grp.open) {
                size_t cap = cap_knob ? cap_knob : std::max<size_t>(1, std::min(PB_GROUP_MAX, PB_ARENA_BUDGET / PbLayout::per_proof(N)));
                cap = std::max<size_t>(1, std::min(cap, left));
                grp.lay.make(N, cap);
                if (c->pb_arena.ensure(grp.lay.total)) return false;
                if (pb_stage_ensure(c, grp.lay.stage_bytes)) return false;
                grp.open = true;
            }
            const size_t j = grp.mem.size();
            char* base = (char*)c->pb_arena.p + j * grp.lay.per_vec;
            slot.a = (u32*)base; slot.b = (u32*)(base + grp.lay.o_b); slot.cG = (u32*)(base + grp.lay.o_cG); slot.cH = (u32*)(base + grp.lay.o_cH);
            return true;
        };
        s->consumed = true; s->running = true;
        WcGuard guard; guard.on = s->check;
        const int rc = r1cs_prove<C>(c, *s->cs<C>(), s->rng32, pfs[k], tm, pre, csc, &defer, resume1, s->check ? &guard : nullptr);
        s->running = false;
        if (rc == BP_E_UNSATISFIED) unsat.emplace_back((uint64_t)k, guard.report);
        if (defer.taken) {
            grp.mem.push_back(PbMember<C>{k, s->cs<C>()->tr, &pfs[k], defer.w});
            pfs[k].L_vec.resize(pb_lg(defer.N)); pfs[k].R_vec.resize(pb_lg(defer.N));
            grouped[k] = 1;
            if (rc) st[k] = rc;   // (a device error after the hand-over: the group's result for this instance is dropped)
        } else {
            st[k] = rc;
            if (!rc) c->pb_single++;
        }
    };
    // does instance k run its front stages in a group?  (what can be known before its randomized phase)
    // the tables are built when the first candidate appears (as r1cs_prove builds them for the first small statement); a failure there
    // means "does not qualify": the instance takes the single route and reports the error as its own status
    const size_t reach_max = c->tune_pb_front && c->shard_world <= 1 && c->tune_direct_max >= 2 ? std::min(c->gens_cap, c->tune_direct_max) : 0;
    size_t reach = 0;
    bool dt_tried = false;
    auto qualifies = [&](size_t k) -> bool {
        bp_cs* s = hs[k];
        const host::ConstraintSystem<C>& cs = *s->cs<C>();
        if (reach_max < 2 || cs.a_L.size() > reach_max) return false;
        if (cs.deferred.empty() && (cs.a_L.size() < 2 || host::next_pow2(cs.a_L.size()) > reach_max)) return false;
        if (!dt_tried) {
            dt_tried = true;
            bool ready = false;
            if (dt_ensure<C>(c, 2, ready) == BP_OK && ready) reach = std::min(c->dt_cap, c->tune_direct_max);   // (built for min(generators, BP_TUNE_DIRECT_MAX))
        }
        if (!reach || cs.a_L.size() > reach) return false;
        if (!cs.deferred.empty()) return true;   // two-phase: its padded size and its constraint index exist after the randomized phase
        const size_t N = host::next_pow2(cs.a_L.size());
        if (cs.a_L.size() == 0 || N < 2 || N > reach) return false;
        const HostCsc* csc = cs_index<C>(s);
        return csc && csc->n == cs.a_L.size() && csc->q == cs.num_constraints();
    };
    for (size_t oi = 0; oi < count;) {
        if (!qualifies(order[oi])) { prove_single(order[oi], count - oi, nullptr); oi++; continue; }
        // a front group: the qualifying instances that follow with the same phase-1 multiplier count
        const size_t n1 = hs[order[oi]]->cs<C>()->a_L.size();
        const int mode1 = mode_of(order[oi]);
        size_t cap1 = cap_knob ? cap_knob : std::min(PF_PHASE1_MAX, std::max<size_t>(1, PB_ARENA_BUDGET / (5 * pb_align(std::max<size_t>(n1, 1) * 32) + 256)));
        std::vector<PfMember<C>> mem;
        while (oi < count && mem.size() < cap1 && hs[order[oi]]->cs<C>()->a_L.size() == n1 && mode_of(order[oi]) == mode1 && qualifies(order[oi])) {
            PfMember<C> m;
            bp_cs* sk = hs[order[oi]];
            m.k = order[oi]; m.s = sk; m.cs = sk->cs<C>(); m.pre = C::ID == 0 ? (ProvePre<C>*)&sk->pre0 : (ProvePre<C>*)&sk->pre1; m.n1 = n1;
            sk->consumed = true; sk->running = true;
            (void)prove_need_aO<C>(c, *m.cs);   // (the group's staging copies a_O from the host; a device witness came over at the entry)
            mem.push_back(std::move(m));
            oi++;
        }
        flush();   // (the arena is the front group's from here)
        int rc = pf_phase1<C>(c, mem, tm);
        // randomized phases, on the calling thread; a member that fails is dropped with its transcript where bp_prover_prove leaves it
        std::map<size_t, std::vector<PfMember<C>*>> parts;
        std::vector<PfMember<C>*> leavers;
        for (auto& m : mem) {
            if (rc) { st[m.k] = rc; continue; }
            const int r = m.cs->run_randomized();
            if (r) { st[m.k] = r; continue; }
            m.n = m.cs->a_L.size(); m.N = host::next_pow2(m.n);
            if (c->gens_cap < m.N) { st[m.k] = BP_E_GENS_LENGTH; continue; }
            if (m.n == 0 || m.N < 2 || m.N > reach) { leavers.push_back(&m); continue; }
            parts[m.N].push_back(&m);
        }
        for (auto& pr : parts) {
            const size_t N = pr.first;
            const size_t capN = cap_knob ? cap_knob : std::max<size_t>(1, std::min(PB_GROUP_MAX, PB_ARENA_BUDGET / PbLayout::per_proof(N)));
            for (size_t lo = 0; lo < pr.second.size(); lo += capN) {
                std::vector<PfMember<C>*> part(pr.second.begin() + lo, pr.second.begin() + std::min(pr.second.size(), lo + capN));
                const std::vector<PfMember<C>*> all = part;
                const int r = pf_run_part<C>(c, part, N, pfs, tm, leavers);
                for (auto* m : all) {
                    if (std::find(leavers.begin(), leavers.end(), m) != leavers.end()) continue;
                    grouped[m->k] = 1;
                    if (r) st[m->k] = r;
                    else if (m->unsat) { st[m->k] = BP_E_UNSATISFIED; unsat.emplace_back((uint64_t)m->k, m->report); }
                }
            }
        }
        for (auto& m : mem) m.s->running = false;
        // members that stopped qualifying: the rest of r1cs_prove on the single-proof workspaces
        for (auto* m : leavers) prove_single(m->k, 1, m->c1);
    }
    flush();
    std::sort(unsat.begin(), unsat.end(), [](const std::pair<uint64_t, bp_witness_report>& a, const std::pair<uint64_t, bp_witness_report>& b) { return a.first < b.first; });
    c->unsat.swap(unsat);
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
        BPCHK(cs_pair_check("prove_batch", c, h, k));
        BPCHK(cs_like_ready("prove_batch", h, k));
        BPCHK(cs_dev_witness_check("prove_batch", c, h, k));
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
    // (a witness in device memory comes to the host first: the front groups stage from host vectors, and no route of a batch keeps it resident)
    for (size_t k = 0; k < count; k++) BPCHK(cs_dev_witness_to_host(c, provers[k]));
    return c->curve == 0 ? cs_prove_batch<Secq>(c, count, provers, proofs_out, proof_stride, proof_lens, status, timing)
                         : cs_prove_batch<Zorro>(c, count, provers, proofs_out, proof_stride, proof_lens, status, timing);
}

template <class C> static int prover_commit_batch_t(bp_ctx* ctx, size_t count, bp_cs* const* hs, const size_t* m_each, const uint64_t* v, const uint64_t* blind,
                                                    uint64_t* V_xy, bp_var* vars) {
    size_t total = 0;
    for (size_t k = 0; k < count; k++) total += m_each[k];
    host::PedersenGens<C> pc; pc_pair<C>(ctx, pc);   // (every prover of the batch holds this pair: checked by the entry point)
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
        BPCHK(cs_pair_check("prover_commit_batch", c, h, k));
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
int bp_ctx_prove_batch_front_stats(bp_ctx* c, uint64_t* front_instances, uint64_t* front_groups, uint64_t* front_waits) {
    if (!c) return BP_E_ARG;
    if (front_instances) *front_instances = c->pf_instances;
    if (front_groups) *front_groups = c->pf_groups;
    if (front_waits) *front_waits = c->pf_waits;
    return BP_OK;
}
