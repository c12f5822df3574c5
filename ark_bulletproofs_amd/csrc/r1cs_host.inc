// Included by arkbp.hip after the MSM / IPA orchestration.  Host side of the R1CS prover and verifier:
// the sequential Fiat-Shamir skeleton of /root/reference/src/r1cs/prover.rs:454-831 and
// src/r1cs/verifier.rs:394-600 with every O(N) step dispatched to the HIP kernels.

struct StageTimes {  // seconds, host wall clock inside prove()
    double rng = 0, upload = 0, commit_msm = 0, flatten = 0, poly = 0, ipa = 0, total = 0;
};
static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// resident scalar words of an ark-Montgomery host value: (x * 2^256) * 2^5 = x * 2^261 (mod p), as an integer
// (pseudo-Mersenne fields keep plain residues on the device, arkbp_params.h P::PM: the canonical integer itself)
template <class P> static F4 to_resident(const F4& x) {
    if (P::PM) { F4 c; host::Fld<P>::to_canon(c.v, x); return c; }
    F4 r = x;
    for (int i = 0; i < 5; i++) r = host::Fld<P>::dbl(r);
    return r;
}

template <class C> static int upload_scalars(bp_ctx* ctx, u32* dst, const F4* src, size_t cnt) {
    if (!cnt) return BP_OK;
    HIPCHK(hipMemcpyAsync(dst, src, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_scalars_import<typename C::Fr>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, dst, dst, (u32)cnt);
    HIPCHK(hipGetLastError());
    return BP_OK;
}

// The same for the prover's big witness vectors (32 B x N each, pageable std::vector memory): an H2D copy from pageable memory goes
// through the runtime's own bounce buffers at ~2 GB/s and serialises ACROSS streams — with several proofs in flight that copy
// (168 MB per 2^20 proof) capped the whole pipeline.  Here the host thread copies into the ctx's pinned slab (parallel across the
// proofs' threads, ~10 GB/s each) and the DMA from pinned memory is asynchronous.  `slot` picks one of the ctx's slabs: each is
// used at most once per prove() call, and the previous call's copies are long complete.
static int upload_slab_ensure(bp_ctx* ctx, size_t bytes) { return pinned_ensure(ctx->h_upload, ctx->h_upload_cap, bytes, 4096); }
template <class C> static int upload_scalars_pinned(bp_ctx* ctx, u32* dst, const F4* src, size_t cnt, size_t slab_offset_bytes) {
    if (!cnt) return BP_OK;
    char* stage = (char*)ctx->h_upload + slab_offset_bytes;
    memcpy(stage, src, cnt * 32);
    HIPCHK(hipMemcpyAsync(dst, stage, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_scalars_import<typename C::Fr>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, dst, dst, (u32)cnt);
    HIPCHK(hipGetLastError());
    return BP_OK;
}

// the five witness vectors of a phase (a_L, a_R, a_O, s_L, s_R: cnt elements each) -> dst[0..4]: a small statement stages them in the
// pinned slab and ONE kernel reads them from there (k_scalars_import5); a large one keeps the asynchronous copies
static constexpr size_t UPLOAD_FUSED_MAX = 8192;
template <class C> static int upload_witness5(bp_ctx* ctx, u32* const dst[5], const F4* const src[5], size_t cnt, int nvec = 5 /* 3: a_L, a_R, a_O only (BP_BLINDING_EXPANDED) */) {
    if (!cnt) return BP_OK;
    if (cnt > UPLOAD_FUSED_MAX) {
        for (int v = 0; v < nvec; v++) BPCHK(upload_scalars_pinned<C>(ctx, dst[v], src[v], cnt, (size_t)v * cnt * 32));
        return BP_OK;
    }
    char* stage = (char*)ctx->h_upload;
    ImportList il; memset(&il, 0, sizeof il);
    il.nseg = nvec;
    for (int v = 0; v < nvec; v++) { memcpy(stage + (size_t)v * cnt * 32, src[v], cnt * 32); il.dst[v] = dst[v]; il.cnt[v] = (u32)cnt; }
    hipLaunchKernelGGL(k_scalars_import_multi<typename C::Fr>, dim3((u32)(((size_t)nvec * cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)stage, il);
    HIPCHK(hipGetLastError());
    return BP_OK;
}

// ---- blinding vectors from a key (BP_BLINDING_EXPANDED; the construction: blind.cuh) ------------------------------------------------
// W(key, t) on the host, as ark Montgomery words: the twin the device kernel is tested against (64-bit Montgomery arithmetic, nothing
// shared with blind.cuh but the definition)
template <class P> static F4 host_blind_scalar(const host::u8 key[32], u32 t) {
    typedef host::Fld<P> S;
    host::ChaChaRng prng(key);
    prng.ctr = t;
    prng.block();
    F4 lo, hi;
    memcpy(lo.v, prng.blk, 32); memcpy(hi.v, prng.blk + 8, 32);
    const F4 r2 = {{P::R2_64[0], P::R2_64[1], P::R2_64[2], P::R2_64[3]}};
    const F4 r = S::add(S::mul(lo, r2), S::mul(S::mul(hi, r2), r2));   // (lo + hi * 2^256) * 2^256 mod r; the products take any 256-bit operand
    memset(prng.k, 0, sizeof prng.k); memset(prng.blk, 0, sizeof prng.blk);
    return r;
}
template <class C> static void host_blind_expand(const F4& kappa, u64 j0, size_t count, F4* sL, F4* sR) {
    typedef typename C::Fr FrP;
    host::u8 key[32];
    host::Fld<FrP>::to_bytes(key, kappa);
    for (size_t i = 0; i < count; i++) {
        sL[i] = host_blind_scalar<FrP>(key, (u32)(2 * (j0 + i)));
        sR[i] = host_blind_scalar<FrP>(key, (u32)(2 * (j0 + i) + 1));
    }
    memset(key, 0, 32);
}
// s_L[0 .. count), s_R[0 .. count) at sL / sR (resident form) for the phase-local indices j0 .. j0 + count - 1: one launch, the key as
// a kernel argument
template <class C> static int blind_expand_launch(bp_ctx* ctx, const F4& kappa, u64 j0, size_t count, u32* sL, u32* sR) {
    if (!count) return BP_OK;
    if (j0 + count > ((u64)1 << 31)) { g_err = "blind_expand: indices reach 2^31"; return BP_E_ARG; }
    BlindKey key;
    host::Fld<typename C::Fr>::to_bytes((host::u8*)key.k, kappa);
    hipLaunchKernelGGL(k_blind_expand<typename C::Fr>, dim3((u32)((2 * count + 255) / 256)), dim3(256), 0, ctx->stream, key, (u32)j0, (u32)count, sL, sR);
    memset(&key, 0, sizeof key);
    HIPCHK(hipGetLastError());
    ctx->bx_scalars += 2 * count; ctx->bx_launches++;
    return BP_OK;
}
// test hook (include/arkbp.h bp_debug_blind_expand): the production kernel on the ctx's stream, its output exported back to ark words
template <class C> static int dbg_blind_expand(bp_ctx* c, const F4& k, uint64_t j0, size_t count, uint64_t* sL, uint64_t* sR) {
    typedef typename C::Fr FrP;
    BPCHK(c->io_scal.ensure(2 * count * 32)); BPCHK(c->io_out.ensure(2 * count * 32));
    u32* res = c->io_scal.as<u32>();
    u32* out = c->io_out.as<u32>();
    BPCHK(blind_expand_launch<C>(c, k, j0, count, res, res + count * 8));
    hipLaunchKernelGGL(k_scalars_export<FrP>, dim3((u32)((2 * count + 255) / 256)), dim3(256), 0, c->stream, (const u32*)res, out, (u32)(2 * count));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sL, out, count * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sR, out + count * 8, count * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemsetAsync(res, 0, 2 * count * 32, c->stream));
    HIPCHK(hipMemsetAsync(out, 0, 2 * count * 32, c->stream));
    HIPCHK(ctx_stream_wait(c));
    return BP_OK;
}

// The precomputed tables are multiples of the resident generators: whatever puts OTHER points there releases them (a shared view is
// let go, not freed).  They come back when asked for again (bp_gens_fold_tables, bp_gens_msm_tables; the direct tables on first use).
static void gens_tables_drop(bp_ctx* ctx) {
    for (DevBuf* b : {&ctx->ftab_G, &ctx->ftab_H, &ctx->fb_G, &ctx->fb_H, &ctx->fb_pc}) b->release();
    ctx->ftab_n = 0; ctx->ftab_first = 0; ctx->ftab_stride = 1;
    ctx->fb_cap = 0;
    ctx->dt_cap = 0;
}
// The ctx's PedersenGens { B, B_blinding } as the resident pair d_pc: every kernel and every table builder reads the two bases from
// there.  The pair is PedersenGens::default() (src/generators.rs:47-66) until bp_pedersen_gens_install puts the caller's there.
template <class C> static void pc_pair(bp_ctx* ctx, host::PedersenGens<C>& pc) {
    if (!ctx->pc_set) { const auto& d = host::PedersenGens<C>::default_ref(); ctx->pc_B = d.B; ctx->pc_Bb = d.B_blinding; ctx->pc_set = true; ctx->pc_custom = false; }
    pc.B = ctx->pc_B; pc.B_blinding = ctx->pc_Bb;
}
template <class C> static int pc_upload(bp_ctx* ctx) {
    host::PedersenGens<C> pc;
    pc_pair<C>(ctx, pc);
    uint64_t two[16];
    memcpy(two, pc.B.x.v, 32); memcpy(two + 4, pc.B.y.v, 32); memcpy(two + 8, pc.B_blinding.x.v, 32); memcpy(two + 12, pc.B_blinding.y.v, 32);
    BPCHK(ctx->d_pc.ensure(128));
    HIPCHK(hipMemcpyAsync(ctx->d_pc.p, two, 128, hipMemcpyHostToDevice, ctx->stream));   // (pageable: the copy has left `two` when the call returns)
    BPCHK(bp_points_import(ctx, ctx->d_pc.p, ctx->d_pc.p, 2));
    return BP_OK;
}
template <class C> static int gens_install(bp_ctx* ctx, const uint64_t* G_xy, const uint64_t* H_xy, size_t cap) {
    gens_tables_drop(ctx);   // (before the first byte changes)
    ctx->gens_derived = false;
    BPCHK(ctx->d_G.ensure(cap * 64 + 64)); BPCHK(ctx->d_H.ensure(cap * 64 + 64));
    HIPCHK(hipMemcpyAsync(ctx->d_G.p, G_xy, cap * 64, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->d_H.p, H_xy, cap * 64, hipMemcpyHostToDevice, ctx->stream));
    BPCHK(bp_points_import(ctx, ctx->d_G.p, ctx->d_G.p, cap));
    BPCHK(bp_points_import(ctx, ctx->d_H.p, ctx->d_H.p, cap));
    BPCHK(pc_upload<C>(ctx));   // the ctx keeps its pair: PedersenGens::default() unless bp_pedersen_gens_install put another there
    HIPCHK(ctx_stream_wait(ctx));
    ctx->gens_cap = cap;
    return BP_OK;
}
// BulletproofGens::new(cap, 1) (src/generators.rs:174-221) with the square roots on the GPU.  GeneratorsChain draws, per
// attempt, x = Fq::rand (8 words, repeated while x >= p) and `greatest` (1 word) — the stream position never depends on whether
// the attempt lands on the curve, so: the host walks the ChaCha20 word stream (cheap, sequential) and records every attempt;
// k_points_decompress tests them all (the accepted raw limbs ARE the Montgomery words, `greatest` is the 0x80 flag); the first
// `cap` successes in stream order are gathered into the resident table.
template <class C> static int derive_table_gpu(bp_ctx* ctx, char which, DevBuf& table, size_t cap) {
    typedef typename C::Fq FqP;
    hipStream_t st = ctx->stream;
    host::u8 msg[20]; memcpy(msg, "GeneratorsChain", 15); msg[15] = (host::u8)which; const u32 party = 0; memcpy(msg + 16, &party, 4);
    host::u8 h[64]; host::sha3_512(h, msg, 20);
    host::ChaChaRng prng(h);
    BPCHK(table.ensure(cap * 64 + 64));
    size_t have = 0;
    while (have < cap) {
        const size_t want = (cap - have) * 2 + (cap - have) / 8 + 64;
        std::vector<F4> xs(want); std::vector<u32> fl(want);
        for (size_t i = 0; i < want; i++) { xs[i] = host::rand_fe<FqP>(prng); fl[i] = ((int32_t)prng.next_u32()) < 0 ? 0x80u : 0u; }
        BPCHK(ctx->io_pts.ensure(want * 32)); BPCHK(ctx->io_scal.ensure(want * 4)); BPCHK(ctx->io_out.ensure(want * 64 + want * 4));
        HIPCHK(hipMemcpyAsync(ctx->io_pts.p, xs.data(), want * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->io_scal.p, fl.data(), want * 4, hipMemcpyHostToDevice, st));
        u32* d_xy = ctx->io_out.as<u32>();
        u32* d_ok = d_xy + want * 16;
        hipLaunchKernelGGL(k_points_decompress<C>, dim3((u32)((want + 255) / 256)), dim3(256), 0, st, ctx->io_pts.as<u32>(), ctx->io_scal.as<u32>(), d_xy, d_ok, (u32)want);
        std::vector<u32> ok(want);
        HIPCHK(hipMemcpyAsync(ok.data(), d_ok, want * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        std::vector<u32> idx;
        for (size_t i = 0; i < want && have + idx.size() < cap; i++) if (ok[i]) idx.push_back((u32)i);
        // attempts past the last accepted one are dropped: the chain is always re-derived from a fresh stream (increase_capacity)
        if (!idx.empty()) {
            HIPCHK(hipMemcpyAsync(ctx->io_scal.p, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_points_gather_import<C>, dim3((u32)((idx.size() + 255) / 256)), dim3(256), 0, st, d_xy, ctx->io_scal.as<u32>(),
                               table.as<u32>() + have * 16, (u32)idx.size());
            HIPCHK(ctx_stream_wait(ctx));
            HIPCHK(hipGetLastError());
            have += idx.size();
        }
    }
    return BP_OK;
}
template <class C> static int gens_derive(bp_ctx* ctx, size_t cap) {
    // deriving to a larger capacity extends the same chain: G[i], H[i] stay what they were for every i the fold tables and the MSM rows
    // cover, and those stay.  After caller-installed points, or down to fewer generators than before, they go.
    if (!ctx->gens_derived || cap < ctx->gens_cap) gens_tables_drop(ctx);
    ctx->gens_derived = false;
    BPCHK(derive_table_gpu<C>(ctx, 'G', ctx->d_G, cap));
    BPCHK(derive_table_gpu<C>(ctx, 'H', ctx->d_H, cap));
    BPCHK(pc_upload<C>(ctx));   // the ctx keeps its pair: PedersenGens::default() unless bp_pedersen_gens_install put another there
    HIPCHK(ctx_stream_wait(ctx));
    ctx->gens_cap = cap;
    ctx->gens_derived = true;
    ctx->dt_cap = 0;   // (the direct window tables are sized by the capacity: built again on first use)
    return BP_OK;
}
// bp_gens_check: the resident generators against party 0's chain, derived again as derive_table_gpu derives it — the same stream walk,
// the same k_points_decompress, the successes gathered in stream order — but in chunks of at most GENS_CHECK_CHUNK attempts, into
// scratch, and compared there with the resident slice (k_points_compare); the resident pair against the pair the ctx holds on the
// host.  Reads and compares only.  Scratch (all sized up front, so that no buffer moves under the counters):
//   io_out = [6 counters | attempts as points | ok flags | the gathered successes],   io_pts = the pair (ark, resident), then the attempts' x.
static constexpr size_t GENS_CHECK_CHUNK = (size_t)1 << 16;
template <class C> static int gens_check(bp_ctx* ctx, bp_gens_report* out) {
    typedef typename C::Fq FqP;
    hipStream_t st = ctx->stream;
    const size_t cap = ctx->gens_cap;
    const size_t wmax = (std::min(GENS_CHECK_CHUNK, cap * 2 + cap / 8 + 64) + 3) & ~(size_t)3;   // (a multiple of 4: the regions below stay 16-byte aligned)
    BPCHK(ctx->io_pts.ensure(std::max<size_t>(wmax * 32, 256))); BPCHK(ctx->io_scal.ensure(wmax * 4)); BPCHK(ctx->io_out.ensure(64 + wmax * (64 + 4 + 64)));
    unsigned long long* d_bad = ctx->io_out.as<unsigned long long>();
    unsigned long long* d_first = d_bad + BP_GENS_KINDS;
    u32* d_xy = ctx->io_out.as<u32>() + 16;
    u32* d_ok = d_xy + wmax * 16;
    u32* d_sel = d_ok + wmax;
    HIPCHK(hipMemsetAsync(d_bad, 0, BP_GENS_KINDS * 8, st));
    HIPCHK(hipMemsetAsync(d_first, 0xff, BP_GENS_KINDS * 8, st));
    {   // the pair: what the ctx holds on the host (default() or the installed one), imported into scratch
        host::PedersenGens<C> pc;
        pc_pair<C>(ctx, pc);
        uint64_t two[16];
        memcpy(two, pc.B.x.v, 32); memcpy(two + 4, pc.B.y.v, 32); memcpy(two + 8, pc.B_blinding.x.v, 32); memcpy(two + 12, pc.B_blinding.y.v, 32);
        u32* d_two = ctx->io_pts.as<u32>();
        HIPCHK(hipMemcpyAsync(d_two, two, 128, hipMemcpyHostToDevice, st));   // (pageable: the copy has left `two` when the call returns)
        BPCHK(bp_points_import(ctx, d_two, d_two + 32, 2));
        hipLaunchKernelGGL(k_points_compare<C>, dim3(1), dim3(256), 0, st, (const u32*)(d_two + 32), (const u32*)ctx->d_pc.as<u32>(), 2u, 0ull, d_bad + BP_GENS_PEDERSEN,
                           d_first + BP_GENS_PEDERSEN);
    }
    std::vector<F4> xs(wmax); std::vector<u32> fl(wmax), ok(wmax), idx;   // (outlive every copy that reads or writes them: each is reused only after a wait)
    for (int v = 0; ctx->gens_derived && v < 2; v++) {
        const u32* table = v ? ctx->d_H.as<u32>() : ctx->d_G.as<u32>();
        host::u8 msg[20]; memcpy(msg, "GeneratorsChain", 15); msg[15] = (host::u8)(v ? 'H' : 'G'); const u32 party = 0; memcpy(msg + 16, &party, 4);
        host::u8 h[64]; host::sha3_512(h, msg, 20);
        host::ChaChaRng prng(h);
        size_t have = 0;
        while (have < cap) {
            const size_t want = std::min(wmax, (cap - have) * 2 + (cap - have) / 8 + 64);
            for (size_t i = 0; i < want; i++) { xs[i] = host::rand_fe<FqP>(prng); fl[i] = ((int32_t)prng.next_u32()) < 0 ? 0x80u : 0u; }
            HIPCHK(hipMemcpyAsync(ctx->io_pts.p, xs.data(), want * 32, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(ctx->io_scal.p, fl.data(), want * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_points_decompress<C>, dim3((u32)((want + 255) / 256)), dim3(256), 0, st, ctx->io_pts.as<u32>(), ctx->io_scal.as<u32>(), d_xy, d_ok, (u32)want);
            HIPCHK(hipMemcpyAsync(ok.data(), d_ok, want * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx_stream_wait(ctx));
            HIPCHK(hipGetLastError());
            idx.clear();
            for (size_t i = 0; i < want && have + idx.size() < cap; i++) if (ok[i]) idx.push_back((u32)i);
            if (idx.empty()) continue;
            const u32 cnt = (u32)idx.size(), gb = (cnt + 255) / 256;
            HIPCHK(hipMemcpyAsync(ctx->io_scal.p, idx.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_points_gather_import<C>, dim3(gb), dim3(256), 0, st, (const u32*)d_xy, (const u32*)ctx->io_scal.as<u32>(), d_sel, cnt);
            hipLaunchKernelGGL(k_points_compare<C>, dim3(gb), dim3(256), 0, st, (const u32*)d_sel, table + have * 16, cnt, (unsigned long long)have, d_bad + v, d_first + v);
            have += cnt;
        }
    }
    HIPCHK(hipGetLastError());
    unsigned long long hres[2 * BP_GENS_KINDS];
    HIPCHK(hipMemcpyAsync(hres, d_bad, sizeof hres, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    for (int k = 0; k < BP_GENS_KINDS; k++) {
        out->checked[k] = k == BP_GENS_PEDERSEN ? 2 : ctx->gens_derived ? cap : 0;
        out->bad[k] = hres[k];
        out->first_bad[k] = hres[BP_GENS_KINDS + k];
    }
    return BP_OK;
}
// bp_gens_digest: the kernels are vfe.hip's (next to the sponge's Keccak-f); one copy back, one wait
static int gens_digest_dev(bp_ctx* ctx, size_t n, uint8_t out[128]) {
    hipStream_t st = ctx->stream;
    BPCHK(ctx->io_out.ensure(128 + vfe::gens_digest_ws_bytes(n)));
    uint8_t* d_out = ctx->io_out.as<uint8_t>();
    if (vfe::launch_gens_digest(ctx->curve, st, ctx->d_pc.as<u32>(), ctx->d_G.as<u32>(), ctx->d_H.as<u32>(), (u32)n, d_out + 128, d_out)) {
        g_err = "bp_gens_digest: launch failed"; return BP_E_HIP;
    }
    HIPCHK(hipMemcpyAsync(out, d_out, 128, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    return BP_OK;
}

// one commitment MSM: blind * B_blinding + <xs, G[off..]> (+ <ys, H[off..]>)   (prover.rs:516-559, 604-649)
template <class C> static int commit_msm(bp_ctx* ctx, const F4& blind, const u32* xs, const u32* ys, size_t off, size_t cnt, A4& out) {
    typedef host::Grp<C> G;
    const size_t terms = 1 + cnt * (ys ? 2 : 1);
    if (cnt == 0) {   // no multipliers in this phase (a k-shuffle's phase 1): the "MSM" is blind * B_blinding — a single Pedersen term, on the host's fixed-base table
        host::PedersenGens<C> pc; pc.B = ctx->pc_B; pc.B_blinding = ctx->pc_Bb;
        out = pc.commit(host::Fld<typename C::Fr>::zero(), blind);
        return BP_OK;
    }
    BPCHK(ctx->r_msmsc.ensure(32));
    u32* sc = ctx->r_msmsc.as<u32>();
    F4 br = to_resident<typename C::Fr>(blind);
    HIPCHK(hipMemcpyAsync(sc, br.v, 32, hipMemcpyHostToDevice, ctx->stream));
    // scalars and bases as runs read in place: [blinding | xs | ys] over [B_blinding | G[off..] | H[off..]] — the reference
    // materialises both concatenations per call (prover.rs:516-531)
    ScalSegs ss; memset(&ss, 0, sizeof ss);
    ss.ptr[0] = sc; ss.start[0] = 0; ss.start[1] = 1; ss.nseg = 1;
    BaseSegs sg; memset(&sg, 0, sizeof sg);
    sg.ptr[0] = ctx->d_pc.as<u32>() + 16; sg.start[0] = 0; sg.start[1] = 1; sg.nseg = 1;
    if (cnt) {
        ss.ptr[1] = xs; ss.start[2] = (u32)(1 + cnt); ss.nseg = 2;
        sg.ptr[1] = ctx->d_G.as<u32>() + off * 16; sg.start[2] = (u32)(1 + cnt); sg.nseg = 2;
        if (ys) {
            ss.ptr[2] = ys; ss.start[3] = (u32)(1 + 2 * cnt); ss.nseg = 3;
            sg.ptr[2] = ctx->d_H.as<u32>() + off * 16; sg.start[3] = (u32)(1 + 2 * cnt); sg.nseg = 3;
        }
    }
    J4 r;
    bool fixed_done = false;
    // Sharded prover with fixed-base rows installed: the commitment keeps the single-GPU schedule — every rank takes a contiguous
    // BLOCK of the terms (all windows in one bucket set, 13 mixed additions per term), then one point-reduce — instead of stepping
    // back to window-sharded Pippenger over all terms.  The choice depends on global quantities only (every rank decides alike); a
    // rank whose block does not go through the fixed-base path (skewed scalars overflow a bin) runs the ordinary MSM over the same
    // block, so the ranks always meet in exactly one reduce.
    const size_t W = (size_t)ctx->shard_world;
    if (W > 1 && cnt && ctx->fb_cap >= off + cnt && terms / W >= std::max<size_t>(ctx->tune_msm_fixed_min, 4096)) {
        const size_t rk = (size_t)ctx->shard_rank, base = cnt / W, rem = cnt % W;
        const size_t lo = rk * base + std::min(rk, rem), len = base + (rk < rem ? 1 : 0);
        if (rk != 0) { const F4 zero = host::Fld<typename C::Fr>::zero(); HIPCHK(hipMemcpyAsync(sc, zero.v, 32, hipMemcpyHostToDevice, ctx->stream)); }   // the blinding term belongs to rank 0
        const size_t bterms = 1 + len * (ys ? 2 : 1);
        ss.ptr[1] = xs + lo * 8; ss.start[2] = (u32)(1 + len);
        sg.ptr[1] = ctx->d_G.as<u32>() + (off + lo) * 16; sg.start[2] = (u32)(1 + len);
        if (ys) {
            ss.ptr[2] = ys + lo * 8; ss.start[3] = (u32)(1 + 2 * len);
            sg.ptr[2] = ctx->d_H.as<u32>() + (off + lo) * 16; sg.start[3] = (u32)(1 + 2 * len);
        }
        FbRun runs[3] = {{2, 1, 1}, {0, off + lo, len}, {1, off + lo, len}};
        BPCHK(msm_fixed_run<C>(ctx, runs, ys ? 3 : 2, ss, bterms, 2, r, fixed_done, 2));
        if (!fixed_done) BPCHK(msm_run<C>(ctx, sg, nullptr, bterms, 2, r, 0, -1, 2, &ss));
        out = G::to_aff(r);
        return BP_OK;
    }
    {   // the bases are runs of the generator tables: fixed-base schedule when the tables have rows (bp_gens_msm_tables)
        FbRun runs[3] = {{2, 1, 1}, {0, off, cnt}, {1, off, cnt}};
        BPCHK(msm_fixed_run<C>(ctx, runs, cnt ? (ys ? 3 : 2) : 1, ss, terms, 2, r, fixed_done));
    }
    if (!fixed_done) BPCHK(msm_run<C>(ctx, sg, nullptr, terms, 2, r, 0, -1, -1, &ss));
    out = G::to_aff(r);
    return BP_OK;
}

// ---- jobs over the direct window tables (small.cuh) that both prover routes build ---------------------------------------------------
// The blinding term of a table sum, blind * B_blinding: the value rides in the job as its immediate term (`imm`: one proof on the
// ctx's workspaces), or is read as ark words where it lies on the device (`dev`: a group's arena), then as the job's last run.
template <class C> static void dt_job_blind(DtJob& jb, const F4* imm, const u32* dev) {
    if (imm) {
        uint64_t cw[4];
        host::Fld<typename C::Fr>::to_canon(cw, *imm);
        memcpy(jb.imm, cw, 32);
        jb.has_imm = 1; jb.imm_base = dt_base_pc(1);
    } else jb.seg[jb.nseg++] = DtSeg{dev, dt_base_pc(1), 1, 2, 0, 0};
    jb.terms++;
}
// A_I, A_O, S of one phase (prover.rs:516-559 / 604-649): <xs, G[off ..]> (+ <ys, H[off ..]>) + blind * B_blinding, cnt resident
// scalars per run.  imm: the three blinding factors, or null and dev: 3 x 8 words on the device
template <class C> static void dt_commit_jobs(bp_ctx* ctx, DtJob jobs[3], const u32* const xs[3], const u32* const ys[3], size_t off, size_t cnt, const F4* imm, const u32* dev) {
    for (int o = 0; o < 3; o++) {
        DtJob& jb = jobs[o];
        memset(&jb, 0, sizeof jb);
        jb.seg[jb.nseg++] = DtSeg{xs[o], dt_base_G(ctx, off), (u32)cnt, 1, 0, 0};
        if (ys[o]) jb.seg[jb.nseg++] = DtSeg{ys[o], dt_base_H(ctx, off), (u32)cnt, 1, 0, 0};
        jb.terms = (u32)(cnt * (ys[o] ? 2 : 1));
        dt_job_blind<C>(jb, imm ? imm + o : nullptr, dev ? dev + 8 * o : nullptr);
    }
}
// T_i = t_i * B + blinding_i * B_blinding for i = 1, 3 .. 6: t_i read as ark words where the t(x) kernels leave the six sums (tsum)
template <class C> static void dt_t_jobs(DtJob jobs[5], const u32* tsum, const F4* imm, const u32* dev) {
    const int slot[5] = {0, 2, 3, 4, 5};
    for (int o = 0; o < 5; o++) {
        DtJob& jb = jobs[o];
        memset(&jb, 0, sizeof jb);
        jb.seg[jb.nseg++] = DtSeg{tsum + slot[o] * 8, dt_base_pc(0), 1, 2, 0, 0};
        jb.terms = 1;
        dt_job_blind<C>(jb, imm ? imm + o : nullptr, dev ? dev + 8 * o : nullptr);
    }
}

// The host-only head of prove() (prover.rs:466-513): `m`, the TranscriptRng and the phase-1 blinding draws — the strictly
// sequential Keccak chain (8 permutations per multiplier).  It needs no GPU, so a service runs it for proof k+1 on another
// core while proof k occupies the GPU; prove() continues from the stored rng state.
template <class C> struct ProvePre {
    std::unique_ptr<host::TranscriptRng> rng;
    F4 i_b1, o_b1, s_b1;
    std::vector<F4> s_L, s_R;
    double t_rng = 0;
    int mode = BP_BLINDING_TRANSCRIPT;   // bp_prover_set_blinding
    F4 kappa1 = F4{{0, 0, 0, 0}};        // BP_BLINDING_EXPANDED: phase 1's key, drawn where s_L[0] would be (n1 > 0); s_L, s_R stay empty
};
// rng_bytes: the 32 bytes `builder.finalize(prng)` draws from the caller's external rng (prover.rs:493; merlin's
// TranscriptRngBuilder::finalize fills exactly one 32-byte array) — all the prover ever takes from it.
template <class C> static void prove_precompute(host::ConstraintSystem<C>& cs, const host::u8* rng_bytes, ProvePre<C>& pre) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    host::Transcript& tr = *cs.tr;
    const double t0 = now_s();
    tr.append_u64("m", cs.v.size());
    pre.rng.reset(new host::TranscriptRng(tr));
    for (auto& vb : cs.v_blinding) { host::u8 b[32]; S::to_bytes(b, vb); pre.rng->rekey("v_blinding", b, 32); }
    pre.rng->finalize_bytes(rng_bytes);
    const size_t n1 = cs.mults();
    pre.i_b1 = host::rand_fe<FrP>(*pre.rng); pre.o_b1 = host::rand_fe<FrP>(*pre.rng); pre.s_b1 = host::rand_fe<FrP>(*pre.rng);
    if (pre.mode == BP_BLINDING_EXPANDED) {   // one draw instead of 2 n1: the vectors come from it on the device
        if (n1) pre.kappa1 = host::rand_fe<FrP>(*pre.rng);
        pre.t_rng = now_s() - t0;
        return;
    }
    host::reserve_huge(pre.s_L, n1); host::reserve_huge(pre.s_R, n1);
    pre.s_L.resize(n1); pre.s_R.resize(n1);
    for (auto& x : pre.s_L) x = host::rand_fe<FrP>(*pre.rng);
    for (auto& x : pre.s_R) x = host::rand_fe<FrP>(*pre.rng);
    pre.t_rng = now_s() - t0;
}

// The same for up to 8 statements of identical shape at once: their TranscriptRng chains perform the identical operation
// sequence, so they advance in lockstep in the 8 lanes of AVX-512 registers (host_proto.hpp::transcript_rng_x8_words).
// Statements that do not fit the pattern (different sizes, CPU without AVX-512) take the scalar path.
template <class C> static void prove_precompute_batch(host::ConstraintSystem<C>** css, const host::u8* const* rngs32, ProvePre<C>** pres, size_t count) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    bool ok = count == 8 && host::cpu_has_avx512();
    for (size_t j = 0; ok && j < count; j++)
        ok = !pres[j]->rng && pres[j]->mode == BP_BLINDING_TRANSCRIPT /* (an expanded head is four draws: the scalar path) */ && css[j]->mults() == css[0]->mults() && css[j]->v.size() == css[0]->v.size() && css[0]->mults() >= 64;
#if !defined(__x86_64__)
    ok = false;
#endif
    if (!ok) {
        for (size_t j = 0; j < count; j++) if (!pres[j]->rng) prove_precompute<C>(*css[j], rngs32[j], *pres[j]);
        return;
    }
#if defined(__x86_64__)
    const double t0 = now_s();
    const size_t n1 = css[0]->mults();
    host::TranscriptRng* rngs[8];
    for (size_t j = 0; j < 8; j++) {
        host::Transcript& tr = *css[j]->tr;
        tr.append_u64("m", css[j]->v.size());
        pres[j]->rng.reset(new host::TranscriptRng(tr));
        for (auto& vb : css[j]->v_blinding) { host::u8 b[32]; S::to_bytes(b, vb); pres[j]->rng->rekey("v_blinding", b, 32); }
        pres[j]->rng->finalize_bytes(rngs32[j]);
        pres[j]->i_b1 = host::rand_fe<FrP>(*pres[j]->rng); pres[j]->o_b1 = host::rand_fe<FrP>(*pres[j]->rng); pres[j]->s_b1 = host::rand_fe<FrP>(*pres[j]->rng);
        rngs[j] = pres[j]->rng.get();
        ok = ok && rngs[j]->s.pos == 8 && rngs[j]->s.pos_begin == 0;
    }
    std::vector<host::TranscriptRng> saved;
    for (size_t j = 0; j < 8; j++) saved.push_back(*rngs[j]);
    bool clean = ok;
    if (ok) {
        const size_t nwords = 8 * n1;  // 4 words per Fr, s_L then s_R
        std::vector<u64> words;
        host::reserve_huge(words, nwords * 8);
        words.resize(nwords * 8);
        host::transcript_rng_x8_words(rngs, words.data(), nwords);
        for (size_t j = 0; j < 8 && clean; j++) {
            host::reserve_huge(pres[j]->s_L, n1); host::reserve_huge(pres[j]->s_R, n1);
            pres[j]->s_L.resize(n1); pres[j]->s_R.resize(n1);
            for (size_t i = 0; i < 2 * n1 && clean; i++) {
                F4 x;
                for (int w = 0; w < 4; w++) x.v[w] = words[(4 * i + w) * 8 + j];
                if (FrP::BITS < 256) x.v[3] &= (~(u64)0) >> (256 - FrP::BITS);
                if (S::geq_p(x.v)) clean = false;  // a rejected sample shifts that instance's stream (probability < 2^-200)
                (i < n1 ? pres[j]->s_L[i] : pres[j]->s_R[i - n1]) = x;
            }
        }
    }
    if (!clean) {  // redo the vector draws one instance at a time from the saved states
        for (size_t j = 0; j < 8; j++) {
            *pres[j]->rng = saved[j];
            pres[j]->s_L.resize(n1); pres[j]->s_R.resize(n1);
            for (auto& x : pres[j]->s_L) x = host::rand_fe<FrP>(*pres[j]->rng);
            for (auto& x : pres[j]->s_R) x = host::rand_fe<FrP>(*pres[j]->rng);
        }
    }
    const double dt = (now_s() - t0) / 8;
    for (size_t j = 0; j < 8; j++) pres[j]->t_rng = dt;
#endif
}

// bp_prover_prove_batch (prove_batch.inc): a statement whose inner-product argument would run over the direct window tables may hand
// it to a lockstep group instead.  take(N, slot) gives the group slot that receives a, b and the factor vectors (false: run it here).
// A taken proof returns with everything but L_vec, R_vec, a and b filled in, and its transcript right after the domain separator.
struct IpaDeferSlot { u32 *a = nullptr, *b = nullptr, *cG = nullptr, *cH = nullptr; };
struct IpaDefer {
    std::function<bool(size_t N, IpaDeferSlot& slot)> take;
    bool taken = false;
    size_t N = 0;
    F4 w;
};

// ---- like-provers (include/arkbp.h bp_prover_new_like) ---------------------------------------------------------------------------------
// a_O of a like-prover on the host: THE place where it is formed there (randomized-phase callbacks read it through eval, the host twin
// of the witness check, the staging of front groups, bp_prover_check's own upload, a poke of a_O) — on the ctx's pool when there is one.
// Once formed the host vector is the truth and goes up like a recorded prover's.
// A witness assigned from device memory (bp_prover_assign_multipliers_dev) comes to the host HERE and nowhere else, in front of the
// products: one D2H copy of the ark words per vector, no kernel; the handle's device copy is wiped and freed, and from then on the
// handle is a host-assigned like-prover.  Its other readers on the host (a sharded ctx, bp_prover_check, a poke, the front groups of
// prove_batch) call this too.
template <class C> static int prove_need_aO(bp_ctx* ctx, host::ConstraintSystem<C>& cs) {
    if (cs.dev.held()) {
        const size_t cnt = cs.dev.count;
        BPCHK(cs.witness_to_host(ctx));
        if (ctx) ctx->wd_gates_down += cnt;
    }
    if (!cs.aO_lazy) return BP_OK;
    const size_t n = cs.a_L.size();
    if (ctx && n > ((size_t)1 << 14)) host_pool_ensure(ctx, 2);
    cs.materialise_aO([&](size_t cnt, const std::function<void(size_t)>& fn) { pool_range(ctx, 0, cnt, fn); });
    if (ctx) ctx->pl_gates_host += n;
    return BP_OK;
}

// ---- a like-prover's witness from device memory (include/arkbp.h bp_prover_assign_multipliers_dev; the kernels: witness_dev.cuh) -------
// the stream that works on a handle's device copy: the given ctx's when it lives on the copy's device, else that device's default one
static hipStream_t wd_stream(const host::DevWitness& w, void* ctxv) {
    bp_ctx* c = (bp_ctx*)ctxv;
    return c && !c->host_only && c->device == w.device ? c->stream : (hipStream_t) nullptr;
}
static hipError_t wd_wait(const host::DevWitness& w, void* ctxv) {
    hipStream_t st = wd_stream(w, ctxv);
    return st ? ctx_stream_wait((bp_ctx*)ctxv) : hipStreamSynchronize(st);
}
// host::DevWitness::fetch: both vectors to the host, ark words as they lie there
static int wd_fetch(const host::DevWitness& w, void* ctxv, F4* left, F4* right) {
    if (!w.count) return BP_OK;
    HIPCHK(hipSetDevice(w.device));
    hipStream_t st = wd_stream(w, ctxv);
    HIPCHK(hipMemcpyAsync(left, w.aL, w.count * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(right, w.aR, w.count * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(wd_wait(w, ctxv));
    return BP_OK;
}
// host::DevWitness::drop: zeroes behind whatever the stream still reads, a wait, then the memory goes back (as prove_wipe treats r_aL
// and the others).  Runs from destructors too: errors have nowhere to go, and the caller's current device is put back.
static void wd_drop(host::DevWitness& w, void* ctxv) {
    if (w.aL || w.aR) {
        int prev = -1;
        (void)hipGetDevice(&prev);
        if (hipSetDevice(w.device) == hipSuccess) {
            hipStream_t st = wd_stream(w, ctxv);
            if (w.aL) (void)hipMemsetAsync(w.aL, 0, std::max<size_t>(w.count, 1) * 32, st);
            if (w.aR) (void)hipMemsetAsync(w.aR, 0, std::max<size_t>(w.count, 1) * 32, st);
            (void)wd_wait(w, ctxv);
            if (w.aL) (void)hipFree(w.aL);
            if (w.aR) (void)hipFree(w.aR);
        }
        if (prev >= 0 && prev != w.device) (void)hipSetDevice(prev);
    }
    w.aL = w.aR = nullptr;
}
// bp_prover_assign_multipliers_dev behind its argument checks: the handle's copy and the range check in ONE kernel, one copy back,
// one wait.  Nothing of the handle changes unless every word is below r.
template <class C> static int wd_assign(bp_ctx* ctx, host::ConstraintSystem<C>& cs, const void* d_left, const void* d_right, size_t count) {
    host::DevWitness w;
    w.count = count; w.device = ctx->device; w.fetch = wd_fetch; w.drop = wd_drop;
    if (count) {
        if (count >= ((size_t)1 << 31)) { g_err = "assign_multipliers_dev: 2^31 multipliers or more"; return BP_E_ARG; }
        BPCHK(ctx->wd_res.ensure(16));
        BPCHK(pinned_ensure(ctx->h_wd, ctx->h_wd_cap, 16, 48));
        hipError_t e = hipMalloc(&w.aL, count * 32);
        if (e == hipSuccess) e = hipMalloc(&w.aR, count * 32);
        if (e != hipSuccess) { if (w.aL) (void)hipFree(w.aL); g_err = std::string("assign_multipliers_dev: hipMalloc: ") + hipGetErrorString(e); return BP_E_HIP; }
        u32* res = ctx->wd_res.as<u32>();
        u32* back = (u32*)ctx->h_wd;
        int rc = BP_OK;
        auto step = [&](hipError_t he, const char* what) { if (!rc && he != hipSuccess) { g_err = std::string("assign_multipliers_dev: ") + what + ": " + hipGetErrorString(he); rc = BP_E_HIP; } };
        step(hipMemsetAsync(res, 0, 8, ctx->stream), "hipMemsetAsync");
        step(hipMemsetAsync(res + 2, 0xff, 8, ctx->stream), "hipMemsetAsync");
        if (!rc) {
            hipLaunchKernelGGL(k_wit_take<typename C::Fr>, dim3((u32)((count + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)d_left, (const u32*)d_right, (u32*)w.aL, (u32*)w.aR, (u32)count, res);
            step(hipGetLastError(), "k_wit_take");
        }
        if (!rc) step(hipMemcpyAsync(back, res, 16, hipMemcpyDeviceToHost, ctx->stream), "hipMemcpyAsync");
        if (!rc) step(ctx_stream_wait(ctx), "wait");
        if (!rc && (back[0] || back[1])) {
            const bool left_first = back[0] && (!back[1] || back[2] <= back[3]);
            g_err = std::string("assign_multipliers_dev: ") + (left_first ? "left" : "right") + "[" + std::to_string(left_first ? back[2] : back[3]) + "] is not a reduced scalar";
            rc = BP_E_ARG;
        }
        if (rc) { wd_drop(w, ctx); return rc; }
    }
    cs.assign_multipliers_dev(w);
    ctx->wd_assigns++;
    return BP_OK;
}
// the builder of the range gadget's witness (bp_witness_range_bits_dev): one launch on the ctx's stream, and a wait
template <class C> static int wd_range_bits(bp_ctx* ctx, const void* d_values, size_t total, unsigned nbits, void* d_left, void* d_right) {
    hipLaunchKernelGGL(k_wit_range_bits<typename C::Fr>, dim3((u32)((total + 255) / 256)), dim3(256), 0, ctx->stream, (const u64*)d_values, (u32)total, (u32)nbits, (u32*)d_left, (u32*)d_right);
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));
    return BP_OK;
}
// the ctx's entry of a recording: expired entries go first, then the least recently used one when PL_CACHE_MAX are kept
static PlResident* pl_entry(bp_ctx* ctx, const std::shared_ptr<const host::FrozenRecording>& rec) {
    auto& cache = ctx->pl_cache;
    cache.erase(std::remove_if(cache.begin(), cache.end(), [](const std::unique_ptr<PlResident>& e) { return e->key.expired(); }), cache.end());
    for (auto& e : cache) if (e->key.lock() == rec) { e->used = ++ctx->pl_clock; return e.get(); }
    if (cache.size() >= PL_CACHE_MAX) cache.erase(std::min_element(cache.begin(), cache.end(), [](const std::unique_ptr<PlResident>& a, const std::unique_ptr<PlResident>& b) { return a->used < b->used; }));
    cache.emplace_back(new PlResident());
    cache.back()->key = rec; cache.back()->used = ++ctx->pl_clock;
    return cache.back().get();
}
static size_t pl_align(size_t x) { return (x + 255) & ~(size_t)255; }
// the recording's column index on the device: uploaded by the first proof of the recording on this ctx, found there by every later one
struct CscPtrs { const u32 *moff, *ment, *mc; };
template <class C> static int pl_csc(bp_ctx* ctx, const std::shared_ptr<const host::FrozenRecording>& rec, const HostCsc& csc, CscPtrs& k, const u32*& coefs) {
    PlResident* e = pl_entry(ctx, rec);
    if (!e->have_csc) {
        const size_t n = csc.n, nnz = csc.ment.size(), nc = csc.coefs.size();
        e->o_ment = pl_align((n + 1) * 4); e->o_mc = e->o_ment + pl_align(nnz * 4); e->o_coefs = e->o_mc + pl_align(nnz * 4);
        const size_t total = e->o_coefs + nc * 32;
        BPCHK(e->csc.ensure_exact(total));
        BPCHK(pinned_ensure(ctx->h_csc, ctx->h_csc_cap, total, 4096));
        char* hs = (char*)ctx->h_csc;
        memcpy(hs, csc.moff.data(), (n + 1) * 4);
        if (nnz) { memcpy(hs + e->o_ment, csc.ment.data(), nnz * 4); memcpy(hs + e->o_mc, csc.mc.data(), nnz * 4); }
        memcpy(hs + e->o_coefs, csc.coefs.data(), nc * 32);
        HIPCHK(hipMemcpyAsync(e->csc.p, hs, total, hipMemcpyHostToDevice, ctx->stream));
        u32* dc = (u32*)((char*)e->csc.p + e->o_coefs);
        hipLaunchKernelGGL(k_scalars_import<typename C::Fr>, dim3((u32)((nc + 255) / 256)), dim3(256), 0, ctx->stream, dc, dc, (u32)nc);
        HIPCHK(hipGetLastError());
        HIPCHK(ctx_stream_wait(ctx));   // (once per recording and ctx: the staging is free again)
        e->have_csc = true;
        ctx->pl_uploads++;
    } else ctx->pl_hits++;
    const char* d = (const char*)e->csc.p;
    k = CscPtrs{(const u32*)d, (const u32*)(d + e->o_ment), (const u32*)(d + e->o_mc)};
    coefs = (const u32*)(d + e->o_coefs);
    return BP_OK;
}
// ... and its row index, for the guard's check kernels (the first guarded proof of the recording on this ctx uploads it)
template <class C> static int pl_row(bp_ctx* ctx, const std::shared_ptr<const host::FrozenRecording>& rec, const HostRowIndex& h, const PlResident*& out) {
    typedef typename C::Fr FrP;
    PlResident* e = pl_entry(ctx, rec);
    if (e->row_of != &h) {
        e->r_pinfo = pl_align(h.poff.size() * 4); e->r_tvar = e->r_pinfo + pl_align(h.pinfo.size() * 4); e->r_tcid = e->r_tvar + pl_align(h.tvar.size() * 4);
        e->r_lrow = e->r_tcid + pl_align(h.tcid.size() * 4); e->r_coefs = e->r_lrow + pl_align(h.lrow.size() * 4);
        const size_t total = e->r_coefs + h.coefs.size() * 32;
        BPCHK(e->row.ensure_exact(total));
        BPCHK(pinned_ensure(ctx->h_csc, ctx->h_csc_cap, total, 4096));
        char* hs = (char*)ctx->h_csc;
        auto put = [&](size_t at, const std::vector<u32>& v) { if (!v.empty()) memcpy(hs + at, v.data(), v.size() * 4); };
        put(0, h.poff); put(e->r_pinfo, h.pinfo); put(e->r_tvar, h.tvar); put(e->r_tcid, h.tcid); put(e->r_lrow, h.lrow);
        F4* co = (F4*)(hs + e->r_coefs);
        for (size_t i = 0; i < h.coefs.size(); i++) co[i] = to_resident<FrP>(h.coefs[i]);   // (as wc_enqueue stages an instance's own table)
        HIPCHK(hipMemcpyAsync(e->row.p, hs, total, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx_stream_wait(ctx));
        e->row_of = &h;
    }
    out = e;
    return BP_OK;
}
static size_t pl_resident_bytes(const bp_ctx* ctx) {
    size_t b = 0;
    for (auto& e : ctx->pl_cache) if (!e->key.expired()) b += e->bytes();
    return b;
}

// ---- witness check (witness_check.cuh; include/arkbp.h bp_prover_check / bp_prover_set_check) -----------------------------------------
// One call's statements share ONE block: the device buffer ctx->wc_dev and its image in the pinned staging ctx->h_wc (behind the
// area the flags return to).  Image: [descriptors | flags | per statement: poff, pinfo, tvar, tcid, lrow, coefs || the witnesses (ark
// words, bp_prover_check only) | per statement: v || partial sums (device only)].  Everything from the witnesses on derives from
// secrets and is wiped after use.
struct WcGuard { bool on = false; bp_witness_report report; };   // r1cs_prove's guard: the report of a refused proof
static size_t wc_align(size_t x) { return (x + 255) & ~(size_t)255; }
template <class C> struct WcItem {
    const host::ConstraintSystem<C>* cs = nullptr;
    const HostRowIndex* idx = nullptr;
    const u32 *aL = nullptr, *aR = nullptr, *aO = nullptr;   // the resident witness; all null: the run uploads it itself
    const PlResident* dev = nullptr;                        // idx is a shared recording's and lives on the device already (pl_row): nothing of it is staged
};
template <class C> struct WcRun {
    std::vector<WcItem<C>> items;
    std::vector<HostRowIndex> own;           // the indices (built by the caller into here)
    size_t back = 0, o_res = 0, o_secret = 0, o_wit = 0, wit_scalars = 0, end_up = 0, total = 0;
    bool enqueued = false;
    bp_ctx* staged_on = nullptr;             // set while the staging holds this run's secrets (wc_enqueue .. wc_wipe_host)
    const u32* flags(const bp_ctx* ctx, size_t j) const { return (const u32*)ctx->h_wc + 4 * j; }
    // a way out that skips wc_wipe_host (a stage failed in between): the stream may still read the staging, so wait, then wipe
    ~WcRun() {
        if (!staged_on) return;
        (void)hipStreamSynchronize(staged_on->stream);
        if (staged_on->h_wc && end_up > o_secret) memset((char*)staged_on->h_wc + back + o_secret, 0, end_up - o_secret);
    }
};
// Index upload and the check launches of a run on the ctx's stream.  res_dev: where the flags live on the device (a front group keeps
// them next to results it copies back anyway), null: in the block.
template <class C> static int wc_enqueue(bp_ctx* ctx, WcRun<C>& r, u32* res_dev) {
    typedef typename C::Fr FrP;
    const size_t B = r.items.size();
    if (!B) return BP_OK;
    hipStream_t st = ctx->stream;
    const bool upload_witness = !r.items[0].aL;
    std::vector<size_t> at(B), v_at(B), wit_at(B), part_at(B);
    size_t o = wc_align(B * sizeof(WcDesc));
    r.o_res = o; o += wc_align(B * 16);
    for (size_t j = 0; j < B; j++) {
        const HostRowIndex& h = *r.items[j].idx;
        at[j] = o;
        if (r.items[j].dev) continue;
        o += wc_align((h.npieces() + 1) * 4) + wc_align(h.npieces() * 4) + 2 * wc_align(h.tvar.size() * 4) + wc_align(h.lrow.size() * 4) + wc_align(h.coefs.size() * 32);
    }
    r.o_secret = r.o_wit = o;
    r.wit_scalars = 0;
    if (upload_witness) for (size_t j = 0; j < B; j++) { wit_at[j] = o; o += 3 * r.items[j].idx->n * 32; r.wit_scalars += 3 * r.items[j].idx->n; }
    o = wc_align(o);
    for (size_t j = 0; j < B; j++) { v_at[j] = o; o += wc_align(r.items[j].idx->m * 32); }
    r.end_up = o;
    for (size_t j = 0; j < B; j++) { part_at[j] = o; o += wc_align(r.items[j].idx->nslots * 32); }
    r.total = o;
    r.back = wc_align(B * 16);
    if (r.wit_scalars >= ((size_t)1 << 32)) { g_err = "witness check: more than 2^32 witness scalars in one call"; return BP_E_ARG; }
    BPCHK(ctx->wc_dev.ensure(r.total));
    BPCHK(pinned_ensure(ctx->h_wc, ctx->h_wc_cap, r.back + r.end_up, (r.back + r.end_up) / 4 + 4096));
    char* img = (char*)ctx->h_wc + r.back;
    char* dev = (char*)ctx->wc_dev.p;
    WcDesc* descs = (WcDesc*)img;
    u32 gx = 0, gl = 0, max_pieces = 0;
    host_pool_ensure(ctx, B);
    struct Copy { char* dst; const char* src; size_t bytes; };
    std::vector<std::vector<Copy>> big(B);   // the long arrays go over in slices, on the pool (a 2^20 statement stages 48 MB)
    static constexpr size_t SLICE = (size_t)4 << 20;
    pool_range(ctx, 0, B, [&](size_t j) {
        const WcItem<C>& it = r.items[j];
        const HostRowIndex& h = *it.idx;
        size_t p = at[j];
        auto put = [&](const void* src, size_t bytes) {
            const size_t here = p;
            if (bytes > SLICE) for (size_t o2 = 0; o2 < bytes; o2 += SLICE) big[j].push_back(Copy{img + p + o2, (const char*)src + o2, std::min(SLICE, bytes - o2)});
            else if (bytes) memcpy(img + p, src, bytes);
            p += wc_align(bytes);
            return (const u32*)(dev + here);
        };
        WcDesc& d = descs[j];
        memset(&d, 0, sizeof d);
        if (it.dev) {
            const char* rb = (const char*)it.dev->row.p;
            d.poff = (const u32*)rb; d.pinfo = (const u32*)(rb + it.dev->r_pinfo); d.tvar = (const u32*)(rb + it.dev->r_tvar); d.tcid = (const u32*)(rb + it.dev->r_tcid);
            d.lrow = (const u32*)(rb + it.dev->r_lrow); d.coefs = (const u32*)(rb + it.dev->r_coefs);
        } else {
            d.poff = put(h.poff.data(), h.poff.size() * 4);
            d.pinfo = put(h.pinfo.data(), h.pinfo.size() * 4);
            d.tvar = put(h.tvar.data(), h.tvar.size() * 4);
            d.tcid = put(h.tcid.data(), h.tcid.size() * 4);
            d.lrow = put(h.lrow.data(), h.lrow.size() * 4);
            d.coefs = (const u32*)(dev + p);
            F4* co = (F4*)(img + p);
            for (size_t i = 0; i < h.coefs.size(); i++) co[i] = to_resident<FrP>(h.coefs[i]);
        }
        d.v = (const u32*)(dev + v_at[j]);
        F4* vv = (F4*)(img + v_at[j]);
        for (size_t i = 0; i < h.m; i++) vv[i] = to_resident<FrP>(it.cs->v[i]);
        if (upload_witness) {
            char* w = img + wit_at[j];
            memcpy(w, it.cs->a_L.data(), h.n * 32); memcpy(w + h.n * 32, it.cs->a_R.data(), h.n * 32); memcpy(w + 2 * h.n * 32, it.cs->a_O.data(), h.n * 32);
            d.aL = (const u32*)(dev + wit_at[j]); d.aR = d.aL + h.n * 8; d.aO = d.aR + h.n * 8;
        } else { d.aL = it.aL; d.aR = it.aR; d.aO = it.aO; }
        d.partial = (u32*)(dev + part_at[j]);
        d.res = res_dev ? res_dev + 4 * j : (u32*)(dev + r.o_res) + 4 * j;
        d.n = (u32)h.n; d.npieces = (u32)h.npieces(); d.nlong = (u32)h.nlong();
        u32* init = (u32*)(img + r.o_res) + 4 * j;
        init[0] = 0; init[1] = 0xFFFFFFFFu; init[2] = 0; init[3] = 0xFFFFFFFFu;
    });
    {
        std::vector<Copy> all;
        for (auto& v : big) all.insert(all.end(), v.begin(), v.end());
        host_pool_ensure(ctx, all.size());
        pool_range(ctx, 0, all.size(), [&](size_t i) { memcpy(all[i].dst, all[i].src, all[i].bytes); });
    }
    for (size_t j = 0; j < B; j++) {
        const HostRowIndex& h = *r.items[j].idx;
        gx = std::max<u32>(gx, (u32)((std::max(h.n, h.npieces()) + 255) / 256)); gl = std::max<u32>(gl, (u32)h.nlong()); max_pieces = std::max(max_pieces, h.max_pieces);
    }
    r.enqueued = true; r.staged_on = ctx;
    HIPCHK(hipMemcpyAsync(dev, img, r.end_up, hipMemcpyHostToDevice, st));
    if (res_dev) HIPCHK(hipMemcpyAsync(res_dev, img + r.o_res, B * 16, hipMemcpyHostToDevice, st));
    if (upload_witness && r.wit_scalars)
        hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((r.wit_scalars + 255) / 256)), dim3(256), 0, st, (const u32*)(dev + r.o_wit), (u32*)(dev + r.o_wit), (u32)r.wit_scalars);
    {
        ScopedK tk(ctx, BP_K_WITNESS_CHECK);
        if (B == 1) {
            if (gx) hipLaunchKernelGGL(k_r1cs_check<C>, dim3(gx), dim3(256), 0, st, descs[0]);
            if (gl) hipLaunchKernelGGL(k_r1cs_check_long<C>, dim3(gl), dim3(256), 0, st, descs[0], max_pieces);
        } else {
            for (size_t lo = 0; lo < B; lo += 32768) {   // (grid.y stays below 65536)
                const u32 cnt = (u32)std::min<size_t>(32768, B - lo);
                if (gx) hipLaunchKernelGGL(k_r1cs_check_multi<C>, dim3(gx, cnt), dim3(256), 0, st, (const WcDesc*)dev + lo);
                if (gl) hipLaunchKernelGGL(k_r1cs_check_long_multi<C>, dim3(gl, cnt), dim3(256), 0, st, (const WcDesc*)dev + lo, max_pieces);
            }
        }
    }
    HIPCHK(hipGetLastError());
    return BP_OK;
}
// the flags of a run whose flags live in the block, on their way to the front of the pinned staging (valid after the next wait)
template <class C> static int wc_fetch(bp_ctx* ctx, WcRun<C>& r) {
    HIPCHK(hipMemcpyAsync(ctx->h_wc, (char*)ctx->wc_dev.p + r.o_res, r.items.size() * 16, hipMemcpyDeviceToHost, ctx->stream));
    return BP_OK;
}
// secret hygiene: the witnesses, the committed values and the partial sums on the device (enqueued), ...
template <class C> static int wc_wipe_dev(bp_ctx* ctx, const WcRun<C>& r) {
    if (r.enqueued && r.total > r.o_secret) HIPCHK(hipMemsetAsync((char*)ctx->wc_dev.p + r.o_secret, 0, r.total - r.o_secret, ctx->stream));
    return BP_OK;
}
// ... and their image in the staging, once the stream has read it (after a wait)
template <class C> static void wc_wipe_host(bp_ctx* ctx, WcRun<C>& r) {
    if (r.enqueued && ctx->h_wc && r.end_up > r.o_secret) memset((char*)ctx->h_wc + r.back + r.o_secret, 0, r.end_up - r.o_secret);
    r.staged_on = nullptr;
}
static bool wc_flags_bad(const u32* f) { return f[0] != 0 || f[2] != 0; }

// ---- Prover::prove_and_return_transcript (src/r1cs/prover.rs:454-831) as stages over one state struct -------------------------------
// ARKBP_PROVE_TRACE=1: microseconds between the marks of one prove() on stderr (where a SMALL proof's latency goes)
struct ProveTrace {
    bool on;
    std::vector<std::pair<const char*, double>> marks;
    void mark(const char* what) { if (on) marks.emplace_back(what, now_s()); }
    void print(size_t n) {
        if (!on) return;
        mark("end");
        std::string line = "prove n=" + std::to_string(n) + ":";
        for (size_t i = 1; i < marks.size(); i++) { char b[96]; snprintf(b, sizeof b, "  %s %.0f", marks[i].first, (marks[i].second - marks[i - 1].second) * 1e6); line += b; }
        fprintf(stderr, "%s us\n", line.c_str());
    }
};
// What one prove() carries from stage to stage
template <class C> struct ProveJob {
    bp_ctx* ctx;
    host::ConstraintSystem<C>& cs;
    ProvePre<C>& pre;            // the head: rng, phase 1's blinding factors, s_L / s_R (or kappa1)
    StageTimes& tm;
    host::PedersenGens<C> pc;
    ProveTrace trace;
    bool expanded = false;       // BP_BLINDING_EXPANDED
    size_t n1 = 0, n = 0, N = 0; // phase-1 multipliers, all multipliers, padded
    F4 b1[3], bl2[3], tb[5];     // i_b, o_b, s_b of the two phases; the blinding factors of T_1, T_3 .. T_6
    A4 c1[3], c2[3], Tc[5];      // A_I, A_O, S of the two phases; T_1, T_3 .. T_6
    F4 y, z, u, x, w;
    F4 ypw[64], tco[6];          // y^(2^k) | y^-(2^k); t_1 .. t_6
    const HostCsc* csc = nullptr;
    HostCsc csc_late;            // a two-phase statement's index, built after its randomized phase
    std::vector<F4> wV;
    F4 t_x, t_x_blinding, e_blinding;
    bool cyclic = false, direct = false, in_place = false, deferred = false;   // how the inner-product argument runs (prove_eval, prove_ipa)
    bool secrets_up = false;     // from the first upload on: every way out wipes
};

// device vectors are sized for the final padded length lazily: phase 1 first
static int prove_ensure_vecs(bp_ctx* ctx, size_t cap) {
    DevBuf* bs[] = {&ctx->r_aL, &ctx->r_aR, &ctx->r_aO, &ctx->r_sL, &ctx->r_sR};
    for (auto b : bs) {
        if (b->cap >= cap * 32) continue;
        DevBuf nb;
        BPCHK(nb.ensure(cap * 32));
        if (b->p && b->cap) { HIPCHK(hipMemcpyAsync(nb.p, b->p, std::min(b->cap, nb.cap), hipMemcpyDeviceToDevice, ctx->stream)); HIPCHK(ctx_stream_wait(ctx)); }
        b->release(); *b = nb;
    }
    return BP_OK;
}

// the witness of one phase — multipliers [off, off + cnt) — to the device; kappa: the phase's key (BP_BLINDING_EXPANDED)
template <class C> static int prove_upload_phase(ProveJob<C>& j, size_t off, size_t cnt, const F4& kappa) {
    bp_ctx* ctx = j.ctx;
    const double t0 = now_s();
    BPCHK(prove_ensure_vecs(ctx, host::next_pow2(std::max<size_t>(off + cnt, 1))));
    HIPCHK(ctx_stream_wait(ctx));   // (the slab's previous use — the last proof of this ctx, or phase 1's copies — is complete)
    BPCHK(upload_slab_ensure(ctx, 5 * std::max(off, cnt) * 32));
    u32* const dst[5] = {ctx->r_aL.as<u32>() + off * 8, ctx->r_aR.as<u32>() + off * 8, ctx->r_aO.as<u32>() + off * 8, ctx->r_sL.as<u32>() + off * 8, ctx->r_sR.as<u32>() + off * 8};
    const F4* const src[5] = {j.cs.a_L.data() + off, j.cs.a_R.data() + off, j.cs.a_O.data() + off, j.expanded ? nullptr : j.pre.s_L.data() + off, j.expanded ? nullptr : j.pre.s_R.data() + off};
    j.secrets_up = true;
    if (j.cs.dev.held()) {   // a witness assigned from device memory: no staging and no copy; ONE kernel imports a_L, a_R from the handle's ark words and takes the products
        const char* wl = (const char*)j.cs.dev.aL + off * 32;
        const char* wr = (const char*)j.cs.dev.aR + off * 32;
        if (off + cnt > j.cs.dev.count) { g_err = "prove: the device witness is shorter than the phase"; return BP_E_ARG; }
        if (cnt) {
            hipLaunchKernelGGL(k_r1cs_import_gate<typename C::Fr>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)wl, (const u32*)wr, dst[0], dst[1], dst[2], (u32)cnt);
            HIPCHK(hipGetLastError());
            ctx->wd_gates_dev += cnt; ctx->pl_gates_dev += cnt;
        }
        if (!j.expanded) BPCHK(upload_witness5<C>(ctx, dst + 3, src + 3, cnt, 2));
    } else if (j.cs.aO_lazy) {   // a like-prover whose a_O nobody has read on the host: two witness vectors go up, the products are taken here
        u32* const d4[4] = {dst[0], dst[1], dst[3], dst[4]};
        const F4* const s4[4] = {src[0], src[1], src[3], src[4]};
        BPCHK(upload_witness5<C>(ctx, d4, s4, cnt, j.expanded ? 2 : 4));
        if (cnt) {
            hipLaunchKernelGGL(k_r1cs_gate_out<typename C::Fr>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, (const u32*)dst[0], (const u32*)dst[1], dst[2], (u32)cnt);
            HIPCHK(hipGetLastError());
            ctx->pl_gates_dev += cnt;
        }
    } else {
        BPCHK(upload_witness5<C>(ctx, dst, src, cnt, j.expanded ? 3 : 5));
    }
    if (j.expanded) BPCHK(blind_expand_launch<C>(ctx, kappa, 0, cnt, dst[3], dst[4]));
    j.tm.upload += now_s() - t0;
    return BP_OK;
}

// A_I, A_O, S of one phase (prover.rs:516-559 / 604-649) over the uploaded multipliers [off, off + cnt)
template <class C> static int prove_commit_phase(ProveJob<C>& j, size_t off, size_t cnt, const F4 blinds[3], A4 out[3]) {
    typedef host::Fld<typename C::Fr> S;
    bp_ctx* ctx = j.ctx;
    const double t0 = now_s();
    const u32* xs[3] = {ctx->r_aL.as<u32>() + off * 8, ctx->r_aO.as<u32>() + off * 8, ctx->r_sL.as<u32>() + off * 8};
    const u32* ys[3] = {ctx->r_aR.as<u32>() + off * 8, nullptr, ctx->r_sR.as<u32>() + off * 8};
    bool direct = false;
    if (cnt) BPCHK(dt_ensure<C>(ctx, host::next_pow2(off + cnt), direct));
    if (cnt == 0) {   // no multipliers in this phase (a k-shuffle's phase 1): three single Pedersen terms on the host's tables, one inversion
        const J4 j3[3] = {j.pc.commit_jac(S::zero(), blinds[0]), j.pc.commit_jac(S::zero(), blinds[1]), j.pc.commit_jac(S::zero(), blinds[2])};
        to_aff_many<C>(j3, 3, out);
    } else if (direct) {   // ONE launch over the direct window tables (small.cuh); the blinding factors ride in the launch
        DtJobs jobs; memset(&jobs, 0, sizeof jobs);
        dt_commit_jobs<C>(ctx, jobs.job, xs, ys, off, cnt, blinds, nullptr);
        J4 r[3];
        BPCHK(msm_direct<C>(ctx, jobs, 3, r));
        to_aff_many<C>(r, 3, out);
    } else {
        for (int o = 0; o < 3; o++) BPCHK(commit_msm<C>(ctx, blinds[o], xs[o], ys[o], off, cnt, out[o]));
    }
    j.tm.commit_msm += now_s() - t0;
    return BP_OK;
}

// the constraint index to the device (36 MB at 2^20 instead of 96 MB of flattened vectors) through pinned memory like the witness (a
// pageable H2D copy serialises across the proofs in flight); a small statement's kernels read the pinned staging memory themselves
static int prove_csc_stage(bp_ctx* ctx, const HostCsc& csc, bool small_stmt, CscPtrs& k) {
    const size_t n = csc.n, nnz = csc.ment.size();
    BPCHK(ctx->p_moff.ensure((n + 1) * 4)); BPCHK(ctx->p_ment.ensure(std::max<size_t>(nnz, 1) * 4)); BPCHK(ctx->p_mc.ensure(std::max<size_t>(nnz, 1) * 4));
    k = CscPtrs{ctx->p_moff.as<u32>(), ctx->p_ment.as<u32>(), ctx->p_mc.as<u32>()};
    const size_t b_off = (n + 1) * 4, b_nz = nnz * 4, a_nz = (b_off + 63) / 64 * 64, a_mc = a_nz + (b_nz + 63) / 64 * 64;
    BPCHK(pinned_ensure(ctx->h_csc, ctx->h_csc_cap, a_mc + b_nz + 64, 4096 - 64));
    char* hs = (char*)ctx->h_csc;
    memcpy(hs, csc.moff.data(), b_off);
    if (nnz) { memcpy(hs + a_nz, csc.ment.data(), b_nz); memcpy(hs + a_mc, csc.mc.data(), b_nz); }
    if (small_stmt) { k = CscPtrs{(const u32*)hs, (const u32*)(hs + a_nz), (const u32*)(hs + a_mc)}; return BP_OK; }
    HIPCHK(hipMemcpyAsync(ctx->p_moff.p, hs, b_off, hipMemcpyHostToDevice, ctx->stream));
    if (nnz) {
        HIPCHK(hipMemcpyAsync(ctx->p_ment.p, hs + a_nz, b_nz, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->p_mc.p, hs + a_mc, b_nz, hipMemcpyHostToDevice, ctx->stream));
    }
    return BP_OK;
}

// w_L, w_R, w_O on the device, wV on the host, the y tables on the device (prover.rs:354-397, 651-698)
template <class C> static int prove_flatten(ProveJob<C>& j) {
    typedef typename C::Fr FrP;
    bp_ctx* ctx = j.ctx;
    hipStream_t st = ctx->stream;
    const size_t n = j.n, N = j.N;
    bool ypw_early = false;   // (a small statement sends the y tables up together with the coefficient table)
    double t0 = now_s();
    BPCHK(ctx->r_wL.ensure(N * 32)); BPCHK(ctx->r_wR.ensure(N * 32)); BPCHK(ctx->r_wO.ensure(N * 32));
    static const bool host_flatten = getenv("ARKBP_HOST_FLATTEN") != nullptr;   // A/B: the host pass over all terms + 3 uploads
    auto fits = [&](const HostCsc* c) { return c && c->n == n && c->q == j.cs.num_constraints(); };
    if (!fits(j.csc) && n > 0 && !host_flatten) {
        // randomized (two-phase) statements: the constraints exist only now (prover.rs:418-441) — index them here, then the
        // same kernel evaluates them
        j.csc = build_host_csc<C>(j.cs, j.csc_late) ? &j.csc_late : nullptr;
    }
    if (fits(j.csc) && n > 0) {   // the constraint index goes up, z^e tables, one launch
        const HostCsc& csc = *j.csc;
        const size_t nc = csc.coefs.size();
        const u32 nzhi = (u32)((csc.q + 1) >> 8) + 1;
        // a like-prover that recorded nothing itself proves from the recording's index, resident on this ctx: no staging, no copy
        const bool resident = j.cs.base && j.cs.own_empty() && j.csc == j.cs.base->csc.get() && ctx->shard_world <= 1;
        if (!resident) BPCHK(ctx->p_coefs.ensure((nc + 32) * 32));
        else BPCHK(ctx->pl_ztab.ensure(32 * 32));
        BPCHK(ctx->p_ztab.ensure((size_t)(256 + nzhi) * 32));
        const bool small_stmt = n <= UPLOAD_FUSED_MAX && nc <= UPLOAD_FUSED_MAX;
        CscPtrs k;
        const u32* d_coefs = ctx->p_coefs.as<u32>();
        if (resident) BPCHK(pl_csc<C>(ctx, j.cs.base, csc, k, d_coefs));
        else BPCHK(prove_csc_stage(ctx, csc, small_stmt, k));
        F4 ztab[32];
        host::prove_pow_tables<C>(j.z, j.y, ztab, small_stmt ? j.ypw : nullptr);
        u32* d_ztab = resident ? ctx->pl_ztab.as<u32>() : ctx->p_coefs.as<u32>() + nc * 8;
        if (small_stmt && resident) {   // the per-proof tables alone: powers of z and the y tables, one launch from the pinned slab
            ypw_early = true;
            BPCHK(ctx->r_ypow.ensure(64 * 32));
            BPCHK(upload_slab_ensure(ctx, 96 * 32));
            char* stage = (char*)ctx->h_upload;
            memcpy(stage, ztab, 32 * 32); memcpy(stage + 32 * 32, j.ypw, 64 * 32);
            ImportList il; memset(&il, 0, sizeof il);
            il.nseg = 2;
            il.dst[0] = d_ztab; il.cnt[0] = 32; il.dst[1] = ctx->r_ypow.as<u32>(); il.cnt[1] = 64;
            hipLaunchKernelGGL(k_scalars_import_multi<FrP>, dim3(1), dim3(256), 0, st, (const u32*)stage, il);
        } else if (small_stmt) {   // coefficient table, powers of z and the y tables (needed by the t(x) kernels below) in one launch, read from the pinned slab
            ypw_early = true;
            BPCHK(ctx->r_ypow.ensure(64 * 32));
            BPCHK(upload_slab_ensure(ctx, (nc + 96) * 32));
            char* stage = (char*)ctx->h_upload;
            memcpy(stage, csc.coefs.data(), nc * 32); memcpy(stage + nc * 32, ztab, 32 * 32); memcpy(stage + (nc + 32) * 32, j.ypw, 64 * 32);
            ImportList il; memset(&il, 0, sizeof il);
            il.nseg = 3;
            il.dst[0] = ctx->p_coefs.as<u32>(); il.cnt[0] = (u32)nc; il.dst[1] = d_ztab; il.cnt[1] = 32; il.dst[2] = ctx->r_ypow.as<u32>(); il.cnt[2] = 64;
            hipLaunchKernelGGL(k_scalars_import_multi<FrP>, dim3((u32)((nc + 96 + 255) / 256)), dim3(256), 0, st, (const u32*)stage, il);
        } else {
            if (!resident) BPCHK(upload_scalars<C>(ctx, ctx->p_coefs.as<u32>(), csc.coefs.data(), nc));
            BPCHK(upload_scalars<C>(ctx, d_ztab, ztab, 32));
        }
        hipLaunchKernelGGL(k_r1cs_ztables<C>, dim3((std::max(256u, nzhi) + 255) / 256), dim3(256), 0, st, d_ztab, nzhi, ctx->p_ztab.as<u32>());
        hipLaunchKernelGGL(k_r1cs_flatten<C>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, k.moff, k.ment, k.mc,
                           d_coefs, ctx->p_ztab.as<u32>(), (u32)n, ctx->r_wL.as<u32>(), ctx->r_wR.as<u32>(), ctx->r_wO.as<u32>());
        HIPCHK(hipGetLastError());
        host::prove_wv<C>(csc, ztab, j.cs.v.size(), j.wV);
        j.tm.flatten += now_s() - t0;
        t0 = now_s();
    } else {
        std::vector<F4> wL, wR, wO; F4 wc;
        j.cs.flatten(j.z, wL, wR, wO, j.wV, wc, j.cs.v.size());
        j.tm.flatten += now_s() - t0;
        t0 = now_s();
        BPCHK(upload_scalars<C>(ctx, ctx->r_wL.as<u32>(), wL.data(), n));
        BPCHK(upload_scalars<C>(ctx, ctx->r_wR.as<u32>(), wR.data(), n));
        BPCHK(upload_scalars<C>(ctx, ctx->r_wO.as<u32>(), wO.data(), n));
        HIPCHK(ctx_stream_wait(ctx));   // wL, wR, wO are locals of this branch
    }
    j.trace.mark("flatten");
    if (!ypw_early) {
        host::prove_pow_tables<C>(j.z, j.y, nullptr, j.ypw);
        BPCHK(ctx->r_ypow.ensure(64 * 32));
        BPCHK(upload_scalars<C>(ctx, ctx->r_ypow.as<u32>(), j.ypw, 64));
    }
    j.tm.upload += now_s() - t0;
    return BP_OK;
}

// t_1 .. t_6 (prover.rs:651-698) and T_1, T_3 .. T_6 (prover.rs:709-714): a small statement's T commitments follow the t(x) kernels
// over the direct window tables, behind k_r1cs_sum in the stream, without a host round trip in between
template <class C> static int prove_poly_t(ProveJob<C>& j) {
    typedef host::Fld<typename C::Fr> S;
    bp_ctx* ctx = j.ctx;
    hipStream_t st = ctx->stream;
    const size_t n = j.n;
    const double t0 = now_s();
    bool t_direct = false;
    J4 Tj[5];
    if (n > 0) {
        const u32 gb = (u32)((n + 255) / 256);
        BPCHK(ctx->r_part.ensure((size_t)gb * 6 * 32)); BPCHK(ctx->r_small.ensure(6 * 32));
        BPCHK(dt_ensure<C>(ctx, j.N, t_direct));
        ScopedK tk(ctx, BP_K_R1CS_POLY);
        hipLaunchKernelGGL(k_r1cs_poly_t<C>, dim3(gb), dim3(256), 0, st, ctx->r_aL.as<u32>(), ctx->r_aR.as<u32>(), ctx->r_aO.as<u32>(), ctx->r_sL.as<u32>(),
                           ctx->r_sR.as<u32>(), ctx->r_wL.as<u32>(), ctx->r_wR.as<u32>(), ctx->r_wO.as<u32>(), ctx->r_ypow.as<u32>(), (u32)n, ctx->r_part.as<u32>(),
                           gb == 1 ? ctx->r_small.as<u32>() : (u32*)nullptr);
        if (gb > 1) hipLaunchKernelGGL(k_r1cs_sum<C>, dim3(1), dim3(256), 0, st, ctx->r_part.as<u32>(), gb, 6u, ctx->r_small.as<u32>());
        tk.stop();
        HIPCHK(hipMemcpyAsync(j.tco, ctx->r_small.p, 6 * 32, hipMemcpyDeviceToHost, st));
        if (t_direct) {
            DtJobs jobs; memset(&jobs, 0, sizeof jobs);
            dt_t_jobs<C>(jobs.job, ctx->r_small.as<u32>() /* k_r1cs_sum writes ark words */, j.tb, nullptr);
            BPCHK(msm_direct_launch<C>(ctx, jobs, 5));
        }
        HIPCHK(ctx_stream_wait(ctx));
        HIPCHK(hipGetLastError());
        if (t_direct) msm_direct_collect<C>(ctx, 5, Tj);
    } else {
        for (auto& t : j.tco) t = S::zero();
    }
    j.tm.poly += now_s() - t0;
    j.trace.mark("poly t");
    const int slot[5] = {0, 2, 3, 4, 5};
    if (t_direct) to_aff_many<C>(Tj, 5, j.Tc);
    else for (int o = 0; o < 5; o++) j.Tc[o] = j.pc.commit(j.tco[slot[o]], j.tb[o]);
    return BP_OK;
}

// l(x), r(x), G_factors, H_factors on the device (prover.rs:723-789); working copies of the generator tables; Q
template <class C> static int prove_eval(ProveJob<C>& j) {
    typedef host::Fld<typename C::Fr> S;
    typedef host::Grp<C> G;
    bp_ctx* ctx = j.ctx;
    hipStream_t st = ctx->stream;
    const size_t N = j.N;
    const double t0 = now_s();
    BPCHK(ctx->ipa_a.ensure(N * 32)); BPCHK(ctx->ipa_b.ensure(N * 32)); BPCHK(ctx->ipa_Gf.ensure(N * 32)); BPCHK(ctx->ipa_Hf.ensure(N * 32));
    if (!ipa_cyclic_applies(ctx, N)) { BPCHK(ctx->ipa_G.ensure(N * 64)); BPCHK(ctx->ipa_H.ensure(N * 64)); }
    BPCHK(ctx->ipa_Q.ensure(64));
    BPCHK(prove_ensure_vecs(ctx, N));
    {
        ScopedK tk(ctx, BP_K_R1CS_POLY);
        hipLaunchKernelGGL(k_r1cs_poly_eval<C>, dim3((u32)((N + 255) / 256)), dim3(256), 0, st, ctx->r_aL.as<u32>(), ctx->r_aR.as<u32>(), ctx->r_aO.as<u32>(),
                           ctx->r_sL.as<u32>(), ctx->r_sR.as<u32>(), ctx->r_wL.as<u32>(), ctx->r_wR.as<u32>(), ctx->r_wO.as<u32>(), ctx->r_ypow.as<u32>(), (u32)j.n,
                           (u32)j.n1, (u32)N, words_of<S>(j.x), words_of<S>(j.u), ctx->ipa_a.as<u32>(), ctx->ipa_b.as<u32>(), ctx->ipa_Gf.as<u32>(),
                           ctx->ipa_Hf.as<u32>());
    }
    j.cyclic = ipa_cyclic_applies(ctx, N);   // sharded prover: the IPA's vectors partitioned index-cyclically across the ranks
    j.direct = false;   // small statements: no folding of G and H at all, every round over the direct window tables
    if (!j.cyclic && N >= 2) BPCHK(dt_ensure<C>(ctx, N, j.direct));
    // with first-round fold tables the round reads the resident generator tables in place: no working copy (2 x 64 B x N)
    j.in_place = !j.cyclic && !j.direct && N >= 128 && (ctx->ftab_n >= N / 2 || ctx->fb_cap >= N);
    if (!j.cyclic && !j.in_place && !j.direct) {
        HIPCHK(hipMemcpyAsync(ctx->ipa_G.p, ctx->d_G.p, N * 64, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->ipa_H.p, ctx->d_H.p, N * 64, hipMemcpyDeviceToDevice, st));
    }
    if (!j.direct) {   // Q = w * B as a point (prover.rs:779); over the direct tables c * Q is (c * w) * B and Q itself is never formed
        const A4 Q = G::to_aff(j.pc.mul_B_jac(j.w));   // (the host's fixed-base tables of the ctx's pair)
        uint64_t Qw[8]; memcpy(Qw, Q.x.v, 32); memcpy(Qw + 4, Q.y.v, 32);
        HIPCHK(hipMemcpyAsync(ctx->ipa_Q.p, Qw, 64, hipMemcpyHostToDevice, st));
        BPCHK(bp_points_import(ctx, ctx->ipa_Q.p, ctx->ipa_Q.p, 1));
    }
    j.tm.poly += now_s() - t0;
    return BP_OK;
}

// The inner-product argument (prover.rs:791-803) — here, or handed to a lockstep group (defer) — into `proof`
template <class C> static int prove_ipa(ProveJob<C>& j, IpaDefer* defer, host::ProofData& proof) {
    typedef host::Fld<typename C::Fr> S;
    typedef host::TP<C> TP;
    bp_ctx* ctx = j.ctx;
    hipStream_t st = ctx->stream;
    host::Transcript& tr = *j.cs.tr;
    const size_t N = j.N, n1 = j.n1;
    const double t0 = now_s();
    IpaDeferSlot dslot;
    j.deferred = defer && j.direct && !j.cyclic && N >= 2 && ctx->dt_cap >= N && defer->take(N, dslot);
    if (j.deferred) {   // (the same copies ipa_create_dev's direct path makes of the factor vectors)
        HIPCHK(hipMemcpyAsync(dslot.a, ctx->ipa_a.p, N * 32, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(dslot.b, ctx->ipa_b.p, N * 32, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(dslot.cG, ctx->ipa_Gf.p, N * 32, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(dslot.cH, ctx->ipa_Hf.p, N * 32, hipMemcpyDeviceToDevice, st));
        defer->taken = true; defer->N = N; defer->w = j.w;
    }
    TP::innerproduct_domain_sep(tr, N);
    size_t lg = 0; while (((size_t)1 << lg) < N) lg++;
    std::vector<uint64_t> Lw(8 * std::max<size_t>(lg, 1)), Rw(8 * std::max<size_t>(lg, 1));
    uint64_t aw[4], bw[4];
    ChallengeFn fn = [&](const uint64_t* L, const uint64_t* R, uint64_t* uo) {
        A4 Lp, Rp; memcpy(Lp.x.v, L, 32); memcpy(Lp.y.v, L + 4, 32); memcpy(Rp.x.v, R, 32); memcpy(Rp.y.v, R + 4, 32);
        const F4 uu = host::prove_round_challenge<C>(tr, Lp, Rp);
        memcpy(uo, uu.v, 32);
        return 0;
    };
    // G_factors = [1]*n1 ++ [u]*(N-n1) (prover.rs:781-784): constant on each half of the first fold iff n1 is 0, N/2 or >= N
    F4 gfh[2] = {n1 >= N / 2 ? S::one() : j.u, n1 >= N ? S::one() : j.u};
    const bool gf_const_halves = N >= 2 && (n1 == 0 || n1 == N / 2 || n1 >= N);
    if (j.deferred) {}
    else if (j.cyclic)
        BPCHK(ipa_create_cyclic<C>(ctx, ctx->ipa_Q.as<u32>(), ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), ctx->d_G.as<u32>(), ctx->d_H.as<u32>(), ctx->ipa_a.as<u32>(),
                                   ctx->ipa_b.as<u32>(), N, fn, Lw.data(), Rw.data(), aw, bw, gf_const_halves ? gfh : nullptr, gf_const_halves ? j.ypw : nullptr,
                                   gf_const_halves ? ctx->r_ypow.as<u32>() + 32 * 8 : nullptr, &j.w));
    else
        BPCHK(ipa_create_dev<C>(ctx, ctx->ipa_Q.as<u32>(), ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), ctx->ipa_G.as<u32>(), ctx->ipa_H.as<u32>(),
                                ctx->ipa_a.as<u32>(), ctx->ipa_b.as<u32>(), N, fn, Lw.data(), Rw.data(), aw, bw, gf_const_halves ? gfh : nullptr,
                                // H_factors[i] = y^-i * G_factors[i] (prover.rs:785-789): rho = y^-1; ypw[k] = y^(2^k) = rho^-(2^k), ypw[32+k] = rho^(2^k)
                                gf_const_halves ? j.ypw : nullptr, gf_const_halves ? ctx->r_ypow.as<u32>() + 32 * 8 : nullptr, true, j.in_place, &j.w, j.direct));
    j.tm.ipa += now_s() - t0;
    j.trace.mark("inner-product argument");

    proof.A_I1 = j.c1[0]; proof.A_O1 = j.c1[1]; proof.S1 = j.c1[2]; proof.A_I2 = j.c2[0]; proof.A_O2 = j.c2[1]; proof.S2 = j.c2[2];
    proof.T_1 = j.Tc[0]; proof.T_3 = j.Tc[1]; proof.T_4 = j.Tc[2]; proof.T_5 = j.Tc[3]; proof.T_6 = j.Tc[4];
    proof.t_x = j.t_x; proof.t_x_blinding = j.t_x_blinding; proof.e_blinding = j.e_blinding;
    if (!j.deferred) {
        proof.L_vec.resize(lg); proof.R_vec.resize(lg);
        for (size_t i = 0; i < lg; i++) {
            memcpy(proof.L_vec[i].x.v, &Lw[8 * i], 32); memcpy(proof.L_vec[i].y.v, &Lw[8 * i + 4], 32);
            memcpy(proof.R_vec[i].x.v, &Rw[8 * i], 32); memcpy(proof.R_vec[i].y.v, &Rw[8 * i + 4], 32);
        }
        memcpy(proof.a.v, aw, 32); memcpy(proof.b.v, bw, 32);
    }
    return BP_OK;
}

// secret hygiene (prover.rs:74-94, 805-812): the witness-derived device vectors, the host copies of s_L / s_R, the key
template <class C> static int prove_wipe(ProveJob<C>& j) {
    typedef host::Fld<typename C::Fr> S;
    bp_ctx* ctx = j.ctx;
    j.secrets_up = false;
    for (auto& s : j.pre.s_L) s = S::zero();
    for (auto& s : j.pre.s_R) s = S::zero();
    j.pre.kappa1 = S::zero();
    DevBuf* wipe[] = {&ctx->r_aL, &ctx->r_aR, &ctx->r_aO, &ctx->r_sL, &ctx->r_sR, &ctx->ipa_a, &ctx->ipa_b, &ctx->cyc_a, &ctx->cyc_b, &ctx->dt_a2, &ctx->dt_b2};
    size_t total = 0;
    int live = 0;
    for (auto b : wipe) if (b->p) { total += b->cap; live++; }
    if (live && live <= ZERO_MAX && total <= ((size_t)64 << 20)) {   // a small proof: one launch instead of eleven memsets
        ZeroList zl; memset(&zl, 0, sizeof zl);
        for (auto b : wipe) if (b->p) { zl.p[zl.count] = (uint4*)b->p; zl.n16[zl.count] = (u32)(b->cap / 16); zl.count++; }   // (allocations are 256-byte multiples + 256: cap / 16 units cover all but < 16 trailing bytes that no kernel addresses)
        hipLaunchKernelGGL(k_zero_many, dim3((u32)std::min<size_t>(1024, (total / 16 + 255) / 256)), dim3(256), 0, ctx->stream, zl);
        HIPCHK(hipGetLastError());
    } else {
        for (auto b : wipe) if (b->p) HIPCHK(hipMemsetAsync(b->p, 0, b->cap, ctx->stream));
    }
    return BP_OK;
}
// ... on every way out once something secret is on the device: a stage that fails returns through this
template <class C> struct ProveWipeScope {
    ProveJob<C>& j;
    ~ProveWipeScope() { if (j.secrets_up) (void)prove_wipe<C>(j); }
};

template <class C>
static int r1cs_prove(bp_ctx* ctx, host::ConstraintSystem<C>& cs, const host::u8* rng_bytes, host::ProofData& proof, StageTimes& tm,
                      ProvePre<C>* pre_in = nullptr, const HostCsc* csc = nullptr /* constraint index built with the statement (single-phase) */,
                      IpaDefer* defer = nullptr,
                      const A4* resume1 = nullptr /* bp_prover_prove_batch, a member that leaves its front group after the randomized phase: A_I1, A_O1,
                      S1 are in the transcript and the phase has run — neither happens again; the whole witness goes up to the workspaces here */,
                      WcGuard* guard = nullptr /* bp_prover_set_check: refuse an unsatisfying witness with BP_E_UNSATISFIED and its report */) {
    typedef host::Fld<typename C::Fr> S;
    typedef host::Grp<C> G;
    typedef host::TP<C> TP;
    host::Transcript& tr = *cs.tr;
    const double t_begin = now_s();
    static const bool trace = getenv("ARKBP_PROVE_TRACE") != nullptr;
    ProvePre<C> pre_local;
    ProvePre<C>& pre = pre_in && pre_in->rng ? *pre_in : pre_local;
    if (pre_in) pre_local.mode = pre_in->mode;
    ProveJob<C> j{ctx, cs, pre, tm};
    j.pc.B = ctx->pc_B; j.pc.B_blinding = ctx->pc_Bb;
    j.trace.on = trace;
    j.csc = csc;
    j.trace.mark("begin");
    j.expanded = pre.mode == BP_BLINDING_EXPANDED;
    if (!pre.rng) prove_precompute<C>(cs, rng_bytes, pre);
    host::TranscriptRng& rng = *pre.rng;
    tm.rng += pre.t_rng;
    // (a like-prover's randomized callbacks read and extend a_O on the host; a witness in device memory stays there only for a
    // single-phase proof on a ctx that is not sharded)
    if (!cs.deferred.empty() || resume1 || (cs.dev.held() && ctx->shard_world > 1)) BPCHK(prove_need_aO<C>(ctx, cs));
    const size_t n1 = j.n1 = resume1 ? cs.n1 : cs.mults();
    if (ctx->gens_cap < n1) return BP_E_GENS_LENGTH;
    j.b1[0] = pre.i_b1; j.b1[1] = pre.o_b1; j.b1[2] = pre.s_b1;

    ProveWipeScope<C> wipe_on_exit{j};
    BPCHK(prove_upload_phase<C>(j, 0, n1, pre.kappa1));
    j.trace.mark("head + upload");
    if (resume1) for (int o = 0; o < 3; o++) j.c1[o] = resume1[o];
    else BPCHK(prove_commit_phase<C>(j, 0, n1, j.b1, j.c1));
    j.trace.mark("commit phase 1");
    if (!resume1) {
        host::prove_append_phase<C>(tr, 1, j.c1[0], j.c1[1], j.c1[2]);
        int rc = cs.run_randomized();
        if (rc) return rc;
    }
    j.trace.mark("randomized phase");

    const size_t n = j.n = cs.mults(), N = j.N = host::next_pow2(n);
    if (ctx->gens_cap < N) return BP_E_GENS_LENGTH;
    const bool has2 = n > n1;
    double t0 = now_s();
    F4 kappa2;
    host::prove_draw_phase2<C>(rng, has2, j.expanded, n1, n, j.bl2, kappa2, pre.s_L, pre.s_R);
    tm.rng += now_s() - t0;
    j.c2[0] = j.c2[1] = j.c2[2] = G::aff_inf();
    if (has2) {
        const int rc = prove_upload_phase<C>(j, n1, n - n1, kappa2);
        kappa2 = S::zero();
        BPCHK(rc);
        BPCHK(prove_commit_phase<C>(j, n1, n - n1, j.bl2, j.c2));
    }
    j.trace.mark("commit phase 2");
    // the guard: the whole witness is resident and every constraint exists.  The check is enqueued here and its flags are read after
    // the wait prove_poly_t makes anyway; a statement without multipliers has no such wait and few rows: the host twin decides it.
    WcRun<C> wc;
    if (guard && guard->on) {
        if (n == 0) {
            BPCHK(prove_need_aO<C>(ctx, cs));
            host::witness_check_host<C>(cs, guard->report);
            if (guard->report.bad_gates || guard->report.bad_constraints) { g_err = "prove: the witness does not satisfy the constraint system"; return BP_E_UNSATISFIED; }
        } else {
            wc.own.resize(1);
            if (cs.num_terms() > ((size_t)1 << 16)) host_pool_ensure(ctx, 2);   // (a large statement's index is built on the pool)
            const host::RowIndexPar par = [&](size_t cnt, const std::function<void(size_t)>& fn) { pool_range(ctx, 0, cnt, fn); };
            WcItem<C> it; it.cs = &cs;
            // a like-prover that recorded nothing itself: the recording's index, built once and resident on this ctx
            std::shared_ptr<const HostRowIndex> shared;
            if (cs.base && cs.own_empty()) shared = host::shared_row_index<C>(*cs.base, cs.v.size(), WC_PIECE, par);
            if (shared) {
                it.idx = shared.get();
                if (ctx->shard_world <= 1) BPCHK(pl_row<C>(ctx, cs.base, *shared, it.dev));
            } else {
                if (!build_row_index<C>(cs, WC_PIECE, wc.own[0], par)) { g_err = "prove: the constraints cannot be indexed for the witness check"; return BP_E_ARG; }
                it.idx = &wc.own[0];
            }
            it.aL = ctx->r_aL.as<u32>(); it.aR = ctx->r_aR.as<u32>(); it.aO = ctx->r_aO.as<u32>();
            wc.items.push_back(it);
            BPCHK(wc_enqueue<C>(ctx, wc, nullptr));
            BPCHK(wc_fetch<C>(ctx, wc));
            BPCHK(wc_wipe_dev<C>(ctx, wc));
        }
    }
    host::prove_append_phase<C>(tr, 2, j.c2[0], j.c2[1], j.c2[2]);
    j.y = TP::challenge_scalar(tr, "y"); j.z = TP::challenge_scalar(tr, "z");
    BPCHK(prove_flatten<C>(j));
    t0 = now_s();
    host::prove_draw_t<C>(rng, j.tb);   // (drawn before t(x): a small statement's T commitments then follow its kernels on the GPU)
    tm.rng += now_s() - t0;
    BPCHK(prove_poly_t<C>(j));
    j.trace.mark("T commitments");
    if (wc.enqueued) {
        wc_wipe_host<C>(ctx, wc);
        if (wc_flags_bad(wc.flags(ctx, 0))) {
            BPCHK(prove_need_aO<C>(ctx, cs));   // (the residual of the failing row may read a_O)
            host::witness_report_from_flags<C>(cs, wc.flags(ctx, 0), guard->report);
            g_err = "prove: the witness does not satisfy the constraint system";
            return BP_E_UNSATISFIED;
        }
    }
    host::prove_t_tail<C>(tr, j.Tc, j.tco, j.tb, j.wV, cs.v_blinding, j.b1, j.bl2, j.u, j.x, j.t_x, j.t_x_blinding, j.e_blinding, j.w);
    j.trace.mark("t_x .. w");
    BPCHK(prove_eval<C>(j));
    j.trace.mark("l(x), r(x), Q");
    BPCHK(prove_ipa<C>(j, defer, proof));
    BPCHK(prove_wipe<C>(j));
    tm.total = now_s() - t_begin + (pre_in && pre_in->rng ? pre.t_rng : 0.0);
    if (ctx->profiling) collect_timers(ctx);
    j.trace.print(n);
    return BP_OK;
}

// ---- batched Pedersen commitments (PedersenGens::commit, src/generators.rs:39-44, for all inputs of a statement) -------
template <class C> static int pedersen_ensure(bp_ctx* ctx) {
    if (!ctx->d_pc.p) {   // a ctx without BulletproofGens still has its PedersenGens
        BPCHK(pc_upload<C>(ctx));
    }
    if (!ctx->pc_table.p) {
        BPCHK(ctx->pc_table.ensure(PC_TABLE_BYTES));
        hipLaunchKernelGGL(k_pc_table_build<C>, dim3(2 * PC_WINDOWS * PC_DIGITS / 256), dim3(256), 0, ctx->stream, ctx->d_pc.as<u32>(), ctx->pc_table.as<u32>());
        HIPCHK(hipGetLastError());
    }
    if (!ctx->pc_dt.p) {   // direct window tables of the two bases (small.cuh): the latency form for a handful of commitments
        DevBuf ws;
        BPCHK(ws.ensure((size_t)2 * DT_WINDOWS * 96));
        BPCHK(ctx->pc_dt.ensure((size_t)2 * DT_BASE_BYTES));
        hipLaunchKernelGGL(k_dt_window_bases<C>, dim3(1), dim3(64), 0, ctx->stream, ctx->d_pc.as<u32>(), 2u, ws.as<u32>());
        hipLaunchKernelGGL(k_dt_entries<C>, dim3((2 * DT_PER_BASE + 255) / 256), dim3(256), 0, ctx->stream, ws.as<u32>(), 2u, ctx->pc_dt.as<u32>());
        HIPCHK(hipGetLastError());
        HIPCHK(ctx_stream_wait(ctx));
        ws.release();
    }
    return BP_OK;
}
// A pair of the caller's choice as two points of the curve: what the affine tables can hold (no identity), canonical coordinates
template <class C> static bool pc_point_ok(const uint64_t* xy, A4& out) {
    typedef host::Fld<typename C::Fq> F;
    memcpy(out.x.v, xy, 32); memcpy(out.y.v, xy + 4, 32);
    if (F::geq_p(out.x.v) || F::geq_p(out.y.v) || out.is_inf()) return false;
    return host::Grp<C>::on_curve(out);
}
// bp_pedersen_gens_install: the pair changes, and with it exactly what was computed from it.  Bases 0 and 1 of the direct window
// tables and the fb_pc rows are rebuilt in place by the builders that made them; tables 5 and 6 go and come back with
// pedersen_ensure.  Nothing that holds multiples of G and H only is read or written.  One wait.
template <class C> static int pedersen_install(bp_ctx* ctx, const A4* B, const A4* Bb) {
    hipStream_t st = ctx->stream;
    if (B) { ctx->pc_B = *B; ctx->pc_Bb = *Bb; ctx->pc_set = true; ctx->pc_custom = true; }
    else ctx->pc_set = false;   // (pc_pair puts the default there)
    BPCHK(pc_upload<C>(ctx));
    DevBuf ws, tmp, pref, outb;
    auto done = [&](int rc) { ws.release(); tmp.release(); pref.release(); outb.release(); return rc; };
    if (ctx->dt_cap && ctx->dt_tab.p) {
        if (int rc = ws.ensure((size_t)2 * DT_WINDOWS * 96)) return done(rc);
        hipLaunchKernelGGL(k_dt_window_bases<C>, dim3(1), dim3(64), 0, st, ctx->d_pc.as<u32>(), 2u, ws.as<u32>());
        hipLaunchKernelGGL(k_dt_entries<C>, dim3((2 * DT_PER_BASE + 255) / 256), dim3(256), 0, st, ws.as<u32>(), 2u, ctx->dt_tab.as<u32>());
    }
    if (ctx->fb_cap && ctx->fb_pc.p) {
        int rc = tmp.ensure((size_t)FB_ROWS * 2 * 96);
        if (!rc) rc = pref.ensure((size_t)FB_ROWS * 2 * 32);
        if (!rc) rc = outb.ensure((size_t)FB_ROWS * 2 * 64);
        if (!rc) rc = fb_rows_build<C>(st, ctx->d_pc.as<u32>(), ctx->fb_pc.as<u32>(), 2, 2, 2, tmp, pref, outb);
        if (rc) return done(rc);
    }
    if (hipGetLastError() != hipSuccess || ctx_stream_wait(ctx) != hipSuccess) { g_err = "bp_pedersen_gens_install: HIP error"; return done(BP_E_HIP); }
    ctx->pc_table.release(); ctx->pc_dt.release();
    return done(BP_OK);
}
static constexpr size_t PC_LATENCY_MAX = 4096;  // commitments per call up to which the wave-per-commitment kernel runs (one wave each: 4096 fill the chip four times)
// v, blind: m Fr values in ark layout (host); out: m affine points in ark layout (host)
template <class C> static int pedersen_commit_batch(bp_ctx* ctx, const uint64_t* v, const uint64_t* blind, size_t m, uint64_t* out_xy) {
    if (!m) return BP_OK;
    BPCHK(pedersen_ensure<C>(ctx));
    if (m <= PC_LATENCY_MAX) {
        BPCHK(ctx->io_scal.ensure(m * 64)); BPCHK(ctx->io_pts.ensure(m * 96));
        BPCHK(upload_slab_ensure(ctx, m * 160));
        char* slab = (char*)ctx->h_upload;
        memcpy(slab, v, m * 32); memcpy(slab + m * 32, blind, m * 32);
        HIPCHK(hipMemcpyAsync(ctx->io_scal.p, slab, m * 64, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_dt_commit<C>, dim3((u32)((m + 3) / 4)), dim3(256), 0, ctx->stream, ctx->pc_dt.as<u32>(), ctx->io_scal.as<u32>(), ctx->io_scal.as<u32>() + m * 8,
                           (u32)m, ctx->io_pts.as<u32>());
        HIPCHK(hipGetLastError());
        const J4* jac = (const J4*)(slab + m * 64);
        HIPCHK(hipMemcpyAsync((void*)jac, ctx->io_pts.p, m * 96, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx_stream_wait(ctx));
        to_aff_many<C>(jac, m, (A4*)out_xy);   // one inversion for the whole batch; the identity (v = blind = 0) stays all-zero words
        return BP_OK;
    }
    const size_t CHUNK = (size_t)1 << 20;   // bounds the staging buffers (128 MiB) for very wide statements
    for (size_t lo = 0; lo < m; lo += CHUNK) {
        const size_t cnt = std::min(CHUNK, m - lo);
        BPCHK(ctx->io_scal.ensure(cnt * 64)); BPCHK(ctx->io_pts.ensure(cnt * 64));
        HIPCHK(hipMemcpyAsync(ctx->io_scal.p, v + 4 * lo, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync((char*)ctx->io_scal.p + cnt * 32, blind + 4 * lo, cnt * 32, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pc_commit<C>, dim3((u32)((cnt + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pc_table.as<u32>(), ctx->io_scal.as<u32>(),
                           ctx->io_scal.as<u32>() + cnt * 8, (u32)cnt, ctx->io_pts.as<u32>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out_xy + 8 * lo, ctx->io_pts.p, cnt * 64, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx_stream_wait(ctx));
    }
    return BP_OK;
}
template <class C> static void pedersen_attach(bp_ctx* ctx, host::PedersenGens<C>& pc) {
    pc.batch = [ctx](const F4* v, const F4* blind, size_t m, A4* out) -> int {
        static_assert(sizeof(F4) == 32 && sizeof(A4) == 64, "F4 / A4 are the ABI's plain word arrays");
        return pedersen_commit_batch<C>(ctx, (const uint64_t*)v, (const uint64_t*)blind, m, (uint64_t*)out);
    };
}

// ---- scenario drivers (statement construction + prove / verify), used by the tests and bench.py ----------
// The scenarios are CALLERS of the generic recorder (host::ConstraintSystem) and of the generic prove / batch-verify cores below:
// nothing in the measured path is specific to them.
template <class C>
static int prove_scenario(bp_ctx* ctx, int scenario, const uint64_t* params, const uint8_t* seed, std::vector<host::u8>& proof_bytes,
                          host::StatementIO& io, double* timing) {
    host::ChaChaRng prng(seed);
    host::Transcript tr(host::scenario_label(scenario));
    host::ConstraintSystem<C> cs;
    cs.tr = &tr; cs.proving = true;
    host::TP<C>::r1cs_domain_sep(tr);  // Prover::new (prover.rs:291-308)
    host::PedersenGens<C> pc; pc.B = ctx->pc_B; pc.B_blinding = ctx->pc_Bb;
    if (!ctx->gens_cap) { g_err = "prove: generators not installed (bp_gens_derive / bp_gens_upload)"; return BP_E_GENS_LENGTH; }
    pedersen_attach<C>(ctx, pc);
    double t0 = now_s();
    BPCHK(host::scenario_prover<C>(cs, pc, prng, scenario, params, io));
    double t1 = now_s();
    host::u8 rng32[32]; prng.fill_bytes(rng32, 32);   // what `prove(prng, ..)` takes from the external rng (TranscriptRngBuilder::finalize)
    host::ProofData pf;
    StageTimes tm;
    HostCsc csc;
    const bool have_csc = build_host_csc<C>(cs, csc);   // statement construction: the constraint index of single-phase statements
    BPCHK(r1cs_prove<C>(ctx, cs, rng32, pf, tm, nullptr, have_csc ? &csc : nullptr));
    proof_bytes = host::proof_to_bytes<C>(pf);
    if (timing) {
        timing[0] = tm.total; timing[1] = t1 - t0; timing[2] = tm.rng; timing[3] = tm.upload; timing[4] = tm.commit_msm; timing[5] = tm.flatten;
        timing[6] = tm.poly; timing[7] = tm.ipa;
    }
    return BP_OK;
}

// ---- Verifier (src/r1cs/verifier.rs:394-600) and batch_verify (:604-691) -------------------------------------
// Host: transcript replay and the O(k), O(m) scalars; GPU: flattened constraints, the 2N g/h scalars and the mega-check MSM.
template <class C> struct VerifyPrep {
    size_t n = 0, n1 = 0, N = 0, k = 0, m = 0, nq = 0;
    std::vector<F4> wL, wR, wO;          // only for bp_r1cs_verification_gh (a caller's own flattened vectors)
    F4 x, u, a, b, allinv;
    std::vector<F4> u_sq;                // k
    F4 ypw[64];                          // y^(2^j), y^-(2^j)
    F4 ztab[32];                         // z^(2^j)
    F4 sB, sBb;                          // scalars of B, B_blinding (sB without the wc + delta term: that sum is formed on the GPU)
    F4 coefD;                            // r * x^2: weight of (wc + delta) inside sB
    F4 rx;                               // r * x
    std::vector<F4> tail_scalars;        // 6 + m + 5 + 2k
    std::vector<A4> tail_points;
    // canonical structure of the instance's recording (host_proto.hpp CanonState): which template evaluates it, with which values
    host::Digest digest;
    host::CanonState canon_own;          // scratch of instances that recorded constraints themselves
    const F4* coef_ptr = nullptr;        // id -> coefficient value (points into canon_own or into the shared base's cache)
    size_t ncoef = 0;
    const char* err = nullptr;           // explanation of a non-zero status set on a worker thread (published by the calling thread)
};

// A circuit template: the constraint matrices of one gadget STRUCTURE as CSC on the GPU, coefficient values factored out (the
// table of the instance that created it is kept as the default).  Keyed by the structure digest; built once per ctx and cached.
template <class C> struct VTemplate {
    size_t n = 0, n1 = 0, q = 0, ncoef = 0;
    std::vector<F4> coefs_host;          // the creator's table: instances with the same values share d_coefs
    DevBuf d_coefs, d_cq, d_cc, d_moff, d_ment, d_mc;
    VfyTemplateDev dev;
    ~VTemplate() { d_coefs.release(); d_cq.release(); d_cc.release(); d_moff.release(); d_ment.release(); d_mc.release(); }
};

// cs: a verifier recording after its randomized phase ran (both phases present)
template <class C> static int build_template(bp_ctx* ctx, const host::ConstraintSystem<C>& cs, VTemplate<C>& t) {
    typedef host::Fld<typename C::Fr> S;
    const size_t n = cs.num_vars;
    t.n = n; t.n1 = cs.n1; t.q = cs.num_constraints();
    if (t.q >= ((size_t)1 << 30) || n >= ((size_t)1 << 31)) { g_err = "verifier template: circuit too large"; return BP_E_ARG; }
    auto vec_of = [](int k) { return k == host::VK_LEFT ? 0 : k == host::VK_RIGHT ? 1 : k == host::VK_OUT ? 2 : -1; };
    // CSC with the three vectors merged: per multiplier index i, the entries of columns i of W_L, W_R, W_O sorted by constraint
    // index (the walk is in constraint order, so every column's run comes out sorted)
    std::vector<u32> moff(n + 1, 0), ment, mc, cq, cc;
    cs.for_each_term([&](size_t, const host::Term& tm) { if (vec_of(tm.v.k) >= 0) moff[tm.v.i + 1]++; });
    for (size_t i = 0; i < n; i++) moff[i + 1] += moff[i];
    ment.resize(moff[n]); mc.resize(moff[n]);
    std::vector<u32> cur(moff.begin(), moff.end() - 1);
    const F4 one = S::one(), mone = S::neg(S::one());
    host::CanonState st;
    bool ok = true;
    auto sink = [&](size_t q, const host::Term& tm, u32 cid) {
        if (!(cid & (host::CID_ONE | host::CID_MONE)) && cid >= (1u << 30)) ok = false;
        if (tm.v.k == host::VK_ONE) { cq.push_back((u32)q); cc.push_back(cid); return; }
        const int v = vec_of(tm.v.k);
        if (v < 0) return;   // committed-variable terms feed wV per instance (verify_prepare)
        const u32 pos = cur[tm.v.i]++;
        ment[pos] = ((u32)v << 30) | (u32)q;
        mc[pos] = cid;
    };
    if (cs.base) st.walk(cs.base->terms.data(), cs.base->off.data(), cs.base->nq(), 0, one, mone, sink);
    st.walk(cs.cs_terms.data(), cs.cs_off.data(), cs.cs_off.size() - 1, cs.base_nq(), one, mone, sink);
    if (!ok) { g_err = "verifier template: too many distinct coefficients"; return BP_E_ARG; }
    t.ncoef = st.coefs.size();
    t.coefs_host = st.coefs;
    hipStream_t stq = ctx->stream;
    BPCHK(t.d_moff.ensure(moff.size() * 4)); BPCHK(t.d_ment.ensure(std::max<size_t>(ment.size(), 1) * 4)); BPCHK(t.d_mc.ensure(std::max<size_t>(mc.size(), 1) * 4));
    HIPCHK(hipMemcpyAsync(t.d_moff.p, moff.data(), moff.size() * 4, hipMemcpyHostToDevice, stq));
    if (!ment.empty()) {
        HIPCHK(hipMemcpyAsync(t.d_ment.p, ment.data(), ment.size() * 4, hipMemcpyHostToDevice, stq));
        HIPCHK(hipMemcpyAsync(t.d_mc.p, mc.data(), mc.size() * 4, hipMemcpyHostToDevice, stq));
    }
    t.dev.m_off = (const u32*)t.d_moff.p; t.dev.m_ent = (const u32*)t.d_ment.p; t.dev.m_c = (const u32*)t.d_mc.p;
    BPCHK(t.d_coefs.ensure(std::max<size_t>(t.ncoef, 1) * 32));
    BPCHK(upload_scalars<C>(ctx, (u32*)t.d_coefs.p, t.coefs_host.data(), t.ncoef));
    BPCHK(t.d_cq.ensure(std::max<size_t>(cq.size(), 1) * 4)); BPCHK(t.d_cc.ensure(std::max<size_t>(cc.size(), 1) * 4));
    if (!cq.empty()) {
        HIPCHK(hipMemcpyAsync(t.d_cq.p, cq.data(), cq.size() * 4, hipMemcpyHostToDevice, stq));
        HIPCHK(hipMemcpyAsync(t.d_cc.p, cc.data(), cc.size() * 4, hipMemcpyHostToDevice, stq));
    }
    t.dev.const_q = (const u32*)t.d_cq.p; t.dev.const_c = (const u32*)t.d_cc.p; t.dev.n_const = (u32)cq.size();
    HIPCHK(hipStreamSynchronize(stq));   // the host arrays above are locals
    t.dev.coefs = (const u32*)t.d_coefs.p;
    return BP_OK;
}

// ---- the ctx's template cache (bp_ctx::templates: structure digest -> VTemplate<C>) ------------------------------------------------
// circuit templates kept per ctx.  A soft bound: a caller that finds the cache full trims it to what it is about to use (vfy_templates_trim)
static constexpr size_t VFY_TEMPLATE_CACHE = 64;
static std::string vfy_template_key(const host::Digest& dg) { return std::string((const char*)&dg, sizeof dg); }
// The eviction: every entry whose key is not in `used` leaves.  Launches enqueued earlier may still read an evicted template's device
// arrays, hence the wait; a front-end class names its template by digest and a rebuilt one may hold other constants, so they go too.
static int vfy_templates_trim(bp_ctx* ctx, const std::set<std::string>& used) {
    HIPCHK(ctx_stream_wait(ctx));
    for (auto it = ctx->templates.begin(); it != ctx->templates.end();) { if (used.count(it->first)) ++it; else it = ctx->templates.erase(it); }
    ctx->vfe_classes.clear();
    return BP_OK;
}
// The template of structure `dg`: cached, or built from `rec` (upload + sync, once per gadget; null: the caller's recording is gone).
// A template found under the digest must match the caller's (n, n1, q, ncoef).  `keep` shares ownership past an eviction.
template <class C>
static int vfy_template_get(bp_ctx* ctx, const host::Digest& dg, const host::ConstraintSystem<C>* rec, size_t n, size_t n1, size_t q, size_t ncoef, const char* who,
                            std::shared_ptr<void>& keep, const VTemplate<C>*& tmpl) {
    const std::string key = vfy_template_key(dg);
    auto it = ctx->templates.find(key);
    if (it == ctx->templates.end()) {
        if (!rec) { g_err = std::string(who) + ": recording released before its template was built"; return BP_E_ARG; }
        VTemplate<C>* t = new VTemplate<C>();
        std::shared_ptr<void> holder(t, [](void* p) { delete (VTemplate<C>*)p; });
        BPCHK(build_template<C>(ctx, *rec, *t));
        it = ctx->templates.emplace(key, holder).first;
    }
    keep = it->second;
    tmpl = (const VTemplate<C>*)keep.get();
    if (tmpl->n != n || tmpl->n1 != n1 || tmpl->q != q || tmpl->ncoef != ncoef) { g_err = std::string(who) + ": structure digest collision"; return BP_E_ARG; }
    return BP_OK;
}
// an instance ships a coefficient table of its own when its values are not the ones the template's creator had
template <class C> static bool vfy_own_table(const VTemplate<C>& t, const VerifyPrep<C>& vp) { return t.ncoef && memcmp(t.coefs_host.data(), vp.coef_ptr, t.ncoef * 32) != 0; }

// Everything of verification_scalars (verifier.rs:394-541) that is not of length N.  cs: the recorded verifier (phase 1 done, its
// transcript positioned after the recording); the randomized phase runs in here (:441), so cs is consumed like `verify(self)`.
// The Fiat-Shamir side of the replay behind a small interface: LiveTr drives the instance's own merlin transcript; PrecompTr hands out
// challenges that were computed beforehand — by replay_challenges_x8, which runs the transcripts of EIGHT same-shaped proofs in
// lockstep (AVX-512 Keccak-f x8).  That is possible because nothing a single-phase verifier appends depends on a challenge: the
// messages are the statement's and the proof's points and scalars, the challenges are outputs only.
template <class C> struct LiveTr {
    typedef host::TP<C> TP;
    host::Transcript& tr;
    void append_u64(const char* l, uint64_t x) { tr.append_u64(l, x); }
    bool vpoint(const char* l, const A4& p) { return TP::validate_and_append_point(tr, l, p); }
    void point(const char* l, const A4& p) { TP::append_point(tr, l, p); }
    void scalar(const char* l, const F4& x) { TP::append_scalar(tr, l, x); }
    F4 chal(const char* l) { return TP::challenge_scalar(tr, l); }
    void ipp(uint64_t n) { TP::innerproduct_domain_sep(tr, n); }
    F4 chal_r() { host::Transcript clone = tr; return TP::challenge_scalar(clone, "r"); }
    bool inverse(F4&) { return false; }
};
struct PrecompTr {
    const F4* ch;       // y, z, u, x, w, u_1 .. u_k, r
    const F4* inv_acc_y = nullptr;   // 1 / (y * product of the non-zero u_i) (1 / product when y = 0): with every challenge known beforehand the
                                     // proof's one field inversion can be shared with the other proofs of its group (Montgomery's trick)
    size_t at = 0;
    bool inverse(F4& out) { if (!inv_acc_y) return false; out = *inv_acc_y; return true; }
    void append_u64(const char*, uint64_t) {}
    bool vpoint(const char*, const A4& p) { return !p.is_inf(); }
    void point(const char*, const A4&) {}
    void scalar(const char*, const F4&) {}
    F4 chal(const char*) { return ch[at++]; }
    void ipp(uint64_t) {}
    F4 chal_r() { return ch[at++]; }
};
template <class C, class TR> static int verify_prepare_t(host::ConstraintSystem<C>& cs, const host::ProofData& pf, size_t gens_cap, VerifyPrep<C>& vp, TR& T) {
    typedef host::Fld<typename C::Fr> S;
    const std::vector<A4>& V = cs.V;
    T.append_u64("m", V.size());
    vp.m = V.size();
    if (!T.vpoint("A_I1", pf.A_I1) || !T.vpoint("A_O1", pf.A_O1) || !T.vpoint("S1", pf.S1)) return BP_E_VERIFICATION;
    { int rc = cs.run_randomized(); if (rc) return rc; }
    const size_t n = cs.num_vars, N = host::next_pow2(n);
    vp.n1 = cs.n1; vp.n = n; vp.N = N; vp.nq = cs.num_constraints();
    if (gens_cap < N) return BP_E_GENS_LENGTH;
    T.point("A_I2", pf.A_I2); T.point("A_O2", pf.A_O2); T.point("S2", pf.S2);
    const F4 y = T.chal("y"), z = T.chal("z");
    if (!T.vpoint("T_1", pf.T_1) || !T.vpoint("T_3", pf.T_3) || !T.vpoint("T_4", pf.T_4) || !T.vpoint("T_5", pf.T_5) || !T.vpoint("T_6", pf.T_6))
        return BP_E_VERIFICATION;
    const F4 u = T.chal("u"), x = T.chal("x");
    T.scalar("t_x", pf.t_x); T.scalar("t_x_blinding", pf.t_x_blinding); T.scalar("e_blinding", pf.e_blinding);
    const F4 w = T.chal("w");
    { F4 c = z; for (int j = 0; j < 32; j++) { vp.ztab[j] = c; c = S::sqr(c); } }
    // flattened constraints (verifier.rs:304-349): W_L, W_R, W_O and the constant terms (wc) are evaluated on the GPU from z and
    // the instance's coefficient table; here only the few terms on committed variables (wV), with wc taken as 0 (its weighted
    // value arrives with the delta sum)
    std::vector<host::VTerm> own_vt;
    const host::CanonState& cst = cs.canonical(vp.canon_own, &own_vt);
    vp.digest = cst.digest(vp.n1, n, vp.nq);
    vp.coef_ptr = cst.coefs.data(); vp.ncoef = cst.coefs.size();
    std::vector<F4> wV(vp.m, S::zero());
    bool missing_commitment = false;
    {
        // terms in constraint order: z^(q+1) is carried from term to term; gadgets lay their constraints out regularly, so the
        // step z^(dq) is usually the one just used
        F4 zq = S::one(), zstep = S::one();
        u32 cur = 0, last_d = 0;
        const F4 one = S::one();
        auto pow_z = [&](u32 e) { F4 r = S::one(); for (u32 j = 0; e; e >>= 1, j++) if (e & 1) r = S::mul(r, vp.ztab[j]); return r; };
        auto feed = [&](const host::VTerm& tm) {
            const u32 q1 = tm.q + 1;
            if (cur == 0) zq = pow_z(q1);
            else if (q1 != cur) {
                const u32 d = q1 - cur;
                if (d != last_d) { zstep = pow_z(d); last_d = d; }
                zq = S::mul(zq, zstep);
            }
            cur = q1;
            if (tm.j >= vp.m) { missing_commitment = true; return; }
            wV[tm.j] = S::sub(wV[tm.j], tm.c == one ? zq : S::mul(zq, tm.c));
        };
        if (cs.base) for (const auto& tm : cs.base->vterms) feed(tm);
        for (const auto& tm : own_vt) feed(tm);
    }
    // a like-instance (bp_verifier_new_like) shares its source's constraints: it must have replayed every commitment they name,
    // or a weaker statement than the recorded one would be checked
    if (missing_commitment) {   // (this runs on a pool thread in batches: g_err is thread_local, so the message travels in vp and the caller's thread publishes it)
        vp.err = "verify: the constraints refer to more commitments than this verifier holds (bp_verifier_commit)";
        g_err = vp.err;
        return BP_E_ARG;
    }
    // InnerProductProof::verification_scalars (src/inner_product_proof.rs:244-314) minus the s vector
    const size_t k = pf.L_vec.size();
    if (k >= 32 || pf.R_vec.size() != k || N != ((size_t)1 << k)) return BP_E_VERIFICATION;
    vp.k = k;
    T.ipp(N);
    std::vector<F4> ch(k);
    for (size_t i = 0; i < k; i++) {
        if (!T.vpoint("L", pf.L_vec[i]) || !T.vpoint("R", pf.R_vec[i])) return BP_E_VERIFICATION;
        ch[i] = T.chal("u");
    }
    // batch_inversion leaves zeros untouched; allinv multiplies the non-zero inverses (:281-288).  Montgomery's trick.
    std::vector<F4> chi(k), pref(k);
    F4 allinv = S::one();
    F4 y_inv;
    {
        F4 acc = S::one();
        for (size_t i = 0; i < k; i++) { pref[i] = acc; if (!ch[i].is_zero()) acc = S::mul(acc, ch[i]); }
        // one field inversion serves both the challenges and y (Montgomery's trick once more): 1 / (acc * y)
        F4 inv, given;
        const bool have = T.inverse(given);
        if (y.is_zero()) { inv = have ? given : S::inv(acc); y_inv = y; }   // Fr::inverse of 0 is None upstream (verifier.rs:473 unwraps): keep 0 -> 0 as before
        else { const F4 both = have ? given : S::inv(S::mul(acc, y)); inv = S::mul(both, y); y_inv = S::mul(both, acc); }
        allinv = inv;
        for (size_t i = k; i-- > 0;) {
            if (ch[i].is_zero()) { chi[i] = ch[i]; continue; }
            chi[i] = S::mul(inv, pref[i]);
            inv = S::mul(inv, ch[i]);
        }
    }
    vp.u_sq.resize(k);
    std::vector<F4> u_inv_sq(k);
    for (size_t i = 0; i < k; i++) { vp.u_sq[i] = S::sqr(ch[i]); u_inv_sq[i] = S::sqr(chi[i]); }
    vp.allinv = allinv; vp.x = x; vp.u = u; vp.a = pf.a; vp.b = pf.b;
    { F4 c = y, ci = y_inv; for (int j = 0; j < 32; j++) { vp.ypw[j] = c; vp.ypw[32 + j] = ci; c = S::sqr(c); ci = S::sqr(ci); } }
    const F4 r = T.chal_r();
    const F4 xx = S::mul(x, x), rxx = S::mul(r, xx), xxx = S::mul(x, xx);
    vp.coefD = rxx;
    vp.rx = S::mul(r, x);
    // B: w*(t_x - a*b) + r*(x^2*(wc + delta) - t_x), delta = <y^-i * wR[i], wL[i]> (:477-484, :529); wc + delta comes from the GPU
    vp.sB = S::sub(S::mul(w, S::sub(pf.t_x, S::mul(pf.a, pf.b))), S::mul(r, pf.t_x));
    vp.sBb = S::sub(S::neg(pf.e_blinding), S::mul(r, pf.t_x_blinding));
    auto& ts = vp.tail_scalars; auto& tp = vp.tail_points;
    ts = {x, xx, xxx, S::mul(u, x), S::mul(u, xx), S::mul(u, xxx)};
    tp = {pf.A_I1, pf.A_O1, pf.S1, pf.A_I2, pf.A_O2, pf.S2};
    for (size_t j = 0; j < vp.m; j++) { ts.push_back(S::mul(wV[j], rxx)); tp.push_back(V[j]); }
    const F4 Tsc[5] = {S::mul(r, x), S::mul(rxx, x), S::mul(rxx, xx), S::mul(rxx, xxx), S::mul(S::mul(rxx, xx), xx)};
    const A4 Tpt[5] = {pf.T_1, pf.T_3, pf.T_4, pf.T_5, pf.T_6};
    for (int j = 0; j < 5; j++) { ts.push_back(Tsc[j]); tp.push_back(Tpt[j]); }
    for (size_t j = 0; j < k; j++) { ts.push_back(vp.u_sq[j]); tp.push_back(pf.L_vec[j]); }
    for (size_t j = 0; j < k; j++) { ts.push_back(u_inv_sq[j]); tp.push_back(pf.R_vec[j]); }
    return BP_OK;
}
template <class C> static int verify_prepare(host::ConstraintSystem<C>& cs, const host::ProofData& pf, size_t gens_cap, VerifyPrep<C>& vp) {
    LiveTr<C> T{*cs.tr};
    return verify_prepare_t<C>(cs, pf, gens_cap, vp, T);
}
#if defined(__x86_64__)
// The challenges of eight single-phase verifications whose transcripts stand at the same position (after their commitments), all
// with the same number of commitments and of inner-product rounds: out[j] = y, z, u, x, w, u_1 .. u_k, r of lane j.  false when the
// eight do not qualify (the caller replays them one by one).  The schedule is verify_prepare_t's, message for message.
template <class C> __attribute__((target("avx512f")))
static bool replay_challenges_x8(host::ConstraintSystem<C>* const cs[8], const host::ProofData* const pf[8], std::vector<F4> (&out)[8]) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    typedef host::Grp<C> G;
    const size_t k = pf[0]->L_vec.size(), m = cs[0]->V.size();
    if (k >= 32) return false;
    const host::Strobe* in[8];
    for (int j = 0; j < 8; j++) {
        if (!cs[j]->deferred.empty() || cs[j]->V.size() != m || pf[j]->L_vec.size() != k || pf[j]->R_vec.size() != k || !cs[j]->tr) return false;
        in[j] = &cs[j]->tr->s;
    }
    host::StrobeX8 sx;
    if (!sx.gather(in)) return false;
    uint8_t buf[8][72];
    uint8_t* wp[8]; const uint8_t* rp[8];
    for (int j = 0; j < 8; j++) { wp[j] = buf[j]; rp[j] = buf[j]; }
    auto pts = [&](const char* label, auto get) { for (int j = 0; j < 8; j++) G::ser_uncompressed(buf[j], get(j)); sx.append_message_each(label, rp, 65); };
    auto scal = [&](const char* label, auto get) { for (int j = 0; j < 8; j++) S::to_bytes(buf[j], get(j)); sx.append_message_each(label, rp, 32); };
    auto chal_on = [&](host::StrobeX8& st, const char* label) {
        st.challenge_bytes_each(label, wp, 32);
        for (int j = 0; j < 8; j++) { host::ChaChaRng prng(buf[j]); out[j].push_back(host::rand_fe<FrP>(prng)); }
    };
    for (int j = 0; j < 8; j++) { out[j].clear(); out[j].reserve(6 + k); }
    { const uint64_t mm = m; sx.append_message_same("m", (const uint8_t*)&mm, 8); }
    pts("A_I1", [&](int j) { return pf[j]->A_I1; }); pts("A_O1", [&](int j) { return pf[j]->A_O1; }); pts("S1", [&](int j) { return pf[j]->S1; });
    sx.append_message_same("dom-sep", (const uint8_t*)"r1cs-1phase", 11);
    pts("A_I2", [&](int j) { return pf[j]->A_I2; }); pts("A_O2", [&](int j) { return pf[j]->A_O2; }); pts("S2", [&](int j) { return pf[j]->S2; });
    chal_on(sx, "y"); chal_on(sx, "z");
    pts("T_1", [&](int j) { return pf[j]->T_1; }); pts("T_3", [&](int j) { return pf[j]->T_3; }); pts("T_4", [&](int j) { return pf[j]->T_4; });
    pts("T_5", [&](int j) { return pf[j]->T_5; }); pts("T_6", [&](int j) { return pf[j]->T_6; });
    chal_on(sx, "u"); chal_on(sx, "x");
    scal("t_x", [&](int j) { return pf[j]->t_x; }); scal("t_x_blinding", [&](int j) { return pf[j]->t_x_blinding; }); scal("e_blinding", [&](int j) { return pf[j]->e_blinding; });
    chal_on(sx, "w");
    sx.append_message_same("dom-sep", (const uint8_t*)"ipp v1", 6);
    { for (int j = 0; j < 8; j++) { const uint64_t nn = host::next_pow2(cs[j]->num_vars); memcpy(buf[j], &nn, 8); } sx.append_message_each("n", rp, 8); }
    for (size_t i = 0; i < k; i++) {
        pts("L", [&](int j) { return pf[j]->L_vec[i]; }); pts("R", [&](int j) { return pf[j]->R_vec[i]; });
        chal_on(sx, "u");
    }
    host::StrobeX8 clone = sx;
    chal_on(clone, "r");
    return true;
}
#endif

// uploads a caller's flattened vectors / constants and launches the g/h kernel: canonical g/h into (g_out, h_out)
template <class C> static int verify_launch_gh(bp_ctx* ctx, const VerifyPrep<C>& vp, u32* g_out, u32* h_out) {
    typedef host::Fld<typename C::Fr> S;
    hipStream_t st = ctx->stream;
    const size_t n = vp.n, N = vp.N;
    BPCHK(ctx->r_wL.ensure(N * 32)); BPCHK(ctx->r_wR.ensure(N * 32)); BPCHK(ctx->r_wO.ensure(N * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->r_wL.as<u32>(), vp.wL.data(), n));
    BPCHK(upload_scalars<C>(ctx, ctx->r_wR.as<u32>(), vp.wR.data(), n));
    BPCHK(upload_scalars<C>(ctx, ctx->r_wO.as<u32>(), vp.wO.data(), n));
    BPCHK(ctx->r_ypow.ensure(64 * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->r_ypow.as<u32>(), vp.ypw, 64));
    std::vector<F4> cst = {vp.allinv, vp.x, vp.a, vp.b, vp.u, S::one()};
    cst.insert(cst.end(), vp.u_sq.begin(), vp.u_sq.end());
    BPCHK(ctx->r_chal.ensure(cst.size() * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->r_chal.as<u32>(), cst.data(), cst.size()));
    const u32* consts = ctx->r_chal.as<u32>();
    const u32* chal = consts + 6 * 8;
    ScopedK tk(ctx, BP_K_VFY_SCALARS);
    hipLaunchKernelGGL((k_vfy_scalars<C, false>), dim3((u32)((N + 255) / 256)), dim3(256), 0, st, ctx->r_wL.as<u32>(), ctx->r_wR.as<u32>(), ctx->r_wO.as<u32>(),
                       ctx->r_ypow.as<u32>(), chal, consts, (u32)n, (u32)vp.n1, (u32)N, (u32)vp.k, g_out, h_out);
    tk.stop();
    HIPCHK(hipGetLastError());
    HIPCHK(ctx_stream_wait(ctx));   // the staging buffers are reused by the next call
    return BP_OK;
}

// The O(N) part of Verifier::verification_scalars for a caller that keeps its own constraint system (src/r1cs/verifier.rs:465-514
// with inner_product_proof.rs:279-311): g_scalars / h_scalars from the flattened vectors and the challenges.
template <class C>
static int verification_gh_host_entry(bp_ctx* ctx, size_t n, size_t n1, const uint64_t* wL, const uint64_t* wR, const uint64_t* wO, const uint64_t* y,
                                      const uint64_t* x, const uint64_t* u, const uint64_t* a, const uint64_t* b, const uint64_t* ch, size_t k,
                                      uint64_t* g_out, uint64_t* h_out) {
    typedef host::Fld<typename C::Fr> S;
    const size_t N = (size_t)1 << k;
    VerifyPrep<C> vp;
    vp.n = n; vp.n1 = n1; vp.N = N; vp.k = k;
    vp.wL.resize(n); vp.wR.resize(n); vp.wO.resize(n);
    if (n) { memcpy(vp.wL.data(), wL, n * 32); memcpy(vp.wR.data(), wR, n * 32); memcpy(vp.wO.data(), wO, n * 32); }
    memcpy(vp.x.v, x, 32); memcpy(vp.u.v, u, 32); memcpy(vp.a.v, a, 32); memcpy(vp.b.v, b, 32);
    F4 yy; memcpy(yy.v, y, 32);
    // batch_inversion semantics of the reference: zero challenges stay zero and are skipped by allinv (:281-288)
    F4 acc = S::one();
    vp.u_sq.resize(k);
    for (size_t i = 0; i < k; i++) { F4 c; memcpy(c.v, ch + 4 * i, 32); vp.u_sq[i] = S::sqr(c); if (!c.is_zero()) acc = S::mul(acc, c); }
    vp.allinv = S::inv(acc);
    const F4 y_inv = S::inv(yy);
    { F4 c = yy, ci = y_inv; for (int j = 0; j < 32; j++) { vp.ypw[j] = c; vp.ypw[32 + j] = ci; c = S::sqr(c); ci = S::sqr(ci); } }
    BPCHK(ctx->r_g.ensure(2 * N * 32));
    u32* dg = ctx->r_g.as<u32>();
    u32* dh = dg + N * 8;
    BPCHK(verify_launch_gh<C>(ctx, vp, dg, dh));   // canonical integers, synchronised
    HIPCHK(hipMemcpyAsync(g_out, dg, N * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h_out, dh, N * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx_stream_wait(ctx));
    return BP_OK;
}

// All proofs of one template in one launch: d_params = the block's parameter blocks (resident form), d_perm = the group's proofs
// as positions in it, d_coef_tabs = per-proof coefficient tables (nullptr: the template's own), k_vfy_batch, fold of the chunk
// partials into the shared accumulators acc_g / acc_h (resident form); the alpha-weighted (wc + delta) sum of the group lands in
// delta_slot (ark words, device).  Nothing here waits for the GPU.
template <class C>
static int verify_launch_template_group(bp_ctx* ctx, const VTemplate<C>& t, const u32* d_params, const u32* d_perm, const u32* d_coef_tabs, size_t P, size_t N,
                                        size_t k, u32* acc_g, u32* acc_h, u32* delta_slot, bool shared_coef_tab = false /* one table for the whole group (stride 0) */) {
    hipStream_t st = ctx->stream;
    const u32 nblk = (u32)((N + 255) / 256);
    static const size_t wgs_env = getenv("ARKBP_VFY_WGS") ? (size_t)atoi(getenv("ARKBP_VFY_WGS")) : 0;   // experiments
    const size_t wgs = wgs_env >= 256 ? wgs_env : 4096;
    u32 nchunks = (u32)std::min<size_t>(P, std::max<size_t>(1, wgs / nblk));   // enough workgroups to fill 256 CUs
    const u32 per_chunk = (u32)((P + nchunks - 1) / nchunks);
    nchunks = (u32)((P + per_chunk - 1) / per_chunk);
    BPCHK(ctx->v_gpart.ensure((size_t)nchunks * N * 32)); BPCHK(ctx->v_hpart.ensure((size_t)nchunks * N * 32));
    BPCHK(ctx->r_part.ensure((size_t)nchunks * nblk * 32));
    const u32 LOB = (u32)((k + 1) / 2), nlo = 1u << LOB, nhi = 1u << (k - LOB);
    const u32 nzhi = (u32)((t.q + 1) >> 8) + 1;   // exponents q + 1 <= t.q
    BPCHK(ctx->v_tables.ensure(P * vfy_tab_stride(nlo, nhi, nzhi) * VT_W * 4));
    {
        ScopedK tk(ctx, BP_K_VFY_TABLES);
        hipLaunchKernelGGL(k_vfy_tables<C>, dim3((std::max(std::max(nlo, nhi), std::max(256u, nzhi)) + 255) / 256, (u32)P), dim3(256), 0, st, d_params, d_perm,
                           (u32)P, (u32)k, LOB, nzhi, ctx->v_tables.as<u32>());
    }
    {
        ScopedK tk(ctx, BP_K_VFY_SCALARS);
        hipLaunchKernelGGL(k_vfy_batch<C>, dim3(nblk, nchunks), dim3(256), 0, st, t.dev, d_params, d_perm, d_coef_tabs, shared_coef_tab ? 0u : (u32)(t.ncoef * 8), (u32)P, per_chunk, (u32)t.n,
                           (u32)t.n1, (u32)N, (u32)k, ctx->v_gpart.as<u32>(), ctx->v_hpart.as<u32>(), ctx->r_part.as<u32>(), ctx->v_tables.as<u32>(), LOB, nzhi);
    }
    hipLaunchKernelGGL(k_vfy_batch_fold<C>, dim3(nblk), dim3(256), 0, st, ctx->v_gpart.as<u32>(), ctx->v_hpart.as<u32>(), nchunks, (u32)N, acc_g, acc_h);
    hipLaunchKernelGGL(k_r1cs_sum<C>, dim3(1), dim3(256), 0, st, ctx->r_part.as<u32>(), nchunks * nblk, 1u, delta_slot);
    HIPCHK(hipGetLastError());
    return BP_OK;
}

template <class F> static void canon_words(uint64_t out[4], const F4& x) { host::Fld<F>::to_canon(out, x); }

// decompresses `n` SW points on the GPU: xs = Montgomery words of x (ark layout), flags = ark-serialize flag bytes
template <class C> static int decompress_points(bp_ctx* ctx, const F4* xs, const u32* flags, size_t n, std::vector<A4>& out, std::vector<u32>& ok) {
    out.resize(n); ok.resize(n);
    if (!n) return BP_OK;
    hipStream_t st = ctx->stream;
    BPCHK(ctx->io_pts.ensure(n * 32)); BPCHK(ctx->io_scal.ensure(n * 4)); BPCHK(ctx->io_out.ensure(n * 64 + n * 4));
    HIPCHK(hipMemcpyAsync(ctx->io_pts.p, xs, n * 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->io_scal.p, flags, n * 4, hipMemcpyHostToDevice, st));
    u32* d_xy = ctx->io_out.as<u32>();
    u32* d_ok = d_xy + n * 16;
    hipLaunchKernelGGL(k_points_decompress<C>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, ctx->io_pts.as<u32>(), ctx->io_scal.as<u32>(), d_xy, d_ok, (u32)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out.data(), d_xy, n * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ok.data(), d_ok, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    return BP_OK;
}

// pinned staging memory of the batch-verify pipeline (two alternating halves, an event each)
static int vfy_stage_ensure(bp_ctx* ctx, int which, size_t bytes) {
    if (ctx->h_vstage_cap[which] >= bytes) return BP_OK;
    BPCHK(pinned_ensure(ctx->h_vstage[which], ctx->h_vstage_cap[which], bytes, bytes / 4 + 4096));
    if (!ctx->vstage_ev[which]) HIPCHK(hipEventCreateWithFlags(&ctx->vstage_ev[which], hipEventDisableTiming));
    return BP_OK;
}
// second pinned buffer per half: the block's launch order and the coefficient tables of instances that carry their own values
// (sized after the replay, when the staging half already holds the block's parameter blocks and tails)
static int vfy_aux_ensure(bp_ctx* ctx, int which, size_t bytes) {
    return pinned_ensure(ctx->h_vaux[which], ctx->h_vaux_cap[which], bytes, bytes / 4 + 4096);
}

// One (Verifier, &R1CSProof) pair of batch_verify (verifier.rs:604-612) as the core sees it: a recorded verifier whose transcript
// stands right after the recording.  `owned_*` keep objects alive that the provider created for this call.
template <class C> struct VfyInstance {
    host::ConstraintSystem<C>* cs = nullptr;
    bool released = false;   // the replay worker dropped an owned recording (its template was cached): cs is null from then on
    std::unique_ptr<host::ConstraintSystem<C>> owned_cs;
    std::unique_ptr<host::Transcript> owned_tr;
};
// A batch whose instances all replay ONE shared single-phase recording (bp_verifier_new_like / the scenario sources): what the device
// front end needs instead of per-instance recorders.  The transcripts stand either before the commitments (one shared state; the
// device appends the m "V" messages of Verifier::commit, verifier.rs:279-287) or right after them (recorded handles).
template <class C> struct VfyDevBatch {
    const host::ConstraintSystem<C>* src = nullptr;          // frozen phase-1 recording, nothing recorded on top, randomized phase not run yet
    size_t m = 0;                                            // commitments per instance
    bool absorb_commitments = false;
    bool shared_state = false;                               // state_of(k) is one object for every k
    std::function<const host::Strobe*(size_t)> state_of;     // the transcript of instance k
    std::function<const uint64_t*(size_t)> commit_xy;        // its m commitments, ark layout (x || y: 8 words per point)
    // or, with absorb_commitments: its m commitments as 33-byte encodings (pending wire commitments, bp_verifier_commit_compressed_batch):
    // k_vfe_points decodes them, they never reach the host in affine form.  Exactly one of commit_xy / commit_wire is set.
    std::function<const uint8_t*(size_t)> commit_wire;
    // two-phase (src->deferred non-empty): the recorder on which instance k's randomized phase runs — needed when its callbacks
    // record through a handle (bp_cs); absent: a like-instance of src made for the purpose (the closures record into the recorder
    // they receive)
    std::function<host::ConstraintSystem<C>*(size_t)> cs_of;
    std::shared_ptr<void> keep;                              // whatever the accessors refer to that has no other owner (an index map)
};
// What makes instance k a like-instance of others, as far as its provider knows: the shared recording (cs->base for handles, the
// scenario source), the commitment count and form, the transcript position.  The core adds the proof length (vfy_class_plan's keys).
struct VfyClassId { const void* rec = nullptr; size_t m = 0; bool wire = false, two = false; unsigned pos = 0, pos_begin = 0; };
template <class C> struct VfyProvider {
    std::function<size_t(size_t)> m_of;                          // number of commitments of instance k (cheap; sizes the tails)
    std::function<int(size_t, VfyInstance<C>&)> get;            // the recorded verifier of instance k; called from pool threads
    // optional: the transcripts of instances [k0, k0 + cnt), cnt <= 8, up to and including their commitments, built in lockstep
    // (host::StrobeX8); out[j] stays empty for an instance it leaves to get().  get() continues from a transcript it is handed.
    std::function<void(size_t, size_t, std::unique_ptr<host::Transcript>*)> head8;
    // optional: the whole batch as like-instances of ONE single-phase recording (the device front end, batch_verify_device)
    std::function<bool(VfyDevBatch<C>&)> dev_batch;
    // optional, both or neither: batches of several gadgets (batch_verify_classes).  class_id(k, id): false for an instance without a
    // shared recording.  dev_class(idx, n, db): instances idx[0 .. n), which have equal ids, as a VfyDevBatch whose accessors take
    // j < n; idx outlives db.
    std::function<bool(size_t, VfyClassId&)> class_id;
    std::function<bool(const uint32_t*, size_t, VfyDevBatch<C>&)> dev_class;
    // optional: instances may still hold their commitments as wire bytes.  Called once, when the device front end did not take the
    // batch and before anything else looks at the instances: decodes and commits them (Verifier::commit).  st: one status per
    // instance, BP_E_FORMAT for an instance with a rejected encoding (it received none); the return value is an error of the call.
    // idx / n: for instances idx[0 .. n) only (the remainder of a call whose device classes keep their bytes pending), st[j] for
    // idx[j]; idx null: every instance.
    std::function<int(const uint32_t*, size_t, int*)> prologue;
};
// The provider whose instance j is instance idx[j] of `full`, which must outlive it (as must idx).  Without head8 — the lockstep heads
// need consecutive instances — and without the prologue: the pending commitments are the whole call's business.
template <class C> static void provider_subset(const VfyProvider<C>& full, const uint32_t* idx, VfyProvider<C>& prov) {
    prov.m_of = [&full, idx](size_t j) { return full.m_of(idx[j]); };
    prov.get = [&full, idx](size_t j, VfyInstance<C>& out) -> int { return full.get(idx[j], out); };
    if (full.dev_batch) prov.dev_batch = [&full, idx](VfyDevBatch<C>& db) -> bool {
        VfyDevBatch<C> all;
        if (!full.dev_batch(all)) return false;   // like-instances of one recording as a whole, so every subset of them is
        db = all;
        db.state_of = [s = all.state_of, idx](size_t j) { return s(idx[j]); };
        if (all.commit_xy) db.commit_xy = [x = all.commit_xy, idx](size_t j) { return x(idx[j]); };
        if (all.commit_wire) db.commit_wire = [w = all.commit_wire, idx](size_t j) { return w(idx[j]); };
        if (all.cs_of) db.cs_of = [f = all.cs_of, idx](size_t j) { return f(idx[j]); };
        return true;
    };
    if (full.class_id && full.dev_class) {
        prov.class_id = [&full, idx](size_t j, VfyClassId& id) { return full.class_id(idx[j], id); };
        prov.dev_class = [&full, idx](const uint32_t* sub, size_t n, VfyDevBatch<C>& db) -> bool {
            auto map = std::make_shared<std::vector<uint32_t>>(n);
            for (size_t j = 0; j < n; j++) (*map)[j] = idx[sub[j]];
            if (!full.dev_class(map->data(), n, db)) return false;
            db.keep = map;
            return true;
        };
    }
}
// ... and with the prologue, for the members of a call that the host replays while the others stay on the device
template <class C> static void provider_subset_with_prologue(const VfyProvider<C>& full, const uint32_t* idx, size_t n, VfyProvider<C>& prov) {
    provider_subset<C>(full, idx, prov);
    if (full.prologue) prov.prologue = [&full, idx, n](const uint32_t* sub, size_t cnt, int* st) -> int {
        if (!sub) return full.prologue(idx, n, st);
        std::vector<uint32_t> map(cnt);
        for (size_t j = 0; j < cnt; j++) map[j] = idx[sub[j]];
        return full.prologue(map.data(), cnt, st);
    };
}

// ---- batch_verify with the per-proof front end on the GPU: the steps over VfyDevJob, vfy_dev_run, batch_verify_device
#include "verify_dev.inc"

// batch_verify on the host-replay route: batch_verify_host, a short sequence of steps over one VfyHostJob
#include "verify_steps.inc"

// ---- batches of several gadgets --------------------------------------------------------------------------------------------------
// The partition of a batch into device classes: the one place the rule lives (bp_debug_vfy_class_plan is this function).  keys[k]
// names the class of instance k — equal keys: like-instances of one recording with the same commitment count and form, proof length
// and transcript position —, eligible[k] = 0 (eligible may be null: all) an instance that stays on the host whatever its class
// (no shared recording, a two-phase statement).  Classes are ordered by size, largest first, ties by their first member; the first
// max_classes of them with at least class_min eligible members become device classes 0, 1, .. in that (launch) order.  class_of[k]:
// the device class of instance k, or -1 for the remainder.
static constexpr uint64_t VFY_CLASS_MIN_DEFAULT = 65535;   // BP_TUNE_VFY_CLASS_MIN = 0: no class size measured so far beats the host replay of
                                                           // the same members in the latency of one call (profiles/r15_vfy_mixed.txt; include/arkbp.h)
static void vfy_class_plan(size_t count, const uint64_t* keys, const uint8_t* eligible, uint64_t class_min, uint32_t max_classes, int32_t* class_of, uint32_t* nclasses) {
    if (!class_min) class_min = VFY_CLASS_MIN_DEFAULT;
    class_min = std::min<uint64_t>(class_min, 65535);
    if (!max_classes) max_classes = BP_VFY_MAX_CLASSES;
    struct Cls { uint64_t key; size_t first, size; };
    std::vector<Cls> cls;
    std::unordered_map<uint64_t, size_t> at;
    std::vector<size_t> of(count, (size_t)-1);
    for (size_t k = 0; k < count; k++) {
        class_of[k] = -1;
        if (eligible && !eligible[k]) continue;
        auto it = at.find(keys[k]);
        if (it == at.end()) { it = at.emplace(keys[k], cls.size()).first; cls.push_back(Cls{keys[k], k, 0}); }
        cls[it->second].size++;
        of[k] = it->second;
    }
    std::vector<size_t> order(cls.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cls[a].size != cls[b].size ? cls[a].size > cls[b].size : cls[a].first < cls[b].first; });
    std::vector<int32_t> num(cls.size(), -1);
    uint32_t n = 0;
    for (size_t i = 0; i < order.size() && n < max_classes; i++) if (cls[order[i]].size >= class_min) num[order[i]] = (int32_t)n++;
    for (size_t k = 0; k < count; k++) if (of[k] != (size_t)-1) class_of[k] = num[of[k]];
    if (nclasses) *nclasses = n;
}
// The host replay of instances idx[0 .. n) of a call (ascending), as a call of its own: their provider with the prologue, their
// proofs and weights gathered.  st / checked / point as batch_verify_host takes them.
template <class C>
static int vfy_host_subset(bp_ctx* ctx, const VfyProvider<C>& prov, const uint32_t* idx, size_t n, const uint8_t* proofs, const size_t* poff, const F4* alphas,
                           uint64_t* point_out, int* st, bool* checked) {
    VfyProvider<C> sub;
    provider_subset_with_prologue<C>(prov, idx, n, sub);
    sub.dev_batch = nullptr; sub.class_id = nullptr; sub.dev_class = nullptr;
    std::vector<size_t> spoff(n + 1, 0);
    for (size_t j = 0; j < n; j++) spoff[j + 1] = spoff[j] + (poff[idx[j] + 1] - poff[idx[j]]);
    std::vector<uint8_t> buf(spoff[n] ? spoff[n] : 1);
    std::vector<F4> sal(n);
    for (size_t j = 0; j < n; j++) { memcpy(buf.data() + spoff[j], proofs + poff[idx[j]], spoff[j + 1] - spoff[j]); sal[j] = alphas[idx[j]]; }
    return batch_verify_host<C>(ctx, n, sub, buf.data(), spoff.data(), sal.data(), nullptr, point_out, st, checked);
}
// A call the device cannot accept because its kernels flagged instances: the host replay of THOSE instances (and whatever else the
// caller puts into idx: the remainder of a class call), in instance order, gives the whole call's answer — every instance that fails
// before its check is among them.  done stays false when that replay finds no failing instance (never expected: the device flagged
// what the host accepts); the caller then replays the whole batch.
template <class C>
static int vfy_replay_flagged(bp_ctx* ctx, size_t count, const VfyProvider<C>& prov, const std::vector<uint32_t>& idx, const uint8_t* proofs, const size_t* poff,
                              const F4* alphas, int* inst_status, bool& done) {
    done = false;
    const size_t n = idx.size();
    bool checked = false;
    if (!inst_status) {   // the first error as the reference orders them (every FormatError before any VerificationError)
        const int rc = vfy_host_subset<C>(ctx, prov, idx.data(), n, proofs, poff, alphas, nullptr, nullptr, &checked);
        if (checked || !rc) return BP_OK;
        done = true;
        return rc;
    }
    std::vector<int> st(n, BP_OK);
    const int rc = vfy_host_subset<C>(ctx, prov, idx.data(), n, proofs, poff, alphas, nullptr, st.data(), &checked);
    bool any = false;
    for (size_t j = 0; j < n; j++) any = any || st[j] != BP_OK;
    if (!any) return rc == BP_E_VERIFICATION ? BP_OK : rc;   // (its mega-check says nothing about the call's)
    std::fill(inst_status, inst_status + count, BP_OK);
    for (size_t j = 0; j < n; j++) inst_status[idx[j]] = st[j];
    done = true;
    return rc;
}
// A batch that is not one class of like-instances: the classes vfy_class_plan names run on the device as ONE launch chain with one
// pair of accumulators, one tail array, one wait and one MSM; everything else (the remainder) is one host replay with its own check
// point.  The call's check point is the group sum of the two — by linearity the reference's single MSM (verifier.rs:685).  done
// stays false when no class runs on the device (the caller replays the whole batch, and nothing is counted).
template <class C>
static int batch_verify_classes(bp_ctx* ctx, size_t count, const VfyProvider<C>& prov, const uint8_t* proofs, const size_t* poff, const F4* alphas, double* timing,
                                uint64_t* point_out, int* inst_status, bool& done) {
    done = false;
    if (!vfy_device_on(ctx) || count < 2 || count >= ((size_t)1 << 31)) return BP_OK;
    // keys: the providers' ids and the proof lengths, numbered in order of appearance
    std::vector<uint64_t> keys(count, 0);
    std::vector<uint8_t> elig(count, 0);
    {
        typedef std::tuple<const void*, size_t, size_t, unsigned, unsigned, unsigned> Id;
        std::map<Id, uint64_t> ids;
        Id last{};
        uint64_t last_key = 0;
        for (size_t k = 0; k < count; k++) {
            VfyClassId id;
            if (!prov.class_id(k, id) || !id.rec) continue;
            const Id t{id.rec, id.m, poff[k + 1] - poff[k], (id.wire ? 1u : 0u) | (id.two ? 2u : 0u), id.pos, id.pos_begin};
            if (!last_key || t != last) { last = t; last_key = ids.emplace(t, ids.size() + 1).first->second; }
            keys[k] = last_key;
            elig[k] = id.two ? 0 : 1;   // (two-phase classes stay on the host replay)
        }
    }
    std::vector<int32_t> class_of(count);
    uint32_t ncls = 0;
    vfy_class_plan(count, keys.data(), elig.data(), ctx->tune_vfy_class_min, BP_VFY_MAX_CLASSES, class_of.data(), &ncls);
    if (!ncls) return BP_OK;
    std::vector<std::vector<uint32_t>> members(ncls);
    for (size_t k = 0; k < count; k++) if (class_of[k] >= 0) members[class_of[k]].push_back((uint32_t)k);
    // the classes the device front end admits, in launch order, while their blocks and tails fit the call's one set of buffers
    std::vector<std::unique_ptr<VfyDevJob<C>>> owned;
    std::vector<VfyDevJob<C>*> jobs;
    std::vector<char> on_device(count, 0);
    VfyDevTotals fit;
    for (uint32_t c = 0; c < ncls; c++) {
        std::unique_ptr<VfyDevJob<C>> J(new VfyDevJob<C>());
        J->count = members[c].size(); J->idx = members[c].data();
        if (!prov.dev_class(J->idx, J->count, J->db)) continue;
        bool ok = false;
        BPCHK(vfy_dev_admit<C>(ctx, *J, proofs, poff, ok));
        if (!ok || J->two || !vfy_dev_fits(fit, J->sh)) continue;
        (void)vfy_dev_append(fit, J->sh);
        for (uint32_t k : members[c]) on_device[k] = 1;
        jobs.push_back(J.get());
        owned.push_back(std::move(J));
    }
    if (jobs.empty()) return BP_OK;
    std::vector<uint32_t> rest, sub;
    for (size_t k = 0; k < count; k++) if (!on_device[k]) rest.push_back((uint32_t)k);
    J4 r;
    VfyDevRun ran;
    BPCHK(vfy_dev_run<C>(ctx, jobs.data(), jobs.size(), proofs, poff, alphas, timing, r, &sub, ran));
    if (ran == VFY_RUN_DECLINED) return BP_OK;
    ctx->vcl_calls++;
    ctx->vcl_remainder += rest.size();
    if (ran == VFY_RUN_FLAGGED) {
        ctx->vfe_fallbacks++;
        sub.insert(sub.end(), rest.begin(), rest.end());
        std::sort(sub.begin(), sub.end());
        ctx->vcl_flagged += sub.size();   // (the flagged instances and the remainder are replayed as one subset)
        return vfy_replay_flagged<C>(ctx, count, prov, sub, proofs, poff, alphas, inst_status, done);
    }
    ctx->vcl_classes += jobs.size();
    for (VfyDevJob<C>* J : jobs) { ctx->vcl_instances += J->count; if (J->sh.wire) ctx->cw_front_end += J->count * J->sh.m; }
    done = true;
    if (!rest.empty()) {
        uint64_t pt[8];
        std::vector<int> st(inst_status ? rest.size() : 0);
        bool checked = false;
        const int rc = vfy_host_subset<C>(ctx, prov, rest.data(), rest.size(), proofs, poff, alphas, pt, inst_status ? st.data() : nullptr, &checked);
        if (inst_status) for (size_t j = 0; j < rest.size(); j++) inst_status[rest[j]] = st[j];
        if (!checked || (rc && rc != BP_E_VERIFICATION)) return rc;   // an instance failed before its check (or the call itself did): no verdict of the sum
        A4 p;
        memcpy(p.x.v, pt, 32); memcpy(p.y.v, pt + 4, 32);
        r = host::Grp<C>::madd(r, p);
    }
    if (point_out) aff_out<C>(point_out, host::Grp<C>::to_aff(r));
    return host::Grp<C>::is_inf(r) ? BP_OK : BP_E_VERIFICATION;
}

// The entry of every batch verification.  A batch of like-instances of one recording goes to the device front end as a whole
// (batch_verify_device), a batch of several gadgets class by class (batch_verify_classes); whatever neither takes, and whatever they
// decline, is the host replay's (batch_verify_host).  A call whose only obstacle is a proof the kernels flagged replays just the
// flagged instances.  The answers are the host replay's in every case.
template <class C>
static int batch_verify_core(bp_ctx* ctx, size_t count, const VfyProvider<C>& prov, const uint8_t* proofs, const size_t* poff /* count + 1 */, const F4* alphas,
                             double* timing, uint64_t* point_out, int* inst_status = nullptr) {
    if (point_out) memset(point_out, 0, 64);   // every early exit leaves a defined (identity) check point
    if (inst_status) std::fill(inst_status, inst_status + count, BP_OK);
    host_pool_ensure(ctx, count);
    // same-shaped single-phase batches: codec, transcript replay and challenge arithmetic on the GPU (batch_verify_device).  It
    // declines (handled = false) whenever anything is unusual — then the replay below reports what the reference would.
    if (prov.dev_batch) {
        VfyDevBatch<C> db;
        if (prov.dev_batch(db)) {
            bool handled = false;
            std::vector<uint32_t> flagged;
            const int rc = batch_verify_device<C>(ctx, count, db, proofs, poff, alphas, timing, point_out, handled, &flagged);
            if (handled || rc) return rc;
            if (!flagged.empty()) {
                ctx->vcl_flagged += flagged.size();
                bool done = false;
                const int frc = vfy_replay_flagged<C>(ctx, count, prov, flagged, proofs, poff, alphas, inst_status, done);
                if (done || frc) return frc;
            }
        } else if (prov.class_id && prov.dev_class) {
            bool done = false;
            const int rc = batch_verify_classes<C>(ctx, count, prov, proofs, poff, alphas, timing, point_out, inst_status, done);
            if (done || rc) return rc;
            if (point_out) memset(point_out, 0, 64);
            if (inst_status) std::fill(inst_status, inst_status + count, BP_OK);
        }
    }
    return batch_verify_host<C>(ctx, count, prov, proofs, poff, alphas, timing, point_out, inst_status, nullptr);
}

// what batch_verify_scenarios hands its provider to: batch_verify_core, or another core over the same instances (verify_each.inc)
template <class C> using VfyCoreFn = std::function<int(const VfyProvider<C>&, const size_t* /* poff */, const F4* /* alphas */)>;

// ---- scenario statements as callers of the core --------------------------------------------------------------------------
// statement recording for one instance (Verifier::new + commits + gadget)
template <class C> static int build_verifier_cs(host::ConstraintSystem<C>& cs, host::Transcript& tr, int scenario, const uint64_t* params,
                                                const host::StatementIO& io) {
    cs.tr = &tr; cs.proving = false;
    host::TP<C>::r1cs_domain_sep(tr);  // Verifier::new (verifier.rs:252-263)
    return host::scenario_verifier<C>(cs, scenario, params, io);
}
// One recorded verifier per (scenario, params, publics), frozen and kept in the ctx: the other instances of that statement shape
// share its phase-1 recording (ConstraintSystem::init_like) and replay only their own commitments into a fresh transcript — what
// bp_verifier_new_like offers a caller with its own gadgets.
template <class C> static std::string scenario_key(int scenario, const uint64_t* params, const uint64_t* publics, size_t npub) {
    std::string k((const char*)&scenario, sizeof scenario);
    k.append((const char*)params, 64);
    k.push_back((char)C::ID);
    if (npub) k.append((const char*)publics, npub * 32);
    return k;
}
template <class C> struct ScenarioSource { host::Transcript tr; host::ConstraintSystem<C> cs; size_t m = 0; };
// The transcripts of up to eight consecutive scenario instances, from the label through their commitments, in lockstep: only for
// instances that replay a shared source recording, with the same scenario, the same leading parameter (the shuffle's k enters the
// transcript) and the same number of commitments as the first of the group — the others are left to the provider's get().
#if defined(__x86_64__)
template <class C, class Src, class MakeIo>
__attribute__((target("avx512f"))) static void scenario_heads_x8(size_t k0, size_t cnt, std::unique_ptr<host::Transcript>* out, const int* scenarios, const uint64_t* params,
                                                                  const size_t* ms, const Src& src, const MakeIo& make_io) {
    if (cnt < 2) return;
    host::StatementIO io[8];
    bool use[8];
    size_t expect0 = 0;
    int nuse = 0;
    host::Transcript proto;
    for (size_t j = 0; j < cnt; j++) {
        const size_t k = k0 + j;
        use[j] = false;
        if (!src[k] || src[k]->m != ms[k] || scenarios[k] != scenarios[k0] || params[8 * k] != params[8 * k0] || ms[k] != ms[k0] || ms[k] == 0) continue;
        make_io(k, io[j]);
        host::Transcript tr(host::scenario_label(scenarios[k]));
        host::TP<C>::r1cs_domain_sep(tr);
        size_t expect = 0;
        if (host::scenario_verifier_prefix<C>(tr, scenarios[k], params + 8 * k, io[j], &expect) || expect != io[j].commitments.size()) continue;
        if (nuse == 0) { proto = tr; expect0 = expect; }
        else if (expect != expect0) continue;
        use[j] = true; nuse++;
    }
    if (nuse < 2) return;
    host::StrobeX8 sx;
    sx.broadcast(proto.s);
    uint8_t ser[8][72];
    const uint8_t* ptr[8];
    int lane_of[8], nl = 0;
    for (size_t j = 0; j < cnt; j++) if (use[j]) lane_of[nl++] = (int)j;
    for (int l = 0; l < 8; l++) ptr[l] = ser[l];
    for (int l = nl; l < 8; l++) memset(ser[l], 0, 65);   // idle lanes absorb zeros
    for (size_t v = 0; v < expect0; v++) {
        for (int l = 0; l < nl; l++) host::Grp<C>::ser_uncompressed(ser[l], io[lane_of[l]].commitments[v]);
        sx.append_message_each("V", ptr, 65);
    }
    host::Strobe* outs[8];
    for (int l = 0; l < nl; l++) { out[lane_of[l]].reset(new host::Transcript()); outs[l] = &out[lane_of[l]]->s; }
    sx.scatter(outs, nl);
}
#endif


template <class C>
static int batch_verify_scenarios(bp_ctx* ctx, size_t count, const int* scenarios, const uint64_t* params, const uint8_t* proofs, const size_t* proof_lens,
                                  const uint64_t* commit_xy, const size_t* ms, const uint64_t* publics, const size_t* npubs, const uint8_t* alpha_seed,
                                  double* timing, size_t alpha_skip, uint64_t* point_out, const VfyCoreFn<C>* other_core = nullptr) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    if (point_out) memset(point_out, 0, 64);
    const std::vector<size_t> poff = prefix_offsets(proof_lens, count), coff = prefix_offsets(ms, count), uoff = prefix_offsets(npubs, count);
    auto make_io = [&](size_t k, host::StatementIO& io) {
        io.commitments.resize(ms[k]); io.publics.resize(npubs[k]);
        if (ms[k]) memcpy(io.commitments.data(), commit_xy + 8 * coff[k], ms[k] * 64);
        if (npubs[k]) memcpy(io.publics.data(), publics + 4 * uoff[k], npubs[k] * 32);
    };
    // sources of the distinct statement shapes (one recording each; later calls find them in the ctx) — for shapes that occur more
    // than once in the batch or were seen before; a one-off statement is recorded inside its own replay.  Instances are classed by a
    // 64-bit hash of (scenario, params, publics) computed on the pool; equal hashes are confirmed byte for byte.
    std::vector<std::shared_ptr<ScenarioSource<C>>> src(count);
    {
        host_pool_ensure(ctx, count);
        std::vector<u64> hk(count);
        auto hash_one = [&](size_t k) {
            u64 h = 0xcbf29ce484222325ULL ^ (u64)(u32)scenarios[k] ^ ((u64)npubs[k] << 40);
            auto mix = [&](const u64* w, size_t nw) { for (size_t i = 0; i < nw; i++) { h = (h ^ w[i]) * 0x100000001b3ULL; h ^= h >> 29; } };
            mix(params + 8 * k, 8);
            mix(publics + 4 * uoff[k], 4 * npubs[k]);
            hk[k] = h;
        };
        if (ctx->pool && count >= 256) ctx->pool->run(0, count, hash_one); else for (size_t k = 0; k < count; k++) hash_one(k);
        auto same = [&](size_t a, size_t b) {
            return scenarios[a] == scenarios[b] && npubs[a] == npubs[b] && !memcmp(params + 8 * a, params + 8 * b, 64) &&
                   (!npubs[a] || !memcmp(publics + 4 * uoff[a], publics + 4 * uoff[b], npubs[a] * 32));
        };
        struct Cls { size_t rep, uses; std::shared_ptr<ScenarioSource<C>> s; bool resolved; };
        // (a one-off statement gets a source of its own only where it can be a device class: BP_TUNE_VFY_CLASS_MIN = 1)
        const size_t src_min = count > 1 && ctx->tune_vfy_class_min == 1 && vfy_device_on(ctx) ? 1 : 2;
        std::unordered_map<u64, std::vector<Cls>> classes;   // (a vector per hash: distinct shapes with equal hashes stay apart)
        std::vector<Cls*> cls_of(count, nullptr);
        classes.reserve(64);
        for (size_t k = 0; k < count; k++) {
            auto& v = classes[hk[k]];
            Cls* c = nullptr;
            for (auto& e : v) if (same(e.rep, k)) { c = &e; break; }
            if (!c) { v.reserve(4); v.push_back(Cls{k, 0, nullptr, false}); c = &v.back(); }
            c->uses++;
        }
        for (size_t k = 0; k < count; k++) { for (auto& e : classes[hk[k]]) if (same(e.rep, k)) { cls_of[k] = &e; break; } }
        for (size_t k = 0; k < count; k++) {
            Cls& c = *cls_of[k];
            if (c.resolved) { src[k] = c.s; continue; }
            c.resolved = true;
            const std::string key = scenario_key<C>(scenarios[k], params + 8 * k, publics + 4 * uoff[k], npubs[k]);
            auto it = ctx->scenario_sources.find(key);
            if (it != ctx->scenario_sources.end()) { c.s = std::static_pointer_cast<ScenarioSource<C>>(it->second); src[k] = c.s; continue; }
            if (c.uses < src_min) continue;
            auto s = std::make_shared<ScenarioSource<C>>();
            s->tr = host::Transcript(host::scenario_label(scenarios[k]));
            host::StatementIO io; make_io(k, io);
            const int rc = build_verifier_cs<C>(s->cs, s->tr, scenarios[k], params + 8 * k, io);
            if (rc) continue;   // (a malformed statement fails in its own replay, in instance order)
            s->m = ms[k];
            BPCHK(s->cs.freeze());
            if (ctx->scenario_sources.size() >= 64 || ctx->scenario_source_terms > ((size_t)1 << 26)) { ctx->scenario_sources.clear(); ctx->scenario_source_terms = 0; }   // bounded host memory
            ctx->scenario_sources[key] = s;
            ctx->scenario_source_terms += s->cs.num_terms();
            c.s = s; src[k] = s;
        }
    }
    // alphas: one sequential rng, in instance order (:649)
    std::vector<F4> alphas(count);
    if (alpha_seed) {
        host::ChaChaRng prng(alpha_seed);
        for (size_t i = 0; i < alpha_skip; i++) (void)host::rand_fe<FrP>(prng);  // proof-sharded batches: alphas of the preceding instances
        for (size_t k = 0; k < count; k++) alphas[k] = host::rand_fe<FrP>(prng);
    } else {
        for (size_t k = 0; k < count; k++) alphas[k] = S::one();
    }
    VfyProvider<C> prov;
    prov.m_of = [&](size_t k) { return ms[k]; };
    prov.get = [&](size_t k, VfyInstance<C>& out) -> int {
        host::StatementIO io; make_io(k, io);
        const bool have_head = (bool)out.owned_tr;   // (head8 built the transcript through the commitments)
        if (!have_head) out.owned_tr.reset(new host::Transcript(host::scenario_label(scenarios[k])));
        out.owned_cs.reset(new host::ConstraintSystem<C>());
        out.cs = out.owned_cs.get();
        if (!src[k] || src[k]->m != ms[k]) {   // no usable source (wrong commitment count, ...): record this instance on its own
            return build_verifier_cs<C>(*out.owned_cs, *out.owned_tr, scenarios[k], params + 8 * k, io);
        }
        out.owned_cs->tr = out.owned_tr.get();
        out.owned_cs->init_like(src[k]->cs);
        if (!have_head) {
            host::TP<C>::r1cs_domain_sep(*out.owned_tr);
            const int rc = host::scenario_verifier_transcript<C>(*out.owned_tr, scenarios[k], params + 8 * k, io);
            if (rc) return rc;
        }
        out.owned_cs->V = std::move(io.commitments);
        return BP_OK;
    };
#if defined(__x86_64__)
    if (host::cpu_has_avx512()) {
        prov.head8 = [&](size_t k0, size_t cnt, std::unique_ptr<host::Transcript>* out) { scenario_heads_x8<C>(k0, cnt, out, scenarios, params, ms, src, make_io); };
    }
#endif
    // one statement shape for the whole batch (every instance replays the same source recording): the device front end takes the
    // transcripts from the state before the commitments — label, r1cs domain separator, the scenario's own prefix
    host::Transcript proto;
    prov.dev_batch = [&](VfyDevBatch<C>& db) -> bool {
        if (!src[0] || src[0]->m != ms[0] || (!src[0]->cs.deferred.empty() && ctx->tune_vfy_device < 2)) return false;
        for (size_t k = 1; k < count; k++) if (src[k] != src[0] || ms[k] != ms[0]) return false;
        proto = host::Transcript(host::scenario_label(scenarios[0]));
        host::TP<C>::r1cs_domain_sep(proto);
        host::StatementIO io0; make_io(0, io0);
        size_t expect = 0;
        if (host::scenario_verifier_prefix<C>(proto, scenarios[0], params, io0, &expect) || expect != ms[0]) return false;
        db.src = &src[0]->cs; db.m = ms[0]; db.absorb_commitments = true; db.shared_state = true;
        db.state_of = [&](size_t) { return (const host::Strobe*)&proto.s; };
        db.commit_xy = [&](size_t k) { return commit_xy + 8 * coff[k]; };
        return true;
    };
    // several statement shapes: an instance's class is its source recording; a class takes its transcripts from its own prefix state
    std::deque<host::Transcript> protos;
    prov.class_id = [&](size_t k, VfyClassId& id) -> bool {
        if (!src[k] || src[k]->m != ms[k]) return false;
        id.rec = src[k].get(); id.m = ms[k]; id.two = !src[k]->cs.deferred.empty();
        return true;
    };
    prov.dev_class = [&](const uint32_t* idx, size_t, VfyDevBatch<C>& db) -> bool {
        const size_t k0 = idx[0];
        host::Transcript pr(host::scenario_label(scenarios[k0]));
        host::TP<C>::r1cs_domain_sep(pr);
        host::StatementIO io0; make_io(k0, io0);
        size_t expect = 0;
        if (host::scenario_verifier_prefix<C>(pr, scenarios[k0], params + 8 * k0, io0, &expect) || expect != ms[k0]) return false;
        protos.push_back(pr);
        const host::Strobe* state = &protos.back().s;
        db.src = &src[k0]->cs; db.m = ms[k0]; db.absorb_commitments = true; db.shared_state = true;
        db.state_of = [state](size_t) { return state; };
        db.commit_xy = [&, idx](size_t j) { return commit_xy + 8 * coff[idx[j]]; };
        return true;
    };
    if (other_core) return (*other_core)(prov, poff.data(), alphas.data());
    return batch_verify_core<C>(ctx, count, prov, proofs, poff.data(), alphas.data(), timing, point_out);
}

// Verifier::verify for a scenario statement = the batch path with one instance and alpha = 1
template <class C>
static int verify_scenario(bp_ctx* ctx, int scenario, const uint64_t* params, const uint8_t* proof, size_t proof_len, const uint64_t* commit_xy, size_t m,
                           const uint64_t* publics, size_t npub) {
    return batch_verify_scenarios<C>(ctx, 1, &scenario, params, proof, &proof_len, commit_xy, &m, publics, &npub, nullptr, nullptr, 0, nullptr);
}

// ---- InnerProductProof::verify (src/inner_product_proof.rs:321-382) -----------------------------------------------
// challenges: u_j in creation order, as the caller's transcript replay produced them (verification_scalars :268-277).
template <class C>
static int ipa_verify_host_entry(bp_ctx* ctx, size_t n, const uint64_t* Gf, const uint64_t* Hf, const uint64_t* P, const uint64_t* Q, const uint64_t* Gv,
                                 const uint64_t* Hv, const uint64_t* L, const uint64_t* R, size_t k, const uint64_t* challenges, const uint64_t* a,
                                 const uint64_t* b) {
    typedef typename C::Fr FrP;
    typedef host::Fld<FrP> S;
    typedef host::Grp<C> G;
    hipStream_t st = ctx->stream;
    if (k >= 32 || n != ((size_t)1 << k)) return BP_E_VERIFICATION;  // :257-264
    std::vector<F4> ch(k), chi(k), u_sq(k), u_inv_sq(k);
    F4 allinv = S::one();
    for (size_t i = 0; i < k; i++) {
        memcpy(ch[i].v, challenges + 4 * i, 32);
        chi[i] = ch[i].is_zero() ? ch[i] : S::inv(ch[i]);
        if (!chi[i].is_zero()) allinv = S::mul(allinv, chi[i]);
        u_sq[i] = S::sqr(ch[i]); u_inv_sq[i] = S::sqr(chi[i]);
    }
    F4 av, bv; memcpy(av.v, a, 32); memcpy(bv.v, b, 32);
    // device: factors, constants, challenges
    BPCHK(ctx->ipa_Gf.ensure(n * 32)); BPCHK(ctx->ipa_Hf.ensure(n * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->ipa_Gf.as<u32>(), (const F4*)Gf, n));
    BPCHK(upload_scalars<C>(ctx, ctx->ipa_Hf.as<u32>(), (const F4*)Hf, n));
    std::vector<F4> cst = {allinv, av, bv};
    cst.insert(cst.end(), u_sq.begin(), u_sq.end());
    BPCHK(ctx->r_chal.ensure(cst.size() * 32));
    BPCHK(upload_scalars<C>(ctx, ctx->r_chal.as<u32>(), cst.data(), cst.size()));
    // scalars: [a*b | g[n] | h[n] | -u_sq[k] | -u_inv_sq[k]] (canonical), bases: Q | G | H | L | R   (:360-373)
    const size_t terms = 1 + 2 * n + 2 * k;
    BPCHK(ctx->r_g.ensure(terms * 32));
    u32* sc = ctx->r_g.as<u32>();
    std::vector<uint64_t> head(4), tail(8 * std::max<size_t>(k, 1));
    canon_words<FrP>(head.data(), S::mul(av, bv));
    for (size_t i = 0; i < k; i++) { canon_words<FrP>(&tail[4 * i], S::neg(u_sq[i])); canon_words<FrP>(&tail[4 * (k + i)], S::neg(u_inv_sq[i])); }
    HIPCHK(hipMemcpyAsync(sc, head.data(), 32, hipMemcpyHostToDevice, st));
    if (k) HIPCHK(hipMemcpyAsync(sc + (1 + 2 * n) * 8, tail.data(), 2 * k * 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ipa_vfy_scalars<C>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, ctx->ipa_Gf.as<u32>(), ctx->ipa_Hf.as<u32>(), ctx->r_chal.as<u32>() + 3 * 8,
                       ctx->r_chal.as<u32>(), (u32)n, (u32)k, sc + 8, sc + (1 + n) * 8);
    HIPCHK(hipGetLastError());
    // bases
    BPCHK(ctx->ipa_G.ensure(n * 64)); BPCHK(ctx->ipa_H.ensure(n * 64)); BPCHK(ctx->ipa_Q.ensure(64)); BPCHK(ctx->r_tail.ensure(std::max<size_t>(2 * k, 1) * 64));
    HIPCHK(hipMemcpyAsync(ctx->ipa_G.p, Gv, n * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_H.p, Hv, n * 64, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->ipa_Q.p, Q, 64, hipMemcpyHostToDevice, st));
    if (k) {
        HIPCHK(hipMemcpyAsync(ctx->r_tail.p, L, k * 64, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->r_tail.as<u32>() + k * 16, R, k * 64, hipMemcpyHostToDevice, st));
        BPCHK(bp_points_import(ctx, ctx->r_tail.p, ctx->r_tail.p, 2 * k));
    }
    BPCHK(bp_points_import(ctx, ctx->ipa_G.p, ctx->ipa_G.p, n));
    BPCHK(bp_points_import(ctx, ctx->ipa_H.p, ctx->ipa_H.p, n));
    BPCHK(bp_points_import(ctx, ctx->ipa_Q.p, ctx->ipa_Q.p, 1));
    BaseSegs sg; memset(&sg, 0, sizeof sg);
    sg.nseg = k ? 4 : 3;
    sg.ptr[0] = ctx->ipa_Q.as<u32>(); sg.ptr[1] = ctx->ipa_G.as<u32>(); sg.ptr[2] = ctx->ipa_H.as<u32>(); sg.ptr[3] = ctx->r_tail.as<u32>();
    sg.start[0] = 0; sg.start[1] = 1; sg.start[2] = (u32)(1 + n); sg.start[3] = (u32)(1 + 2 * n); sg.start[4] = (u32)terms;
    J4 r;
    BPCHK(msm_run<C>(ctx, sg, sc, terms, 0, r));
    A4 expect = G::to_aff(r), Pp;
    memcpy(Pp.x.v, P, 32); memcpy(Pp.y.v, P + 4, 32);
    if (ctx->profiling) collect_timers(ctx);
    return expect == Pp ? BP_OK : BP_E_VERIFICATION;  // `expect_P == *P` (:377)
}
