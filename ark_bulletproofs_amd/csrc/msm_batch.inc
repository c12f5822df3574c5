// bp_msm_batch / bp_msm_batch_dev: `count` independent VariableBaseMSM::msm calls in one (included by arkbp.hip; kernels: msm_batch.cuh).
//
// Every job takes one of three routes by its length (msb_route): SHORT jobs run through k_ve_tail, BUCKETED ones through k_msb_accum +
// k_msb_combine, the rest — and every job of a window-sharded ctx — through msm_run, one after the other, as bp_msm_dev would.
// Consecutive short and bucketed jobs form a GROUP: one staging copy into ve_arena, one sequence of launches on the ctx's stream, one
// host wait, one shared inversion for the affine results.  A group ends where the arena budget is reached or where a single-route job
// stands (its terms are not staged), so a group's terms are one contiguous range of the caller's arrays and resident operands are read
// in place.  k_ve_tail takes prefix offsets, so it is launched once per run of consecutive short jobs of the group.

// defaults of BP_TUNE_MSM_BATCH_SHORT / _MAX / _MIN_JOBS (measured: DESIGN.md section 5 "Many MSMs per call", profiles/r08_msm_batch.txt;
// the slice cap has no fixed default: msb_auto_slice)
static constexpr uint64_t MSB_DEFAULT_SHORT = 8, MSB_DEFAULT_MAX = 4096, MSB_DEFAULT_MIN_JOBS = 6;
static constexpr size_t MSB_ARENA_BUDGET = (size_t)256 << 20;

struct MsbKnobs { uint64_t short_max, slice, batch_max; };
// the knob values in force for a call over these jobs (0 = the default; the default slice cap follows from the call's bucketed terms)
static MsbKnobs msb_knobs(uint64_t short_max, uint64_t slice, uint64_t batch_max, size_t count, const size_t* offsets) {
    MsbKnobs k;
    k.short_max = short_max ? short_max : MSB_DEFAULT_SHORT;
    k.batch_max = batch_max ? batch_max : MSB_DEFAULT_MAX;
    k.slice = std::min<uint64_t>(slice, (uint64_t)1 << 30);
    if (!slice) {
        uint64_t T = 0;
        for (size_t j = 0; j < count; j++) { const size_t nj = offsets[j + 1] - offsets[j]; if (msb_route(nj, k.short_max, k.batch_max, false) == MSB_ROUTE_BUCKETED) T += nj; }
        k.slice = msb_auto_slice(T);
    }
    return k;
}
// the arena budget: 256 MB; ARKBP_MSM_BATCH_ARENA=<bytes> narrows it (documented in include/arkbp.h: the cut into groups on small
// inputs; read per call, one getenv against a group's launches and host wait)
static size_t msb_budget() {
    if (const char* v = getenv("ARKBP_MSM_BATCH_ARENA")) { const long long b = atoll(v); if (b > 0 && (size_t)b < MSB_ARENA_BUDGET) return (size_t)b; }
    return MSB_ARENA_BUDGET;
}
// arena bytes of a group of `cnt` jobs with n terms and ns slices (an upper bound: every part aligned)
static size_t msb_group_bytes(size_t n, size_t cnt, size_t ns, bool stage_pts, bool stage_sc) {
    return (stage_pts ? ve_align(n * 64) : 0) + (stage_sc ? ve_align(n * 32) : 0) + ve_align((cnt + 1) * 4 + ns * sizeof(MsbSlice) + cnt * sizeof(MsbJob)) +
           ve_align(ns * (size_t)MSB_PART_WORDS * 4) + ve_align(cnt * 96);
}

// one group: jobs [j0, j1), none of them single-route.  host_in: (h_bases, h_scalars) are staged; otherwise (d_bases, d_scalars) are read in place.
template <class C>
static int msb_group(bp_ctx* ctx, const MsbKnobs& kn, size_t j0, size_t j1, const size_t* offsets, const uint64_t* h_bases, const uint64_t* h_scalars,
                     const void* d_bases, const void* d_scalars, bool host_in, int canonical, uint64_t* out_xy) {
    typedef typename C::Fr FrP;
    hipStream_t st = ctx->stream;
    const size_t cnt = j1 - j0, lo = offsets[j0], n = offsets[j1] - lo;
    // tables: prefix offsets | slice table | bucketed jobs
    std::vector<u32> toff(cnt + 1);
    std::vector<MsbSlice> slices;
    std::vector<MsbJob> bjobs;
    std::vector<std::pair<u32, u32>> runs;   // (first job, jobs) of every run of consecutive short jobs
    u32 max_short = 0, max_slice_terms = 0, max_slices = 0;
    for (size_t j = 0; j <= cnt; j++) toff[j] = (u32)(offsets[j0 + j] - lo);
    for (size_t j = 0; j < cnt; j++) {
        const u32 nj = toff[j + 1] - toff[j];
        if (msb_route(nj, kn.short_max, kn.batch_max, false) == MSB_ROUTE_SHORT) {
            if (!runs.empty() && runs.back().first + runs.back().second == (u32)j) runs.back().second++; else runs.push_back({(u32)j, 1u});
            max_short = std::max(max_short, nj);
            continue;
        }
        const u32 S = msb_slice_count(nj, (u32)kn.slice);
        bjobs.push_back(MsbJob{(u32)j, (u32)slices.size(), S});
        max_slices = std::max(max_slices, S);
        for (u32 s = 0; s < S; s++) {
            const u32 len = msb_slice_terms(nj, S, s);
            slices.push_back(MsbSlice{(u32)j, toff[j] + msb_slice_first(nj, S, s), len});
            max_slice_terms = std::max(max_slice_terms, len);
        }
    }
    const size_t ns = slices.size(), nb = bjobs.size();
    const bool stage_sc = host_in || !canonical;
    const size_t o_pts = 0, o_sc = host_in ? ve_align(n * 64) : 0, o_tab = o_sc + (stage_sc ? ve_align(n * 32) : 0);
    const size_t tab_toff = 0, tab_sl = (cnt + 1) * 4, tab_jb = tab_sl + ns * sizeof(MsbSlice), tab_bytes = tab_jb + nb * sizeof(MsbJob);
    const size_t o_part = o_tab + ve_align(tab_bytes), o_out = o_part + ve_align(ns * (size_t)MSB_PART_WORDS * 4), total = o_out + ve_align(cnt * 96);
    BPCHK(ctx->ve_arena.ensure(total));
    char* d = (char*)ctx->ve_arena.p;
    const u32* pts = host_in ? (const u32*)(d + o_pts) : (const u32*)d_bases + lo * 16;
    const u32* sc = stage_sc ? (const u32*)(d + o_sc) : (const u32*)d_scalars + lo * 8;
    if (n) {
        if (host_in) {
            HIPCHK(hipMemcpyAsync(d + o_pts, h_bases + 8 * lo, n * 64, hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d + o_sc, h_scalars + 4 * lo, n * 32, hipMemcpyHostToDevice, st));
            BPCHK(bp_points_import(ctx, d + o_pts, d + o_pts, n));
        }
        if (!canonical) {   // Montgomery -> canonical on the arena's copy (resident scalars are left as they are)
            const u32* src = host_in ? (const u32*)(d + o_sc) : (const u32*)d_scalars + lo * 8;
            hipLaunchKernelGGL(k_scalars_import<FrP>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, src, (u32*)(d + o_sc), (u32)n);
            hipLaunchKernelGGL(k_scalars_to_canon<FrP>, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (u32*)(d + o_sc), (u32)n);
        }
    }
    std::vector<char> tab(tab_bytes);
    memcpy(tab.data() + tab_toff, toff.data(), (cnt + 1) * 4);
    if (ns) memcpy(tab.data() + tab_sl, slices.data(), ns * sizeof(MsbSlice));
    if (nb) memcpy(tab.data() + tab_jb, bjobs.data(), nb * sizeof(MsbJob));
    HIPCHK(hipMemcpyAsync(d + o_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, st));   // (pageable source: copied before the call returns)
    if (!runs.empty()) {
        ScopedK tk(ctx, BP_K_VE_TAIL);
        for (const auto& r : runs)
            hipLaunchKernelGGL(k_ve_tail<C>, dim3(r.second), dim3(256), 0, st, pts, sc, (const u32*)(d + o_tab + tab_toff) + r.first, max_short, (u32*)(d + o_out) + (size_t)r.first * 24);
    }
    if (nb) {
        ScopedK tk(ctx, BP_K_MSM_BATCH);
        hipLaunchKernelGGL(k_msb_accum<C>, dim3((u32)ns), dim3(256), 0, st, pts, sc, (const MsbSlice*)(d + o_tab + tab_sl), max_slice_terms, (u32*)(d + o_part));
        hipLaunchKernelGGL(k_msb_combine<C>, dim3((u32)nb), dim3(256), 0, st, (const u32*)(d + o_part), (const MsbJob*)(d + o_tab + tab_jb), max_slices, (u32*)(d + o_out));
    }
    HIPCHK(hipGetLastError());
    std::vector<u64> res(cnt * 12);
    HIPCHK(hipMemcpyAsync(res.data(), d + o_out, cnt * 96, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx_stream_wait(ctx));
    ctx->mb_groups++; ctx->mb_waits += BP_MSM_BATCH_WAITS_PER_GROUP;
    std::vector<J4> jp(cnt);
    std::vector<A4> ap(cnt);
    pf_points_in(res.data(), cnt, jp.data());
    to_aff_many<C>(jp.data(), cnt, ap.data());   // one shared inversion
    for (size_t j = 0; j < cnt; j++) { memcpy(out_xy + 8 * (j0 + j), ap[j].x.v, 32); memcpy(out_xy + 8 * (j0 + j) + 4, ap[j].y.v, 32); }
    return BP_OK;
}

template <class C>
static int msm_batch_entry(bp_ctx* ctx, size_t count, const size_t* offsets, const uint64_t* h_bases, const uint64_t* h_scalars, const void* d_bases,
                           const void* d_scalars, bool host_in, int canonical, uint64_t* out_xy) {
    MsmLatencyScope latency(ctx);   // as the other bp_msm* entry points: the caller waits for these results
    const MsbKnobs kn = msb_knobs(ctx->tune_msb_short, ctx->tune_msb_slice, ctx->tune_msb_max, count, offsets);
    const size_t budget = msb_budget();
    const bool stage_sc = host_in || !canonical;
    // a job no group could hold takes the single route; so does EVERY job of a sharded ctx, and of a call with fewer than
    // BP_TUNE_MSM_BATCH_MIN_JOBS jobs for the groups: a group costs the latency of one Horner chain (~1.2 ms), a bp_msm_dev ~0.25 ms
    auto fits = [&](size_t nj) { return msb_group_bytes(nj, 1, msb_slice_count((u32)nj, (u32)kn.slice), host_in, stage_sc) <= budget; };
    bool sharded = ctx->shard_world > 1;
    if (!sharded) {
        size_t grouped = 0;
        for (size_t j = 0; j < count; j++) { const size_t nj = offsets[j + 1] - offsets[j]; if (msb_route(nj, kn.short_max, kn.batch_max, false) != MSB_ROUTE_SINGLE && fits(nj)) grouped++; }
        if (grouped < (ctx->tune_msb_min_jobs ? ctx->tune_msb_min_jobs : MSB_DEFAULT_MIN_JOBS)) sharded = true;
    }
    size_t g0 = 0, g_n = 0, g_ns = 0;   // the open group: jobs [g0, j), its terms and slices
    auto flush = [&](size_t j) -> int {
        if (j > g0) BPCHK(msb_group<C>(ctx, kn, g0, j, offsets, h_bases, h_scalars, d_bases, d_scalars, host_in, canonical, out_xy));
        g0 = j; g_n = 0; g_ns = 0;
        return BP_OK;
    };
    for (size_t j = 0; j < count; j++) {
        const size_t nj = offsets[j + 1] - offsets[j];
        u32 route = msb_route(nj, kn.short_max, kn.batch_max, sharded);
        const size_t sj = route == MSB_ROUTE_BUCKETED ? msb_slice_count((u32)nj, (u32)kn.slice) : 0;
        if (route != MSB_ROUTE_SINGLE && !fits(nj)) route = MSB_ROUTE_SINGLE;
        if (route == MSB_ROUTE_SINGLE) {
            BPCHK(flush(j));
            g0 = j + 1;
            ctx->mb_single++;
            if (host_in) BPCHK(bp_msm(ctx, h_bases + 8 * offsets[j], h_scalars + 4 * offsets[j], nj, canonical, out_xy + 8 * j));
            else BPCHK(bp_msm_dev(ctx, (const u32*)d_bases + offsets[j] * 16, (const u32*)d_scalars + offsets[j] * 8, nj, canonical, out_xy + 8 * j));
            continue;
        }
        if (j > g0 && msb_group_bytes(g_n + nj, j - g0 + 1, g_ns + sj, host_in, stage_sc) > budget) BPCHK(flush(j));
        g_n += nj; g_ns += sj;
        if (route == MSB_ROUTE_SHORT) ctx->mb_short++; else ctx->mb_bucketed++;
    }
    BPCHK(flush(count));
    if (ctx->profiling) collect_timers(ctx);
    return BP_OK;
}

static int msm_batch_checks(const char* who, bp_ctx* c, size_t count, const size_t* offsets, const void* bases, const void* scalars, uint64_t* out_xy) {
    auto bad = [&](const char* what) { g_err = std::string(who) + ": " + what; return BP_E_ARG; };
    if (!c || !offsets || !out_xy) return bad("bad argument");
    for (size_t j = 0; j < count; j++) if (offsets[j + 1] < offsets[j]) return bad("offsets must not decrease");
    const size_t n = offsets[count] - offsets[0];
    if (n >= ((size_t)1 << 31)) return bad("too many terms");
    if (n && (!bases || !scalars)) return bad("bad argument");
    return BP_OK;
}
int bp_msm_batch(bp_ctx* c, size_t count, const size_t* offsets, const uint64_t* bases_xy, const uint64_t* scalars, int scalars_canonical, uint64_t* out_xy) {
    if (count == 0) return BP_OK;
    BPCHK(msm_batch_checks("bp_msm_batch", c, count, offsets, bases_xy, scalars, out_xy));
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_batch_entry<Secq>(c, count, offsets, bases_xy, scalars, nullptr, nullptr, true, scalars_canonical, out_xy)
                         : msm_batch_entry<Zorro>(c, count, offsets, bases_xy, scalars, nullptr, nullptr, true, scalars_canonical, out_xy);
}
int bp_msm_batch_dev(bp_ctx* c, size_t count, const size_t* offsets, const void* d_bases, const void* d_scalars, int scalars_canonical, uint64_t* out_xy) {
    if (count == 0) return BP_OK;
    BPCHK(msm_batch_checks("bp_msm_batch_dev", c, count, offsets, d_bases, d_scalars, out_xy));
    if (c->host_only) return BP_E_NO_DEVICE;
    HIPCHK(hipSetDevice(c->device));
    return c->curve == 0 ? msm_batch_entry<Secq>(c, count, offsets, nullptr, nullptr, d_bases, d_scalars, false, scalars_canonical, out_xy)
                         : msm_batch_entry<Zorro>(c, count, offsets, nullptr, nullptr, d_bases, d_scalars, false, scalars_canonical, out_xy);
}
int bp_ctx_msm_batch_stats(bp_ctx* c, uint64_t* short_jobs, uint64_t* bucketed_jobs, uint64_t* single_jobs, uint64_t* groups, uint64_t* host_waits) {
    if (!c) return BP_E_ARG;
    if (short_jobs) *short_jobs = c->mb_short;
    if (bucketed_jobs) *bucketed_jobs = c->mb_bucketed;
    if (single_jobs) *single_jobs = c->mb_single;
    if (groups) *groups = c->mb_groups;
    if (host_waits) *host_waits = c->mb_waits;
    return BP_OK;
}
int bp_debug_msm_batch_plan(size_t count, const size_t* offsets, uint64_t short_max, uint64_t slice_terms, uint64_t batch_max, const uint64_t* scalars_canonical,
                            size_t job, uint8_t* route, uint32_t* nslices, uint32_t* slice_first, uint32_t* slice_len, int8_t* digits) {
    if (!offsets) return BP_E_ARG;
    const bool per_job = slice_first || slice_len || digits;
    if (per_job && job >= count) return BP_E_ARG;
    for (size_t j = 0; j < count; j++) if (offsets[j + 1] < offsets[j]) return BP_E_ARG;
    if (offsets[count] - offsets[0] >= ((size_t)1 << 31)) return BP_E_ARG;
    const MsbKnobs kn = msb_knobs(short_max, slice_terms, batch_max, count, offsets);
    for (size_t j = 0; j < count; j++) {
        const size_t nj = offsets[j + 1] - offsets[j];
        if (route) route[j] = (uint8_t)msb_route(nj, kn.short_max, kn.batch_max, false);
        if (nslices) nslices[j] = msb_slice_count((u32)nj, (u32)kn.slice);
    }
    if (!per_job) return BP_OK;
    const u32 t0 = (u32)(offsets[job] - offsets[0]), nt = (u32)(offsets[job + 1] - offsets[job]), S = msb_slice_count(nt, (u32)kn.slice);
    for (u32 s = 0; s < S; s++) {
        if (slice_first) slice_first[s] = t0 + msb_slice_first(nt, S, s);
        if (slice_len) slice_len[s] = msb_slice_terms(nt, S, s);
    }
    if (digits) {
        if (nt && !scalars_canonical) return BP_E_ARG;
        for (u32 t = 0; t < nt; t++) {
            const u32* k = (const u32*)(scalars_canonical + 4 * (size_t)(t0 + t));
            for (u32 w = 0; w < VE_WINDOWS; w++) digits[(size_t)VE_WINDOWS * t + w] = (int8_t)msb_digit(k, w);
        }
    }
    return BP_OK;
}
