// Stand-alone check of a like-prover's device-witness state (host_proto.hpp: DevWitness, ConstraintSystem::assign_multipliers_dev,
// mults, witness_to_host, drop_dev_witness; include/arkbp.h bp_prover_assign_multipliers_dev) — pure host code with its own main, no
// HIP, not loaded into anything: built and run by tests/test_witness_dev_cpu.py, once with the address and undefined-behaviour
// sanitizers and once with the thread sanitizer.  The "device" here is heap memory behind the two hooks the library installs (fetch,
// drop), which count their calls and check that a copy is zeroed before it is freed: the state machine around them is what is tested —
// exactly one drop on every way out (download, consumption, destruction), a failed download leaves the handle as it was, and a
// downloaded witness is a host-assigned one: same vectors, same lazily formed a_O (on several threads), same row index, same report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include "host_proto.hpp"
#include "prove_steps.hpp"

using namespace arkbp;
using namespace arkbp::host;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static int g_fetches = 0, g_drops = 0, g_fail_next_fetch = 0;
static void* g_last_ctx = nullptr;
static int fake_fetch(const DevWitness& w, void* ctx, F4* left, F4* right) {
    g_fetches++; g_last_ctx = ctx;
    if (g_fail_next_fetch) { g_fail_next_fetch--; memset((void*)left, 0x5A, w.count * sizeof(F4)); return BP_E_HIP; }   // (a copy that broke half way)
    memcpy((void*)left, w.aL, w.count * sizeof(F4)); memcpy((void*)right, w.aR, w.count * sizeof(F4));
    return BP_OK;
}
static void fake_drop(DevWitness& w, void* ctx) {
    g_drops++; g_last_ctx = ctx;
    if (w.aL) { memset(w.aL, 0, w.count * sizeof(F4)); free(w.aL); }
    if (w.aR) { memset(w.aR, 0, w.count * sizeof(F4)); free(w.aR); }
    w.aL = w.aR = nullptr;
}
static DevWitness fake_device_copy(const std::vector<F4>& l, const std::vector<F4>& r) {
    DevWitness w;
    w.count = l.size(); w.device = 0; w.fetch = fake_fetch; w.drop = fake_drop;
    if (w.count) {
        w.aL = malloc(w.count * sizeof(F4)); w.aR = malloc(w.count * sizeof(F4));
        memcpy(w.aL, l.data(), w.count * sizeof(F4)); memcpy(w.aR, r.data(), w.count * sizeof(F4));
    }
    return w;
}

// n chained multipliers over two committed variables, and one row on top that no witness satisfies
template <class C> static void record(ConstraintSystem<C>& cs, size_t n) {
    typedef Fld<typename C::Fr> S;
    const Var v0{VK_COMMITTED, 0}, v1{VK_COMMITTED, 1}, one{VK_ONE, 0};
    cs.v = {S::from_u64(7), S::from_u64(0xFFFFFFFFFFull)}; cs.v_blinding = {S::from_u64(1001), S::from_u64(1002)};
    Var prev = v0;
    for (size_t i = 0; i < n; i++) {
        Var o[3];
        cs.multiply(LinComb{Term{prev, S::one()}, Term{one, S::from_u64(3 + i % 5)}}, LinComb{Term{v1, S::from_u64(2 + i % 3)}, Term{v0, S::one()}}, o);
        prev = i % 7 ? o[2] : v1;   // (keeps the values from collapsing)
    }
    cs.constrain(LinComb{Term{prev, S::one()}, Term{v1, S::from_u64(4)}, Term{one, S::neg(S::one())}});
}
static bool same_row(const HostRowIndex& a, const HostRowIndex& b) {
    return a.n == b.n && a.q == b.q && a.m == b.m && a.poff == b.poff && a.pinfo == b.pinfo && a.tvar == b.tvar && a.tcid == b.tcid && a.lrow == b.lrow;
}
// fn(0) .. fn(count - 1) on two threads
static void par2(size_t count, const std::function<void(size_t)>& fn) {
    std::thread t([&] { for (size_t c = 1; c < count; c += 2) fn(c); });
    for (size_t c = 0; c < count; c += 2) fn(c);
    t.join();
}

template <class C> static void check_size(size_t n) {
    Transcript tr("witness_dev selftest");
    ConstraintSystem<C> flat; flat.tr = &tr; flat.proving = true;
    record(flat, n);
    ConstraintSystem<C> src; src.tr = &tr; src.proving = true;
    record(src, n);
    CHECK(src.freeze(true) == BP_OK);
    int ctx_tag = 0;
    const int d0 = g_drops, f0 = g_fetches;
    {
        ConstraintSystem<C> like; like.tr = &tr;
        like.init_like_prover(src);
        like.v = flat.v; like.v_blinding = flat.v_blinding;
        CHECK(!like.dev.held() && like.mults() == 0);
        like.assign_multipliers_dev(fake_device_copy(flat.a_L, flat.a_R));
        CHECK(like.assigned && like.dev.held() && !like.aO_lazy && like.mults() == n && like.a_L.empty() && like.a_R.empty() && like.a_O.empty());
        // the row index of a prover whose witness is elsewhere is the host-assigned one's
        HostRowIndex r_flat, r_dev;
        CHECK(build_row_index<C>(flat, 4, r_flat) && build_row_index<C>(like, 4, r_dev) && same_row(r_flat, r_dev));
        // a download that fails: still held, nothing on the host, nothing dropped
        g_fail_next_fetch = 1;
        CHECK(like.witness_to_host(&ctx_tag) == (n ? BP_E_HIP : BP_OK));
        if (n) CHECK(like.dev.held() && like.mults() == n && like.a_L.empty() && like.a_R.empty() && !like.aO_lazy && g_drops == d0);
        g_fail_next_fetch = 0;
        // the download: the ctx is handed through, the copy is dropped exactly once, the handle is a host-assigned like-prover
        CHECK(like.witness_to_host(&ctx_tag) == BP_OK);
        CHECK(!like.dev.held() && like.aO_lazy && like.mults() == n && like.a_L.size() == n && like.a_R.size() == n && like.a_O.empty());
        CHECK(g_drops == d0 + 1 && g_last_ctx == &ctx_tag && g_fetches == f0 + (n ? 2 : 0));
        for (size_t i = 0; i < n; i++) CHECK(like.a_L[i] == flat.a_L[i] && like.a_R[i] == flat.a_R[i]);
        CHECK(like.witness_to_host(&ctx_tag) == BP_OK && g_drops == d0 + 1);   // (nothing left to bring over)
        like.materialise_aO(par2);
        CHECK(!like.aO_lazy && like.a_O.size() == n);
        for (size_t i = 0; i < n; i++) CHECK(like.a_O[i] == flat.a_O[i]);
        bp_witness_report w_flat, w_like;
        witness_check_host<C>(flat, w_flat); witness_check_host<C>(like, w_like);
        CHECK(memcmp(&w_flat, &w_like, sizeof w_flat) == 0 && w_like.gates_checked == n && w_like.bad_gates == 0 && w_like.bad_constraints == 1);   // (the last row is not satisfied by construction: both see it)
    }
    CHECK(g_drops == d0 + 1);   // (the destructor found nothing to drop)
    // consumed without a download: dropped by the explicit call, not again by the destructor
    {
        ConstraintSystem<C> like; like.tr = &tr;
        like.init_like_prover(src);
        like.assign_multipliers_dev(fake_device_copy(flat.a_L, flat.a_R));
        like.drop_dev_witness(&ctx_tag);
        CHECK(g_drops == d0 + 2 && g_last_ctx == &ctx_tag && !like.dev.held() && like.assigned && like.mults() == 0);
    }
    CHECK(g_drops == d0 + 2);
    // freed while the witness is still on the device: the destructor drops it, without a ctx
    {
        ConstraintSystem<C> like; like.tr = &tr;
        like.init_like_prover(src);
        like.assign_multipliers_dev(fake_device_copy(flat.a_L, flat.a_R));
    }
    CHECK(g_drops == d0 + 3 && g_last_ctx == nullptr);
}

int main() {
    for (size_t n : {(size_t)0, (size_t)1, (size_t)257, (size_t)40000}) { check_size<Secq>(n); check_size<Zorro>(n); }
    if (g_fail) { printf("witness_dev selftest: %d failure(s)\n", g_fail); return 1; }
    printf("witness_dev selftest ok\n");
    return 0;
}
