// Stand-alone ThreadSanitizer exercise of the host's per-pair fixed-base tables (host_proto.hpp PedersenGens::fixed_tables): two
// threads, two pairs per curve used alternately, a few hundred commitments each, every result compared with the double-and-add ladder.
// More distinct pairs than the cache holds go through it as well, so that eviction runs while the other thread reads.  CPU only:
//   clang++ -std=c++17 -O1 -g -march=x86-64-v3 -fsanitize=thread -pthread tools/tsan_pedersen_tables.cpp -o /tmp/tsan_pedersen_tables && /tmp/tsan_pedersen_tables
#include <cstdio>
#include <thread>

#include "../ark_bulletproofs_amd/csrc/host_proto.hpp"

using namespace arkbp;
using namespace arkbp::host;

template <class C> static int run(const char* name) {
    typedef Grp<C> G;
    typedef Fld<typename C::Fr> S;
    typedef PedersenGens<C> PG;
    // pairs: the default one, the first points of a generators chain, and enough further ones to overflow the cache
    std::vector<A4> chain;
    derive_generators<C>(chain, 'G', 0x50434731u, 2 * (PG::FIXED_CACHE_MAX + 3), 1);
    std::vector<PG> pairs;
    pairs.push_back(PG::make_default());
    for (size_t i = 0; i + 1 < chain.size(); i += 2) { PG p; p.B = chain[i]; p.B_blinding = chain[i + 1]; pairs.push_back(p); }
    { PG p; p.B = chain[0]; p.B_blinding = chain[0]; pairs.push_back(p); }   // B == B_blinding
    std::atomic<int> bad{0};
    auto work = [&](int tid) {
        u8 seed[32]; memset(seed, 17 + tid, 32);
        ChaChaRng rng(seed);
        for (int i = 0; i < 300; i++) {
            // the two threads walk the first two pairs in opposite order; every 25th commitment uses one of the others
            const PG& pc = i % 25 == 24 ? pairs[2 + (size_t)(i / 25 + 5 * tid) % (pairs.size() - 2)] : pairs[(size_t)(i + tid) & 1];
            F4 v = rand_fe<typename C::Fr>(rng), b = rand_fe<typename C::Fr>(rng);
            if (i % 50 == 7) v = S::zero();
            if (i % 50 == 9) b = S::zero();
            const A4 got = pc.commit(v, b);
            const A4 want = G::to_aff(G::add(G::mul(pc.B, v), G::mul(pc.B_blinding, b)));
            const A4 q = G::to_aff(pc.mul_B_jac(v));
            const A4 qw = G::to_aff(G::mul(pc.B, v));
            if (!(got == want) || !(q == qw)) bad++;
        }
    };
    std::thread t0(work, 0), t1(work, 1);
    t0.join(); t1.join();
    printf("%s: %d mismatches\n", name, bad.load());
    return bad.load();
}

int main() {
    int bad = run<Secq>("secq256k1") + run<Zorro>("zorro");
    printf(bad ? "FAILED\n" : "ok\n");
    return bad ? 1 : 0;
}
