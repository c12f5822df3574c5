// Stand-alone check of csrc/gens_digest.hpp, the host twin of bp_gens_digest (pure host code; its own main, no HIP, not loaded into
// anything): built and run by tests/test_gens_check_cpu.py with the address and undefined-behaviour sanitizers.
//   - sha3_256 against FIPS 202's published answers and at the lengths around the 136-byte rate;
//   - the digest of synthetic "points" (word w of point i of vector t = 0x9E3779B97F4A7C15 * (8 i + w + 1) + t; the digest hashes bytes
//     and validates nothing) at n = 1, 2, 3, 5 against roots that hashlib.sha3_256 gave for the definition in include/arkbp.h;
//   - the tree rules spelled out by hand: one point is its leaf, two points one node, a third goes up unchanged and joins at level 2;
//   - a swapped pair of generators changes the root and that vector's root only.
// The last line of stdout is "gens_digest selftest ok"; a failed check is printed and the exit status is 1.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "gens_digest.hpp"

using namespace arkbp::host;

static int g_fail = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); g_fail++; } } while (0)

static std::string hex(const u8* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
static std::string sha_hex(const std::vector<u8>& m) {
    u8 out[32];
    sha3_256(out, m.data(), m.size());
    return hex(out, 32);
}
static std::vector<uint64_t> synth(uint64_t t, size_t n) {
    std::vector<uint64_t> v(n * 8);
    for (size_t i = 0; i < n; i++) for (size_t w = 0; w < 8; w++) v[i * 8 + w] = 0x9E3779B97F4A7C15ull * (8 * i + w + 1) + t;
    return v;
}
struct Roots { u8 b[128]; std::string root() const { return hex(b, 32); } std::string pair() const { return hex(b + 32, 32); } std::string G() const { return hex(b + 64, 32); } std::string H() const { return hex(b + 96, 32); } };
static Roots digest(int curve, const std::vector<uint64_t>& G, const std::vector<uint64_t>& H, size_t n, const uint64_t* B, const uint64_t* Bb) {
    Roots d;
    gens_digest(curve, G.data(), H.data(), n, B, Bb, d.b);
    return d;
}

int main() {
    // ---- SHA3-256 ----
    CHECK(sha_hex({}) == "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a");
    CHECK(sha_hex({'a', 'b', 'c'}) == "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532");
    CHECK(sha_hex(std::vector<u8>(200, 0xa3)) == "79f38adec5c20307a98ef76e8324afbfd46cfd81b22e3973c65fa1bd9de31787");
    {   // one byte short of the rate (both pad bytes fall on byte 135) and exactly the rate (the pad is a block of its own)
        std::vector<u8> m(136);
        for (size_t i = 0; i < 136; i++) m[i] = (u8)i;
        CHECK(sha_hex(m) == "cf3ccff92480a29160c2d38317c430e14749bfee1788106957dfe73f8c4930e5");
        m.pop_back();
        CHECK(sha_hex(m) == "fded8fd9d6551c601eeb3b7c6bc5e5cfd8aad1d015b7e9aaa9c9b9475231d5e2");
    }
    // ---- fixed vectors ----
    uint64_t B[8], Bb[8];
    for (int w = 0; w < 8; w++) { B[w] = 0x0101010101010101ull * (w + 1); Bb[w] = 0x0202020202020202ull * (w + 1); }
    static const struct { size_t n; const char *root, *G, *H; } FIXED[] = {
        {1, "48c278122f976b6e1fb40e027bebbc916325ebc2fef8644fb9731e90fa4f8a5f", "9ac55df9ca08f5a0e0cd1f4f51a7d5c7fc6500baf942af5904b0ec7f565a7e2f", "45cd690401058f4a1ccab095f9bb5ff18ebb9aec1f67b8fb0bcfab0fe0d4755c"},
        {2, "291fc3b0853716ecbc3e084783a9df0e3e670df05d96cdff996df8781a65ae56", "587c53ae045ed85d3004bf6c9b27aa2d64fad0f4ded56bf4a30a1dee11c9017b", "b51c2da9d617c6a4d02674fe529e466545b9ede42093ba06284b327d47f4aa5d"},
        {3, "6cf48fc17aceb3365d2eb89543a434a5eaa79ecc3d5657f84003b73e4047dd2a", "13913e2fcfafe6565d92de338739bbc2204003206141465dda0b27338a090c5f", "935317e7383c77b9205827a5e7f58a05ddc9ea40ffb9d147775f2e3a0c53fce3"},
        {5, "3b80ff2bee3174259be36c26cd874b5c6da7fb384e1e7c9ddace5c5dd2ff8e6d", "a8b3b4d009f59be4d4e47e8eb033ee299cb561f3b11bae5fb095fa9a6b3e3fce", "f8bc92de42f7b9c5bd0a704e01dfb6dd84f04d04648e924f15d4c9a3d60b28b9"},
    };
    const std::vector<uint64_t> G = synth(1, 5), H = synth(2, 5);
    for (const auto& f : FIXED) {
        const Roots d = digest(0, G, H, f.n, B, Bb);   // (a prefix of the same points: exactly n * 64 bytes of each vector are read)
        CHECK(d.root() == f.root); CHECK(d.G() == f.G); CHECK(d.H() == f.H);
        CHECK(d.pair() == "b0cdffa5bbd80b18187068bedf355ebbd1340594d7ea728d695fb6eb2f12d1da");
    }
    // ---- the tree, by hand ----
    u8 leaf[3][32], n01[32], n2[32], r[32], cat[64];
    for (size_t i = 0; i < 3; i++) gens_hash(leaf[i], "arkbp-gens-leaf-v1", 1, i, (const u8*)&G[i * 8], 64);
    gens_vector_root(r, 1, G.data(), 1);
    CHECK(!memcmp(r, leaf[0], 32));                                  // n = 1: the leaf itself
    memcpy(cat, leaf[0], 32); memcpy(cat + 32, leaf[1], 32);
    gens_hash(n01, "arkbp-gens-node-v1", 1, 0, cat, 64);
    gens_vector_root(r, 1, G.data(), 2);
    CHECK(!memcmp(r, n01, 32));                                      // n = 2: one node of level 1
    memcpy(cat, n01, 32); memcpy(cat + 32, leaf[2], 32);             // n = 3: leaf 2 is node 1 of level 1 unchanged, then joins at level 2
    gens_hash(n2, "arkbp-gens-node-v1", 2, 0, cat, 64);
    gens_vector_root(r, 1, G.data(), 3);
    CHECK(!memcmp(r, n2, 32));
    // ---- what a change changes ----
    const Roots base = digest(0, G, H, 5, B, Bb);
    std::vector<uint64_t> Gs = G;
    for (int w = 0; w < 8; w++) std::swap(Gs[1 * 8 + w], Gs[2 * 8 + w]);
    const Roots sw = digest(0, Gs, H, 5, B, Bb);
    CHECK(sw.root() != base.root() && sw.G() != base.G() && sw.H() == base.H() && sw.pair() == base.pair());
    const Roots pr = digest(0, G, H, 5, Bb, B);                     // B and B_blinding swapped
    CHECK(pr.root() != base.root() && pr.pair() != base.pair() && pr.G() == base.G() && pr.H() == base.H());
    const Roots cv = digest(1, G, H, 5, B, Bb);
    CHECK(cv.root() != base.root() && cv.pair() == base.pair() && cv.G() == base.G() && cv.H() == base.H());
    const Roots gh = digest(0, H, G, 5, B, Bb);                     // the vectors exchanged: the tags tell G from H
    CHECK(gh.G() != base.H() && gh.H() != base.G());
    if (g_fail) { printf("gens_digest selftest: %d check(s) failed\n", g_fail); return 1; }
    printf("gens_digest selftest ok\n");
    return 0;
}
