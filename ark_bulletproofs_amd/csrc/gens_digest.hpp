// Host twin of bp_gens_digest (include/arkbp.h has the definition): the digest of a set of generators from the caller's own copy of
// the points, in plain C++.  It shares nothing with the kernels of vfe.hip but the definition, and it validates nothing: it hashes
// the 64 bytes of every point as they are (x then y, four little-endian 64-bit Montgomery words each — the host is little-endian, as
// everywhere in this layer).  Host only: csrc/gens_digest_selftest.cpp runs it stand-alone.
#pragma once
#include <vector>
#include "host_proto.hpp"

namespace arkbp {
namespace host {

// SHA3-256(label (18 bytes) || byte18 || LE64(index) || payload)
static inline void gens_hash(u8 out[32], const char* label18, u8 byte18, uint64_t index, const u8* payload, size_t len) {
    u8 m[27 + 96];
    memcpy(m, label18, 18);
    m[18] = byte18;
    memcpy(m + 19, &index, 8);
    memcpy(m + 27, payload, len);
    sha3_256(out, m, 27 + len);
}
// root of a vector of m >= 1 points under `tag`: the leaves, then level by level; an odd last node goes up unchanged
static inline void gens_vector_root(u8 out[32], u8 tag, const uint64_t* xy, size_t m) {
    std::vector<u8> cur(m * 32), next;
    for (size_t i = 0; i < m; i++) gens_hash(&cur[i * 32], "arkbp-gens-leaf-v1", tag, i, (const u8*)(xy + i * 8), 64);
    for (u8 level = 1; m > 1; level++) {
        const size_t parents = (m + 1) / 2;
        next.assign(parents * 32, 0);
        for (size_t j = 0; j < parents; j++) {
            if (2 * j + 1 < m) gens_hash(&next[j * 32], "arkbp-gens-node-v1", level, j, &cur[2 * j * 32], 64);
            else memcpy(&next[j * 32], &cur[2 * j * 32], 32);
        }
        cur.swap(next);
        m = parents;
    }
    memcpy(out, cur.data(), 32);
}
// out = root | pair root | G root | H root
static inline void gens_digest(int curve, const uint64_t* G_xy, const uint64_t* H_xy, size_t n, const uint64_t B_xy[8], const uint64_t Bb_xy[8], u8 out[128]) {
    uint64_t pair[16];
    memcpy(pair, B_xy, 64);
    memcpy(pair + 8, Bb_xy, 64);
    gens_vector_root(out + 32, 0, pair, 2);
    gens_vector_root(out + 64, 1, G_xy, n);
    gens_vector_root(out + 96, 2, H_xy, n);
    gens_hash(out, "arkbp-gens-root-v1", (u8)curve, n, out + 32, 96);
}

}  // namespace host
}  // namespace arkbp
