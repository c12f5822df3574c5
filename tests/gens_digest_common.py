"""The generator digest of include/arkbp.h (bp_gens_digest, bp_host_gens_digest) restated over hashlib: independent of the library's
Keccak, of its host twin and of its kernels.  Points are (m, 8) arrays of uint64 ark words; their bytes are the little-endian words."""
import hashlib
import struct

import numpy as np


def _h(label, byte, index, payload):
    return hashlib.sha3_256(label + bytes([byte]) + struct.pack("<Q", index) + payload).digest()


def vector_root(tag, pts):
    pts = np.ascontiguousarray(pts, dtype="<u8").reshape(-1, 8)
    nodes = [_h(b"arkbp-gens-leaf-v1", tag, i, p.tobytes()) for i, p in enumerate(pts)]
    level = 0
    while len(nodes) > 1:
        level += 1
        nodes = [_h(b"arkbp-gens-node-v1", level, j, nodes[2 * j] + nodes[2 * j + 1]) if 2 * j + 1 < len(nodes) else nodes[2 * j]
                 for j in range((len(nodes) + 1) // 2)]
    return nodes[0]


def digest(curve, G, H, n, B, Bb):
    """(root, pair root, G root, H root)"""
    pair = vector_root(0, np.stack([np.asarray(B, dtype=np.uint64), np.asarray(Bb, dtype=np.uint64)]))
    g, h = vector_root(1, G[:n]), vector_root(2, H[:n])
    return _h(b"arkbp-gens-root-v1", curve, n, pair + g + h), pair, g, h
