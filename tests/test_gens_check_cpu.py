"""The host side of the generator digest (include/arkbp.h: bp_host_gens_digest; csrc/gens_digest.hpp) without a GPU.

The digest is restated in tests/gens_digest_common.py over hashlib.sha3_256 — nothing of the library in it — and the library's host
twin must give the same 4 x 32 bytes on host-derived generators, at the sizes where the tree changes shape: one leaf, one node, an odd
node carried up, and the 255 / 256 / 257 that straddle a workgroup of the device's kernels (tests/test_gpu_gens_check.py compares the
kernels with this twin at the same sizes).  csrc/gens_digest_selftest.cpp, a program of its own, runs the twin under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gens_digest_common as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")
NMAX = 257


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def P(request, E):
    """(curve, G, H, B, B_blinding): host-derived points, once per curve"""
    cv = request.param
    B, Bb = E.pedersen_gens(cv)
    return cv, E.host_derive_generators(cv, False, 0, NMAX), E.host_derive_generators(cv, True, 0, NMAX), B, Bb


@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257])
def test_host_digest_equals_the_restatement(E, P, n):
    cv, G, H, B, Bb = P
    got = E.host_gens_digest(cv, G, H, B, Bb, n=n)
    assert tuple(got) == D.digest(cv, G, H, n, B, Bb)
    assert all(len(x) == 32 for x in got) and len(set(got)) == 4


def test_what_a_change_changes(E, P):
    cv, G, H, B, Bb = P
    n = 5
    base = E.host_gens_digest(cv, G, H, B, Bb, n=n)
    Gs = G.copy()
    Gs[[1, 2]] = Gs[[2, 1]]
    sw = E.host_gens_digest(cv, Gs, H, B, Bb, n=n)
    assert sw.root != base.root and sw.G != base.G and sw.H == base.H and sw.pair == base.pair
    assert tuple(sw) == D.digest(cv, Gs, H, n, B, Bb)
    B2 = B.copy()
    B2[3] ^= np.uint64(1)            # no point of the curve any more: the twin hashes bytes and validates nothing
    pr = E.host_gens_digest(cv, G, H, B2, Bb, n=n)
    assert pr.root != base.root and pr.pair != base.pair and pr.G == base.G and pr.H == base.H
    other = E.host_gens_digest(1 - cv, G, H, B, Bb, n=n)
    assert other.root != base.root and other[1:] == base[1:]
    assert tuple(other) == D.digest(1 - cv, G, H, n, B, Bb)
    # n is part of the root, and a longer prefix is another G root
    assert E.host_gens_digest(cv, G, H, B, Bb, n=4).G != base.G


def test_bad_arguments(E, P):
    from ark_bulletproofs_amd import _lib

    cv, G, H, B, Bb = P
    L, out = _lib.lib(), (C.c_uint8 * 128)()
    g, h, b, bb = (_lib.ptr(np.ascontiguousarray(a)) for a in (G, H, B, Bb))
    ok = [cv, g, h, C.c_size_t(3), b, bb, out]
    assert L.bp_host_gens_digest(*ok) == _lib.BP_OK
    for at in (1, 2, 4, 5, 6):       # each pointer null in turn
        args = list(ok)
        args[at] = None
        assert L.bp_host_gens_digest(*args) == _lib.BP_E_ARG, at
    assert L.bp_host_gens_digest(cv, g, h, C.c_size_t(0), b, bb, out) == _lib.BP_E_ARG
    assert L.bp_host_gens_digest(2, g, h, C.c_size_t(3), b, bb, out) == _lib.BP_E_ARG
    # the device calls refuse a null ctx and null outputs before they touch anything
    assert L.bp_gens_check(None, None) == _lib.BP_E_ARG
    assert L.bp_gens_digest(None, C.c_size_t(1), out) == _lib.BP_E_ARG


def test_host_only_ctx_has_no_device(E):
    from ark_bulletproofs_amd import _lib

    e = E.Engine.host_only(curve=0, gens_capacity=16)
    try:
        L, out, rep = _lib.lib(), (C.c_uint8 * 128)(), E._GensReportC()
        assert L.bp_gens_check(e.ctx, C.byref(rep)) == _lib.BP_E_NO_DEVICE
        assert L.bp_gens_check(e.ctx, None) == _lib.BP_E_ARG
        assert L.bp_gens_digest(e.ctx, C.c_size_t(4), out) == _lib.BP_E_NO_DEVICE
        assert L.bp_gens_digest(e.ctx, C.c_size_t(4), None) == _lib.BP_E_ARG
    finally:
        e.close()


def test_new_symbols_are_exported(E):
    from ark_bulletproofs_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "arkbp.h")).read()
    for name in ("bp_gens_check", "bp_gens_digest", "bp_host_gens_digest"):
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(_lib.lib(), name), name
    for name, value in (("BP_GENS_G", 0), ("BP_GENS_H", 1), ("BP_GENS_PEDERSEN", 2), ("BP_GENS_KINDS", 3)):
        assert "#define %s %d" % (name, value) in hdr
    assert (E.GENS_G, E.GENS_H, E.GENS_PEDERSEN, E.GENS_KINDS) == (0, 1, 2, 3)
    assert C.sizeof(E._GensReportC) == 9 * 8


def _build_selftest():
    exe = os.path.join(OUT, "gens_digest_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("gens_digest_selftest.cpp", "gens_digest.hpp", "host_proto.hpp", "host_math.hpp", "keccak_unrolled.inc")]
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs):
        return exe
    os.makedirs(OUT, exist_ok=True)
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", exe, srcs[0]]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        assert "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
        subprocess.check_call(base)
    return exe


def test_selftest_under_sanitizers():
    r = subprocess.run([_build_selftest()], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "gens_digest selftest ok", (r.stdout[-1000:] + r.stderr)[-3000:]
