"""A like-prover's witness from device memory, without a GPU (include/arkbp.h bp_prover_assign_multipliers_dev,
bp_witness_range_bits_dev, bp_ctx_witness_dev_stats): the handle's rules come first and are those of the host form, a host-only ctx
has no device memory, every refusal leaves the handle as it was, and the builder's argument checks run before any device use.  The
device pointers handed over here are never read: every call is refused before that."""
import ctypes as C

import pytest

import gadgets as GD
import likecommon as LC

FAKE_L, FAKE_R = C.c_void_p(0x10000), C.c_void_p(0x20000)   # stand for device memory: refused calls do not look at them


@pytest.fixture(scope="module")
def E():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import engine

    return engine


@pytest.fixture(scope="module")
def L(E):
    from ark_bulletproofs_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def hosts(E):
    out = {cv: E.Engine.host_only(curve=cv) for cv in (0, 1)}
    yield out
    for e in out.values():
        e.close()


def assign_dev(L, p, ctx, count, left=FAKE_L, right=FAKE_R):
    return L.lib().bp_prover_assign_multipliers_dev(p.h if p is not None else None, ctx, left, right, C.c_size_t(count))


def stats(L, eng):
    v = [C.c_uint64(99) for _ in range(3)]
    assert L.lib().bp_ctx_witness_dev_stats(eng.ctx, *[C.byref(x) for x in v]) == L.BP_OK
    return tuple(x.value for x in v)


def test_exports(L, hosts):
    for name in ("bp_prover_assign_multipliers_dev", "bp_witness_range_bits_dev", "bp_ctx_witness_dev_stats"):
        assert name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().bp_ctx_witness_dev_stats(None, None, None, None) == L.BP_E_ARG
    assert L.lib().bp_ctx_witness_dev_stats(hosts[0].ctx, None, None, None) == L.BP_OK      # null outputs are accepted
    a = C.c_uint64(7)
    assert L.lib().bp_ctx_witness_dev_stats(hosts[0].ctx, None, C.byref(a), None) == L.BP_OK and a.value == 0
    assert stats(L, hosts[0]) == (0, 0, 0) and hosts[0].witness_dev_stats() == (0, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_handle_rules_come_first_and_change_nothing(E, L, oracle, hosts, curve):
    F, host = GD.Field(oracle, curve), hosts[curve]
    spec = ("single", 3, 31)
    src = LC.record(E, curve, F, spec, 1)
    tw = LC.record(E, curve, F, spec, 2)
    n = src.n1
    # a null handle, a verifier handle, a self-recorded prover (src is one until the first new_like freezes it; tw stays one)
    v = E.VerifierCS(curve, LC.transcript(E))
    v.commit(src.V)
    before = (v.metrics(), tw.p.metrics(), tw.p.check())
    assert assign_dev(L, None, host.ctx, n) == L.BP_E_ARG
    assert assign_dev(L, v, host.ctx, n) == L.BP_E_ARG
    assert assign_dev(L, tw.p, host.ctx, n) == L.BP_E_ARG
    assert (v.metrics(), tw.p.metrics(), tw.p.check()) == before
    # a like-prover that already has an assignment: refused with a ctx that would otherwise give BP_E_NO_DEVICE, and with none at all
    lk = LC.like(E, src, tw)
    rep = lk.p.check()
    assert assign_dev(L, lk.p, host.ctx, n) == L.BP_E_ARG
    assert assign_dev(L, lk.p, None, n) == L.BP_E_ARG
    assert lk.p.check() == rep == tw.p.check()
    # a count that differs from the recording's
    lk = LC.like(E, src, tw, assign=False)
    for count in (n - 1, n + 1, 0):
        assert assign_dev(L, lk.p, host.ctx, count) == L.BP_E_ARG
        assert "as many values" in L.lib().bp_last_error().decode()
    # a null ctx; a null vector with count > 0
    assert assign_dev(L, lk.p, None, n) == L.BP_E_ARG
    assert assign_dev(L, lk.p, host.ctx, n, left=None) == L.BP_E_ARG
    assert assign_dev(L, lk.p, host.ctx, n, right=None) == L.BP_E_ARG
    # a valid handle on a host-only ctx: no device
    assert assign_dev(L, lk.p, host.ctx, n) == L.BP_E_NO_DEVICE
    with pytest.raises(E.ArkbpError) as ei:
        lk.p.assign_multipliers_dev(host, None, None, n)
    assert ei.value.code == L.BP_E_ARG
    assert stats(L, host) == (0, 0, 0)
    # nothing changed: still unassigned (checking it is refused), and the host form takes the witness now
    with pytest.raises(E.ArkbpError) as ei:
        lk.p.check()
    assert ei.value.code == L.BP_E_ARG and "no witness" in str(ei.value)
    lk.p.assign_multipliers(tw.left, tw.right)
    assert lk.p.check() == tw.p.check() and lk.p.check().satisfied
    assert assign_dev(L, lk.p, host.ctx, n) == L.BP_E_ARG
    # a prover on which precompute has run
    lk2 = LC.like(E, src, tw, assign=False)
    lk3 = LC.like(E, src, tw)
    lk3.p.precompute(LC.rng(3))
    assert assign_dev(L, lk3.p, host.ctx, n) == L.BP_E_ARG and "head of prove" in L.lib().bp_last_error().decode()
    assert assign_dev(L, lk2.p, host.ctx, n) == L.BP_E_NO_DEVICE
    assert stats(L, host) == (0, 0, 0)


@pytest.mark.parametrize("curve", [0, 1])
def test_count_zero_follows_the_same_order(E, L, oracle, hosts, curve):
    """a recording without phase-1 multipliers: count == 0 with null vectors passes the handle's rules and the argument checks, and
    ends at the ctx that has no device"""
    F, host = GD.Field(oracle, curve), hosts[curve]
    src = LC.record(E, curve, F, ("shuffle", 2), 4)
    lk = LC.like(E, src, src, assign=False)
    assert assign_dev(L, lk.p, host.ctx, 1) == L.BP_E_ARG
    assert assign_dev(L, lk.p, None, 0, left=None, right=None) == L.BP_E_ARG
    assert assign_dev(L, lk.p, host.ctx, 0, left=None, right=None) == L.BP_E_NO_DEVICE
    lk.p.assign_multipliers([], [])
    assert assign_dev(L, lk.p, host.ctx, 0, left=None, right=None) == L.BP_E_ARG


@pytest.mark.parametrize("curve", [0, 1])
def test_range_bits_argument_checks(L, hosts, curve):
    host = hosts[curve]

    def bits(ctx, count, nbits, vals=FAKE_L, left=FAKE_L, right=FAKE_R):
        return L.lib().bp_witness_range_bits_dev(ctx, vals, C.c_size_t(count), C.c_uint(nbits), left, right)

    assert bits(None, 1, 8) == L.BP_E_ARG
    assert bits(host.ctx, 1, 0) == L.BP_E_ARG
    assert bits(host.ctx, 1, 65) == L.BP_E_ARG
    # count * nbits at and beyond 2^31: refused before the ctx's device is asked for
    assert bits(host.ctx, 1 << 25, 64) == L.BP_E_ARG
    assert bits(host.ctx, 1 << 31, 1) == L.BP_E_ARG
    assert bits(host.ctx, (1 << 31) // 3 + 1, 3) == L.BP_E_ARG
    assert bits(host.ctx, 1 << 62, 64) == L.BP_E_ARG
    assert "2^31" in L.lib().bp_last_error().decode()
    # the largest product that passes reaches the ctx: it has no device
    assert bits(host.ctx, (1 << 25) - 1, 64) == L.BP_E_NO_DEVICE
    assert bits(host.ctx, 3, 8) == L.BP_E_NO_DEVICE
    assert bits(host.ctx, 0, 8, vals=None, left=None, right=None) == L.BP_E_NO_DEVICE


@pytest.mark.parametrize("san", ["address,undefined", "thread"], ids=["asan_ubsan", "tsan"])
def test_device_witness_state_selftest(san):
    """csrc/witness_dev_selftest.cpp, a stand-alone program: the handle's device-witness state behind fake fetch / drop hooks — one
    drop on every way out, a failed download changes nothing, a downloaded witness equals the host-assigned one"""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc, out = os.path.join(root, "ark_bulletproofs_amd", "csrc"), os.path.join(root, "ark_bulletproofs_amd", "_obj")
    exe = os.path.join(out, "witness_dev_selftest_" + san.split(",")[0])
    srcs = [os.path.join(csrc, f) for f in ("witness_dev_selftest.cpp", "prove_steps.hpp", "host_proto.hpp", "host_math.hpp", "keccak_unrolled.inc", "arkbp_params.h")]
    if not (os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs)):
        os.makedirs(out, exist_ok=True)
        base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", exe, srcs[0]]
        r = subprocess.run(base + ["-fsanitize=" + san, "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
        if r.returncode != 0:
            assert "asan" in r.stderr or "ubsan" in r.stderr or "tsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
            subprocess.check_call(base)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "witness_dev selftest ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
