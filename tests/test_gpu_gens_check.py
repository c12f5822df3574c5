"""bp_gens_check and bp_gens_digest (include/arkbp.h): the resident generators pinned — the anchors that bp_gens_tables_check and
bp_gens_direct_tables_check take for granted.

Capacity 300 = one full workgroup of 256 lanes and 44 lanes of a second one, so index 299 is the last live lane of the last
workgroup; the digest sizes 255 / 256 / 257 straddle a workgroup and 3, 255, 257, 300 make odd levels (a node carried up).  Entries are
corrupted in device memory as tests/test_gpu_tables_check.py does it (the address from bp_debug_tables_ptr, bp_dev_download /
bp_dev_upload); after a poke only the checks and the digest run, then the original bytes go back and the check is seen clean again.
The digest's reference is tests/gens_digest_common.py (hashlib.sha3_256 over the definition), and the library's host twin."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import gens_digest_common as D

pytestmark = pytest.mark.gpu

CAP = 300
NONE = 2**64 - 1
G_, H_, PC_ = 0, 1, 2
CLEAN = ((CAP, CAP, 2), (0, 0, 0), (NONE, NONE, NONE))
PAIR_PARTY = 0x50434731      # the custom pair: the first two points of another party's 'G' chain (points of the curve, no known relation)


class Ctx:
    pass


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def T(request):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E

    t = Ctx()
    t.A, t.E, t.cv = A, E, request.param
    e = t.eng = A.Engine(curve=t.cv)
    e.gens_derive(CAP)
    t.G, t.H = e.gens_download(CAP)                  # the reference of the digests: downloaded once, never changed
    t.B, t.Bb, dflt = e.pedersen_gens()
    assert dflt
    assert e.gens_check().astuple() == CLEAN
    yield t
    assert e.gens_check().astuple() == CLEAN
    e.close()


def raw(eng, which, index):
    base, _ = eng.debug_tables_ptr(which)
    return eng.debug_poke(base + index * 64, nbytes=64)


@contextlib.contextmanager
def poked(eng, which, index, data):
    """entry `index` of resident table `which` (7: the pair, 8: G, 9: H) holds `data` (64 raw bytes) inside the block"""
    base, nbytes = eng.debug_tables_ptr(which)
    assert base and (index + 1) * 64 <= nbytes
    old = eng.debug_poke(base + index * 64, nbytes=64)
    data = np.asarray(data, dtype=np.uint8)
    assert data.shape == (64,) and (data != old).any()
    eng.debug_poke(base + index * 64, data)
    try:
        yield
    finally:
        eng.debug_poke(base + index * 64, old)
        assert (eng.debug_poke(base + index * 64, nbytes=64) == old).all()


@contextlib.contextmanager
def swapped_g5_g6(eng):
    g5, g6 = raw(eng, 8, 5), raw(eng, 8, 6)
    with poked(eng, 8, 5, g6), poked(eng, 8, 6, g5):
        yield


def custom_pair(T):
    p = T.E.host_derive_generators(T.cv, 0, PAIR_PARTY, 2)
    return p[0].copy(), p[1].copy()


# ---- bp_gens_check -----------------------------------------------------------------------------------------------------------------
def test_fresh_chain_is_clean(T):
    r = T.eng.gens_check()
    assert r.checked == (300, 300, 2) and r.bad == (0, 0, 0) and r.first_bad == (NONE, NONE, NONE) and r.clean
    # the resident points are the host's chain too (bp_host_derive_generators shares no code with the GPU's square roots)
    assert (T.G == T.E.host_derive_generators(T.cv, False, 0, CAP)).all() and (T.H == T.E.host_derive_generators(T.cv, True, 0, CAP)).all()


def test_swapped_generators(T):
    e = T.eng
    assert e.debug_tables_ptr(4) == (None, 0)        # no direct tables on this ctx: nothing anchors G
    with swapped_g5_g6(e):
        # THE BLIND SPOT this call closes: two points of the curve are two points of the curve
        bad, first, checked = e.gens_direct_tables_check()
        assert bad[3] == 0 and first[3] == NONE and checked[3] == 2 + 2 * CAP
        r = e.gens_check()
        assert r.checked == (CAP, CAP, 2) and r.bad == (2, 0, 0) and r.first_bad == (5, NONE, NONE) and not r.clean
    assert e.gens_check().astuple() == CLEAN


def test_replaced_last_entry(T):
    """H[299] is the last live lane of the second workgroup; G[0] is a valid point in the wrong place"""
    e = T.eng
    with poked(e, 9, CAP - 1, raw(e, 8, 0)):
        r = e.gens_check()
        assert r.checked == (CAP, CAP, 2) and r.bad == (0, 1, 0) and r.first_bad == (NONE, CAP - 1, NONE)
    with poked(e, 9, 0, raw(e, 8, 0)), poked(e, 8, 255, raw(e, 8, 256)), poked(e, 8, 256, raw(e, 8, 257)):   # both sides of a workgroup's edge
        r = e.gens_check()
        assert r.bad == (2, 1, 0) and r.first_bad == (255, 0, NONE)
    assert e.gens_check().astuple() == CLEAN


def test_extended_chain(T):
    e = T.A.Engine(curve=T.cv)
    try:
        e.gens_derive(300)
        e.gens_derive(700)
        r = e.gens_check()
        assert r.checked == (700, 700, 2) and r.bad == (0, 0, 0) and r.first_bad == (NONE, NONE, NONE)
        G, H = e.gens_download(300)
        assert (G == T.G).all() and (H == T.H).all()
        with poked(e, 8, 699, raw(e, 9, 699)):
            r = e.gens_check()
            assert r.bad == (1, 0, 0) and r.first_bad == (699, NONE, NONE)
    finally:
        e.close()


def test_chain_longer_than_one_chunk(T):
    """the walk takes 2^16 attempts at a time and about half of them are points: 40000 generators need a second chunk, whose entries
    are compared at indices that continue where the first chunk's stopped; the digest's tree has 16 levels, several of them odd"""
    big = 40000
    e = T.A.Engine(curve=T.cv)
    try:
        e.gens_derive(big)
        clean = ((big, big, 2), (0, 0, 0), (NONE, NONE, NONE))
        assert e.gens_check().astuple() == clean
        with poked(e, 8, big - 1, raw(e, 8, 0)), poked(e, 9, 35001, raw(e, 9, 35000)):
            r = e.gens_check()
            assert r.bad == (1, 1, 0) and r.first_bad == (big - 1, 35001, NONE)
        assert e.gens_check().astuple() == clean
        G, H = e.gens_download(big)
        assert (G[:CAP] == T.G).all() and (H[:CAP] == T.H).all()
        assert e.gens_digest() == T.E.host_gens_digest(T.cv, G, H, T.B, T.Bb)
    finally:
        e.close()


def test_caller_installed_generators(T):
    """the chain is not their truth: nothing to compare G and H with, the pair still is; a swap goes unseen HERE and the digest sees it"""
    e = T.A.Engine(curve=T.cv)
    try:
        e.gens_upload(T.G, T.H)
        r = e.gens_check()
        assert r.checked == (0, 0, 2) and r.bad == (0, 0, 0) and r.first_bad == (NONE, NONE, NONE)
        v = T.A.Engine(curve=T.cv)
        try:
            v.share_gens_from(e)
            assert v.gens_check() == r
        finally:
            v.close()
        with swapped_g5_g6(e):
            assert e.gens_check() == r
            assert e.gens_digest().G != T.eng.gens_digest().G
        e.gens_derive(CAP)                           # derived again: the chain is the truth again
        assert e.gens_check().astuple() == CLEAN
    finally:
        e.close()


def test_custom_pedersen_pair(T):
    e = T.A.Engine(curve=T.cv)
    try:
        e.gens_derive(16)
        B, Bb = custom_pair(T)
        e.pedersen_gens_install(B, Bb)
        clean = ((16, 16, 2), (0, 0, 0), (NONE, NONE, NONE))
        assert e.gens_check().astuple() == clean
        for index in (1, 0):
            data = raw(e, 7, index)
            data[8] ^= 1                             # one word of table 7
            with poked(e, 7, index, data):
                r = e.gens_check()
                assert r.checked == (16, 16, 2) and r.bad == (0, 0, 1) and r.first_bad == (NONE, NONE, index)
        with poked(e, 7, 0, raw(e, 7, 1)):           # B_blinding in B's place
            assert e.gens_check().bad == (0, 0, 1)
        assert e.gens_check().astuple() == clean
        e.pedersen_gens_install()                    # back to the default pair
        assert e.gens_check().astuple() == clean
    finally:
        e.close()


def test_view_reports_what_the_owner_reports(T):
    v = T.A.Engine(curve=T.cv)
    try:
        v.share_gens_from(T.eng)
        assert v.gens_check() == T.eng.gens_check() and v.gens_check().astuple() == CLEAN
        with swapped_g5_g6(T.eng):
            mine = T.eng.gens_check()
            assert v.gens_check() == mine and mine.bad == (2, 0, 0) and mine.first_bad == (5, NONE, NONE)
        assert v.gens_check().astuple() == CLEAN
    finally:
        v.close()


def test_check_error_codes(T):
    from ark_bulletproofs_amd import _lib

    L, rep = _lib.lib(), T.E._GensReportC()
    h = T.A.Engine.host_only(curve=T.cv, gens_capacity=16)
    e = T.A.Engine(curve=T.cv)
    try:
        assert L.bp_gens_check(h.ctx, C.byref(rep)) == _lib.BP_E_NO_DEVICE
        assert L.bp_gens_check(e.ctx, C.byref(rep)) == _lib.BP_E_GENS_LENGTH      # no generators installed
        assert L.bp_gens_check(e.ctx, None) == _lib.BP_E_ARG and L.bp_gens_check(None, C.byref(rep)) == _lib.BP_E_ARG
    finally:
        h.close()
        e.close()


# ---- bp_gens_digest ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 300])
def test_digest_equals_host_twin_and_restatement(T, n):
    got = T.eng.gens_digest(n)
    assert got == T.E.host_gens_digest(T.cv, T.G, T.H, T.B, T.Bb, n=n)
    assert tuple(got) == D.digest(T.cv, T.G, T.H, n, T.B, T.Bb)


def test_digest_defaults_to_the_capacity(T):
    assert T.eng.gens_digest() == T.eng.gens_digest(CAP)


def test_derived_uploaded_and_view_agree(T):
    want = T.eng.gens_digest()
    u, v = T.A.Engine(curve=T.cv), T.A.Engine(curve=T.cv)
    try:
        u.gens_upload(T.G, T.H)
        v.share_gens_from(T.eng)
        assert u.gens_digest() == want and v.gens_digest() == want
        assert v.gens_digest(257) == T.eng.gens_digest(257)
    finally:
        u.close()
        v.close()


def test_digest_sees_the_swap(T):
    base = T.eng.gens_digest()
    v = T.A.Engine(curve=T.cv)
    try:
        v.share_gens_from(T.eng)
        with swapped_g5_g6(T.eng):
            sw = T.eng.gens_digest()
            assert sw.root != base.root and sw.G != base.G and sw.H == base.H and sw.pair == base.pair
            assert v.gens_digest() == sw
            Gs = T.G.copy()
            Gs[[5, 6]] = Gs[[6, 5]]
            assert tuple(sw) == D.digest(T.cv, Gs, T.H, CAP, T.B, T.Bb)
            assert T.eng.gens_digest(5) == T.E.host_gens_digest(T.cv, T.G, T.H, T.B, T.Bb, n=5)    # a prefix that ends before the swap
    finally:
        v.close()
    assert T.eng.gens_digest() == base


def test_custom_pair_changes_the_pair_root_only(T):
    e = T.A.Engine(curve=T.cv)
    try:
        e.gens_derive(CAP)
        base = e.gens_digest()
        assert base == T.eng.gens_digest()
        B, Bb = custom_pair(T)
        e.pedersen_gens_install(B, Bb)
        got = e.gens_digest()
        assert got.root != base.root and got.pair != base.pair and got.G == base.G and got.H == base.H
        assert tuple(got) == D.digest(T.cv, T.G, T.H, CAP, B, Bb)
        hB, hBb, dflt = e.pedersen_gens()
        assert not dflt and got == T.E.host_gens_digest(T.cv, T.G, T.H, hB, hBb)
    finally:
        e.close()


def test_digest_error_codes(T):
    from ark_bulletproofs_amd import _lib

    L, out = _lib.lib(), (C.c_uint8 * 128)()
    ctx = T.eng.ctx
    assert L.bp_gens_digest(ctx, C.c_size_t(CAP), out) == _lib.BP_OK
    assert L.bp_gens_digest(ctx, C.c_size_t(CAP + 1), out) == _lib.BP_E_GENS_LENGTH
    assert L.bp_gens_digest(ctx, C.c_size_t(0), out) == _lib.BP_E_ARG
    assert L.bp_gens_digest(ctx, C.c_size_t(CAP), None) == _lib.BP_E_ARG
    h = T.A.Engine.host_only(curve=T.cv, gens_capacity=16)
    e = T.A.Engine(curve=T.cv)
    try:
        assert L.bp_gens_digest(h.ctx, C.c_size_t(4), out) == _lib.BP_E_NO_DEVICE
        assert L.bp_gens_digest(e.ctx, C.c_size_t(1), out) == _lib.BP_E_GENS_LENGTH       # no generators installed
    finally:
        h.close()
        e.close()
