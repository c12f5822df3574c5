"""bp_gens_direct_tables_check: the integrity check of the direct window tables (csrc/small.cuh k_dt_check), of the two commitment
tables (the same kernel; csrc/pedersen.cuh k_pc_table_check) and of the resident points they are anchored at (csrc/msm.cuh
k_points_on_curve), on tables that are corrupted one entry at a time.

An entry is overwritten with Engine.debug_poke at the address bp_debug_tables_ptr gives; after a poke ONLY the check runs, then the
original bytes go back and the check is seen clean again: no proof, sum or commitment ever reads a poked table.  The counts follow
from the rules include/arkbp.h states — every entry is judged by its own rule from its stored neighbours, so one wrong entry also
fails the entries derived from it.  Where a valid point is put in the wrong place the same rules are applied on the CPU, with the
oracle's point addition, to a copy of the table that carries the same replacement: that model, the closed-form count and the engine
must agree."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GENS, CAP = 16, 4
NB = 2 + 2 * CAP
W, D = 64, 15
NONE = 2**64 - 1
DIRECT, PC_DIRECT, PC_WIDE, RESIDENT = 0, 1, 2, 3
CHECKED = [NB * W * D, 2 * W * D, 2 * 32 * 256, 2 + 2 * GENS]
CLEAN = ([0, 0, 0, 0], [NONE] * 4, CHECKED)


def bG(i):
    return 2 + i


def bH(i):
    return 2 + CAP + i


def idx(b, w, d):
    """tables 4 and 5"""
    return (b * W + w) * D + d - 1


def idx6(b, w, d):
    return (b * 32 + w) * 256 + d


class Ctx:
    pass


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def T(request, oracle):
    import ark_bulletproofs_amd as A

    t = Ctx()
    t.O, t.cv = oracle, request.param
    e = t.eng = A.Engine(curve=t.cv)
    e.gens_derive(GENS)
    e.gens_direct_tables(CAP)
    FR = oracle.fid(t.cv, True)
    t.five = np.array([oracle.fe_from_int(FR, 3 + i) for i in range(5)])
    e.pedersen_commit_batch(t.five, t.five)          # tables 5 and 6 exist from here on
    Bp, Bb = oracle.pedersen_default(t.cv)
    G, H = oracle.bp_gens(t.cv, GENS)
    t.bases = np.concatenate([Bp.reshape(1, 8), Bb.reshape(1, 8), G[:CAP], H[:CAP]])
    t.tab4 = e.debug_table_points(4).reshape(NB, W, D, 8)     # clean copies, ark words: what the CPU model works on
    t.tab5 = e.debug_table_points(5).reshape(2, W, D, 8)
    t.old = e.gens_tables_check()
    assert e.gens_direct_tables_check() == CLEAN
    yield t
    assert e.gens_direct_tables_check() == CLEAN
    e.close()


@contextlib.contextmanager
def poked(T, which, index, data, clean_after=True):
    """entry `index` of table `which` holds `data` (64 raw bytes) inside the block; the original bytes are back, and the check clean
    (unless this poke lies inside another one), after it"""
    e = T.eng
    base, nbytes = e.debug_tables_ptr(which)
    assert base and (index + 1) * 64 <= nbytes
    old = e.debug_poke(base + index * 64, nbytes=64)
    data = np.asarray(data, dtype=np.uint8)
    assert data.shape == (64,) and (data != old).any()
    e.debug_poke(base + index * 64, data)
    try:
        yield
    finally:
        e.debug_poke(base + index * 64, old)
        assert (e.debug_poke(base + index * 64, nbytes=64) == old).all()
        if clean_after:
            assert e.gens_direct_tables_check() == CLEAN


def raw(T, which, index):
    base, _ = T.eng.debug_tables_ptr(which)
    return T.eng.debug_poke(base + index * 64, nbytes=64)


def model_dt(T, tab, bases, b):
    """the rules of tables 4 and 5 on the CPU for base b of `tab` (bases, windows, digits, 8 ark words): the indices that fail"""
    add, bad = T.O.point_add, []
    for w in range(W):
        for d in range(1, D + 1):
            cur = tab[b, w, d - 1]
            if d >= 2:
                exp = add(T.cv, tab[b, w, d - 2], tab[b, w, 0])
            elif w:
                exp = add(T.cv, tab[b, w - 1, D - 1], tab[b, w - 1, 0])
            else:
                exp = bases[b]
            if not cur.any() or (cur != exp).any():
                bad.append(idx(b, w, d))
    return bad


def replaced(T, which, dst, src, closed_form, other_clean=()):
    """entry dst = (b, w, d) of table 4 / 5 overwritten with the bytes of entry src: model, closed form and engine agree"""
    kind = DIRECT if which == 4 else PC_DIRECT
    tab = (T.tab4 if which == 4 else T.tab5).copy()
    tab[dst[0], dst[1], dst[2] - 1] = tab[src[0], src[1], src[2] - 1]
    model = model_dt(T, tab, T.bases, dst[0])
    assert len(model) == closed_form and min(model) == idx(*dst)
    with poked(T, which, idx(*dst), raw(T, which, idx(*src))):
        bad, first, checked = T.eng.gens_direct_tables_check()
    exp_bad, exp_first = [0] * 4, [NONE] * 4
    exp_bad[kind], exp_first[kind] = closed_form, idx(*dst)
    assert (bad, first, checked) == (exp_bad, exp_first, CHECKED)
    return model


# ---- 1: clean tables ----------------------------------------------------------------------------------------------------------------------
def test_clean_tables(T):
    e = T.eng
    bad, first, checked = e.gens_direct_tables_check()
    assert bad == [0, 0, 0, 0] and first == [NONE] * 4
    assert checked == [9600, 1920, 16384, 34]
    assert e.gens_tables_check() == T.old == (0, 0)
    # the CPU model of the rules finds the clean tables clean too (a G base and B_blinding of table 5)
    assert model_dt(T, T.tab4, T.bases, bG(1)) == [] and model_dt(T, T.tab5, T.bases, 1) == []


# ---- 2 .. 5, 8: a valid point in the wrong place ----------------------------------------------------------------------------------------------
def test_middle_digit(T):
    """itself and the next digit, which is derived from it"""
    model = replaced(T, 4, (bG(1), 17, 7), (bG(1), 17, 9), 2)
    assert model == [idx(bG(1), 17, 7), idx(bG(1), 17, 8)]


def test_unit_entry(T):
    """a window's unit: itself, the 14 digits of the window that add it, and the next window's unit"""
    model = replaced(T, 4, (bH(3), 5, 1), (bH(3), 5, 2), 16)
    assert model == [idx(bH(3), 5, d) for d in range(1, 16)] + [idx(bH(3), 6, 1)]


def test_last_digit_of_a_window(T):
    """d = 15 of the last window is nobody's neighbour; that of window 62 is the next unit's.  Bases 0 and 1 of table 4 and table 5
    hold the same points, and a poke of table 4 leaves table 5 clean (replaced() asserts that every other kind stays at 0)"""
    assert (raw(T, 4, idx(1, 63, 15)) == raw(T, 5, idx(1, 63, 15))).all()
    assert replaced(T, 4, (1, 63, 15), (1, 63, 14), 1) == [idx(1, 63, 15)]
    assert replaced(T, 4, (0, 62, 15), (0, 62, 14), 2) == [idx(0, 62, 15), idx(0, 63, 1)]


def test_anchor(T):
    model = replaced(T, 4, (bG(0), 0, 1), (bG(0), 0, 2), 16)
    assert model[0] == (2 * 64 + 0) * 15 and model[-1] == idx(bG(0), 1, 1)


def test_table_5(T):
    model = replaced(T, 5, (1, 9, 2), (1, 9, 3), 2)
    assert model == [idx(1, 9, 2), idx(1, 9, 3)]


# ---- 6: garbage ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["bit", "zeros", "ones"])
def test_garbage_is_counted_and_nothing_else(T, what):
    """a flipped bit in y (off the curve), all-zero words (the identity's encoding) and all-ones words (no canonical coordinates) at
    (G[2], w = 30, d = 5): the call returns, the entry and the digit derived from it are counted, every other kind stays at 0"""
    at = idx(bG(2), 30, 5)
    data = raw(T, 4, at)
    if what == "bit":
        data[32 + 11] ^= 0x10
    else:
        data[:] = 0 if what == "zeros" else 0xFF
    with poked(T, 4, at, data):
        bad, first, checked = T.eng.gens_direct_tables_check()
    assert bad == [2, 0, 0, 0] and first == [at, NONE, NONE, NONE] and checked == CHECKED


# ---- 7: the 8-bit commitment tables ------------------------------------------------------------------------------------------------------
def test_table_6(T):
    """d = 0 must be the all-zero identity (it is nobody's neighbour); the last digit of the last window is nobody's neighbour either;
    a middle digit fails with the one derived from it, a unit with its whole window and the next unit"""
    e = T.eng
    for dst, src, count in [((1, 3, 0), (1, 3, 1), 1), ((1, 31, 255), (1, 31, 254), 1), ((0, 7, 100), (0, 7, 99), 2), ((0, 12, 1), (0, 12, 2), 256)]:
        with poked(T, 6, idx6(*dst), raw(T, 6, idx6(*src))):
            bad, first, checked = e.gens_direct_tables_check()
        assert bad[PC_WIDE] >= 1 and first[PC_WIDE] == idx6(*dst), (dst, bad, first)
        assert bad == [0, 0, count, 0] and first == [NONE, NONE, idx6(*dst), NONE] and checked == CHECKED, (dst, bad, first)
    zeros = np.zeros(64, dtype=np.uint8)
    with poked(T, 6, idx6(0, 20, 77), zeros):          # an identity where a point belongs: itself and d = 78
        assert e.gens_direct_tables_check()[0] == [0, 0, 2, 0]


# ---- 9: the resident points ----------------------------------------------------------------------------------------------------------------
def flipped(data):
    data = data.copy()
    data[32] ^= 1          # y -> y +- 1: canonical still (but for one y in 2^255), and off the curve
    return data


def test_resident_points(T):
    e = T.eng
    with poked(T, 8, 2, flipped(raw(T, 8, 2))):        # G[2], within the tables' reach: its anchor fails too
        bad, first, _ = e.gens_direct_tables_check()
        assert bad == [1, 0, 0, 1] and first == [idx(bG(2), 0, 1), NONE, NONE, 2 + 2]
    with poked(T, 9, 10, flipped(raw(T, 9, 10))):      # H[10], beyond it
        bad, first, _ = e.gens_direct_tables_check()
        assert bad == [0, 0, 0, 1] and first == [NONE, NONE, NONE, 2 + GENS + 10]
    with poked(T, 7, 1, flipped(raw(T, 7, 1))):        # B_blinding: the anchor of all three tables
        bad, first, _ = e.gens_direct_tables_check()
        assert bad == [1, 1, 1, 1] and first == [idx(1, 0, 1), idx(1, 0, 1), idx6(1, 0, 1), 1]
    with poked(T, 8, 5, np.zeros(64, dtype=np.uint8)):  # the identity is no generator
        assert e.gens_direct_tables_check()[0] == [0, 0, 0, 1]
    # THE BLIND SPOT: two on-curve generators swapped are two points of the curve; only the tables' anchors notice
    g0, g1 = raw(T, 8, 0), raw(T, 8, 1)
    with poked(T, 8, 0, g1):
        with poked(T, 8, 1, g0, clean_after=False):
            bad, first, checked = e.gens_direct_tables_check()
            assert bad == [2, 0, 0, 0] and first == [idx(bG(0), 0, 1), NONE, NONE, NONE] and checked == CHECKED
        # (the inner block has put G[1] back: G[0] == G[1] now, one anchor fails)
        assert e.gens_direct_tables_check()[0] == [1, 0, 0, 0]


# ---- 10: tables that are not built -----------------------------------------------------------------------------------------------------
def test_tables_not_built(T):
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=T.cv)
    try:
        assert e.gens_direct_tables_check() == ([0, 0, 0, 0], [NONE] * 4, [0, 0, 0, 0])
        e.gens_derive(GENS)
        assert e.gens_direct_tables_check() == ([0, 0, 0, 0], [NONE] * 4, [0, 0, 0, 2 + 2 * GENS])
        assert e.debug_tables_ptr(4) == (None, 0)      # the check has built nothing
        assert e.debug_tables_ptr(5) == (None, 0) and e.debug_tables_ptr(6) == (None, 0)
    finally:
        e.close()


# ---- 11: a ctx that shares the generators ------------------------------------------------------------------------------------------------
def test_sharing(T):
    """the sharer looks at the owner's points and direct tables through its view (tables 5 and 6 are each ctx's own: it has them from
    a commitment batch of its own)"""
    import ark_bulletproofs_amd as A

    o = A.Engine(curve=T.cv)
    try:
        o.share_gens_from(T.eng)
        assert o.gens_direct_tables_check() == ([0, 0, 0, 0], [NONE] * 4, [CHECKED[0], 0, 0, CHECKED[3]])
        o.pedersen_commit_batch(T.five, T.five)
        assert o.debug_tables_ptr(4) == T.eng.debug_tables_ptr(4) and o.debug_tables_ptr(8) == T.eng.debug_tables_ptr(8)
        assert o.gens_direct_tables_check() == T.eng.gens_direct_tables_check() == CLEAN
        at = idx(bG(1), 17, 7)
        with poked(T, 4, at, raw(T, 4, idx(bG(1), 17, 9))):
            mine = T.eng.gens_direct_tables_check()
            assert o.gens_direct_tables_check() == mine == ([2, 0, 0, 0], [at, NONE, NONE, NONE], CHECKED)
        assert o.gens_direct_tables_check() == CLEAN
    finally:
        o.close()
