"""The direct window tables T[base][w][d - 1] = d * 16^w * base (csrc/small.cuh) entry by entry, the two Pedersen tables beside them
(pc_dt: the same layout for B, B_blinding; pc_table: d * 256^w * base, csrc/pedersen.cuh), and the kernels that sum over them —
k_dt_accum / k_dt_finish through the prover's own msm_direct (bp_debug_msm_direct), k_dt_commit and k_pc_commit through
bp_pedersen_commit_batch — against the oracle's double-and-add, bit for bit.

Whole proofs select table entries by whatever digits the protocol produces; on zorro (r = 2^255 - 19) a reduced scalar never has a
top 4-bit digit above 7 (nor a top byte above 127), so those entries are built, are read for canonical integers >= r
(DtSeg::resident = 0), and no proof ever looks at them.  Here every entry is compared and every entry is selected."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP = 65                     # G[64] and H[64] are a one-lane second workgroup of k_dt_window_bases; the G | H boundary (entry 67 * 960)
NB = 2 + 2 * CAP             # is no multiple of k_dt_entries' 256 lanes
W, D = 64, 15
K_MSM_ACCUM = 0              # BP_K_MSM_ACCUM: msm_direct_launch times k_dt_accum (+ k_dt_finish) as one region


def bG(i):
    return 2 + i


def bH(i):
    return 2 + CAP + i


FULL_BASES = [0, 1, bG(0), bG(63), bG(64), bH(0), bH(63), bH(64)]
SAMPLES = [(0, 1), (0, 15), (31, 8), (63, 1), (63, 15)]


class Tables:
    pass


@pytest.fixture(scope="module", params=[0, 1], ids=["secq256k1", "zorro"])
def T(request, oracle):
    import ark_bulletproofs_amd as A

    t = Tables()
    t.O, t.cv = oracle, request.param
    t.FR = oracle.fid(t.cv, True)
    t.r = oracle.modulus(t.FR)
    e = t.eng = A.Engine(curve=t.cv)
    e.gens_derive(128)
    assert e.debug_tables_ptr(4) == (None, 0)
    t.dt_bytes = e.gens_direct_tables(CAP)
    Bp, Bb = oracle.pedersen_default(t.cv)
    G, H = oracle.bp_gens(t.cv, 128)
    t.bases = np.concatenate([Bp.reshape(1, 8), Bb.reshape(1, 8), G[:CAP], H[:CAP]])
    t.tab = e.debug_table_points(4).reshape(NB, W, D, 8)
    # the Pedersen tables exist after the first commitment batch (pedersen_ensure)
    t.pc_before = (e.debug_tables_ptr(5), e.debug_tables_ptr(6))
    one = np.array([oracle.fe_from_int(t.FR, 77)])
    assert (e.pedersen_commit_batch(one, one)[0] == oracle.pedersen_commit(t.cv, one[0], one[0])).all()
    t.pc_dt = e.debug_table_points(5).reshape(2, W, D, 8)
    t.pc_table = e.debug_table_points(6).reshape(2, 32, 256, 8)
    yield t
    e.close()


# ---- helpers ------------------------------------------------------------------------------------------------------------------------
def canon(k):
    return np.array([(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def canons(ks):
    return np.array([canon(k) for k in ks], dtype=np.uint64).reshape(-1, 4)


def monts(T, ks):
    return np.array([T.O.fe_from_int(T.FR, k % T.r) for k in ks], dtype=np.uint64).reshape(-1, 4)


def smul(T, P, k):
    """(k mod r) * P by the oracle; the identity is all-zero words"""
    k %= T.r
    if k == 0:
        return np.zeros(8, dtype=np.uint64)
    return T.O.scalar_mul(T.cv, P, T.O.fe_from_int(T.FR, k))


def msm_ref(T, idx, ks):
    """sum of (k mod r) * base[i] over the pairs; all-zero for the identity"""
    pairs = [(i, k % T.r) for i, k in zip(idx, ks) if k % T.r]
    if not pairs:
        return np.zeros(8, dtype=np.uint64)
    return T.O.msm(T.cv, T.bases[[i for i, _ in pairs]], monts(T, [k for _, k in pairs]))


def rand_ints(T, tag, n):
    """n distinct non-zero reduced scalars"""
    ks = [T.O.fe_to_int(T.FR, x) for x in T.O.fe_rand(T.FR, bytes([tag, T.cv]) + bytes(30), n)]
    assert len(set(ks)) == n and all(ks)
    return ks


def seg(T, base0, ks, fmt=0, fold_n=0, fold_hi=0, count=None):
    """one run over consecutive bases; ks: one integer per ELEMENT.  format 0 takes them as they are, 1 and 2 as ark words of k mod r"""
    return (base0, len(ks) if count is None else count, fmt, fold_n, fold_hi, canons(ks) if fmt == 0 else monts(T, ks))


def same(got, exp):
    got, exp = np.asarray(got).reshape(-1, 8), np.asarray(exp).reshape(-1, 8)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert not len(bad), "%d of %d points differ, first at %s" % (len(bad), len(got), bad[:8])


def sample_entries(T, tab, bases):
    exp = np.array([smul(T, bases[b], d << (4 * w)) for b in range(len(bases)) for w, d in SAMPLES])
    got = np.array([tab[b, w, d - 1] for b in range(len(bases)) for w, d in SAMPLES])
    same(got, exp)


# ---- 1 .. 3: the tables themselves ----------------------------------------------------------------------------------------------------
def test_dt_tab_entry_by_entry(T):
    """every entry of eight bases (the Pedersen pair; first, last of the first workgroup and the lone lane of the second for G and H)
    and five entries of all 132, against (d << 4w) mod r times the base; no entry is the identity"""
    assert T.dt_bytes == NB * 64 * 15 * 64
    assert T.eng.debug_tables_ptr(4)[1] == T.dt_bytes and T.eng.direct_stats()[1] == CAP
    assert T.tab.reshape(-1, 8).any(axis=1).all()
    for b in FULL_BASES:
        exp = np.array([smul(T, T.bases[b], d << (4 * w)) for w in range(W) for d in range(1, D + 1)])
        same(T.tab[b], exp)
    sample_entries(T, T.tab, T.bases)


def test_pc_dt_is_the_head_of_dt_tab(T):
    """bases 0 and 1 of pc_dt and of dt_tab are the same resident bytes (both come from k_dt_window_bases + k_dt_entries)"""
    assert T.pc_before == ((None, 0), (None, 0))
    e = T.eng
    p4, _ = e.debug_tables_ptr(4)
    p5, n5 = e.debug_tables_ptr(5)
    assert n5 == 2 * W * D * 64 and p5 != p4
    assert (e.debug_poke(p5, nbytes=n5) == e.debug_poke(p4, nbytes=n5)).all()
    same(T.pc_dt, T.tab[:2])


def test_pc_table_in_full(T):
    """all 2 x 32 x 256 entries d * 256^w * base of k_pc_table_build; d = 0 is the identity"""
    assert T.eng.debug_tables_ptr(6)[1] == 2 * 32 * 256 * 64
    assert not T.pc_table[:, :, 0].any()
    assert T.pc_table[:, :, 1:].reshape(-1, 8).any(axis=1).all()
    for b in range(2):
        exp = np.array([smul(T, T.bases[b], d << (8 * w)) for w in range(32) for d in range(256)])
        same(T.pc_table[b], exp)


# ---- 4 .. 9: k_dt_accum / k_dt_finish through msm_direct ------------------------------------------------------------------------------
def test_every_entry_is_selected_by_its_digit(T):
    """a one-term job with the canonical integer d << 4w returns exactly entry (w, d) — for all 960 of one G and one H base, six jobs
    per call.  On zorro 15 << 252 .. 8 << 252 are >= r: the entries no reduced scalar selects"""
    for b in (bG(64), bH(64)):
        wd = [(w, d) for w in range(W) for d in range(1, D + 1)]
        got = []
        for lo in range(0, len(wd), 6):
            got.append(T.eng.debug_msm_direct([([seg(T, b, [d << (4 * w)])], None) for w, d in wd[lo:lo + 6]]))
        got = np.concatenate(got).reshape(W, D, 8)
        same(got, T.tab[b])
        same(got[63], np.array([smul(T, T.bases[b], d << 252) for d in range(1, D + 1)]))
    if T.cv == 1:
        assert (8 << 252) >= T.r > (7 << 252)


def test_scalar_formats_agree(T):
    """canonical integers (0), ark words imported to the resident form (1), ark words read in place (2): one job of three runs over
    [B, B_blinding, G[0..4)], G[58..65), H[57..65) with 0, 1, r - 1 and the all-fifteens integer in every run"""
    r, ones = T.r, (1 << 256) - 1     # sum of 15 << 4w: >= r, taken digit by digit in format 0 and reduced by the caller otherwise
    rnd = rand_ints(T, 31, 9)
    runs = [(0, [0, 1, r - 1, ones, rnd[0], rnd[1]]), (bG(58), [rnd[2], ones, 0, 1, r - 1, rnd[3], rnd[4]]),
            (bH(57), [r - 1, rnd[5], rnd[6], rnd[7], ones, 1, 0, rnd[8]])]
    idx = [b0 + i for b0, ks in runs for i in range(len(ks))]
    exp = msm_ref(T, idx, [k for _, ks in runs for k in ks])
    assert idx[-1] == NB - 1 and exp.any()
    for fmt in (0, 1, 2):
        same(T.eng.debug_msm_direct([([seg(T, b0, ks, fmt) for b0, ks in runs], None)]), exp)
    # ... and one format per run in the same job
    same(T.eng.debug_msm_direct([([seg(T, b0, ks, fmt) for fmt, (b0, ks) in enumerate(runs)], None)]), exp)


def test_segments_and_immediate_term(T):
    """0 .. 3 runs, with and without the immediate term (on B_blinding, on an H base): the terms on either side of every run boundary
    carry distinct non-zero scalars, so a term decoded into the wrong run, or off by one, changes the sum.  Six jobs in one call, then
    each alone"""
    k = rand_ints(T, 41, 64)
    im = rand_ints(T, 42, 4)
    c0, c1, c2 = 5, 7, 3
    jobs = [
        ([], (1, im[0]), [1], [im[0]]),
        ([], (bH(64), T.r - 1), [bH(64)], [T.r - 1]),
        ([(bG(3), k[0:c0], 0)], None, [], []),
        ([(bG(3), k[5:5 + c0], 1), (bH(3), k[10:10 + c1], 0)], (1, im[1]), [1], [im[1]]),
        ([(bG(60), k[17:17 + c0], 0), (bH(0), k[22:22 + c1], 1), (0, k[29:29 + c2], 2)], (bH(7), im[2]), [bH(7)], [im[2]]),
        ([(bH(62), k[32:32 + c2], 2), (bG(0), k[35:35 + c0], 2), (bG(5), k[40:40 + c1], 0)], None, [], []),
    ]
    calls, exps = [], []
    for runs, imm, ib, ik in jobs:
        calls.append(([seg(T, b0, ks, fmt) for b0, ks, fmt in runs], imm))
        idx = ib + [b0 + i for b0, ks, _ in runs for i in range(len(ks))]
        exps.append(msm_ref(T, idx, ik + [x for _, ks, _ in runs for x in ks]))
    exps = np.array(exps)
    assert len({tuple(p) for p in exps}) == 6 and exps.any(axis=1).all()
    same(T.eng.debug_msm_direct(calls), exps)
    for c, p in zip(calls, exps):
        same(T.eng.debug_msm_direct([c]), p)


@pytest.mark.parametrize("fold_hi", [0, 1])
def test_fold_remapping(T, fold_hi):
    """DtSeg::fold_n: term j of a run stands for element (j // n) * 2n + j % n + (n if fold_hi else 0), as
    test_host_logic.py::test_direct_table_round_visits_exactly_the_bases_with_nonzero_scalars states it.  Sixteen consecutive bases of G
    take one half, the same sixteen of H the other (a round's L or R); every element carries a non-zero scalar, visited or not"""
    n0, cnt = 16, 8
    jobs, exps = [], []
    for n in (1, 2, 4, 8):
        kg, kh = rand_ints(T, 50 + n, n0), rand_ints(T, 60 + n, n0)

        def visited(hi):
            return [(j // n) * 2 * n + j % n + (n if hi else 0) for j in range(cnt)]
        vg, vh = visited(fold_hi), visited(not fold_hi)
        assert sorted(vg + vh) == list(range(n0))
        jobs.append(([seg(T, bG(40), kg, 1, n, fold_hi, cnt), seg(T, bH(40), kh, 0, n, 1 - fold_hi, cnt)], None))
        exps.append(msm_ref(T, [bG(40) + t for t in vg] + [bH(40) + t for t in vh], [kg[t] for t in vg] + [kh[t] for t in vh]))
    same(T.eng.debug_msm_direct(jobs), np.array(exps))


def test_launch_regimes(T):
    """msm_direct_launch: ceil(terms / 4) workgroups per sum — one (its point is the result), 2 and 16 (the host adds the partial
    points), 17 (k_dt_finish adds them); and six sums of 172 terms, where 43 workgroups each would exceed 256 and 22 take two units
    per quad.  Every call is ONE timed region of BP_K_MSM_ACCUM (k_dt_finish runs inside it), so the hook's count of workgroups tells
    the regimes apart where the timer cannot"""
    e = T.eng
    e.set_profiling(True)
    try:
        for terms, nblk in [(4, 1), (5, 2), (64, 16), (65, 17)]:
            ks = rand_ints(T, 70 + terms, terms)
            e.reset_profiling()
            got, wgs = e.debug_msm_direct([([seg(T, bG(0), ks[1:], 2)], (1, ks[0]))], with_workgroups=True)
            assert e.kernel_time(K_MSM_ACCUM)[1] == 1 and wgs == nblk
            same(got, msm_ref(T, [1] + [bG(i) for i in range(terms - 1)], ks))
        ks = rand_ints(T, 79, 6 * 172)
        runs = [(bG(0), 65), (bH(0), 65), (bG(23), 42)]   # all of G, all of H, the tail of G once more
        idx = [b0 + i for b0, c in runs for i in range(c)]
        jobs, exps = [], []
        for j in range(6):
            kj, segs, lo = ks[172 * j:172 * (j + 1)], [], 0
            for s, (b0, c) in enumerate(runs):
                segs.append(seg(T, b0, kj[lo:lo + c], (j + s) % 3))
                lo += c
            jobs.append((segs, None))
            exps.append(msm_ref(T, idx, kj))
        e.reset_profiling()
        got, wgs = e.debug_msm_direct(jobs, with_workgroups=True)
        assert e.kernel_time(K_MSM_ACCUM)[1] == 1 and wgs == 22
        same(got, np.array(exps))
        # five such sums stay below 256 workgroups: 43 each
        got, wgs = e.debug_msm_direct(jobs[:5], with_workgroups=True)
        assert wgs == 43
        same(got, np.array(exps[:5]))
    finally:
        e.set_profiling(False)


def test_exceptional_operands_of_the_additions(T):
    """equal and opposite points meeting in the quad tree (slots j and j + 16 of a two-term job hold the same units of the two
    terms) and in the host's sum of two workgroups' points, zero scalars, runs that cancel"""
    r = T.r
    s, k5, k4 = rand_ints(T, 81, 1)[0], rand_ints(T, 82, 5), rand_ints(T, 83, 4)
    lone = sum(1 << (16 * u) for u in range(16))   # one digit 1 per unit of four windows: the quad's accumulator IS the next entry
    b = bG(10)
    jobs = [
        ([seg(T, b, [s]), seg(T, b, [s], 1)], None),                                       # P + P in the tree
        ([seg(T, b, [s], 2), seg(T, b, [r - s])], None),                                   # P - P in the tree: the identity
        ([seg(T, 0, [0, 0, 0]), seg(T, bH(1), [0, 0, 0], 1), seg(T, bG(1), [0], 2)], (1, 0)),   # nothing to add
        ([seg(T, b, k5), seg(T, b, [r - x for x in k5[:4]], 2)], None),                     # all but the last term cancel
        ([seg(T, b, [lone]), seg(T, bH(2), [0, 0, 0]), seg(T, b, [lone])], None),           # P + P in the host's sum of two partial points
        ([seg(T, bH(20), k4, 1), seg(T, bH(20), [r - x for x in k4], 1)], (bH(64), 1)),    # the runs cancel, the immediate term stays
    ]
    exp = np.array([smul(T, T.bases[b], 2 * s), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), smul(T, T.bases[b + 4], k5[4]),
                    smul(T, T.bases[b], 2 * lone), T.bases[bH(64)]])
    got = T.eng.debug_msm_direct(jobs)
    same(got, exp)
    assert not got[1].any() and not got[2].any() and exp[[0, 3, 4, 5]].any(axis=1).all()
    for j, p in zip(jobs, exp):
        same(T.eng.debug_msm_direct([j]), p)


def test_equal_points_in_a_quads_own_mixed_additions(T):
    """with six sums of 172 terms a quad takes two units: those of terms t and t + 88.  Both are the same base with one digit 1 in
    every unit of four windows and nothing else is non-zero, so each quad's accumulator IS the entry it adds next (qjac_madd's
    doubling case) — on B, B_blinding and four G bases"""
    lone = sum(1 << (16 * u) for u in range(16))
    bs = [0, 1, bG(10), bG(18), bG(28), bG(46)]
    jobs = [([seg(T, b, [lone], j % 3), seg(T, 0, [0] * 87, (j + 1) % 3), seg(T, b, [lone] + [0] * 83, (j + 2) % 3)], None) for j, b in enumerate(bs)]
    got, wgs = T.eng.debug_msm_direct(jobs, with_workgroups=True)
    assert wgs == 22          # 64 * 22 quads: units u and u + 1408 share one
    same(got, np.array([smul(T, T.bases[b], 2 * lone) for b in bs]))


def test_hook_refuses_what_the_kernel_would_read_out_of_bounds(T):
    import ark_bulletproofs_amd as A

    e = T.eng
    ok = seg(T, bH(60), [1, 2, 3, 4, 5])
    same(e.debug_msm_direct([([ok], None)]), msm_ref(T, [bH(60) + i for i in range(5)], [1, 2, 3, 4, 5]))
    bad = [
        ([seg(T, bH(60), [1, 2, 3, 4, 5, 6])], None),               # one element past the last base
        ([seg(T, NB, [1])], None),
        ([seg(T, 0, [1, 2, 3], count=0)], None),                    # a used run without terms
        ([seg(T, 0, [1, 2, 3], count=4)], None),                    # more terms than scalars
        ([seg(T, bG(0), [1] * 8, 0, 4, 1, 5)], None),               # fold: term 4 stands for element 12
        ([seg(T, bH(58), [1] * 16, 0, 4, 1, 5)], None),             # ... which lies outside the tables here
        ([seg(T, 0, [1], 3)], None),                                # no such format
        ([], (NB, 1)),
        ([], None),                                                 # no terms at all
    ]
    for job in bad:
        with pytest.raises(A.ArkbpError):
            e.debug_msm_direct([job])
    with pytest.raises(A.ArkbpError):
        e.debug_msm_direct([([ok], None)] * 7)
    same(e.debug_msm_direct([([seg(T, bG(0), list(range(1, 14)), 0, 4, 1, 5)], None)]), msm_ref(T, [bG(t) for t in (4, 5, 6, 7, 12)], [5, 6, 7, 8, 13]))
    fresh = A.Engine(curve=T.cv)
    try:
        fresh.gens_derive(8)
        with pytest.raises(A.ArkbpError):
            fresh.debug_msm_direct([([seg(T, 0, [1])], None)])      # tables not built
    finally:
        fresh.close()


# ---- 10, 11: the commitment kernels -----------------------------------------------------------------------------------------------------
def edge_rows(r):
    """the edge rows of test_gpu_primitives.py::test_pedersen_commit_batch"""
    return [(0, 5), (5, 0), (0, 0), (r - 1, r - 1), (1, 1), (255, 256), (1 << 248, 1 << 255 if (1 << 255) < r else 1 << 254), (r - 1, 1), (2**64 - 1, r - 2)]


def test_dt_commit_every_window_and_digit(T):
    """k_dt_commit (up to 4096 rows per call): the commitment to (d << 4w, 0) is entry (w, d) of B, to (0, d << 4w) that of
    B_blinding — every entry a reduced scalar can select, in one call"""
    rows = [(b, w, d) for b in range(2) for w in range(W) for d in range(1, D + 1) if (d << (4 * w)) < T.r]
    assert 1900 <= len(rows) <= 1920
    v = monts(T, [(d << (4 * w)) if b == 0 else 0 for b, w, d in rows])
    bl = monts(T, [(d << (4 * w)) if b == 1 else 0 for b, w, d in rows])
    got = T.eng.pedersen_commit_batch(v, bl)
    same(got, np.array([T.pc_dt[b, w, d - 1] for b, w, d in rows]))


def test_pc_commit_single_digits_and_edge_rows(T):
    """k_pc_commit (more than 4096 rows per call), which the suite otherwise reaches only at full size: one row per table entry a
    reduced scalar can select, the edge rows of the small batches at the first row, across a workgroup boundary and in the last,
    partly filled workgroup; the first 4096 rows again through k_dt_commit"""
    O, r = T.O, T.r
    rows = [(b, w, d) for b in range(2) for w in range(32) for d in range(1, 256) if (d << (8 * w)) < r]
    vb = [((d << (8 * w)), 0) if b == 0 else (0, d << (8 * w)) for b, w, d in rows]
    src = list(range(len(rows)))                     # row -> index into `rows`, or -1 - i for edge row i
    edge = edge_rows(r)
    vb.insert(0, edge[0]); src.insert(0, -1)
    vb[255:255] = [edge[1], edge[2]]; src[255:255] = [-2, -3]
    vb += edge[3:]; src += [-1 - i for i in range(3, 9)]
    n = len(vb)
    assert n > 16000 and n % 256 and src[255] == -2 and src[256] == -3 and src[-1] == -9
    v, bl = monts(T, [x for x, _ in vb]), monts(T, [y for _, y in vb])
    got = T.eng.pedersen_commit_batch(v, bl)
    exp = np.array([T.pc_table[rows[s]] if s >= 0 else O.pedersen_commit(T.cv, v[i], bl[i]) for i, s in enumerate(src)])
    same(got, exp)
    assert not got[src.index(-3)].any()              # (0, 0): the identity
    same(T.eng.pedersen_commit_batch(v[:4096], bl[:4096]), got[:4096])


# ---- 12: the tables follow their generators -----------------------------------------------------------------------------------------
def test_tables_follow_their_generators(T):
    """installing other generators drops the direct tables; rebuilt, they are the new generators' (B, B_blinding stay); a ctx that
    shares the generators reads the owner's tables"""
    import ark_bulletproofs_amd as A

    e, o = A.Engine(curve=T.cv), A.Engine(curve=T.cv)
    try:
        e.gens_derive(128)
        assert e.gens_direct_tables(CAP) == T.dt_bytes
        G, H = T.O.bp_gens_party(T.cv, CAP, 1)
        assert (G[0] != T.bases[bG(0)]).any()
        e.gens_upload(G, H)
        assert e.direct_stats()[1] == 0 and e.debug_tables_ptr(4) == (None, 0)
        assert e.gens_direct_tables(CAP) == T.dt_bytes and e.direct_stats()[1] == CAP
        bases = np.concatenate([T.bases[:2], G, H])
        sample_entries(T, e.debug_table_points(4).reshape(NB, W, D, 8), bases)
        o.share_gens_from(e)
        assert o.debug_tables_ptr(4) == e.debug_tables_ptr(4) and o.debug_tables_ptr(4)[1] == T.dt_bytes
        ks = rand_ints(T, 91, 3)
        same(o.debug_msm_direct([([seg(T, bH(62), ks, 1)], None)]), T.O.msm(T.cv, H[62:65], monts(T, ks)))
    finally:
        o.close()
        e.close()
