"""Engine: one bp_ctx (one GPU, one HIP stream) and typed wrappers over the C ABI."""
import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ArkbpError, check, lib, ptr, u64arr  # noqa: F401

SECQ256K1, ZORRO = 0, 1


class DeviceBuffer:
    """HBM allocation owned by an Engine."""

    def __init__(self, eng, nbytes):
        self.eng, self.nbytes = eng, nbytes
        p = C.c_void_p()
        check(lib().bp_dev_alloc(eng.ctx, C.c_size_t(nbytes), C.byref(p)), "bp_dev_alloc")
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().bp_dev_upload(self.eng.ctx, self.ptr, ptr(arr), C.c_size_t(arr.nbytes)), "bp_dev_upload")
        return self

    def download(self, dtype=np.uint64, nbytes=None):
        nbytes = self.nbytes if nbytes is None else nbytes
        out = np.zeros(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        check(lib().bp_dev_download(self.eng.ctx, ptr(out), self.ptr, C.c_size_t(nbytes)), "bp_dev_download")
        return out

    def free(self):
        if self.ptr:
            lib().bp_dev_free(self.eng.ctx, self.ptr)
            self.ptr = None


class Engine:
    def __init__(self, curve=SECQ256K1, device=0):
        self.curve = curve
        self.ctx = C.c_void_p()
        check(lib().bp_ctx_create(curve, device, C.byref(self.ctx)), "bp_ctx_create")

    @classmethod
    def host_only(cls, curve=SECQ256K1, gens_capacity=256):
        """a ctx WITHOUT a device (bp_debug_ctx_create_hostonly): the host side of batch verification as a dry run, for sanitizer
        builds on machines with no GPU.  Nothing is verified in that mode."""
        self = cls.__new__(cls)
        self.curve = curve
        self.ctx = C.c_void_p()
        check(lib().bp_debug_ctx_create_hostonly(curve, C.c_size_t(gens_capacity), C.byref(self.ctx)), "bp_debug_ctx_create_hostonly")
        return self

    def close(self):
        if self.ctx:
            lib().bp_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- memory -------------------------------------------------------------------------------
    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def upload_points(self, pts_xy):
        """ark-layout affine points (n x 8 u64) -> resident engine layout"""
        pts = u64arr(pts_xy, 8)
        buf = DeviceBuffer(self, max(pts.nbytes, 64)).upload(pts)
        check(lib().bp_points_import(self.ctx, buf.ptr, buf.ptr, C.c_size_t(len(pts))), "bp_points_import")
        return buf

    def upload_scalars(self, scalars):
        sc = u64arr(scalars, 4)
        return DeviceBuffer(self, max(sc.nbytes, 32)).upload(sc)

    def sync(self):
        check(lib().bp_ctx_sync(self.ctx), "bp_ctx_sync")

    # ---- VariableBaseMSM::msm -------------------------------------------------------------------
    def msm(self, bases_xy, scalars, canonical=False):
        b, s = u64arr(bases_xy, 8), u64arr(scalars, 4)
        if len(b) != len(s):
            raise ValueError("msm: %d bases vs %d scalars" % (len(b), len(s)))  # ark: Err(min_len)
        out = np.zeros(8, dtype=np.uint64)
        check(lib().bp_msm(self.ctx, ptr(b), ptr(s), C.c_size_t(len(b)), int(canonical), ptr(out)), "bp_msm")
        return out

    def msm_gens(self, n, scalars, use_G=True, use_H=True, off=0, extra_bases=None, canonical=False):
        """MSM over the resident generator tables: G[off:off+n] || H[off:off+n] || extra_bases, scalars in that order"""
        ex = u64arr(extra_bases, 8) if extra_bases is not None and len(extra_bases) else np.zeros((0, 8), dtype=np.uint64)
        s = u64arr(scalars, 4)
        if len(s) != (n if use_G else 0) + (n if use_H else 0) + len(ex):
            raise ValueError("msm_gens: bases and scalars differ in length")
        out = np.zeros(8, dtype=np.uint64)
        check(lib().bp_msm_gens(self.ctx, int(use_G), int(use_H), C.c_size_t(off), C.c_size_t(n), ptr(ex) if len(ex) else None, C.c_size_t(len(ex)),
                                ptr(s) if len(s) else None, int(canonical), ptr(out)), "bp_msm_gens")
        return out

    def msm_dev(self, d_bases, d_scalars, n, canonical=False):
        out = np.zeros(8, dtype=np.uint64)
        check(lib().bp_msm_dev(self.ctx, d_bases.ptr, d_scalars.ptr, C.c_size_t(n), int(canonical), ptr(out)), "bp_msm_dev")
        return out

    def set_window_shard(self, rank, world, reduce_fn=None):
        """window-sharded mode (bp_ctx_set_window_shard): reduce_fn(xy: (8,) u64) -> (8,) u64 = sum of all ranks' partial points"""
        if world <= 1:
            check(lib().bp_ctx_set_window_shard(self.ctx, 0, 1, None, None), "bp_ctx_set_window_shard")
            self._shard_cb = None
            return
        errs = self._shard_errors = []

        def cb(_user, xy):
            try:
                out = reduce_fn(np.array(xy[:8], dtype=np.uint64))
                for i in range(8):
                    xy[i] = int(out[i])
                return 0
            except Exception as e:  # never unwind through C
                errs.append(e)
                return 1

        self._shard_cb = _POINT_REDUCE_CB(cb)   # keep the thunk alive as long as the mode is on
        check(lib().bp_ctx_set_window_shard(self.ctx, int(rank), int(world), self._shard_cb, None), "bp_ctx_set_window_shard")

    def set_shard_allgather(self, gather_fn=None):
        """second collective of the sharded mode (bp_ctx_set_shard_allgather): gather_fn(block: uint8 array) -> (world, len) uint8
        array in rank order.  With it the prover partitions the inner-product argument index-cyclically across the ranks."""
        if gather_fn is None:
            check(lib().bp_ctx_set_shard_allgather(self.ctx, None, None), "bp_ctx_set_shard_allgather")
            self._gather_cb = None
            return
        errs = self._gather_errors = []

        def cb(_user, send, nbytes, recv):
            try:
                blk = np.frombuffer((C.c_uint8 * nbytes).from_address(send), dtype=np.uint8)
                out = np.ascontiguousarray(gather_fn(blk.copy()), dtype=np.uint8).reshape(-1)
                C.memmove(recv, out.ctypes.data, out.nbytes)
                return 0
            except Exception as e:  # never unwind through C
                errs.append(e)
                return 1

        self._gather_cb = _ALLGATHER_CB(cb)
        check(lib().bp_ctx_set_shard_allgather(self.ctx, self._gather_cb, None), "bp_ctx_set_shard_allgather")

    def set_tuning(self, knob, value):
        """knob: 0 fold-batch minimum lanes, 1 MSM two-level-sort minimum terms, .. 6 host threads of the ctx's pool (include/arkbp.h BP_TUNE_*)"""
        check(lib().bp_ctx_set_tuning(self.ctx, int(knob), C.c_uint64(int(value))), "bp_ctx_set_tuning")

    # ---- profiling ------------------------------------------------------------------------------
    def set_profiling(self, on=True):
        check(lib().bp_ctx_set_profiling(self.ctx, int(on)), "bp_ctx_set_profiling")

    def reset_profiling(self):
        check(lib().bp_ctx_reset_profiling(self.ctx), "bp_ctx_reset_profiling")

    def kernel_time(self, which):
        ms, cnt = C.c_double(0), C.c_uint64(0)
        check(lib().bp_ctx_kernel_time(self.ctx, which, C.byref(ms), C.byref(cnt)), "bp_ctx_kernel_time")
        return ms.value, cnt.value

    # ---- unit-test hooks ---------------------------------------------------------------------------
    def debug_field_op(self, field, op, a, b):
        a, b = u64arr(a, 4), u64arr(b, 4)
        out = np.zeros_like(a)
        check(lib().bp_debug_field_op(self.ctx, field, op, ptr(a), ptr(b), ptr(out), C.c_size_t(len(a))), "bp_debug_field_op")
        return out

    def debug_point_op(self, op, p, q, k=None):
        p, q = u64arr(p, 8), u64arr(q, 8)
        k = np.zeros((len(p), 4), dtype=np.uint64) if k is None else u64arr(k, 4)
        out = np.zeros_like(p)
        check(lib().bp_debug_point_op(self.ctx, op, ptr(p), ptr(q), ptr(k), ptr(out), C.c_size_t(len(p))), "bp_debug_point_op")
        return out

    def debug_field_raw(self, field, op, limbs):
        """raw 9 x u32 limbs in and out (csrc/dbg_raw.cuh): limbs (n, 36) = a | b | c | d -> (n, 18)"""
        a = np.ascontiguousarray(limbs, dtype=np.uint32).reshape(-1, 36)
        out = np.zeros((len(a), 18), dtype=np.uint32)
        check(lib().bp_debug_field_raw(self.ctx, field, op, ptr(a), ptr(out), C.c_size_t(len(a))), "bp_debug_field_raw")
        return out

    def debug_point_raw(self, op, limbs):
        """limbs (n, 54) = P.X P.Y P.Z Q.X Q.Y Q.Z -> (n, lanes, 28) = X Y Z flag per lane; lanes = 4 for the quad ops 4..6"""
        a = np.ascontiguousarray(limbs, dtype=np.uint32).reshape(-1, 54)
        out = np.zeros((len(a), 1 if op < 4 else 4, 28), dtype=np.uint32)
        check(lib().bp_debug_point_raw(self.ctx, op, ptr(a), ptr(out), C.c_size_t(len(a))), "bp_debug_point_raw")
        return out


# ---- InnerProductProof::create ---------------------------------------------------------------------
_POINT_REDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64))
_ALLGATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_CHALLENGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))


def _ipa_create(self, Q, G_factors, H_factors, G_vec, H_vec, a_vec, b_vec, challenge):
    """challenge(L_xy, R_xy) -> u (4 x u64 Montgomery words): the caller's transcript step
    (append_point L, R; challenge_scalar u — src/inner_product_proof.rs:132-135)."""
    G, H = u64arr(G_vec, 8), u64arr(H_vec, 8)
    n = len(G)
    arrs = [u64arr(Q, 8)] + [u64arr(x, 4) for x in (G_factors, H_factors)] + [G, H] + [u64arr(x, 4) for x in (a_vec, b_vec)]
    for x in arrs[1:]:
        if len(x) != n:
            raise ValueError("ipa_create: vector lengths differ")  # the reference asserts
    lg = max(n.bit_length() - 1, 0)
    L = np.zeros((max(lg, 1), 8), dtype=np.uint64)
    R = np.zeros((max(lg, 1), 8), dtype=np.uint64)
    ao, bo = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    err = []

    def cb(_user, Lp, Rp, up):
        try:
            u = challenge(np.array(Lp[:8], dtype=np.uint64), np.array(Rp[:8], dtype=np.uint64))
            for i in range(4):
                up[i] = int(u[i])
            return 0
        except Exception as e:  # never unwind through C
            err.append(e)
            return 1

    cfn = _CHALLENGE_CB(cb)
    rc = lib().bp_ipa_create(self.ctx, *[ptr(x) for x in arrs], C.c_size_t(n), cfn, None, ptr(L), ptr(R), ptr(ao), ptr(bo))
    if err:
        raise err[0]
    check(rc, "bp_ipa_create")
    return L[:lg], R[:lg], ao, bo


Engine.ipa_create = _ipa_create


# InnerProductProof::create cut at the Fiat-Shamir step (bp_ipa_begin .. bp_ipa_finish): the stepping interface that
# parallel.sharded_ipa_create drives on every rank
def _ipa_begin(self, Q, G_factors, H_factors, G_vec, H_vec, a_vec, b_vec):
    G, H = u64arr(G_vec, 8), u64arr(H_vec, 8)
    n = len(G)
    arrs = [u64arr(Q, 8)] + [u64arr(x, 4) for x in (G_factors, H_factors)] + [G, H] + [u64arr(x, 4) for x in (a_vec, b_vec)]
    for x in arrs[1:]:
        if len(x) != n:
            raise ValueError("ipa_begin: vector lengths differ")
    check(lib().bp_ipa_begin(self.ctx, *[ptr(x) for x in arrs], C.c_size_t(n)), "bp_ipa_begin")


def _ipa_round_LR(self):
    L, R = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    check(lib().bp_ipa_round_LR(self.ctx, ptr(L), ptr(R)), "bp_ipa_round_LR")
    return L, R


def _ipa_round_fold(self, u):
    u = np.ascontiguousarray(u, dtype=np.uint64).reshape(4)
    check(lib().bp_ipa_round_fold(self.ctx, ptr(u)), "bp_ipa_round_fold")


def _ipa_finish(self):
    a, b = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    check(lib().bp_ipa_finish(self.ctx, ptr(a), ptr(b)), "bp_ipa_finish")
    return a, b


def _ipa_export(self, n_max):
    """current (a, b, G, H, gamma_G, gamma_H); G_true = gamma_G * G, H_true = gamma_H * H"""
    a, b = np.zeros((n_max, 4), dtype=np.uint64), np.zeros((n_max, 4), dtype=np.uint64)
    G, H = np.zeros((n_max, 8), dtype=np.uint64), np.zeros((n_max, 8), dtype=np.uint64)
    gG, gH = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    n = C.c_size_t(0)
    check(lib().bp_ipa_export(self.ctx, ptr(a), ptr(b), ptr(G), ptr(H), ptr(gG), ptr(gH), C.byref(n)), "bp_ipa_export")
    return a[: n.value], b[: n.value], G[: n.value], H[: n.value], gG, gH


Engine.ipa_begin = _ipa_begin
Engine.ipa_round_LR = _ipa_round_LR
Engine.ipa_round_fold = _ipa_round_fold
Engine.ipa_finish = _ipa_finish
Engine.ipa_export = _ipa_export


# ---- generators / prover ---------------------------------------------------------------------------
SC_SHUFFLE, SC_RANGE, SC_EXAMPLE, SC_SQUARE_CHAIN, SC_MULTI_RANGE = 0, 1, 2, 3, 4


def _gens_derive(self, cap):
    """BulletproofGens::new(cap, 1) + the engine's PedersenGens (default() unless pedersen_gens_install put a pair there), installed in HBM"""
    check(lib().bp_gens_derive(self.ctx, C.c_size_t(cap)), "bp_gens_derive")
    self.gens_capacity = cap


def _gens_upload(self, G_xy, H_xy):
    G, H = u64arr(G_xy, 8), u64arr(H_xy, 8)
    assert len(G) == len(H)
    check(lib().bp_gens_upload(self.ctx, ptr(G), ptr(H), C.c_size_t(len(G))), "bp_gens_upload")
    self.gens_capacity = len(G)


def _gens_download(self, n):
    G, H = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64)
    check(lib().bp_gens_download(self.ctx, ptr(G), ptr(H), C.c_size_t(n)), "bp_gens_download")
    return G, H


class Proved:
    def __init__(self, proof, commitments, publics, timing):
        self.proof, self.commitments, self.publics, self.timing = proof, commitments, publics, timing
        self.t_prove, self.t_setup = timing[0], timing[1]


def _prove_scenario(self, scenario, params, seed, m_cap=None):
    prm = np.zeros(8, dtype=np.uint64)
    prm[: len(params)] = np.array(params, dtype=np.uint64)
    if m_cap is None:
        m_cap = 2 * int(prm[0]) + 8
    buf = C.create_string_buffer(1 << 16)
    plen = C.c_size_t(len(buf))
    commits = np.zeros((m_cap, 8), dtype=np.uint64)
    m, npub = C.c_size_t(0), C.c_size_t(0)
    pubs = np.zeros((8, 4), dtype=np.uint64)
    timing = (C.c_double * 8)()
    check(lib().bp_r1cs_prove_scenario(self.ctx, scenario, ptr(prm), bytes(seed), buf, C.byref(plen), ptr(commits), C.c_size_t(m_cap), C.byref(m),
                                       ptr(pubs), C.byref(npub), timing), "bp_r1cs_prove_scenario")
    return Proved(buf.raw[: plen.value], commits[: m.value].copy(), pubs[: npub.value].copy(), list(timing))


Engine.gens_derive = _gens_derive
Engine.gens_upload = _gens_upload
Engine.gens_download = _gens_download
Engine.prove_scenario = _prove_scenario


class HostTranscript:
    """The product's merlin::Transcript (host C++), for tests and for driving bp_ipa_create."""

    def __init__(self, label):
        self.h = C.c_void_p(lib().bp_transcript_new(bytes(label), C.c_size_t(len(label))))

    def __del__(self):
        try:
            lib().bp_transcript_free(self.h)
        except Exception:
            pass

    def append_message(self, label, msg):
        lib().bp_transcript_append_message(self.h, bytes(label), bytes(msg), C.c_size_t(len(msg)))

    def append_u64(self, label, x):
        self.append_message(label, int(x).to_bytes(8, "little"))

    def challenge_bytes(self, label, n):
        out = C.create_string_buffer(n)
        lib().bp_transcript_challenge_bytes(self.h, bytes(label), out, C.c_size_t(n))
        return out.raw

    def append_point(self, curve, label, xy):
        check(lib().bp_transcript_append_point(curve, self.h, bytes(label), ptr(np.ascontiguousarray(xy, dtype=np.uint64))), "append_point")

    def challenge_scalar(self, curve, label):
        out = np.zeros(4, dtype=np.uint64)
        check(lib().bp_transcript_challenge_scalar(curve, self.h, bytes(label), ptr(out)), "challenge_scalar")
        return out


def debug_rng_draws(curve, transcript, witness, seeds, count):
    """seeds: one 32-byte seed (scalar path) or eight (AVX-512 x8 path); returns (lanes, count, 4) u64 or None if unavailable"""
    w = np.ascontiguousarray(witness, dtype=np.uint64).reshape(-1, 4)
    lanes = len(seeds) // 32
    out = np.zeros((lanes, count, 4), dtype=np.uint64)
    rc = lib().bp_debug_rng_draws(curve, transcript.h, ptr(w), C.c_size_t(len(w)), bytes(seeds), lanes, C.c_size_t(count), ptr(out))
    if rc == _lib.BP_E_ARG and lanes == 8:
        return None
    check(rc, "bp_debug_rng_draws")
    return out


def debug_append_points_x8(curve, transcripts, label, points):
    """points: (lanes, npts, 8) u64; appends them to the HostTranscripts in lockstep (AVX-512 Keccak-f x8); False if unavailable"""
    pts = np.ascontiguousarray(points, dtype=np.uint64)
    lanes, npts = pts.shape[0], pts.shape[1]
    arr = (C.c_void_p * lanes)(*[t.h for t in transcripts])
    rc = lib().bp_debug_append_points_x8(curve, arr, lanes, bytes(label), ptr(pts), C.c_size_t(npts))
    if rc == _lib.BP_E_ARG:
        return False
    check(rc, "bp_debug_append_points_x8")
    return True


def debug_challenge_x8(transcripts, msg_label, msg, chal_label, nbytes):
    """eight HostTranscripts at the same STROBE position: append `msg` under `msg_label` and draw `nbytes` challenge bytes each under
    `chal_label`, all in lockstep (AVX-512 Keccak-f x8); returns an (8, nbytes) u8 array, or None if unavailable"""
    arr = (C.c_void_p * 8)(*[t.h for t in transcripts])
    out = np.zeros((8, nbytes), dtype=np.uint8)
    m = np.frombuffer(bytes(msg), dtype=np.uint8).copy() if len(msg) else np.zeros(1, dtype=np.uint8)
    rc = lib().bp_debug_challenge_x8(arr, bytes(msg_label), ptr(m), C.c_size_t(len(msg)), bytes(chal_label), C.c_size_t(nbytes), ptr(out))
    if rc == _lib.BP_E_ARG:
        return None
    check(rc, "bp_debug_challenge_x8")
    return out


def pedersen_gens(curve):
    B, Bb = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    check(lib().bp_pedersen_gens(curve, ptr(B), ptr(Bb)), "bp_pedersen_gens")
    return B, Bb


def host_derive_generators(curve, which_H, party, count):
    out = np.zeros((count, 8), dtype=np.uint64)
    check(lib().bp_host_derive_generators(curve, int(which_H), party, C.c_size_t(count), ptr(out)), "bp_host_derive_generators")
    return out


def host_sha3_512(msg):
    out = C.create_string_buffer(64)
    lib().bp_host_sha3_512(bytes(msg), C.c_size_t(len(msg)), out)
    return out.raw


# ---- verifier ----------------------------------------------------------------------------------------
def _prm(params):
    prm = np.zeros(8, dtype=np.uint64)
    prm[: len(params)] = np.array(params, dtype=np.uint64)
    return prm


def _verify_scenario(self, scenario, params, proof, commitments, publics):
    """Verifier::verify for a scenario statement; returns the C status (0 = Ok, -4 VerificationError, -6 FormatError, ...)"""
    cm = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(-1, 8)
    pb = np.ascontiguousarray(publics, dtype=np.uint64).reshape(-1, 4)
    return lib().bp_r1cs_verify_scenario(self.ctx, scenario, ptr(_prm(params)), bytes(proof), C.c_size_t(len(proof)), ptr(cm), C.c_size_t(len(cm)),
                                         ptr(pb), C.c_size_t(len(pb)))


class PackedInstances:
    """The flat arrays bp_r1cs_batch_verify_scenarios takes (what a caller in the reference's language would hand over directly),
    built once from a list of (scenario, params, proof_bytes, commitments, publics)."""

    def __init__(self, instances):
        n = len(instances)
        self.n = n
        if n == 0:   # an empty batch is valid (the reference's mega-check of nothing is the identity)
            self.scen = (C.c_int * 1)()
            self.prm = np.zeros(8, dtype=np.uint64)
            self.proofs = b""
            self.plens = (C.c_size_t * 1)()
            self.cms = np.zeros((1, 8), dtype=np.uint64)
            self.ms = (C.c_size_t * 1)()
            self.pubs = np.zeros((1, 4), dtype=np.uint64)
            self.npubs = (C.c_size_t * 1)()
            return
        self.scen = (C.c_int * n)(*[i[0] for i in instances])
        self.prm = np.concatenate([_prm(i[1]) for i in instances])
        self.proofs = b"".join(i[2] for i in instances)
        self.plens = (C.c_size_t * n)(*[len(i[2]) for i in instances])
        cm_l = [np.asarray(i[3], dtype=np.uint64).reshape(-1, 8) for i in instances]
        self.cms = np.ascontiguousarray(np.concatenate(cm_l))
        self.ms = (C.c_size_t * n)(*[len(c) for c in cm_l])
        pubs_l = [np.asarray(i[4], dtype=np.uint64).reshape(-1, 4) for i in instances]
        self.pubs = np.ascontiguousarray(np.concatenate(pubs_l + [np.zeros((1, 4), dtype=np.uint64)]))
        self.npubs = (C.c_size_t * n)(*[len(p) for p in pubs_l])


def pack_instances(instances):
    return PackedInstances(instances)


def _batch_verify(self, instances, alpha_seed, alpha_skip=0, want_point=False):
    """batch_verify; instances: list of (scenario, params, proof_bytes, commitments, publics) or a PackedInstances.  Returns
    (status, timing[5]) or (status, timing, check_point) when want_point (proof-sharded multi-GPU use, see parallel.py)."""
    pk = instances if isinstance(instances, PackedInstances) else PackedInstances(instances)
    timing = (C.c_double * 5)()
    pt = np.zeros(8, dtype=np.uint64)
    rc = lib().bp_r1cs_batch_verify_scenarios(self.ctx, C.c_size_t(pk.n), pk.scen, ptr(pk.prm), pk.proofs, pk.plens, ptr(pk.cms), pk.ms, ptr(pk.pubs), pk.npubs,
                                              bytes(alpha_seed), timing, C.c_size_t(alpha_skip), ptr(pt))
    if want_point:
        return rc, list(timing), pt
    return rc, list(timing)


def _verification_gh(self, n1, wL, wR, wO, y, x, u, a, b, ipa_challenges):
    """g_scalars / h_scalars of Verifier::verification_scalars (canonical integers, 2^k each) from the caller's flattened vectors"""
    wL, wR, wO = u64arr(wL, 4), u64arr(wR, 4), u64arr(wO, 4)
    ch = u64arr(ipa_challenges, 4)
    k = len(ch)
    N = 1 << k
    g, h = np.zeros((N, 4), dtype=np.uint64), np.zeros((N, 4), dtype=np.uint64)
    sc = [np.ascontiguousarray(v, dtype=np.uint64).reshape(4) for v in (y, x, u, a, b)]
    check(lib().bp_r1cs_verification_gh(self.ctx, C.c_size_t(len(wL)), C.c_size_t(n1), ptr(wL), ptr(wR), ptr(wO), *[ptr(v) for v in sc], ptr(ch),
                                        C.c_size_t(k), ptr(g), ptr(h)), "bp_r1cs_verification_gh")
    return g, h


Engine.verification_gh = _verification_gh
Engine.verify_scenario = _verify_scenario
Engine.batch_verify = _batch_verify


def host_points_sum(curve, pts_xy):
    pts = u64arr(pts_xy, 8)
    out = np.zeros(8, dtype=np.uint64)
    check(lib().bp_host_points_sum(curve, ptr(pts), C.c_size_t(len(pts)), ptr(out)), "bp_host_points_sum")
    return out


# ---- witness check (include/arkbp.h: bp_prover_check, bp_prover_set_check) ------------------------------------------------------
NONE_BAD = (1 << 64) - 1             # first_bad_gate / first_bad_constraint of a report without one (UINT64_MAX)


class _WitnessReportC(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("gates_checked", "constraints_checked", "bad_gates", "first_bad_gate", "bad_constraints", "first_bad_constraint", "deferred_callbacks")] + [("first_bad_residual", C.c_uint64 * 4)]


class WitnessReport:
    """bp_witness_report: what was examined, how many gates / constraints are violated and the smallest index of each (NONE_BAD when
    none), the randomized-phase callbacks that have not run (their constraints are not covered), and the value of the first violated
    constraint's combination (4 ark words)."""

    def __init__(self, c):
        for n, _ in _WitnessReportC._fields_[:-1]:
            setattr(self, n, int(getattr(c, n)))
        self.first_bad_residual = np.array(list(c.first_bad_residual), dtype=np.uint64)

    @property
    def satisfied(self):
        return self.bad_gates == 0 and self.bad_constraints == 0

    def astuple(self):
        return (self.gates_checked, self.constraints_checked, self.bad_gates, self.first_bad_gate, self.bad_constraints, self.first_bad_constraint,
                self.deferred_callbacks, tuple(int(x) for x in self.first_bad_residual))

    def __eq__(self, other):
        return isinstance(other, WitnessReport) and self.astuple() == other.astuple()

    def __repr__(self):
        return "WitnessReport(gates=%d, constraints=%d, bad_gates=%d, first_bad_gate=%d, bad_constraints=%d, first_bad_constraint=%d, deferred_callbacks=%d)" % self.astuple()[:7]


def witness_check_piece():
    """most terms one lane of the constraint check walks (bp_witness_check_piece)"""
    return int(lib().bp_witness_check_piece())


def _witness_check(handle, engine):
    r = _WitnessReportC()
    check(lib().bp_prover_check(engine.ctx if engine is not None else None, handle, C.byref(r)), "bp_prover_check")
    return WitnessReport(r)


def _set_check(handle, on):
    check(lib().bp_prover_set_check(handle, 1 if on else 0), "bp_prover_set_check")


def _checking(handle):
    on = C.c_int(-1)
    check(lib().bp_prover_checking(handle, C.byref(on)), "bp_prover_checking")
    return bool(on.value)


def debug_poke_witness(prover, vec, index, value):
    """test hook (bp_debug_prover_poke_witness): overwrite one recorded assignment; vec 0 a_L, 1 a_R, 2 a_O, 3 v; value: 4 ark words"""
    v = np.ascontiguousarray(value, dtype=np.uint64).reshape(4)
    check(lib().bp_debug_prover_poke_witness(_prover_handle(prover), int(vec), C.c_size_t(index), ptr(v)), "bp_debug_prover_poke_witness")


# ---- statements (setup separated from prove(), several proofs in flight) -----------------------------------
class Statement:
    """Prover::new + commits + gadget for a scenario.  Host only by default; with `engine` the statement's Pedersen
    commitments are one GPU batch (same statement either way).  prove(engine) consumes it."""

    def __init__(self, curve, scenario, params, seed, engine=None):
        self.h = C.c_void_p()
        if engine is not None:
            if engine.curve != curve:
                raise ValueError("Statement: engine curve differs")
            check(lib().bp_stmt_prover_create_dev(engine.ctx, scenario, ptr(_prm(params)), bytes(seed), C.byref(self.h)), "bp_stmt_prover_create_dev")
        else:
            check(lib().bp_stmt_prover_create(curve, scenario, ptr(_prm(params)), bytes(seed), C.byref(self.h)), "bp_stmt_prover_create")
        self.curve = curve

    def info(self, m_cap=1 << 16):
        commits = np.zeros((m_cap, 8), dtype=np.uint64)
        pubs = np.zeros((8, 4), dtype=np.uint64)
        m, npub, nm, nq = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(lib().bp_stmt_info(self.h, ptr(commits), C.c_size_t(m_cap), C.byref(m), ptr(pubs), C.byref(npub), C.byref(nm), C.byref(nq)), "bp_stmt_info")
        return commits[: m.value].copy(), pubs[: npub.value].copy(), nm.value, nq.value

    def precompute(self):
        """host-only head of prove(): the TranscriptRng chain (needs no GPU)"""
        check(lib().bp_stmt_precompute(self.h), "bp_stmt_precompute")

    def set_blinding(self, mode):
        """BLINDING_TRANSCRIPT / BLINDING_EXPANDED for this statement's prove() (bp_prover_set_blinding through bp_stmt_as_prover)"""
        check(lib().bp_prover_set_blinding(C.c_void_p(lib().bp_stmt_as_prover(self.h)), int(mode)), "bp_prover_set_blinding")

    @property
    def blinding(self):
        m = C.c_int(-1)
        check(lib().bp_prover_blinding(C.c_void_p(lib().bp_stmt_as_prover(self.h)), C.byref(m)), "bp_prover_blinding")
        return m.value

    def check(self, engine=None):
        """WitnessReport of this statement's witness (bp_prover_check): on the GPU with an engine, the host twin without; consumes nothing"""
        return _witness_check(C.c_void_p(lib().bp_stmt_as_prover(self.h)), engine)

    def set_check(self, on):
        """the guard: prove() refuses an unsatisfying witness with UnsatisfiedError instead of emitting a proof no verifier accepts"""
        _set_check(C.c_void_p(lib().bp_stmt_as_prover(self.h)), on)

    def checking(self):
        return _checking(C.c_void_p(lib().bp_stmt_as_prover(self.h)))

    def prove(self, eng):
        buf = C.create_string_buffer(1 << 16)
        plen = C.c_size_t(len(buf))
        timing = (C.c_double * 8)()
        check(lib().bp_stmt_prove(eng.ctx, self.h, buf, C.byref(plen), timing), "bp_stmt_prove")
        return buf.raw[: plen.value], list(timing)

    def free(self):
        if self.h:
            lib().bp_stmt_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _pedersen_commit_batch(self, v, blind):
    """PedersenGens::commit for m (value, blinding) pairs (ark words, m x 4 each) -> m x 8 affine words"""
    v, blind = u64arr(v, 4), u64arr(blind, 4)
    if v.shape != blind.shape:
        raise ValueError("pedersen_commit_batch: length mismatch")
    out = np.zeros((v.shape[0], 8), dtype=np.uint64)
    check(lib().bp_pedersen_commit_batch(self.ctx, ptr(v), ptr(blind), C.c_size_t(v.shape[0]), ptr(out)), "bp_pedersen_commit_batch")
    return out


def _share_gens_from(self, other):
    check(lib().bp_gens_share(self.ctx, other.ctx), "bp_gens_share")
    self.gens_capacity = getattr(other, "gens_capacity", 0)
    self._gens_owner = other  # keep the owner alive


def _pedersen_gens_install(self, B=None, Bb=None):
    """PedersenGens { B, B_blinding } of the caller's choice for everything this engine does; no arguments: PedersenGens::default()"""
    if B is None and Bb is None:
        check(lib().bp_pedersen_gens_install(self.ctx, None, None), "bp_pedersen_gens_install")
        return
    b = None if B is None else np.ascontiguousarray(B, dtype=np.uint64).reshape(8)
    bb = None if Bb is None else np.ascontiguousarray(Bb, dtype=np.uint64).reshape(8)
    check(lib().bp_pedersen_gens_install(self.ctx, ptr(b) if b is not None else None, ptr(bb) if bb is not None else None), "bp_pedersen_gens_install")


def _engine_pedersen_gens(self):
    """the pair this engine holds now: (B, B_blinding, is_default)"""
    B, Bb = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    dflt = C.c_int(0)
    check(lib().bp_ctx_pedersen_gens(self.ctx, ptr(B), ptr(Bb), C.byref(dflt)), "bp_ctx_pedersen_gens")
    return B, Bb, bool(dflt.value)


Engine.pedersen_gens_install = _pedersen_gens_install
Engine.pedersen_gens = _engine_pedersen_gens
Engine.share_gens_from = _share_gens_from
Engine.pedersen_commit_batch = _pedersen_commit_batch


def precompute_batch(stmts):
    """host-only head of prove() for many statements; groups of 8 same-shaped ones share one AVX-512 Keccak-f x8 stream"""
    arr = (C.c_void_p * len(stmts))(*[s.h for s in stmts])
    check(lib().bp_stmt_precompute_batch(arr, C.c_size_t(len(stmts))), "bp_stmt_precompute_batch")


def _ipa_verify(self, n, G_factors, H_factors, P, Q, G_vec, H_vec, L_vec, R_vec, challenges, a, b):
    """InnerProductProof::verify; challenges = the u_j the caller's transcript replay produced.  Returns the C status."""
    Lv = np.ascontiguousarray(L_vec, dtype=np.uint64).reshape(-1, 8)
    Rv = np.ascontiguousarray(R_vec, dtype=np.uint64).reshape(-1, 8)
    ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4)
    k = len(Lv)
    pad8, pad4 = np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    arrs = [u64arr(G_factors, 4), u64arr(H_factors, 4), u64arr(P, 8), u64arr(Q, 8), u64arr(G_vec, 8), u64arr(H_vec, 8)]
    return lib().bp_ipa_verify(self.ctx, C.c_size_t(n), *[ptr(x) for x in arrs], ptr(Lv if k else pad8), ptr(Rv if k else pad8), C.c_size_t(k),
                               ptr(ch if k else pad4), ptr(u64arr(a, 4)), ptr(u64arr(b, 4)))


Engine.ipa_verify = _ipa_verify


def msm_window_count(curve, n):
    """(windows, window_bits) of the engine's Pippenger schedule for an n-term MSM; depends only on (curve, n)"""
    w, c = C.c_int(0), C.c_int(0)
    check(lib().bp_msm_window_count(curve, C.c_size_t(n), C.byref(w), C.byref(c)), "bp_msm_window_count")
    return w.value, c.value


def _msm_dev_windows(self, d_bases, d_scalars, n, w_lo, w_hi, canonical=False):
    out = np.zeros(8, dtype=np.uint64)
    check(lib().bp_msm_dev_windows(self.ctx, d_bases.ptr, d_scalars.ptr, C.c_size_t(n), int(canonical), int(w_lo), int(w_hi), ptr(out)), "bp_msm_dev_windows")
    return out


Engine.msm_dev_windows = _msm_dev_windows


def _debug_decompress(self, compressed):
    """compressed: bytes of n x 33; returns (points (n,8) u64, ok (n,) u32)"""
    n = len(compressed) // 33
    out = np.zeros((n, 8), dtype=np.uint64)
    ok = np.zeros(n, dtype=np.uint32)
    check(lib().bp_debug_decompress(self.ctx, bytes(compressed), C.c_size_t(n), ptr(out), ptr(ok)), "bp_debug_decompress")
    return out, ok


Engine.debug_decompress = _debug_decompress


# ---- r1cs::ConstraintSystem / Prover / Verifier for the caller's own gadgets (include/arkbp.h "bp_cs") ----------------------
# Variables are (kind, index) pairs; a linear combination is a list of (variable, coefficient) with coefficients as 4 x u64
# Montgomery words — the shapes the reference's `Variable` and `LinearCombination` have (src/r1cs/linear_combination.rs).
VAR_COMMITTED, VAR_MULT_LEFT, VAR_MULT_RIGHT, VAR_MULT_OUT, VAR_ONE = 0, 1, 2, 3, 4
ONE_VAR = (VAR_ONE, 0)
_RANDOMIZE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)


def _lc_arrays(lc):
    n = len(lc)
    vars_ = np.zeros((max(n, 1), 2), dtype=np.uint32)
    coefs = np.zeros((max(n, 1), 4), dtype=np.uint64)
    for i, (v, c) in enumerate(lc):
        vars_[i] = v
        coefs[i] = np.asarray(c, dtype=np.uint64).reshape(4)
    return vars_, coefs, n


def _vars_out(arr):
    return [(int(arr[i, 0]), int(arr[i, 1])) for i in range(len(arr))]


class _ConstraintSystem:
    """What `impl ConstraintSystem for Prover / Verifier` offers (src/r1cs/constraint_system.rs:19-135), over a bp_cs handle."""

    def __init__(self, curve, transcript, handle=None):
        self.curve, self.transcript_obj = curve, transcript   # the transcript is borrowed: keep it alive
        self.h = handle if handle is not None else C.c_void_p()
        self._cbs = []
        self._cb_errors = []

    def free(self):
        if self.h:
            lib().bp_cs_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def transcript(self):
        return self.transcript_obj

    def multiply(self, left, right):
        lv, lc, nl = _lc_arrays(left)
        rv, rc, nr = _lc_arrays(right)
        out = np.zeros((3, 2), dtype=np.uint32)
        check(lib().bp_cs_multiply(self.h, ptr(lv), ptr(lc), C.c_size_t(nl), ptr(rv), ptr(rc), C.c_size_t(nr), ptr(out)), "bp_cs_multiply")
        return _vars_out(out)

    def allocate(self, assignment=None):
        out = np.zeros((1, 2), dtype=np.uint32)
        a = None if assignment is None else np.ascontiguousarray(assignment, dtype=np.uint64).reshape(4)
        check(lib().bp_cs_allocate(self.h, ptr(a) if a is not None else None, ptr(out)), "bp_cs_allocate")
        return _vars_out(out)[0]

    def allocate_multiplier(self, assignments=None):
        out = np.zeros((3, 2), dtype=np.uint32)
        if assignments is None:
            check(lib().bp_cs_allocate_multiplier(self.h, None, None, ptr(out)), "bp_cs_allocate_multiplier")
        else:
            l, r = [np.ascontiguousarray(x, dtype=np.uint64).reshape(4) for x in assignments]
            check(lib().bp_cs_allocate_multiplier(self.h, ptr(l), ptr(r), ptr(out)), "bp_cs_allocate_multiplier")
        return _vars_out(out)

    def constrain(self, lc):
        v, c, n = _lc_arrays(lc)
        check(lib().bp_cs_constrain(self.h, ptr(v), ptr(c), C.c_size_t(n)), "bp_cs_constrain")

    def allocate_multipliers(self, left=None, right=None, count=None):
        """bulk allocate_multiplier: returns the index of the first new multiplier"""
        first = C.c_uint32(0)
        if left is None:
            check(lib().bp_cs_allocate_multipliers(self.h, None, None, C.c_size_t(count), C.byref(first)), "bp_cs_allocate_multipliers")
        else:
            l, r = u64arr(left, 4), u64arr(right, 4)
            check(lib().bp_cs_allocate_multipliers(self.h, ptr(l), ptr(r), C.c_size_t(len(l)), C.byref(first)), "bp_cs_allocate_multipliers")
        return first.value

    def constrain_many(self, vars_, coefs, offsets):
        """bulk constrain in CSR form: constraint q owns terms [offsets[q], offsets[q+1])"""
        v = np.ascontiguousarray(vars_, dtype=np.uint32).reshape(-1, 2)
        c = u64arr(coefs, 4)
        off = (C.c_size_t * len(offsets))(*[int(x) for x in offsets])
        check(lib().bp_cs_constrain_many(self.h, ptr(v), ptr(c), off, C.c_size_t(len(offsets) - 1)), "bp_cs_constrain_many")

    def specify_randomized_constraints(self, fn):
        """fn(cs) runs in the randomized phase of prove / verify; cs.challenge_scalar(label) is available inside it"""
        me = self

        def thunk(_user, handle):
            try:
                view = me if handle == me.h.value else _ConstraintSystem(me.curve, None, C.c_void_p(handle))
                try:
                    fn(view)
                finally:
                    if view is not me:
                        view.h = None   # a borrowed handle (a like-instance of this gadget): not ours to free
                return 0
            except Exception as e:  # never unwind through C
                me._cb_errors.append(e)
                return -100

        cb = _RANDOMIZE_CB(thunk)
        self._cbs.append(cb)
        check(lib().bp_cs_specify_randomized_constraints(self.h, cb, None), "bp_cs_specify_randomized_constraints")

    def challenge_scalar(self, label):
        out = np.zeros(4, dtype=np.uint64)
        check(lib().bp_cs_challenge_scalar(self.h, bytes(label) + b"\0", ptr(out)), "bp_cs_challenge_scalar")
        return out

    def metrics(self):
        a, b, c = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        check(lib().bp_cs_metrics(self.h, C.byref(a), C.byref(b), C.byref(c)), "bp_cs_metrics")
        return a.value, b.value, c.value


class ProverCS(_ConstraintSystem):
    """r1cs::Prover (src/r1cs/prover.rs): `ProverCS(curve, transcript)` = Prover::new(&pc_gens, transcript) with
    PedersenGens::default(); pc_gens=(B, B_blinding) (8 ark words each) for a pair of the caller's choice"""

    def __init__(self, curve, transcript, pc_gens=None):
        super().__init__(curve, transcript)
        if pc_gens is None:
            check(lib().bp_prover_new(curve, transcript.h, C.byref(self.h)), "bp_prover_new")
        else:
            B, Bb = [np.ascontiguousarray(x, dtype=np.uint64).reshape(8) for x in pc_gens]
            check(lib().bp_prover_new_gens(curve, transcript.h, ptr(B), ptr(Bb), C.byref(self.h)), "bp_prover_new_gens")

    def new_like(self, transcript):
        """the next prover of this gadget without recording it again (bp_prover_new_like): freezes what this prover has recorded into
        a recording both share, and returns a prover on `transcript` with this one's Pedersen pair, no commitments and no witness.
        From here both accept only commits and, inside their randomized phase, recording calls."""
        p = ProverCS.__new__(ProverCS)
        _ConstraintSystem.__init__(p, self.curve, transcript)
        check(lib().bp_prover_new_like(self.h, transcript.h, C.byref(p.h)), "bp_prover_new_like")
        p._like = self   # its callbacks (ctypes thunks) serve this instance too
        return p

    def assign_multipliers(self, left, right):
        """the witness of a like-prover: a_L = left, a_R = right, (count, 4) ark words each, count = the recording's multipliers;
        a_O is their product and is not passed (bp_prover_assign_multipliers).  Exactly once, before proving or checking."""
        l, r = u64arr(left, 4), u64arr(right, 4)
        if len(l) != len(r):
            raise ValueError("assign_multipliers: left and right differ in length")
        check(lib().bp_prover_assign_multipliers(self.h, ptr(l), ptr(r), C.c_size_t(len(l))), "bp_prover_assign_multipliers")

    def assign_multipliers_dev(self, engine, left, right, count):
        """the same witness from device memory (bp_prover_assign_multipliers_dev): left and right are DeviceBuffers of `engine` (or
        None with count == 0) holding count x 4 ark words each, complete before the call.  The handle takes its own copy: the
        buffers are unread afterwards.  Proving, checking and batches then need an engine of the same device."""
        check(lib().bp_prover_assign_multipliers_dev(self.h, engine.ctx if engine is not None else None, left.ptr if left is not None else None,
                                                     right.ptr if right is not None else None, C.c_size_t(count)), "bp_prover_assign_multipliers_dev")

    def commit(self, v, v_blinding, engine=None):
        """Prover::commit for one value or for arrays of values: returns (V points (count, 8), variables)"""
        v, b = u64arr(v, 4), u64arr(v_blinding, 4)
        V = np.zeros((len(v), 8), dtype=np.uint64)
        vars_ = np.zeros((len(v), 2), dtype=np.uint32)
        check(lib().bp_prover_commit(self.h, engine.ctx if engine is not None else None, ptr(v), ptr(b), C.c_size_t(len(v)), ptr(V), ptr(vars_)), "bp_prover_commit")
        return V, _vars_out(vars_)

    def set_blinding(self, mode):
        """how prove() obtains s_L, s_R: BLINDING_TRANSCRIPT (the reference's draws, the default) or BLINDING_EXPANDED (one drawn key
        per phase, expanded on the GPU; include/arkbp.h).  Refused once the head of prove() has run."""
        check(lib().bp_prover_set_blinding(self.h, int(mode)), "bp_prover_set_blinding")

    @property
    def blinding(self):
        m = C.c_int(-1)
        check(lib().bp_prover_blinding(self.h, C.byref(m)), "bp_prover_blinding")
        return m.value

    def check(self, engine=None):
        """WitnessReport of what has been recorded so far (bp_prover_check): gates and constraints evaluated on the GPU with an
        engine, by the host twin without.  Consumes nothing and touches no transcript; pending randomized-phase callbacks are
        counted in deferred_callbacks and their constraints are not covered."""
        return _witness_check(self.h, engine)

    def set_check(self, on):
        """the guard (bp_prover_set_check): every proving route evaluates the whole witness after the randomized phase and refuses a
        violating one with BP_E_UNSATISFIED (UnsatisfiedError; in a batch: the instance's status) — no proof bytes.  Default off."""
        _set_check(self.h, on)

    def checking(self):
        return _checking(self.h)

    def precompute(self, rng_bytes=None):
        """the host-only head of prove() (bp_prover_precompute)"""
        check(lib().bp_prover_precompute(self.h, bytes(rng_bytes) if rng_bytes is not None else None), "bp_prover_precompute")

    def prove(self, engine, rng_bytes):
        """Prover::prove(prng, &bp_gens): rng_bytes = the 32 bytes the external prng yields; returns R1CSProof::to_bytes()"""
        buf = C.create_string_buffer(1 << 16)
        plen = C.c_size_t(len(buf))
        rc = lib().bp_prover_prove(engine.ctx, self.h, bytes(rng_bytes), buf, C.byref(plen), None)
        if self._cb_errors:
            raise self._cb_errors[0]
        src = getattr(self, "_like", None)
        if src is not None and src._cb_errors:
            raise src._cb_errors[0]
        check(rc, "bp_prover_prove")
        return buf.raw[: plen.value]


class VerifierCS(_ConstraintSystem):
    """r1cs::Verifier (src/r1cs/verifier.rs): `VerifierCS(curve, transcript)` = Verifier::new(transcript);
    `VerifierCS(curve, transcript, like=v0)` = the next instance of v0's gadget without recording it again."""

    def __init__(self, curve, transcript, like=None):
        super().__init__(curve, transcript)
        if like is None:
            check(lib().bp_verifier_new(curve, transcript.h, C.byref(self.h)), "bp_verifier_new")
        else:
            check(lib().bp_verifier_new_like(like.h, transcript.h, C.byref(self.h)), "bp_verifier_new_like")
            self._like = like   # its callbacks (ctypes thunks) serve this instance too

    def commit(self, V):
        V = u64arr(V, 8)
        vars_ = np.zeros((len(V), 2), dtype=np.uint32)
        check(lib().bp_verifier_commit(self.h, ptr(V), C.c_size_t(len(V)), ptr(vars_)), "bp_verifier_commit")
        return _vars_out(vars_)

    def commit_compressed(self, blob, defer=True, engine=None):
        """`commit(G::deserialize_compressed(..)?)` for the len(blob) / 33 encodings of blob, in order.  defer=True: stored as
        pending wire commitments (decoded by whatever verifies, or by materialize()); defer=False: decoded and committed now,
        which needs an engine.  Returns the variables."""
        return _verifier_commit_compressed_batch(engine, [self], [blob], defer=defer)[0]

    def materialize(self, engine=None):
        """decodes and commits the pending wire commitments (GPU with an engine, host square roots without); returns the C status"""
        return lib().bp_verifier_materialize(engine.ctx if engine is not None else None, self.h)

    def verify(self, engine, proof):
        """Verifier::verify(&proof, &pc_gens, &bp_gens): returns the C status (0 = Ok(()))"""
        return lib().bp_verifier_verify(engine.ctx, self.h, bytes(proof), C.c_size_t(len(proof)))


def points_compress(curve, xy):
    """affine ark words (n, 8) -> n x 33 bytes of ark-serialize's compressed encoding (all-zero words: the identity)"""
    xy = u64arr(xy, 8)
    out = C.create_string_buffer(max(33 * len(xy), 1))
    check(lib().bp_points_compress(int(curve), ptr(xy), C.c_size_t(len(xy)), out), "bp_points_compress")
    return out.raw[: 33 * len(xy)]


def _points_decompress(self, compressed):
    """compressed: bytes of n x 33; returns (points (n, 8) u64, ok (n,) u8): a rejected encoding gives zero words and ok = 0"""
    n = len(compressed) // 33
    out = np.zeros((n, 8), dtype=np.uint64)
    ok = np.zeros(n, dtype=np.uint8)
    check(lib().bp_points_decompress(self.ctx, bytes(compressed), C.c_size_t(n), ptr(out), ptr(ok)), "bp_points_decompress")
    return out, ok


def _verifier_commit_compressed_batch(self, verifiers, blobs, defer=False, want_status=False):
    """bp_verifier_commit_compressed_batch: verifier k receives the len(blobs[k]) / 33 encodings of blobs[k].  Returns the
    variables per verifier; with want_status (rc, per-verifier statuses, variables) instead of raising on a rejected encoding."""
    n = len(verifiers)
    hs = (C.c_void_p * max(n, 1))(*[v.h for v in verifiers])
    ms = [len(b) // 33 for b in blobs]
    m_each = (C.c_size_t * max(n, 1))(*ms)
    blob = b"".join(bytes(b) for b in blobs)
    vars_ = np.zeros((max(sum(ms), 1), 2), dtype=np.uint32)
    st = np.zeros(max(n, 1), dtype=np.int32)
    rc = lib().bp_verifier_commit_compressed_batch(self.ctx if self is not None else None, C.c_size_t(n), hs, m_each, blob if blob else None, int(bool(defer)), ptr(vars_), ptr(st))
    out, at = [], 0
    for m in ms:
        out.append(_vars_out(vars_[at:at + m]))
        at += m
    if want_status:
        return rc, st[:n].copy(), out
    check(rc, "bp_verifier_commit_compressed_batch")
    return out


def _commit_wire_stats(self):
    """wire commitments decoded since ctx creation: (by the device front end, by the GPU codec launch, by host square roots)"""
    a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_commit_wire_stats(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "bp_ctx_commit_wire_stats")
    return a.value, b.value, c.value


Engine.points_decompress = _points_decompress
Engine.verifier_commit_compressed_batch = _verifier_commit_compressed_batch
Engine.commit_wire_stats = _commit_wire_stats


def batch_verify_cs(engine, verifiers, proofs, alphas, want_point=False):
    """batch_verify(prng, instances, ..) over VerifierCS objects; alphas: (count, 4) words, the per-instance weights the
    reference draws from its prng (src/r1cs/verifier.rs:649) — required: equal weights would let the errors of two invalid
    proofs cancel.  Only a batch of ONE instance (Verifier::verify) may pass None.
    Returns the status, or (status, mega-check point) with want_point."""
    n = len(verifiers)
    if alphas is None and n > 1:
        raise ValueError("batch_verify_cs: per-instance weights (alphas) are required for more than one instance")
    hs = (C.c_void_p * max(n, 1))(*[v.h for v in verifiers])
    blob = b"".join(bytes(p) for p in proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    al = None if alphas is None else u64arr(alphas, 4)
    pt = np.zeros(8, dtype=np.uint64)
    rc = lib().bp_r1cs_batch_verify(engine.ctx, C.c_size_t(n), hs, blob, lens, ptr(al) if al is not None else None, None, ptr(pt))
    for v in verifiers:
        if v._cb_errors:
            raise v._cb_errors[0]
        src = getattr(v, "_like", None)
        if src is not None and src._cb_errors:
            raise src._cb_errors[0]
    return (rc, pt) if want_point else rc


def transcript_state(t):
    out = C.create_string_buffer(203)
    check(lib().bp_transcript_export_state(t.h, out), "bp_transcript_export_state")
    return out.raw


def transcript_from_state(state):
    t = HostTranscript(b"")
    check(lib().bp_transcript_import_state(t.h, bytes(state)), "bp_transcript_import_state")
    return t


def _debug_exp_iter(self, x, n):
    out = np.zeros((n, 4), dtype=np.uint64)
    check(lib().bp_debug_exp_iter(self.ctx, ptr(np.ascontiguousarray(x, dtype=np.uint64).reshape(4)), C.c_size_t(n), ptr(out)), "bp_debug_exp_iter")
    return out


def _debug_inner_product(self, a, b):
    a, b = u64arr(a, 4), u64arr(b, 4)
    out = np.zeros(4, dtype=np.uint64)
    check(lib().bp_debug_inner_product(self.ctx, ptr(a), ptr(b), C.c_size_t(len(a)), ptr(out)), "bp_debug_inner_product")
    return out


Engine.debug_exp_iter = _debug_exp_iter


# ---- blinding vectors from a key (include/arkbp.h BP_BLINDING_*) ------------------------------------------------------------
BLINDING_TRANSCRIPT = 0
BLINDING_EXPANDED = 1


def host_blind_expand(curve, kappa, j0, count):
    """(s_L, s_R), each (count, 4) ark words: the expansion of kappa (4 ark words) at the phase-local indices j0 .. j0 + count - 1, on the host"""
    sL, sR = np.zeros((count, 4), dtype=np.uint64), np.zeros((count, 4), dtype=np.uint64)
    k = np.ascontiguousarray(kappa, dtype=np.uint64).reshape(4)
    check(lib().bp_host_blind_expand(curve, ptr(k), C.c_uint64(j0), C.c_size_t(count), ptr(sL), ptr(sR)), "bp_host_blind_expand")
    return sL, sR


def _debug_blind_expand(self, kappa, j0, count):
    """the same through the production kernel (test hook)"""
    sL, sR = np.zeros((count, 4), dtype=np.uint64), np.zeros((count, 4), dtype=np.uint64)
    k = np.ascontiguousarray(kappa, dtype=np.uint64).reshape(4)
    check(lib().bp_debug_blind_expand(self.ctx, ptr(k), C.c_uint64(j0), C.c_size_t(count), ptr(sL), ptr(sR)), "bp_debug_blind_expand")
    return sL, sR


def _blinding_stats(self):
    """(scalars the expansion kernels wrote, their launches) since the engine was created"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_blinding_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_blinding_stats")
    return a.value, b.value


def _prover_like_stats(self):
    """like-provers on this engine since it was created (bp_ctx_prover_like_stats): (uploads of a recording's constraint index, proofs
    that found it resident, bytes resident now, gate outputs formed by the GPU kernel, gate outputs formed on the host)"""
    v = [C.c_uint64(0) for _ in range(5)]
    check(lib().bp_ctx_prover_like_stats(self.ctx, *[C.byref(x) for x in v]), "bp_ctx_prover_like_stats")
    return tuple(x.value for x in v)


def _witness_range_bits(self, values, nbits=64):
    """the witness of the range gadget built on the GPU (bp_witness_range_bits_dev): uploads the 64-bit `values` (8 bytes each) and
    returns two DeviceBuffers (left, right) of len(values) * nbits ark scalars: element j * nbits + i is 1 - bit i of value j on the
    left and the bit on the right.  A helper: any kernel that writes ark words serves assign_multipliers_dev equally well."""
    v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    total = len(v) * int(nbits)
    d_v = DeviceBuffer(self, max(v.nbytes, 8)).upload(v)
    left, right = DeviceBuffer(self, max(total * 32, 32)), DeviceBuffer(self, max(total * 32, 32))
    try:
        check(lib().bp_witness_range_bits_dev(self.ctx, d_v.ptr, C.c_size_t(len(v)), C.c_uint(int(nbits)), left.ptr, right.ptr), "bp_witness_range_bits_dev")
    except Exception:
        left.free(); right.free()
        raise
    finally:
        d_v.free()
    return left, right


def _witness_dev_stats(self):
    """witnesses assigned from device memory on this engine since it was created (bp_ctx_witness_dev_stats): (assignments accepted,
    multipliers the import kernel read from device memory, multipliers taken to the host instead)"""
    v = [C.c_uint64(0) for _ in range(3)]
    check(lib().bp_ctx_witness_dev_stats(self.ctx, *[C.byref(x) for x in v]), "bp_ctx_witness_dev_stats")
    return tuple(x.value for x in v)


Engine.witness_range_bits = _witness_range_bits
Engine.witness_dev_stats = _witness_dev_stats
Engine.prover_like_stats = _prover_like_stats
Engine.debug_blind_expand = _debug_blind_expand
Engine.blinding_stats = _blinding_stats
Engine.debug_inner_product = _debug_inner_product


def _gens_fold_tables(self, count, window_bits=0, budget_bytes=0, rank=0, world=1):
    """fixed-base tables of G[0..count), H[0..count) for the first fold round(s) of the prover (bp_gens_fold_tables); with
    world > 1 only this rank's slice of them (the generators rank + i * world: bp_gens_fold_tables_slice) — what the index-cyclic
    inner-product argument of a sharded prover looks up.  Returns (window bits chosen, table bytes)"""
    w, nbytes = C.c_int(0), C.c_size_t(0)
    if world > 1:
        check(lib().bp_gens_fold_tables_slice(self.ctx, C.c_size_t(count), int(window_bits), C.c_size_t(budget_bytes), int(rank), int(world), C.byref(w), C.byref(nbytes)),
              "bp_gens_fold_tables_slice")
    else:
        check(lib().bp_gens_fold_tables(self.ctx, C.c_size_t(count), int(window_bits), C.c_size_t(budget_bytes), C.byref(w), C.byref(nbytes)), "bp_gens_fold_tables")
    return w.value, nbytes.value


Engine.gens_fold_tables = _gens_fold_tables


def _gens_msm_tables(self, count):
    """fixed-base rows of G[0..count), H[0..count) and PedersenGens for the prover's MSMs over the generator tables
    (bp_gens_msm_tables); returns the table bytes"""
    nbytes = C.c_size_t(0)
    check(lib().bp_gens_msm_tables(self.ctx, C.c_size_t(count), C.byref(nbytes)), "bp_gens_msm_tables")
    return nbytes.value


Engine.gens_msm_tables = _gens_msm_tables


def _gens_tables_check(self):
    """bp_gens_tables_check: (fold-table entries, fixed-base MSM rows) that break the chain rule — (0, 0) for sound tables"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_gens_tables_check(self.ctx, C.byref(a), C.byref(b)), "bp_gens_tables_check")
    return a.value, b.value


TABLES_DIRECT, TABLES_PC_DIRECT, TABLES_PC_WIDE, TABLES_RESIDENT, TABLES_KINDS = 0, 1, 2, 3, 4   # include/arkbp.h BP_TABLES_*
K_DT_CHECK = 17                          # BP_K_DT_CHECK (Engine.kernel_time)
K_WITNESS_CHECK = 18                     # BP_K_WITNESS_CHECK: the witness-check kernels


def _gens_direct_tables_check(self):
    """bp_gens_direct_tables_check: (bad, first_bad, checked), three lists of TABLES_KINDS integers — per kind of table (the direct
    window tables, those of B and B_blinding alone, the 8-bit commitment tables, the resident points) the entries that fail their
    own rule, the smallest index of one (2**64 - 1: none) and the entries examined (0: the table is not built)"""
    arrs = [(C.c_uint64 * TABLES_KINDS)() for _ in range(3)]
    check(lib().bp_gens_direct_tables_check(self.ctx, *arrs), "bp_gens_direct_tables_check")
    return tuple([int(v) for v in a] for a in arrs)


GENS_G, GENS_H, GENS_PEDERSEN, GENS_KINDS = 0, 1, 2, 3   # include/arkbp.h BP_GENS_*


class _GensReportC(C.Structure):
    _fields_ = [(n, C.c_uint64 * GENS_KINDS) for n in ("checked", "bad", "first_bad")]


class GensReport:
    """bp_gens_report: per kind (GENS_G, GENS_H, GENS_PEDERSEN) the resident entries compared (0: nothing to compare with — the
    generators were installed by the caller, not derived), those whose words differ, and the smallest index of one (NONE_BAD when none)."""

    def __init__(self, c):
        self.checked, self.bad, self.first_bad = (tuple(int(v) for v in getattr(c, n)) for n in ("checked", "bad", "first_bad"))

    @property
    def clean(self):
        return not any(self.bad)

    def astuple(self):
        return (self.checked, self.bad, self.first_bad)

    def __eq__(self, other):
        return isinstance(other, GensReport) and self.astuple() == other.astuple()

    def __repr__(self):
        return "GensReport(checked=%r, bad=%r, first_bad=%r)" % self.astuple()


# bp_gens_digest / bp_host_gens_digest: 32 bytes each — the root over everything, and the roots of the Pedersen pair, of G[0..n) and of
# H[0..n) it is made of
GensDigest = collections.namedtuple("GensDigest", "root pair G H")


def _gens_digest_of(raw128):
    raw128 = bytes(raw128)
    return GensDigest(*(raw128[k * 32:(k + 1) * 32] for k in range(4)))


def _gens_check(self):
    """bp_gens_check: the resident generators against party 0's chain derived again (derived generators only), and the resident
    Pedersen pair against the pair this engine holds.  Reads and compares; repairs nothing."""
    r = _GensReportC()
    check(lib().bp_gens_check(self.ctx, C.byref(r)), "bp_gens_check")
    return GensReport(r)


def _gens_digest(self, n=None):
    """bp_gens_digest of the resident pair and G[0..n), H[0..n) (n: the installed capacity unless given); host_gens_digest over a copy
    of the same points gives the same GensDigest"""
    out = (C.c_uint8 * 128)()
    check(lib().bp_gens_digest(self.ctx, C.c_size_t(getattr(self, "gens_capacity", 0) if n is None else n), out), "bp_gens_digest")
    return _gens_digest_of(out)


def host_gens_digest(curve, G_xy, H_xy, B, Bb, n=None):
    """bp_host_gens_digest: the same digest from the caller's own points (ark words), on the host; it hashes bytes and validates nothing"""
    G, H = u64arr(G_xy, 8), u64arr(H_xy, 8)
    n = min(len(G), len(H)) if n is None else n
    assert n <= len(G) and n <= len(H)
    b, bb = (np.ascontiguousarray(p, dtype=np.uint64).reshape(8) for p in (B, Bb))
    out = (C.c_uint8 * 128)()
    check(lib().bp_host_gens_digest(int(curve), ptr(G), ptr(H), C.c_size_t(n), ptr(b), ptr(bb), out), "bp_host_gens_digest")
    return _gens_digest_of(out)


def _debug_tables_ptr(self, which):
    p, n = C.c_void_p(), C.c_size_t(0)
    check(lib().bp_debug_tables_ptr(self.ctx, int(which), C.byref(p), C.byref(n)), "bp_debug_tables_ptr")
    return p.value, n.value


def _debug_poke(self, dptr, data=None, nbytes=0):
    """reads (data is None) or writes raw device bytes at an address of this ctx's device (tests corrupt a table entry with it)"""
    if data is None:
        out = np.zeros(nbytes, dtype=np.uint8)
        check(lib().bp_dev_download(self.ctx, ptr(out), C.c_void_p(dptr), C.c_size_t(nbytes)), "bp_dev_download")
        return out
    arr = np.ascontiguousarray(data, dtype=np.uint8)
    check(lib().bp_dev_upload(self.ctx, C.c_void_p(dptr), ptr(arr), C.c_size_t(arr.nbytes)), "bp_dev_upload")


def _debug_table_points(self, which):
    """every entry of table `which` (bp_debug_tables_ptr) as ark words, (entries, 8): bp_points_export into a buffer of its own, then
    one download.  None when the table is not built."""
    dptr, nbytes = self.debug_tables_ptr(which)
    if not dptr:
        return None
    buf = DeviceBuffer(self, nbytes)
    try:
        check(lib().bp_points_export(self.ctx, C.c_void_p(dptr), buf.ptr, C.c_size_t(nbytes // 64)), "bp_points_export")
        self.sync()
        return buf.download().reshape(-1, 8)
    finally:
        buf.free()


DT_MAXSEG, DT_MAXOUT, DT_DESC_WORDS = 3, 6, 18   # csrc/small.cuh; include/arkbp.h BP_DEBUG_DT_DESC_WORDS


def _debug_msm_direct(self, jobs, with_workgroups=False):
    """bp_debug_msm_direct: sums over the direct window tables through the prover's msm_direct.  jobs = 1 .. 6 of (segments, imm):
    segments = up to three (base0, count, format, fold_n, fold_hi, scalars (n, 4) u64), imm = None or (base, 256-bit integer).
    Returns the (len(jobs), 8) affine results (the identity is all-zero), with_workgroups: and k_dt_accum's workgroups per job."""
    n = len(jobs)
    desc = np.zeros((n, DT_DESC_WORDS), dtype=np.uint32)
    imm = np.zeros((n, 4), dtype=np.uint64)
    ptrs, lens, keep = (C.c_void_p * (DT_MAXSEG * n))(), (C.c_size_t * (DT_MAXSEG * n))(), []
    for j, (segs, im) in enumerate(jobs):
        if len(segs) > DT_MAXSEG:
            raise ValueError("debug_msm_direct: more than %d segments" % DT_MAXSEG)
        desc[j, 0] = len(segs)
        if im is not None:
            desc[j, 1], desc[j, 2] = 1, im[0]
            imm[j] = [(int(im[1]) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
        for s, (base0, count, fmt, fold_n, fold_hi, sc) in enumerate(segs):
            desc[j, 3 + 5 * s: 8 + 5 * s] = [base0, count, fmt, fold_n, fold_hi]
            sc = u64arr(sc, 4)
            keep.append(sc)
            ptrs[DT_MAXSEG * j + s], lens[DT_MAXSEG * j + s] = sc.ctypes.data, len(sc)
    out = np.zeros((n, 8), dtype=np.uint64)
    nblk = C.c_uint32(0)
    check(lib().bp_debug_msm_direct(self.ctx, C.c_size_t(n), ptr(desc), ptr(imm), ptrs, lens, ptr(out), C.byref(nblk)), "bp_debug_msm_direct")
    return (out, nblk.value) if with_workgroups else out


Engine.gens_tables_check = _gens_tables_check
Engine.gens_direct_tables_check = _gens_direct_tables_check
Engine.gens_check = _gens_check
Engine.gens_digest = _gens_digest
Engine.debug_tables_ptr = _debug_tables_ptr
Engine.debug_table_points = _debug_table_points
Engine.debug_msm_direct = _debug_msm_direct
Engine.debug_poke = _debug_poke


# ---- native collectives (RCCL inside the library) -------------------------------------------------------------------------
def rccl_unique_id():
    """ncclGetUniqueId (128 bytes): one rank makes it, the host's bootstrap hands it to the others"""
    out = C.create_string_buffer(128)
    check(lib().bp_rccl_unique_id(out), "bp_rccl_unique_id")
    return out.raw


def _rccl_init(self, unique_id, rank, world):
    """ncclCommInitRank on this ctx (collective): window-sharded mode with both exchanges as ncclAllGather on the ctx's stream"""
    check(lib().bp_ctx_rccl_init(self.ctx, bytes(unique_id), int(rank), int(world)), "bp_ctx_rccl_init")


def _rccl_shutdown(self):
    check(lib().bp_ctx_rccl_shutdown(self.ctx), "bp_ctx_rccl_shutdown")


def _collective_stats(self):
    n, s = C.c_uint64(0), C.c_double(0)
    check(lib().bp_ctx_collective_stats(self.ctx, C.byref(n), C.byref(s)), "bp_ctx_collective_stats")
    return n.value, s.value


def _debug_rccl_allgather(self, block, world):
    blk = np.ascontiguousarray(block, dtype=np.uint8).reshape(-1)
    out = np.zeros((world, blk.size), dtype=np.uint8)
    check(lib().bp_debug_rccl_allgather(self.ctx, ptr(blk), C.c_size_t(blk.size), ptr(out)), "bp_debug_rccl_allgather")
    return out


Engine.rccl_init = _rccl_init
Engine.rccl_shutdown = _rccl_shutdown
Engine.collective_stats = _collective_stats
Engine.debug_rccl_allgather = _debug_rccl_allgather


# ---- verifier front end on the device (csrc/vfe.hip): test hooks ----------------------------------------------------------
TUNE_VFY_DEVICE = 11                 # include/arkbp.h BP_TUNE_VFY_DEVICE (Engine.set_tuning)
VFY_DEVICE_OFF, VFY_DEVICE_SINGLE_PHASE, VFY_DEVICE_TWO_PHASE = 0, 1, 2   # its values: host replay / single-phase like-instances (default) / two-phase ones too


def vfe_schedule_replay(state203, absorb_commitments, m, k, n, items):
    """CPU run of the data-independent sponge schedule of one verification (bp_debug_vfe_schedule_replay).  items: (count, 72)
    uint8.  Returns ((6 + k, 32) uint8 challenge seeds, number of Keccak-f permutations)."""
    items = np.ascontiguousarray(items, dtype=np.uint8)
    seeds = np.zeros((6 + k, 32), dtype=np.uint8)
    nb = C.c_uint32(0)
    check(lib().bp_debug_vfe_schedule_replay(bytes(state203), int(bool(absorb_commitments)), C.c_uint64(m), C.c_uint32(k), C.c_uint64(n), ptr(items), ptr(seeds), C.byref(nb)),
          "bp_debug_vfe_schedule_replay")
    return seeds, nb.value


def vfe_schedule_replay_2phase(state203, absorb_commitments, m, k, n, labels, items):
    """The same for a two-phase statement (bp_debug_vfe_schedule_replay_2phase): after S1 the "r1cs-2phase" separator and one
    challenge per gadget label (bytes, drawing order).  Returns ((6 + k + G, 32) uint8 seeds in the order y z u x w u_1..u_k r
    g_1..g_G, number of Keccak-f permutations)."""
    items = np.ascontiguousarray(items, dtype=np.uint8)
    G = len(labels)
    seeds = np.zeros((6 + k + G, 32), dtype=np.uint8)
    nb = C.c_uint32(0)
    arr = (C.c_char_p * max(G, 1))(*[bytes(l) for l in labels])
    check(lib().bp_debug_vfe_schedule_replay_2phase(bytes(state203), int(bool(absorb_commitments)), C.c_uint64(m), C.c_uint32(k), C.c_uint64(n), arr, C.c_size_t(G),
                                                    ptr(items), ptr(seeds), C.byref(nb)), "bp_debug_vfe_schedule_replay_2phase")
    return seeds, nb.value


def _debug_vfe_challenges(self, proofs, commitments, states203, absorb_commitments):
    """k_vfe_points + k_vfe_sponge for same-shaped proofs.  proofs: list of equal-length bytes; commitments: (count, m, 8) uint64 ark
    words; states203: one 203-byte state (shared) or one per proof.  Returns (seeds (count, 6 + k, 32) uint8,
    challenges (count, 6 + k, 4) uint64 ark words, status)."""
    count, plen = len(proofs), len(proofs[0])
    assert all(len(p) == plen for p in proofs)
    k = (plen - 539) // 66
    V = np.ascontiguousarray(commitments, dtype=np.uint64).reshape(count, -1, 8)
    m = V.shape[1]
    shared = isinstance(states203, (bytes, bytearray))
    st = bytes(states203) if shared else b"".join(bytes(s) for s in states203)
    seeds = np.zeros((count, 6 + k, 32), dtype=np.uint8)
    chal = np.zeros((count, 6 + k, 4), dtype=np.uint64)
    status = C.c_uint32(0)
    blob = b"".join(proofs)
    check(lib().bp_debug_vfe_challenges(self.ctx, C.c_size_t(count), blob, C.c_size_t(plen), ptr(V) if m else None, C.c_size_t(m), st, int(shared), int(bool(absorb_commitments)),
                                        ptr(seeds), ptr(chal), C.byref(status)), "bp_debug_vfe_challenges")
    return seeds, chal, status.value


def _vfe_stats(self):
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_vfe_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_vfe_stats")
    return a.value, b.value


Engine.debug_vfe_challenges = _debug_vfe_challenges
Engine.vfe_stats = _vfe_stats

# batches of several gadgets: classes of like-instances inside one call (include/arkbp.h "Batches of several gadgets")
TUNE_VFY_CLASS_MIN = 24              # include/arkbp.h BP_TUNE_VFY_CLASS_MIN (Engine.set_tuning; 0 = default, 1 = every class)
VFY_MAX_CLASSES = 8                  # BP_VFY_MAX_CLASSES


def _vfe_class_stats(self):
    """(calls that took the class path, classes the device finished, their members, instances the host replay took in such calls,
    instances replayed because the device flagged something) since ctx creation (bp_ctx_vfe_class_stats)"""
    v = [C.c_uint64(0) for _ in range(5)]
    check(lib().bp_ctx_vfe_class_stats(self.ctx, *[C.byref(x) for x in v]), "bp_ctx_vfe_class_stats")
    return tuple(x.value for x in v)


def debug_vfy_class_plan(keys, eligible=None, class_min=0, max_classes=0):
    """host only (bp_debug_vfy_class_plan): the partition of a batch into device classes.  keys: one 64-bit class key per instance;
    eligible: one truth value per instance (None: all).  class_min / max_classes 0 = the defaults.  Returns (class_of, nclasses):
    class_of[k] is the device class of instance k in launch order, or -1 for the remainder."""
    n = len(keys)
    ks = np.ascontiguousarray(list(keys) + [0], dtype=np.uint64)
    el = None if eligible is None else np.ascontiguousarray([1 if x else 0 for x in eligible] + [0], dtype=np.uint8)
    out = np.full(n + 1, -2, dtype=np.int32)
    nc = C.c_uint32(0)
    check(lib().bp_debug_vfy_class_plan(C.c_size_t(n), ptr(ks), ptr(el) if el is not None else None, C.c_uint64(class_min), C.c_uint32(max_classes), ptr(out), C.byref(nc)),
          "bp_debug_vfy_class_plan")
    return [int(x) for x in out[:n]], nc.value


Engine.vfe_class_stats = _vfe_class_stats


def debug_verify_challenges(curve, instances, use_x8):
    """host only: the challenge sequences of up to eight scenario verifications (bp_debug_verify_challenges).  Returns a list of
    (nchal, 4) uint64 arrays, or None when the lockstep replay does not apply to the group."""
    pk = instances if isinstance(instances, PackedInstances) else PackedInstances(instances)
    out = np.zeros((pk.n, 40, 4), dtype=np.uint64)
    nch = (C.c_size_t * pk.n)()
    rc = lib().bp_debug_verify_challenges(curve, C.c_size_t(pk.n), pk.scen, ptr(pk.prm), pk.proofs, pk.plens, ptr(pk.cms), pk.ms, ptr(pk.pubs), pk.npubs, int(bool(use_x8)),
                                          ptr(out), nch)
    if rc == 1:
        return None
    check(rc, "bp_debug_verify_challenges")
    return [out[j, : nch[j]].copy() for j in range(pk.n)]


def _msm_stats(self):
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_msm_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_msm_stats")
    return a.value, b.value


Engine.msm_stats = _msm_stats


def _direct_stats(self):
    """(MSMs answered from the direct window tables of the small-statement path, generators per vector the tables cover)"""
    a, b = C.c_uint64(0), C.c_size_t(0)
    check(lib().bp_ctx_direct_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_direct_stats")
    return a.value, b.value


Engine.direct_stats = _direct_stats


def _gens_direct_tables(self, count):
    """bp_gens_direct_tables: build (count > 0) or free (0) the direct window tables of the small-statement path; returns their size in bytes"""
    nbytes = C.c_size_t(0)
    check(lib().bp_gens_direct_tables(self.ctx, C.c_size_t(count), C.byref(nbytes)), "bp_gens_direct_tables")
    return nbytes.value


Engine.gens_direct_tables = _gens_direct_tables


def _fold_stats(self):
    """(first folds deferred, second folds produced straight from the fold tables) — the two-rounds-from-the-tables schedule"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_fold_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_fold_stats")
    return a.value, b.value


Engine.fold_stats = _fold_stats

TUNE_MSM_PAIR = 21                   # include/arkbp.h BP_TUNE_MSM_PAIR (Engine.set_tuning)
MSM_PAIR_RUNS = 6                    # BP_DEBUG_MSM_PAIR_RUNS


def _msm_pair_stats(self):
    """(passes in which the L and R MSMs of an inner-product round ran as two jobs of one launch chain, jobs of those redone alone)"""
    a, b = C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_msm_pair_stats(self.ctx, C.byref(a), C.byref(b)), "bp_ctx_msm_pair_stats")
    return a.value, b.value


def _debug_msm_pair(self, runs, d_scalars, n, canonical=False, latency_first=False):
    """bp_debug_msm_pair: two MSMs of n terms through the prover's msm_run_pair.  runs: per job a list of up to MSM_PAIR_RUNS
    (DeviceBuffer of resident points, first point, count); d_scalars: two DeviceBuffers of n scalars.  Returns the two affine sums
    as a (2, 8) uint64 array (ark words)."""
    if len(runs) != 2 or len(d_scalars) != 2 or any(len(r) > MSM_PAIR_RUNS for r in runs):
        raise ValueError("debug_msm_pair: two jobs of at most %d runs" % MSM_PAIR_RUNS)
    ptrs = (C.c_void_p * (2 * MSM_PAIR_RUNS))()
    counts = (C.c_size_t * (2 * MSM_PAIR_RUNS))()
    for j, job in enumerate(runs):
        for r, (buf, first, count) in enumerate(job):
            ptrs[j * MSM_PAIR_RUNS + r] = buf.ptr.value + 64 * int(first)
            counts[j * MSM_PAIR_RUNS + r] = int(count)
    sc = (C.c_void_p * 2)(d_scalars[0].ptr.value, d_scalars[1].ptr.value)
    out = np.zeros((2, 8), dtype=np.uint64)
    check(lib().bp_debug_msm_pair(self.ctx, ptrs, counts, sc, C.c_size_t(n), int(canonical), int(latency_first), ptr(out)), "bp_debug_msm_pair")
    return out


Engine.msm_pair_stats = _msm_pair_stats
Engine.debug_msm_pair = _debug_msm_pair


FOLD_LADDER, FOLD_LADDER_NAF, FOLD_TAB, FOLD_TAB2 = 0, 1, 2, 3   # include/arkbp.h BP_DEBUG_FOLD_*
FOLD_TOOK_GLV, FOLD_TOOK_NAF, FOLD_TOOK_QUAD, FOLD_TOOK_FINISH, FOLD_TOOK_TAB, FOLD_TOOK_TAB2 = 1, 2, 4, 8, 16, 32   # bits of its *took


def _debug_fold(self, route, n, tG, tH, t2G=None, t2H=None, gens_first=0, gens_stride=1, G=None, H=None):
    """bp_debug_fold: one fold of n outputs per vector through the prover's launchers.  tG, tH (and t2G, t2H for FOLD_TAB2): the
    multipliers as ark words; G, H: the caller's 2n points each for the ladder routes.  Returns (G_out (n, 8), H_out (n, 8), took) —
    took = 0: the launcher declined and the outputs are all zero."""
    def words(t):
        return None if t is None else ptr(np.ascontiguousarray(t, dtype=np.uint64).reshape(4))
    keep = [None if v is None else u64arr(v, 8) for v in (G, H)]
    if any(v is not None and len(v) != 2 * n for v in keep):
        raise ValueError("debug_fold: the ladder routes take 2n points per vector")
    Go, Ho = np.zeros((n, 8), dtype=np.uint64), np.zeros((n, 8), dtype=np.uint64)
    took = C.c_uint32(0)
    check(lib().bp_debug_fold(self.ctx, int(route), C.c_size_t(n), words(tG), words(tH), words(t2G), words(t2H), C.c_uint32(gens_first), C.c_uint32(gens_stride),
                              None if keep[0] is None else ptr(keep[0]), None if keep[1] is None else ptr(keep[1]), ptr(Go), ptr(Ho), C.byref(took)), "bp_debug_fold")
    return Go, Ho, took.value


Engine.debug_fold = _debug_fold


def _prover_handle(p):
    """bp_cs* of a ProverCS or a scenario Statement (bp_stmt_as_prover)"""
    if isinstance(p, Statement):
        return C.c_void_p(lib().bp_stmt_as_prover(p.h))
    return p.h


def _prove_batch(self, provers, rng_bytes=None, timing=None, return_rc=False):
    """bp_prover_prove_batch over ProverCS objects and/or Statements (every one consumed).  rng_bytes: one 32-byte string per
    instance, or None when every prover has its rng already.  Returns [(status, proof_bytes)] in instance order (b"" for a failed
    instance) — a failing instance does not raise; the call raises only when the up-front checks refuse the whole batch.
    return_rc: return (the call's status — the first non-zero instance status —, the list) instead."""
    n = len(provers)
    if n == 0:
        return (0, []) if return_rc else []
    hs = (C.c_void_p * n)(*[_prover_handle(p) for p in provers])
    rb = None
    if rng_bytes is not None:
        if len(rng_bytes) != n or any(len(r) != 32 for r in rng_bytes):
            raise ValueError("prove_batch: one 32-byte rng string per instance")
        rb = b"".join(bytes(r) for r in rng_bytes)
    stride = 1 << 12
    out = C.create_string_buffer(stride * n)
    lens = (C.c_size_t * n)()
    st = (C.c_int * n)()
    tm = (C.c_double * 8)()
    rc = lib().bp_prover_prove_batch(self.ctx, C.c_size_t(n), hs, rb, out, C.c_size_t(stride), lens, st, tm)
    if timing is not None:
        timing[:] = list(tm)
    if rc != 0 and all(s == 0 for s in st):   # refused as a whole (nothing consumed) or a device error before any instance
        check(rc, "bp_prover_prove_batch")
    raw = out.raw
    res = [(st[k], raw[k * stride: k * stride + lens[k]]) for k in range(n)]
    return (rc, res) if return_rc else res


def _prover_commit_batch(self, provers, values, blindings):
    """bp_prover_commit_batch: values[k] / blindings[k] are the (m_k, 4) ark-word arrays of prover k.  Returns [(V (m_k, 8), variables)]."""
    n = len(provers)
    if n == 0:
        return []
    vs = [u64arr(v, 4) for v in values]
    bs = [u64arr(b, 4) for b in blindings]
    if any(a.shape != b.shape for a, b in zip(vs, bs)) or len(vs) != n or len(bs) != n:
        raise ValueError("prover_commit_batch: one (values, blindings) pair of equal length per prover")
    m = [len(a) for a in vs]
    tot = sum(m)
    v = np.ascontiguousarray(np.concatenate(vs) if tot else np.zeros((0, 4), dtype=np.uint64))
    b = np.ascontiguousarray(np.concatenate(bs) if tot else np.zeros((0, 4), dtype=np.uint64))
    V = np.zeros((max(tot, 1), 8), dtype=np.uint64)
    vars_ = np.zeros((max(tot, 1), 2), dtype=np.uint32)
    hs = (C.c_void_p * n)(*[_prover_handle(p) for p in provers])
    me = (C.c_size_t * n)(*m)
    check(lib().bp_prover_commit_batch(self.ctx, C.c_size_t(n), hs, me, ptr(v), ptr(b), ptr(V), ptr(vars_)), "bp_prover_commit_batch")
    res, off = [], 0
    for k in range(n):
        res.append((V[off: off + m[k]].copy(), _vars_out(vars_[off: off + m[k]])))
        off += m[k]
    return res


def _prove_batch_stats(self):
    """(instances whose inner-product argument ran in a lockstep group, instances proved one at a time, lockstep groups)"""
    a, b, g = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_prove_batch_stats(self.ctx, C.byref(a), C.byref(b), C.byref(g)), "bp_ctx_prove_batch_stats")
    return a.value, b.value, g.value


def _prove_batch_front_stats(self):
    """(instances whose front stages ran group-wide, front groups after the re-partition by padded size, host waits of those stages)"""
    a, g, w = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_prove_batch_front_stats(self.ctx, C.byref(a), C.byref(g), C.byref(w)), "bp_ctx_prove_batch_front_stats")
    return a.value, g.value, w.value


def _check_batch(self, provers):
    """bp_prover_check_batch: the WitnessReports of several provers (ProverCS and / or Statements) from one launch sequence and one wait"""
    n = len(provers)
    if n == 0:
        return []
    hs = (C.c_void_p * n)(*[_prover_handle(p) for p in provers])
    out = (_WitnessReportC * n)()
    check(lib().bp_prover_check_batch(self.ctx, C.c_size_t(n), hs, out), "bp_prover_check_batch")
    return [WitnessReport(r) for r in out]


def _last_unsatisfied(self):
    """[(instance index, WitnessReport)] of the instances this engine's most recent proving call refused with BP_E_UNSATISFIED"""
    cnt = C.c_size_t(0)
    check(lib().bp_ctx_last_unsatisfied(self.ctx, C.c_size_t(0), None, None, C.byref(cnt)), "bp_ctx_last_unsatisfied")
    n = cnt.value
    if n == 0:
        return []
    inst = (C.c_uint64 * n)()
    out = (_WitnessReportC * n)()
    check(lib().bp_ctx_last_unsatisfied(self.ctx, C.c_size_t(n), inst, out, C.byref(cnt)), "bp_ctx_last_unsatisfied")
    return [(int(inst[i]), WitnessReport(out[i])) for i in range(min(n, cnt.value))]


Engine.prove_batch = _prove_batch
Engine.check_batch = _check_batch
Engine.last_unsatisfied = _last_unsatisfied
Engine.prover_commit_batch = _prover_commit_batch
Engine.prove_batch_stats = _prove_batch_stats
Engine.prove_batch_front_stats = _prove_batch_front_stats


# ---- verification with a verdict per instance (bp_verifier_verify_batch) ----------------------------------------------------
TUNE_VERIFY_EACH = 15                # include/arkbp.h BP_TUNE_VERIFY_EACH (Engine.set_tuning)
VERIFY_EACH_WAITS_PER_GROUP = 1      # BP_VERIFY_EACH_WAITS_PER_GROUP


def _verify_each(self, verifiers, proofs, want_points=False, timing=None):
    """bp_verifier_verify_batch over VerifierCS objects (every one consumed): Verifier::verify for each instance, weight 1, in one
    call.  Returns (rc, statuses) — rc = the first non-zero status in instance order — or (rc, statuses, points (count, 8)) with
    want_points: the affine value of every instance's own mega-check, all-zero iff it is the identity.  Raises only when the
    up-front checks refuse the whole batch (nothing consumed then)."""
    n = len(verifiers)
    if len(proofs) != n:
        raise ValueError("verify_each: one proof per verifier")
    hs = (C.c_void_p * max(n, 1))(*[v.h for v in verifiers])
    blob = b"".join(bytes(p) for p in proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    st = (C.c_int * max(n, 1))(*([1] * max(n, 1)))   # (a status the library never returns: an instance it skipped would show)
    pts = np.zeros((max(n, 1), 8), dtype=np.uint64)
    tm = (C.c_double * 5)()
    rc = lib().bp_verifier_verify_batch(self.ctx, C.c_size_t(n), hs, blob, lens, st, ptr(pts) if want_points else None, tm)
    if timing is not None:
        timing[:] = list(tm)
    for v in verifiers:
        if v._cb_errors:
            raise v._cb_errors[0]
        src = getattr(v, "_like", None)
        if src is not None and src._cb_errors:
            raise src._cb_errors[0]
    if n and rc != 0 and all(s == 1 for s in st):   # refused as a whole
        check(rc, "bp_verifier_verify_batch")
    statuses = [st[k] for k in range(n)]
    return (rc, statuses, pts[:n]) if want_points else (rc, statuses)


def _verify_each_scenarios(self, instances, want_points=False, timing=None):
    """bp_r1cs_verify_each_scenarios; instances: list of (scenario, params, proof_bytes, commitments, publics) or a PackedInstances.
    Returns as verify_each."""
    pk = instances if isinstance(instances, PackedInstances) else PackedInstances(instances)
    n = pk.n
    st = (C.c_int * max(n, 1))(*([1] * max(n, 1)))
    pts = np.zeros((max(n, 1), 8), dtype=np.uint64)
    tm = (C.c_double * 5)()
    rc = lib().bp_r1cs_verify_each_scenarios(self.ctx, C.c_size_t(n), pk.scen, ptr(pk.prm), pk.proofs, pk.plens, ptr(pk.cms), pk.ms, ptr(pk.pubs), pk.npubs, st,
                                             ptr(pts) if want_points else None, tm)
    if timing is not None:
        timing[:] = list(tm)
    if n and rc != 0 and all(s == 1 for s in st):
        check(rc, "bp_r1cs_verify_each_scenarios")
    statuses = [st[k] for k in range(n)]
    return (rc, statuses, pts[:n]) if want_points else (rc, statuses)


def _verify_each_stats(self):
    """(instances that took the grouped path, instances verified by the single route, groups launched, host waits of the groups)"""
    a, b, g, w = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_verify_each_stats(self.ctx, C.byref(a), C.byref(b), C.byref(g), C.byref(w)), "bp_ctx_verify_each_stats")
    return a.value, b.value, g.value, w.value


def _debug_msm_each(self, jobs, canonical=False):
    """bp_debug_msm_each: jobs = list of (bases (n_j, 8), scalars (n_j, 4)); one variable-base MSM per job through k_ve_tail.
    Returns the (len(jobs), 8) affine results."""
    n = len(jobs)
    bs = [u64arr(b, 8) if len(b) else np.zeros((0, 8), dtype=np.uint64) for b, _ in jobs]
    ss = [u64arr(s, 4) if len(s) else np.zeros((0, 4), dtype=np.uint64) for _, s in jobs]
    if any(len(b) != len(s) for b, s in zip(bs, ss)):
        raise ValueError("msm_each: bases and scalars differ in length")
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(b) for b in bs])
    off_c = (C.c_size_t * (n + 1))(*[int(o) for o in offs])
    B = np.ascontiguousarray(np.concatenate(bs + [np.zeros((1, 8), dtype=np.uint64)]))
    S = np.ascontiguousarray(np.concatenate(ss + [np.zeros((1, 4), dtype=np.uint64)]))
    out = np.zeros((max(n, 1), 8), dtype=np.uint64)
    check(lib().bp_debug_msm_each(self.ctx, C.c_size_t(n), off_c, ptr(B), ptr(S), int(canonical), ptr(out)), "bp_debug_msm_each")
    return out[:n]


def debug_ve_plan(offsets, scalars_canonical, job):
    """host only (bp_debug_ve_plan): k_ve_tail's layout and digit functions for one job.  Returns (first term, terms,
    digits (terms, 64) uint8, planes (terms, 64) uint8, lanes (64,) uint32, group slots (64,) uint32)."""
    n = len(offsets) - 1
    off_c = (C.c_size_t * (n + 1))(*[int(o) for o in offsets])
    sc = u64arr(scalars_canonical, 4) if len(scalars_canonical) else np.zeros((1, 4), dtype=np.uint64)
    nt = int(offsets[job + 1]) - int(offsets[job])
    first, terms = C.c_uint32(0), C.c_uint32(0)
    dg, pl = np.zeros((max(nt, 1), 64), dtype=np.uint8), np.zeros((max(nt, 1), 64), dtype=np.uint8)
    lanes, groups = np.zeros(64, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    check(lib().bp_debug_ve_plan(C.c_size_t(n), off_c, ptr(sc), C.c_size_t(job), C.byref(first), C.byref(terms), ptr(dg), ptr(pl), ptr(lanes), ptr(groups)),
          "bp_debug_ve_plan")
    return first.value, terms.value, dg[:nt], pl[:nt], lanes, groups


Engine.verify_each = _verify_each
Engine.verify_each_scenarios = _verify_each_scenarios
Engine.verify_each_stats = _verify_each_stats
Engine.debug_msm_each = _debug_msm_each


# ---- batch verification that names the failing instances (bp_r1cs_batch_verify_locate) ----------------------------------------
TUNE_VERIFY_LOCATE_LEAF = 22         # include/arkbp.h BP_TUNE_VERIFY_LOCATE_LEAF (Engine.set_tuning; 0 = default: 1)


def batch_verify_locate_cs(engine, verifiers, proofs, alphas, timing=None):
    """bp_r1cs_batch_verify_locate over VerifierCS objects (every one consumed); alphas: (count, 4) words, non-zero, required for
    more than one instance.  Returns (rc, statuses): statuses[k] is what Verifier::verify returns for instance k alone — exact for
    a valid proof and for every instance decided on its own, with batch_verify's soundness over the weights for an invalid proof
    inside a subset that passed — and rc the first non-zero status in instance order.  Raises only when the up-front checks refuse
    the whole batch (nothing consumed then)."""
    n = len(verifiers)
    if len(proofs) != n:
        raise ValueError("batch_verify_locate_cs: one proof per verifier")
    hs = (C.c_void_p * max(n, 1))(*[v.h for v in verifiers])
    blob = b"".join(bytes(p) for p in proofs)
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    al = None if alphas is None else u64arr(alphas, 4)
    st = (C.c_int * max(n, 1))(*([1] * max(n, 1)))   # (a status the library never returns: an instance it skipped would show)
    tm = (C.c_double * 4)()
    rc = lib().bp_r1cs_batch_verify_locate(engine.ctx, C.c_size_t(n), hs, blob, lens, ptr(al) if al is not None else None, st, tm)
    if timing is not None:
        timing[:] = list(tm)
    for v in verifiers:
        if v._cb_errors:
            raise v._cb_errors[0]
        src = getattr(v, "_like", None)
        if src is not None and src._cb_errors:
            raise src._cb_errors[0]
    if n and rc != 0 and all(s == 1 for s in st):   # refused as a whole
        check(rc, "bp_r1cs_batch_verify_locate")
    return rc, [st[k] for k in range(n)]


def _batch_verify_locate(self, instances, alpha_seed, timing=None):
    """bp_r1cs_batch_verify_locate_scenarios; instances: list of (scenario, params, proof_bytes, commitments, publics) or a
    PackedInstances; the weights are batch_verify's (alpha_seed, instance order).  Returns as batch_verify_locate_cs."""
    pk = instances if isinstance(instances, PackedInstances) else PackedInstances(instances)
    n = pk.n
    st = (C.c_int * max(n, 1))(*([1] * max(n, 1)))
    tm = (C.c_double * 4)()
    rc = lib().bp_r1cs_batch_verify_locate_scenarios(self.ctx, C.c_size_t(n), pk.scen, ptr(pk.prm), pk.proofs, pk.plens, ptr(pk.cms), pk.ms, ptr(pk.pubs), pk.npubs,
                                                     bytes(alpha_seed) if alpha_seed is not None else None, st, tm)
    if timing is not None:
        timing[:] = list(tm)
    if n and rc != 0 and all(s == 1 for s in st):
        check(rc, "bp_r1cs_batch_verify_locate_scenarios")
    return rc, [st[k] for k in range(n)]


def _verify_locate_stats(self):
    """(calls, passes of the batch verifier's core, instances in those passes, instances decided exactly) since ctx creation"""
    a, b, g, w = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    check(lib().bp_ctx_verify_locate_stats(self.ctx, C.byref(a), C.byref(b), C.byref(g), C.byref(w)), "bp_ctx_verify_locate_stats")
    return a.value, b.value, g.value, w.value


def debug_locate_plan(fails_check, fails_before=None):
    """host only (bp_debug_locate_plan): the planner of batch_verify_locate over a simulated core.  fails_check / fails_before:
    one truth value per instance.  Returns (statuses, passes, instances_in_passes) with passes = [(lo, n, outcome)] over the list of
    instances still in the batch at that time; outcome 0 passed, 1 failed its check, 2 reported members failing before it."""
    n = len(fails_check)
    fc = np.ascontiguousarray([1 if x else 0 for x in fails_check] + [0], dtype=np.uint8)
    fb = None if fails_before is None else np.ascontiguousarray([1 if x else 0 for x in fails_before] + [0], dtype=np.uint8)
    cap = 2 * n + 2
    lo, cnt, failed = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint8)
    st = (C.c_int * max(n, 1))()
    npasses, inst = C.c_uint32(0), C.c_uint64(0)
    check(lib().bp_debug_locate_plan(C.c_size_t(n), ptr(fc), ptr(fb) if fb is not None else None, C.byref(npasses), ptr(lo), ptr(cnt), ptr(failed), C.byref(inst), st),
          "bp_debug_locate_plan")
    p = npasses.value
    return [st[k] for k in range(n)], [(int(lo[i]), int(cnt[i]), int(failed[i])) for i in range(p)], inst.value


Engine.batch_verify_locate = _batch_verify_locate
Engine.verify_locate_stats = _verify_locate_stats


# ---- many variable-base MSMs per call (bp_msm_batch) ---------------------------------------------------------------------------
TUNE_MSM_BATCH_SHORT, TUNE_MSM_BATCH_SLICE, TUNE_MSM_BATCH_MAX, TUNE_MSM_BATCH_MIN_JOBS = 16, 17, 18, 19   # include/arkbp.h BP_TUNE_MSM_BATCH_* (Engine.set_tuning; 0 = default)
MSM_BATCH_DEFAULTS = (8, None, 4096, 6)  # what 0 stands for: short, slice (None: msm_batch_default_slice), max, min jobs (csrc/msm_batch.inc MSB_DEFAULT_*)


def msm_batch_default_slice(bucketed_terms):
    """the slice cap in force when BP_TUNE_MSM_BATCH_SLICE is 0, for a call whose bucketed jobs hold this many terms (csrc/msm_batch.cuh msb_auto_slice)"""
    return min(max(-(-int(bucketed_terms) // 128), 64), 512)

MSM_BATCH_WAITS_PER_GROUP = 1            # BP_MSM_BATCH_WAITS_PER_GROUP
K_MSM_BATCH = 16                         # BP_K_MSM_BATCH (Engine.kernel_time)


def _job_offsets(lengths):
    offs = [0]
    for n in lengths:
        offs.append(offs[-1] + int(n))
    return offs, (C.c_size_t * len(offs))(*offs)


def _msm_batch(self, jobs, canonical=False):
    """bp_msm_batch: jobs = list of (bases (n_j, 8), scalars (n_j, 4)), as debug_msm_each takes them; one VariableBaseMSM::msm per job,
    in one call.  Returns the (len(jobs), 8) affine results (the identity is all-zero)."""
    n = len(jobs)
    bs = [u64arr(b, 8) if len(b) else np.zeros((0, 8), dtype=np.uint64) for b, _ in jobs]
    ss = [u64arr(s, 4) if len(s) else np.zeros((0, 4), dtype=np.uint64) for _, s in jobs]
    if any(len(b) != len(s) for b, s in zip(bs, ss)):
        raise ValueError("msm_batch: bases and scalars differ in length")
    _, off_c = _job_offsets([len(b) for b in bs])
    B = np.ascontiguousarray(np.concatenate(bs + [np.zeros((1, 8), dtype=np.uint64)]))
    S = np.ascontiguousarray(np.concatenate(ss + [np.zeros((1, 4), dtype=np.uint64)]))
    out = np.zeros((max(n, 1), 8), dtype=np.uint64)
    check(lib().bp_msm_batch(self.ctx, C.c_size_t(n), off_c, ptr(B), ptr(S), int(canonical), ptr(out)), "bp_msm_batch")
    return out[:n]


def _msm_batch_dev(self, d_bases, d_scalars, lengths, canonical=False):
    """bp_msm_batch_dev: resident operands (upload_points / upload_scalars), job j = the next lengths[j] terms.  Neither buffer is
    modified.  Returns the (len(lengths), 8) affine results."""
    n = len(lengths)
    _, off_c = _job_offsets(lengths)
    out = np.zeros((max(n, 1), 8), dtype=np.uint64)
    check(lib().bp_msm_batch_dev(self.ctx, C.c_size_t(n), off_c, d_bases.ptr, d_scalars.ptr, int(canonical), ptr(out)), "bp_msm_batch_dev")
    return out[:n]


def _msm_batch_stats(self):
    """(short jobs, bucketed jobs, single-route jobs, groups launched, host waits of the groups) since ctx creation"""
    v = [C.c_uint64(0) for _ in range(5)]
    check(lib().bp_ctx_msm_batch_stats(self.ctx, *[C.byref(x) for x in v]), "bp_ctx_msm_batch_stats")
    return tuple(x.value for x in v)


def debug_msm_batch_plan(lengths, scalars_canonical=None, job=0, short_max=0, slice_terms=0, batch_max=0):
    """host only (bp_debug_msm_batch_plan): the plan bp_msm_batch makes for jobs of these lengths under the given knob values (0 =
    default).  Returns (routes (count,) uint8, nslices (count,) uint32, slice_first, slice_len (nslices[job],) uint32,
    digits (terms of `job`, 64) int8 or None without scalars)."""
    n = len(lengths)
    offs, off_c = _job_offsets(lengths)
    route, nsl = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32)
    knobs = (C.c_uint64(int(short_max)), C.c_uint64(int(slice_terms)), C.c_uint64(int(batch_max)))
    check(lib().bp_debug_msm_batch_plan(C.c_size_t(n), off_c, *knobs, None, C.c_size_t(job), ptr(route), ptr(nsl), None, None, None), "bp_debug_msm_batch_plan")
    S, nt = int(nsl[job]), int(lengths[job])
    first, length = np.zeros(max(S, 1), dtype=np.uint32), np.zeros(max(S, 1), dtype=np.uint32)
    dg = np.zeros((max(nt, 1), 64), dtype=np.int8) if scalars_canonical is not None else None
    sc = u64arr(scalars_canonical, 4) if scalars_canonical is not None and len(scalars_canonical) else np.zeros((1, 4), dtype=np.uint64)
    if scalars_canonical is not None and len(sc) < offs[-1]:
        raise ValueError("debug_msm_batch_plan: scalars of ALL terms are needed")
    check(lib().bp_debug_msm_batch_plan(C.c_size_t(n), off_c, *knobs, ptr(sc), C.c_size_t(job), None, None, ptr(first), ptr(length), ptr(dg) if dg is not None else None),
          "bp_debug_msm_batch_plan")
    return route[:n], nsl[:n], first[:S], length[:S], (dg[:nt] if dg is not None else None)


Engine.msm_batch = _msm_batch
Engine.msm_batch_dev = _msm_batch_dev
Engine.msm_batch_stats = _msm_batch_stats
