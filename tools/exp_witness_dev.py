"""A like-prover's witness from device memory timed (include/arkbp.h bp_prover_assign_multipliers_dev, bp_witness_range_bits_dev)
against the same like-prover assigned from host vectors, on secq256k1, 2^logn multipliers, single-phase, expanded blinding — the
method of tools/exp_prover_like.py:

  b        like-provers of one recording (the chain statement of exp_prover_like.py), witness assigned from the host
  c        the same words assigned from device buffers that were filled outside the timed region
  d-host   a range statement of 2^(logn - 6) values of 64 bits (the reference's range gadget per value): the bits are decomposed on
           the host (numpy) and assigned from host vectors, inside the timed region
  d-dev    the same statement: bp_witness_range_bits_dev builds the witness from the 64-bit values inside the timed region

  python tools/exp_witness_dev.py --parent-lib PATH/libarkbp_hip.so [--out profiles/r18_witness_dev.txt] [--logn 20] [--reps 3]

Timed per proof: new_like, commit, the assignment (d: and the construction of the witness), prove.  Per proof: wall time, host CPU
(user + system time of every thread of the process, from /proc/self/task/*/stat around the timed region) and the witness bytes copied
to the device, computed from the statement's sizes (the library keeps no copy counter; the recording's index is resident after the
untimed first proof and the commitments' few words are left out everywhere).  Every leg is a child process of its own (one library per
process: ARKBP_LIB_PATH).  Leg b also runs on the parent commit's build, twice: the parent's run-to-run spread is the margin leg b of
this build must lie within.  In b and c the witnesses are random field elements: timing does not depend on satisfiability with the
guard off.  Legs c and d-dev assert that every multiplier came through the import kernel and none was downloaded."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CURVE = 0
NBITS = 64


def cpu_seconds():
    tck, tot = os.sysconf("SC_CLK_TCK"), 0
    for t in os.listdir("/proc/self/task"):
        try:
            st = open("/proc/self/task/%s/stat" % t).read()
            f = st[st.rindex(")") + 2:].split()
            tot += int(f[11]) + int(f[12])
        except Exception:
            pass
    return tot / tck


def measured(fn):
    c0, t0 = cpu_seconds(), time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3, (cpu_seconds() - c0) * 1e3


def random_scalars(rs, n):
    a = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)      # below 2^253: a reduced scalar of either curve, read as Montgomery words
    return np.ascontiguousarray(a)


def range_statement(F, n):
    """the reference's range gadget over n / 64 committed values of 64 bits in bulk form (bp_cs_constrain_many): (vars, coefs, offsets)"""
    m = n // NBITS
    one, mone = np.array(F.w(1), dtype=np.uint64), np.array(F.w(F.p - 1), dtype=np.uint64)
    # the range gadget per value, in bulk: per multiplier i the rows [a_O[i]] and [a_L[i] + a_R[i] - 1], per value v_j - sum 2^i a_R[j * 64 + i]
    idx = np.arange(n, dtype=np.uint32)
    per_mul = np.zeros((n, 4, 2), dtype=np.uint32)
    per_mul[:, 0, 0] = 3; per_mul[:, 1, 0] = 1; per_mul[:, 2, 0] = 2; per_mul[:, 3, 0] = 4
    per_mul[:, 0:3, 1] = idx[:, None]
    mul_coefs = np.zeros((n, 4, 4), dtype=np.uint64)
    mul_coefs[:, 0] = one; mul_coefs[:, 1] = one; mul_coefs[:, 2] = one; mul_coefs[:, 3] = mone
    per_val = np.zeros((m, NBITS + 1, 2), dtype=np.uint32)
    per_val[:, 0, 0] = 0; per_val[:, 0, 1] = np.arange(m)
    per_val[:, 1:, 0] = 2; per_val[:, 1:, 1] = (np.arange(m, dtype=np.uint32)[:, None] * NBITS + np.arange(NBITS, dtype=np.uint32)[None, :])
    pow2 = np.array([F.w(F.p - (1 << i)) for i in range(NBITS)], dtype=np.uint64).reshape(NBITS, 4)
    val_coefs = np.zeros((m, NBITS + 1, 4), dtype=np.uint64)
    val_coefs[:, 0] = one; val_coefs[:, 1:] = pow2[None, :, :]
    vars_ = np.ascontiguousarray(np.concatenate([per_mul.reshape(-1, 2), per_val.reshape(-1, 2)]))
    coefs = np.ascontiguousarray(np.concatenate([mul_coefs.reshape(-1, 4), val_coefs.reshape(-1, 4)]))
    mul_offs = np.zeros(2 * n, dtype=np.uint64)
    mul_offs[0::2] = np.arange(n, dtype=np.uint64) * np.uint64(4); mul_offs[1::2] = np.arange(n, dtype=np.uint64) * np.uint64(4) + np.uint64(1)
    val_offs = np.uint64(4 * n) + np.arange(m + 1, dtype=np.uint64) * np.uint64(NBITS + 1)
    offs = np.ascontiguousarray(np.concatenate([mul_offs, val_offs]))
    return vars_, coefs, offs


def host_bits(F, values):
    """the range gadget's witness built on the host: (left, right), 64 bytes per bit"""
    w01 = np.array([F.w(0), F.w(1)], dtype=np.uint64).reshape(2, 4)
    shifts = np.arange(NBITS, dtype=np.uint64)
    bits = ((values[:, None] >> shifts[None, :]) & np.uint64(1)).reshape(-1).astype(np.int64)
    return w01[1 - bits], w01[bits]


def child(leg, logn, reps):
    import ctypes as C

    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib, ptr
    from oracle import pyoracle as O

    import gadgets as GD

    F = GD.Field(O, CURVE)
    rs = np.random.default_rng(18)
    one, mone = np.array(F.w(1), dtype=np.uint64), np.array(F.w(F.p - 1), dtype=np.uint64)
    n = 1 << logn
    e = A.Engine(curve=CURVE)
    e.gens_derive(n)

    def transcript():
        return E.HostTranscript(b"exp_witness_dev")

    def constrain_many(p, vars_, coefs, offs):
        E.check(lib().bp_cs_constrain_many(p.h, ptr(vars_), ptr(coefs), ptr(offs), C.c_size_t(len(offs) - 1)), "constrain_many")

    proofs = []
    if leg in ("b", "c"):
        v, b = random_scalars(rs, 1), random_scalars(rs, 1)
        # rows: a_O[i] - a_L[i + 1] for i < n - 1, then 1 * v0 - 1 * v0 (committed)
        vars_ = np.zeros((2 * n, 2), dtype=np.uint32)
        vars_[0:2 * (n - 1):2, 0] = 3; vars_[0:2 * (n - 1):2, 1] = np.arange(n - 1)
        vars_[1:2 * (n - 1):2, 0] = 1; vars_[1:2 * (n - 1):2, 1] = np.arange(1, n)
        coefs = np.zeros((2 * n, 4), dtype=np.uint64)
        coefs[0::2] = one; coefs[1::2] = mone
        offs = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
        wits = [(random_scalars(rs, n), random_scalars(rs, n)) for _ in range(reps + 1)]
        src = E.ProverCS(CURVE, transcript())
        src.commit(v, b)
        src.allocate_multipliers(*wits[0])
        constrain_many(src, vars_, coefs, offs)
        bufs = [(e.upload_scalars(l), e.upload_scalars(r)) for l, r in wits] if leg == "c" else None   # (outside the timed region)

        def one_proof(j):
            p = src.new_like(transcript())
            p.commit(v, b)
            if leg == "c":
                p.assign_multipliers_dev(e, bufs[j][0], bufs[j][1], n)
            else:
                p.assign_multipliers(*wits[j])
            p.set_blinding(E.BLINDING_EXPANDED)
            proofs.append(p.prove(e, bytes([j + 1]) * 32))
            p.free()

        h2d = 0 if leg == "c" else 2 * n * 32
    else:
        m = n // NBITS
        blinds = random_scalars(rs, m)

        def values_of(j):
            return np.random.default_rng(100 + j).integers(0, 1 << 63, size=m, dtype=np.uint64) * np.uint64(2) + np.uint64(j & 1)

        def committed(values):   # the 64-bit values as ark scalars (the oracle's conversion, one call per value)
            return np.array([F.w(int(x)) for x in values], dtype=np.uint64).reshape(m, 4)

        vars_, coefs, offs = range_statement(F, n)
        vals = [values_of(j) for j in range(reps + 1)]
        coms = [committed(x) for x in vals]   # (the commitments' scalars: the same work for both legs, outside the timed region)
        src = E.ProverCS(CURVE, transcript())
        src.commit(coms[0], blinds, engine=e)
        src.allocate_multipliers(*host_bits(F, vals[0]))
        constrain_many(src, vars_, coefs, offs)
        if leg == "d-host":   # (once, untimed: the recorded statement is satisfied by the witness both legs build)
            assert src.check(e).satisfied

        def one_proof(j):
            p = src.new_like(transcript())
            p.commit(coms[j], blinds, engine=e)
            if leg == "d-dev":
                left, right = e.witness_range_bits(vals[j], NBITS)
                p.assign_multipliers_dev(e, left, right, n)
                left.free(); right.free()
            else:
                p.assign_multipliers(*host_bits(F, vals[j]))
            p.set_blinding(E.BLINDING_EXPANDED)
            proofs.append(p.prove(e, bytes([j + 1]) * 32))
            p.free()

        h2d = 8 * m if leg == "d-dev" else 2 * n * 32

    one_proof(0)   # untimed: tables, workspaces, the recording's index upload
    s0 = e.witness_dev_stats() if hasattr(e, "witness_dev_stats") and hasattr(lib(), "bp_ctx_witness_dev_stats") else None
    runs = [measured(lambda j=j: one_proof(j)) for j in range(1, reps + 1)]
    row = {"leg": leg, "n": n, "wall_ms": [w for w, _ in runs], "cpu_ms": [c for _, c in runs], "h2d_bytes": h2d, "proof_bytes": len(proofs[-1])}
    if s0 is not None:
        s1 = e.witness_dev_stats()
        row["stats"] = [a - b for a, b in zip(s1, s0)]
        if leg in ("c", "d-dev"):
            assert row["stats"] == [reps, reps * n, 0], row["stats"]
    e.close()
    print("RESULT " + json.dumps(row), flush=True)


def main():
    a = sys.argv[1:]
    opt = lambda name, d: a[a.index(name) + 1] if name in a else d
    logn, reps = int(opt("--logn", 20)), int(opt("--reps", 3))
    if "--child" in a:
        return child(opt("--child", "b"), logn, reps)
    parent, out = opt("--parent-lib", None), opt("--out", None)
    legs = [("parent run 1, (b) host-assigned", "b", parent), ("this build, (b) host-assigned", "b", None), ("this build, (c) device-assigned", "c", None),
            ("this build, (d) range, bits on the host", "d-host", None), ("this build, (d) range, bits on the GPU", "d-dev", None),
            ("parent run 2, (b) host-assigned", "b", parent)]
    rows = []
    for title, leg, libpath in legs:
        if libpath is None and title.startswith("parent"):
            continue
        env = dict(os.environ)
        if libpath:
            env["ARKBP_LIB_PATH"] = libpath
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--logn", str(logn), "--reps", str(reps)], env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("leg failed: %s\n%s" % (title, (r.stdout + r.stderr)[-2000:]))
            return 1   # (nothing more is started on the GPU)
        rows.append((title, json.loads(line[0][7:])))
        print("done: " + title, file=sys.stderr, flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    text = ["a like-prover's witness from device memory against the same like-prover assigned from the host, secq256k1, 2^%d multipliers, single-phase, expanded blinding" % logn,
            "per proof: wall ms / host CPU ms (median, spread = max - min over the runs) / witness bytes to the device (computed); every leg is a child process of its own; %d timed proofs per leg after one untimed" % reps,
            "timed: new_like, commit, the assignment (d: and building the witness, 2^%d values of 64 bits), prove" % (logn - 6), ""]
    for title, row in rows:
        text.append("  %-42s wall %9.3f (spread %7.3f)   cpu %9.3f (spread %7.3f)   h2d %d" % (title, med(row["wall_ms"]), max(row["wall_ms"]) - min(row["wall_ms"]), med(row["cpu_ms"]),
                                                                                             max(row["cpu_ms"]) - min(row["cpu_ms"]), row["h2d_bytes"]))
        if "stats" in row:
            text.append("  %-42s device assignments %d, multipliers imported from device memory %d, taken to the host %d" % ("", *row["stats"]))
    text = "\n".join(text) + "\n"
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
