"""Like-provers timed (include/arkbp.h bp_prover_new_like) against provers that record their gadget per proof, on secq256k1:

  single    one 2^logn-multiplier single-phase statement in the expanded blinding mode (n multipliers, n - 1 two-term rows chaining
            a_O[i] to a_L[i + 1], one row on the commitment; recorded through the bulk calls, one FFI call each)
  shuffle   k = 1024 shuffles, one at a time
  batch     k = 1024 shuffles as a prove_batch of 256

  python tools/exp_prover_like.py --parent-lib PATH/libarkbp_hip.so [--out profiles/r17_prover_like.txt] [--logn 20] [--reps 3] [--cases single,shuffle,batch]

For every case: (a) provers that record per proof — ProverCS, commit, the gadget, prove — and (b) like-provers of ONE recording —
new_like, commit, assign_multipliers, prove.  Per proof: wall time, host CPU (user + system time of every thread of the process, read
from /proc/self/task/*/stat around the timed region: tools/thread_cpu.py's method), and the bytes copied to the device, computed from
the statement's sizes (witness vectors, constraint index, coefficient table; the library keeps no copy counter).  Every measurement is
a child process of its own (one library per process: ARKBP_LIB_PATH).  (a) also runs on the parent commit's build, twice: the
parent's run-to-run spread is the margin path (a) on this build must lie within.  The witnesses are random field elements: timing
does not depend on satisfiability with the guard off.  The shuffle's multipliers and constraints all come from its randomized
callback, which runs per instance for (a) and (b) alike — through Python here, which dominates those two cases' host time."""
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


def measured(fn, count):
    c0, t0 = cpu_seconds(), time.perf_counter()
    fn()
    return (time.perf_counter() - t0) / count * 1e3, (cpu_seconds() - c0) / count * 1e3


def random_scalars(rs, n):
    a = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    a[:, 3] >>= np.uint64(2)      # below 2^253: a reduced scalar of either curve, read as Montgomery words
    return np.ascontiguousarray(a)


def child(leg, cases, logn, reps):
    import ctypes as C

    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd._lib import lib, ptr
    from oracle import pyoracle as O

    import gadgets as GD
    import wcheck as W

    F = GD.Field(O, CURVE)
    like = leg == "like"
    row = {"leg": leg}
    rs = np.random.default_rng(17)
    one, mone = F.w(1), F.w(F.p - 1)

    def transcript():
        return E.HostTranscript(b"exp_prover_like")

    if "single" in cases:
        n = 1 << logn
        e = A.Engine(curve=CURVE)
        e.gens_derive(n)
        v, b = random_scalars(rs, 1), random_scalars(rs, 1)
        # rows: a_O[i] - a_L[i + 1] for i < n - 1, then 1 * v0 - 1 * v0 (committed)
        vars_ = np.zeros((2 * n, 2), dtype=np.uint32)
        vars_[0:2 * (n - 1):2, 0] = 3; vars_[0:2 * (n - 1):2, 1] = np.arange(n - 1)
        vars_[1:2 * (n - 1):2, 0] = 1; vars_[1:2 * (n - 1):2, 1] = np.arange(1, n)
        coefs = np.zeros((2 * n, 4), dtype=np.uint64)
        coefs[0::2] = one; coefs[1::2] = mone
        offs = np.arange(0, 2 * n + 1, 2, dtype=np.uint64)
        nnz, ncoef = 2 * (n - 1), 1
        index_bytes = (n + 1) * 4 + 2 * nnz * 4 + ncoef * 32

        def record(p, l, r):
            p.commit(v, b)
            p.allocate_multipliers(l, r)
            E.check(lib().bp_cs_constrain_many(p.h, ptr(vars_), ptr(coefs), ptr(offs), C.c_size_t(n)), "constrain_many")

        wits = [(random_scalars(rs, n), random_scalars(rs, n)) for _ in range(reps + 1)]
        src = None
        if like:
            src = E.ProverCS(CURVE, transcript())
            record(src, *wits[0])
        proofs = []

        def one_proof(j):
            l, r = wits[j]
            if like:
                p = src.new_like(transcript())
                p.commit(v, b)
                p.assign_multipliers(l, r)
            else:
                p = E.ProverCS(CURVE, transcript())
                record(p, l, r)
            p.set_blinding(E.BLINDING_EXPANDED)
            proofs.append(p.prove(e, bytes([j + 1]) * 32))
            p.free()

        one_proof(0)   # untimed: tables, workspaces, the like-provers' index upload
        runs = [measured(lambda j=j: one_proof(j), 1) for j in range(1, reps + 1)]
        row["single"] = {"wall_ms": [w for w, _ in runs], "cpu_ms": [c for _, c in runs], "n": n,
                         "h2d_bytes": (2 if like else 3) * n * 32 + (0 if like else index_bytes)}
        if like:
            row["single"]["stats"] = list(e.prover_like_stats())
        e.close()

    if "shuffle" in cases or "batch" in cases:
        k = 1024
        e = A.Engine(curve=CURVE)
        e.gens_derive(4096)
        e.gens_direct_tables(4096)

        ins = [F.w(31 * i + 5) for i in range(k)]
        values = np.array(ins + ins[1:] + ins[:1], dtype=np.uint64)

        def committed(j):   # (the same values under fresh blinding factors: the commitments, and with them every challenge, differ)
            return values, random_scalars(rs, 2 * k)

        src = None
        if like:
            src = E.ProverCS(CURVE, transcript())
            _, sv = src.commit(*committed(0))
            W.shuffle_gadget(src, F, sv[:k], sv[k:])

        def make(vb):
            if like:
                p = src.new_like(transcript())
                p.commit(*vb)
                p.assign_multipliers(np.zeros((0, 4), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64))
            else:
                p = E.ProverCS(CURVE, transcript())
                _, pv = p.commit(*vb)
                W.shuffle_gadget(p, F, pv[:k], pv[k:])
            return p

        n2 = 2 * (k - 1)
        h2d = 5 * n2 * 32 + (n2 + 1) * 4 + 2 * (3 * n2) * 4   # witness and blinding vectors, the per-proof index (about three entries per column)
        if "shuffle" in cases:
            cnt = 4 * reps
            vbs = [committed(j) for j in range(cnt + 1)]
            make(vbs[0]).prove(e, bytes([9]) * 32)
            runs = [measured(lambda j=j: make(vbs[j]).prove(e, bytes([j & 255]) * 32), 1) for j in range(1, cnt + 1)]
            row["shuffle"] = {"wall_ms": [w for w, _ in runs], "cpu_ms": [c for _, c in runs], "h2d_bytes": h2d}
        if "batch" in cases:
            B = 256
            vbs = [committed(j) for j in range(B)]
            e.prove_batch([make(vbs[j]) for j in range(8)], [bytes([j + 1]) * 32 for j in range(8)])
            runs = []
            for r in range(reps):
                res = []
                runs.append(measured(lambda: res.extend(e.prove_batch([make(vb) for vb in vbs], [bytes([j & 255, r]) + bytes(30) for j in range(B)])), B))
                assert all(st == 0 for st, _ in res)
            row["batch"] = {"wall_ms": [w for w, _ in runs], "cpu_ms": [c for _, c in runs], "h2d_bytes": h2d}
        e.close()
    print("RESULT " + json.dumps(row), flush=True)


def main():
    a = sys.argv[1:]
    opt = lambda name, d: a[a.index(name) + 1] if name in a else d
    logn, reps, cases = int(opt("--logn", 20)), int(opt("--reps", 3)), opt("--cases", "single,shuffle,batch").split(",")
    if "--child" in a:
        return child(opt("--child", "record"), cases, logn, reps)
    parent, out = opt("--parent-lib", None), opt("--out", None)
    legs = [("parent run 1, (a) record per proof", "record", parent), ("this build, (a) record per proof", "record", None),
            ("this build, (b) like-provers", "like", None), ("parent run 2, (a) record per proof", "record", parent)]
    rows = []
    for title, leg, libpath in legs:
        if libpath is None and title.startswith("parent"):
            continue
        env = dict(os.environ)
        if libpath:
            env["ARKBP_LIB_PATH"] = libpath
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--logn", str(logn), "--reps", str(reps), "--cases", ",".join(cases)],
                           env=env, capture_output=True, text=True, timeout=900)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print("leg failed: %s\n%s" % (title, (r.stdout + r.stderr)[-2000:]))
            return 1
        rows.append((title, json.loads(line[0][7:])))
        print("done: " + title, file=sys.stderr, flush=True)
    med = lambda xs: sorted(xs)[len(xs) // 2]
    text = ["like-provers against provers that record per proof, secq256k1; per proof: wall ms / host CPU ms (median, spread = max - min over the runs) / bytes to the device (computed)",
            "every leg is a child process of its own; %d timed runs per leg and case after one untimed (single: 2^%d multipliers, expanded blinding; shuffle: k = 1024, %d proofs; batch: 256 x k = 1024)" % (reps, logn, 4 * reps)]
    for case in cases:
        text.append("")
        text.append(case)
        for title, row in rows:
            c = row[case]
            text.append("  %-38s wall %9.3f (spread %7.3f)   cpu %9.3f (spread %7.3f)   h2d %d" % (title, med(c["wall_ms"]), max(c["wall_ms"]) - min(c["wall_ms"]), med(c["cpu_ms"]),
                                                                                                 max(c["cpu_ms"]) - min(c["cpu_ms"]), c["h2d_bytes"]))
            if "stats" in c:
                text.append("  %-38s index uploads %d, hits %d, resident bytes %d, gates on device %d, on host %d" % ("", *c["stats"]))
    text = "\n".join(text) + "\n"
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
