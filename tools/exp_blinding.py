"""Both blinding modes timed (include/arkbp.h BP_BLINDING_TRANSCRIPT / BP_BLINDING_EXPANDED), and the default mode of this build
against the parent commit's build, alternately.

  python tools/exp_blinding.py --parent-lib PATH/libarkbp_hip.so [--out profiles/r14_blinding.txt] [--rounds 3] [--curve 0] [--logn 20]

Every measurement is a child process of its own (one library per process: ARKBP_LIB_PATH), in the order parent, this build, parent,
... for the default mode, then the expanded mode on this build.  A child runs, after one untimed proof of each kind:
  chain     one 2^logn square-chain proof alone, `reps` times: wall seconds, timing[2] (TranscriptRng), timing[3] (upload), host CPU seconds
  shuffle   one k = 1024 shuffle alone
  batch     prove_batch with B = 256 at k = 128 and at k = 1024
and prints one JSON line.  The parent's library has no bp_prover_set_blinding: it is only ever asked for the default mode.
cpu = host CPU seconds of the process per proof (all threads)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    c0, t0 = time.process_time(), time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, time.process_time() - c0, r


def child(curve, mode, logn, reps):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd.engine import SC_SHUFFLE, SC_SQUARE_CHAIN, Statement

    def stmt(e, sc, prm, tag, j, dev=True):
        s = Statement(curve, sc, prm, bytes([tag, j & 255, j >> 8]) + bytes(29), e if dev else None)
        if mode:
            s.set_blinding(mode)
        return s

    row = {"mode": mode, "lib": "parent build" if os.environ.get("ARKBP_LIB_PATH") else "this build"}
    e = A.Engine(curve=curve)
    e.gens_derive(4096)
    e.gens_direct_tables(4096)
    stmt(e, SC_SHUFFLE, [1024], 1, 0).prove(e)
    runs = []
    for j in range(2 * reps):
        s = stmt(e, SC_SHUFFLE, [1024], 2, j)
        w, c, (_, tm) = timed(lambda: s.prove(e))
        runs.append([w, tm[2], tm[3], c])
    row["shuffle1024"] = runs
    for k in (128, 1024):
        e.prove_batch([stmt(e, SC_SHUFFLE, [k], 3, j) for j in range(4)])
        runs = []
        for r in range(reps):
            ss = [stmt(e, SC_SHUFFLE, [k], 4 + r, j) for j in range(256)]
            tm = [0.0] * 8
            w, c, res = timed(lambda: e.prove_batch(ss, timing=tm))
            assert all(st == 0 for st, _ in res)
            runs.append([w / 256, tm[2] / 256, tm[3] / 256, c / 256])
        row["batch256_k%d" % k] = runs
    e.close()
    n = 1 << logn
    e = A.Engine(curve=curve)
    e.gens_derive(n)
    stmt(e, SC_SQUARE_CHAIN, [n, 0], 9, 0, dev=False).prove(e)
    runs = []
    for j in range(reps):
        s = stmt(e, SC_SQUARE_CHAIN, [n, 0], 10, j, dev=False)
        w, c, (_, tm) = timed(lambda: s.prove(e))
        runs.append([w, tm[2], tm[3], c])
    row["chain_2p%d" % logn] = runs
    row["blinding_stats"] = list(e.blinding_stats()) if hasattr(e, "blinding_stats") and mode else None
    e.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    a = sys.argv[1:]

    def opt(name, default):
        return a[a.index(name) + 1] if name in a else default

    curve, logn, rounds = int(opt("--curve", 0)), int(opt("--logn", 20)), int(opt("--rounds", 3))
    if "--child" in a:
        return child(curve, int(opt("--child", 0)), logn, int(opt("--reps", 3)))
    parent, out = opt("--parent-lib", None), opt("--out", os.path.join(ROOT, "profiles", "r14_blinding.txt"))
    if not parent or not os.path.exists(parent):
        sys.exit("exp_blinding: --parent-lib must name the parent commit's libarkbp_hip.so")
    parent = os.path.abspath(parent)

    def run(lib, mode):
        env = dict(os.environ)
        env.pop("ARKBP_LIB_PATH", None)
        if lib:
            env["ARKBP_LIB_PATH"] = lib
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(mode), "--curve", str(curve), "--logn", str(logn), "--reps", opt("--reps", "3")],
                           env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("exp_blinding: a child failed with status %d" % p.returncode)   # (nothing more is started on the GPU)
        print("done: %s, mode %d" % (lib or "this build", mode), flush=True)
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("ROW ")][-1][4:])

    rows = {"parent": [], "this": [], "expanded": []}
    for _ in range(rounds):
        rows["parent"].append(run(parent, 0))
        rows["this"].append(run(None, 0))
    for _ in range(rounds):
        rows["expanded"].append(run(None, 1))
    kinds = [k for k in rows["this"][0] if k not in ("mode", "lib", "blinding_stats")]
    lines = ["blinding modes, curve %d: per proof [wall ms, TranscriptRng ms (timing[2]), upload ms (timing[3]), host CPU ms]" % curve,
             "%d child processes per column, alternating parent / this build; each child: %s timed runs per kind after one untimed" % (rounds, opt("--reps", "3")),
             "median over all runs of a column; spread = (max - min) of the per-child medians of wall ms", ""]

    def med(v):
        v = sorted(v)
        return v[len(v) // 2]

    for kind in kinds:
        lines.append(kind)
        for col in ("parent", "this", "expanded"):
            allruns = [r for row in rows[col] for r in row[kind]]
            per_child = [med([r[0] for r in row[kind]]) for row in rows[col]]
            m = [1e3 * med([r[i] for r in allruns]) for i in range(4)]
            lines.append("  %-28s wall %10.3f  rng %10.3f  upload %9.3f  cpu %10.3f   spread of wall %.3f" %
                         ({"parent": "default, parent build", "this": "default, this build", "expanded": "expanded, this build"}[col], m[0], m[1], m[2], m[3],
                          1e3 * (max(per_child) - min(per_child))))
        lines.append("")
    lines.append("raw: " + json.dumps(rows))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-1]))


if __name__ == "__main__":
    main()
