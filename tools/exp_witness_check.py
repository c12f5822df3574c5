"""The witness-check guard timed (include/arkbp.h bp_prover_set_check) at a user's sizes: one 2^logn square-chain proof and a B = 256
batch of k = 1024 shuffles, on the parent commit's build, on this build with the guard off, and on this build with the guard on.

  python tools/exp_witness_check.py --parent-lib PATH/libarkbp_hip.so [--out profiles/r16_witness_check.txt] [--rounds 2] [--reps 3] [--curve 0] [--logn 20]

Every measurement is a child process of its own (one library per process: ARKBP_LIB_PATH), in the order parent, guard off, guard on,
parent, ...  A child runs, after one untimed run of each kind, `reps` timed runs of
  chain     one 2^logn square-chain proof (BP_BLINDING_EXPANDED: the 70 ms proof the guard is meant for, and the default mode)
  batch     prove_batch with B = 256 at k = 1024
and prints one JSON line.  A last child of this build ("probe") turns profiling on and reports the HIP-event time of the check
kernels (BP_K_WITNESS_CHECK) inside a guarded chain proof and a guarded batch, the wall time of the diagnostic bp_prover_check on the
device, and the host twin's time on one core at 2^logn."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def child(curve, leg, logn, reps):
    import ark_bulletproofs_amd as A
    from ark_bulletproofs_amd import engine as E
    from ark_bulletproofs_amd.engine import SC_SHUFFLE, SC_SQUARE_CHAIN, Statement

    guard, probe = leg in ("on", "probe"), leg == "probe"

    def stmt(e, sc, prm, tag, j, dev=True, mode=0):
        s = Statement(curve, sc, prm, bytes([tag, j & 255, j >> 8]) + bytes(29), e if dev else None)
        if mode:
            s.set_blinding(mode)
        if guard:
            s.set_check(True)
        return s

    row = {"leg": leg}
    e = A.Engine(curve=curve)
    e.gens_derive(4096)
    e.gens_direct_tables(4096)
    e.prove_batch([stmt(e, SC_SHUFFLE, [1024], 3, j) for j in range(4)])
    if probe:
        e.set_profiling(True)
        e.reset_profiling()
    runs = []
    for r in range(reps):
        ss = [stmt(e, SC_SHUFFLE, [1024], 4 + r, j) for j in range(256)]
        w, res = timed(lambda: e.prove_batch(ss))
        assert all(st == 0 for st, _ in res)
        runs.append(w / 256)
    row["batch256_k1024"] = runs
    if probe:
        ms, launches = e.kernel_time(E.K_WITNESS_CHECK)
        row["batch_check_kernels_ms_per_batch"] = ms / reps
        row["batch_check_regions_per_batch"] = launches / reps
        ss = [stmt(e, SC_SHUFFLE, [1024], 9, j) for j in range(256)]
        row["check_batch256_k1024_wall"] = timed(lambda: e.check_batch(ss))[0]
    e.close()
    n = 1 << logn
    e = A.Engine(curve=curve)
    e.gens_derive(n)
    for mode, name in ((1, "chain_2p%d_expanded" % logn), (0, "chain_2p%d_default" % logn)):
        stmt(e, SC_SQUARE_CHAIN, [n, 0], 9, 0, dev=False, mode=mode).prove(e)
        if probe:
            e.set_profiling(True)
            e.reset_profiling()
        runs = []
        for j in range(reps):
            s = stmt(e, SC_SQUARE_CHAIN, [n, 0], 10, j, dev=False, mode=mode)
            s.precompute()     # (the TranscriptRng head runs on another core in a service: keep it out of the guarded span)
            w, _ = timed(lambda: s.prove(e))
            runs.append(w)
        row[name] = runs
        if probe:
            ms, launches = e.kernel_time(E.K_WITNESS_CHECK)
            row[name + "_check_kernels_ms"] = ms / reps
            e.set_profiling(False)
    if probe:
        # the guard at this size refuses what it should: the chain whose public output is one off fails its last constraint, row 2n
        bad = stmt(e, SC_SQUARE_CHAIN, [n, 1], 12, 0, dev=False, mode=1)
        try:
            bad.prove(e)
            raise SystemExit("exp_witness_check: the guard let an unsatisfiable 2^%d statement through" % logn)
        except A.UnsatisfiedError:
            (inst, rep), = e.last_unsatisfied()
            assert (inst, rep.bad_gates, rep.bad_constraints, rep.first_bad_constraint) == (0, 0, 1, 2 * n), rep
            row["refused_first_bad_constraint"] = rep.first_bad_constraint
        s = stmt(e, SC_SQUARE_CHAIN, [n, 0], 11, 0, dev=False)
        s.check(e)
        row["check_device_wall_2p%d" % logn] = [timed(lambda: s.check(e))[0] for _ in range(reps)]
        row["check_host_twin_wall_2p%d" % logn] = [timed(lambda: s.check())[0] for _ in range(2)]
    e.close()
    print("ROW " + json.dumps(row), flush=True)


def main():
    a = sys.argv[1:]

    def opt(name, default):
        return a[a.index(name) + 1] if name in a else default

    curve, logn, rounds, reps = int(opt("--curve", 0)), int(opt("--logn", 20)), int(opt("--rounds", 2)), opt("--reps", "3")
    if "--child" in a:
        return child(curve, opt("--child", "off"), logn, int(reps))
    parent, out = opt("--parent-lib", None), opt("--out", os.path.join(ROOT, "profiles", "r16_witness_check.txt"))
    if not parent or not os.path.exists(parent):
        sys.exit("exp_witness_check: --parent-lib must name the parent commit's libarkbp_hip.so")
    parent = os.path.abspath(parent)

    def run(leg):
        env = dict(os.environ)
        env.pop("ARKBP_LIB_PATH", None)
        if leg == "parent":
            env["ARKBP_LIB_PATH"] = parent
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "off" if leg == "parent" else leg, "--curve", str(curve), "--logn", str(logn), "--reps", reps],
                           env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit("exp_witness_check: a child failed with status %d" % p.returncode)   # (nothing more is started on the GPU)
        print("done: %s" % leg, flush=True)
        return json.loads([l for l in p.stdout.splitlines() if l.startswith("ROW ")][-1][4:])

    rows = {"parent": [], "off": [], "on": []}
    for _ in range(rounds):
        for leg in ("parent", "off", "on"):
            rows[leg].append(run(leg))
    probe = run("probe")

    def med(v):
        v = sorted(v)
        return v[len(v) // 2]

    kinds = [k for k in rows["off"][0] if k != "leg"]
    lines = ["witness-check guard, curve %d: wall ms per proof" % curve,
             "%d child processes per column, alternating parent / guard off / guard on; each child: %s timed runs per kind after one untimed" % (rounds, reps),
             "median over all runs of a column; spread = (max - min) over all runs of the column", ""]
    for kind in kinds:
        lines.append(kind)
        meds = {}
        for col, name in (("parent", "parent build"), ("off", "this build, guard off"), ("on", "this build, guard on")):
            allruns = [r for row in rows[col] for r in row[kind]]
            meds[col] = med(allruns)
            lines.append("  %-24s %10.3f   spread %.3f" % (name, 1e3 * meds[col], 1e3 * (max(allruns) - min(allruns))))
        lines.append("  guard off - parent       %+10.3f" % (1e3 * (meds["off"] - meds["parent"])))
        lines.append("  guard on  - guard off    %+10.3f   (the added time per proof)" % (1e3 * (meds["on"] - meds["off"])))
        lines.append("")
    lines.append("probe (this build, guard on, profiling on)")
    for k, v in probe.items():
        if k in kinds or k == "leg":
            continue
        lines.append("  %-44s %s" % (k, ", ".join("%.3f" % (1e3 * x if k.endswith(("wall", "wall_2p%d" % logn)) else x) for x in (v if isinstance(v, list) else [v]))))
    lines.append("  (check_* wall values are ms; *_ms values are HIP-event ms)")
    lines.append("")
    lines.append("raw: " + json.dumps({"rows": rows, "probe": probe}))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:-1]))


if __name__ == "__main__":
    main()
