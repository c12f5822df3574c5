"""Times of bp_gens_derive, bp_gens_check and bp_gens_digest at one capacity (default 2^20) on one curve (default secq256k1), one GPU.
Each leg runs in a child process of its own, under a time limit, so that a leg that hangs or dies costs its own line and nothing else;
this process never opens the GPU.  A child derives the generators once (allocation, code objects), runs its call once more as a
warm-up and then `reps` times on the host clock — every one of the three calls ends in its own stream wait.  The derive leg times
bp_gens_derive to the SAME capacity again: the whole chain is derived again into the resident table, which is exactly the work
bp_gens_check does into scratch.  Prints one JSON line per leg; --out FILE also appends them there.
usage: python tools/exp_gens_check.py [--logn 20] [--curve 0] [--reps 3] [--limit 300] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("derive", "check", "digest")


def leg(name, cap, curve, reps):
    sys.path.insert(0, ROOT)
    import ark_bulletproofs_amd as A

    e = A.Engine(curve=curve)
    try:
        t0 = time.perf_counter()
        e.gens_derive(cap)
        first_s = time.perf_counter() - t0
        call = {"derive": lambda: e.gens_derive(cap), "check": e.gens_check, "digest": e.gens_digest}[name]
        res = call()                                  # warm-up
        if name == "check":
            assert res.checked == (cap, cap, 2) and res.clean, res
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            wall.append(time.perf_counter() - t0)
        rec = {"leg": name, "curve": ["secq256k1", "zorro"][curve], "generators": cap, "first_derive_ms": round(first_s * 1e3, 2),
               "wall_ms": [round(t * 1e3, 2) for t in wall], "wall_ms_median": round(sorted(wall)[reps // 2] * 1e3, 2)}
        if name == "digest":
            rec["root"] = res.root.hex()
        print(json.dumps(rec), flush=True)
    finally:
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per leg")
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=LEGS, help="(internal) run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, 1 << a.logn, a.curve, a.reps)
    lines = []
    for name in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--logn", str(a.logn), "--curve", str(a.curve), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
            line = r.stdout.strip().splitlines()[-1] if r.returncode == 0 and r.stdout.strip() else json.dumps({"leg": name, "failed": r.returncode, "stderr": r.stderr[-500:]})
        except subprocess.TimeoutExpired:
            line = json.dumps({"leg": name, "failed": "time limit of %g s" % a.limit})
        print(line, flush=True)
        lines.append(line)
        if '"failed"' in line:
            break                                     # nothing more is started on a GPU that a leg has just failed on
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if any('"failed"' in ln for ln in lines) else 0


if __name__ == "__main__":
    sys.exit(main())
