"""The MSM planners (csrc/msm_plan.hpp) through their stand-alone self-test (csrc/msm_plan_selftest.cpp, its own main): built with
the address and undefined-behaviour sanitizers and run as a child process.  Pure host code — no GPU, nothing loaded into this process.
Where the compiler's sanitizer runtime is not installed the same program is built and run without it.

The program asserts what the kernels rely on (LDS sizes, index widths, per-job strides) and prints every plan — route x scalar width
x size x knob set — as one JSON record; tests/golden/msm_plans.json holds the same records as the planning code gave them while it was
still part of the launch code in arkbp.hip, and every field must be equal."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")
GOLDEN = os.path.join(ROOT, "tests", "golden", "msm_plans.json")


def _build():
    exe = os.path.join(OUT, "msm_plan_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("msm_plan_selftest.cpp", "msm_plan.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs):
        return exe
    os.makedirs(OUT, exist_ok=True)
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-o", exe, srcs[0]]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        assert "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
        subprocess.check_call(base)
    return exe


def test_msm_plan_selftest_and_recorded_plans():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "msm_plan selftest ok", (r.stdout[-1000:] + r.stderr)[-3000:]
    got = [json.loads(ln) for ln in lines[:-1]]
    with open(GOLDEN) as f:
        want = [json.loads(ln) for ln in f if ln.strip()]
    assert len(want) > 500 and len(got) == len(want)
    case = lambda rec: tuple(rec[k] for k in ("route", "knobs", "bits", "n")) + (rec.get("J"),)
    assert len({case(w) for w in want}) == len(want)
    for g, w in zip(got, want):
        assert case(g) == case(w)
        assert sorted(g) == sorted(w), "%r: fields %r, recorded %r" % (case(w), sorted(g), sorted(w))
        for k in w:
            assert g[k] == w[k], "%r: %s = %r, recorded %r" % (case(w), k, g[k], w[k])
    # every route is there, both as a plan that fits and as one that steps aside
    for route in ("fixed-shape", "glv"):
        assert {w["fits"] for w in want if w["route"] == route} == {0, 1}
    assert {w["decline"] for w in want if w["route"] == "fixed-base"} >= {0, 2}
