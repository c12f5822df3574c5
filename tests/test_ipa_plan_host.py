"""The layout of an inner-product round's L and R (csrc/ipa_plan.hpp) through its stand-alone self-test (csrc/ipa_plan_selftest.cpp,
its own main): built with the address and undefined-behaviour sanitizers and run as a child process.  Pure host code — no GPU, nothing
loaded into this process.  Where the compiler's sanitizer runtime is not installed the same program is built and run without it.

The program asserts the plain, deferred and frozen layouts as literal segment lists (unit and strided), that the sides of a round
split G and H exactly over a sweep of sizes and strides, the runner policy of every route, and the gather length of the index-cyclic
argument."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")


def _build():
    exe = os.path.join(OUT, "ipa_plan_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("ipa_plan_selftest.cpp", "ipa_plan.hpp")]
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs):
        return exe
    os.makedirs(OUT, exist_ok=True)
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-o", exe, srcs[0]]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        assert "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
        subprocess.check_call(base)
    return exe


def test_ipa_plan_selftest():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "ipa_plan selftest ok", (r.stdout[-1000:] + r.stderr)[-3000:]
