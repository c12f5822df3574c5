"""The arithmetic of a call of the verifier's device front end (csrc/vfy_dev_plan.hpp: shape rules, placement of the jobs in the shared
buffers, the buffers' layouts and sizes) through its stand-alone self-test (csrc/vfy_dev_plan_selftest.cpp, its own main): built with
the address and undefined-behaviour sanitizers and run as a child process.  Pure host code — no GPU, nothing loaded into this process.
Where the compiler's sanitizer runtime is not installed the same program is built and run without it.

The program asserts literal placements worked out by hand (one small job, the verify benchmark's shape, a call of three jobs), over a
sweep of shapes that the staging parts and the jobs of a call never overlap and stay inside what is reserved, every decline reason at
its boundary, and the rule under which a call takes one more class."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")


def _build():
    exe = os.path.join(OUT, "vfy_dev_plan_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("vfy_dev_plan_selftest.cpp", "vfy_dev_plan.hpp", "vfe_sched.hpp")]
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


def test_vfy_dev_plan_selftest():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "vfy_dev_plan selftest ok", (r.stdout[-1000:] + r.stderr)[-3000:]
