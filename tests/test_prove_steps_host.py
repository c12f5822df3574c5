"""The prover's shared host steps (csrc/prove_steps.hpp) through their stand-alone self-test (csrc/prove_steps_selftest.cpp, its own
main): built with the address and undefined-behaviour sanitizers and run as a child process.  Pure host code — no GPU, nothing loaded
into this process.  Where the compiler's sanitizer runtime is not installed the same program is built and run without it."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ark_bulletproofs_amd", "csrc")
OUT = os.path.join(ROOT, "ark_bulletproofs_amd", "_obj")


def _build():
    exe = os.path.join(OUT, "prove_steps_selftest")
    srcs = [os.path.join(CSRC, f) for f in ("prove_steps_selftest.cpp", "prove_steps.hpp", "host_proto.hpp", "host_math.hpp", "keccak_unrolled.inc", "arkbp_params.h")]
    if os.path.exists(exe) and all(os.path.getmtime(s) <= os.path.getmtime(exe) for s in srcs):
        return exe
    os.makedirs(OUT, exist_ok=True)
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-pthread", "-o", exe, srcs[0]]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(base + san, capture_output=True, text=True)
    if r.returncode != 0:
        assert "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr, r.stderr[-3000:]   # (only a missing runtime is excused)
        subprocess.check_call(base)
    return exe


def test_prove_steps_selftest():
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prove_steps selftest ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
