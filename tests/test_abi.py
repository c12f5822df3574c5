"""CPU-side checks of the product boundary: the C-ABI library loads, exports every symbol that
include/arkbp.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ark_bulletproofs_amd import build

    build.build()
    from ark_bulletproofs_amd import _lib

    return _lib


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "arkbp.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(bp_[A-Za-z0-9_]+)\s*\(", hdr)))
    assert declared, "no declarations parsed"
    L = lib.lib()
    for name in declared:
        assert hasattr(L, name), "libarkbp_hip.so does not export %s" % name
    assert sorted(declared) == sorted(lib.EXPORTS)


def test_no_cpu_fallback(lib):
    # (asked through the library, not torch: torch brings its own HIP runtime, and when that one opens the GPU first, the library's
    # runtime in the same process finds no device and every GPU test after this one fails)
    L = lib.lib()
    if L.bp_device_count() > 0:
        pytest.skip("GPU present")
    assert L.bp_device_count() == 0
    ctx = C.c_void_p()
    assert L.bp_ctx_create(0, 0, C.byref(ctx)) == lib.BP_E_NO_DEVICE
    from ark_bulletproofs_amd import ArkbpError, Engine

    with pytest.raises(ArkbpError):
        Engine()


def test_product_does_not_reference_oracle():
    # the product path must not import, link or call anything under oracle/
    pkg = os.path.join(ROOT, "ark_bulletproofs_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cuh", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert "pyoracle" not in txt and "liboracle" not in txt and "oracle/" not in txt.replace("Independent of oracle/", ""), f


def test_bench_statement_seeds_do_not_overflow():
    """bench.py derives one 32-byte ChaCha20 seed per synthetic statement; the driver's `--steps 20 --warmup 5` needs
    400 of them (round 1 crashed at k = 255)."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seeds = {bench.statement_seed(tag, k) for tag in (0, 1, 100, 120) for k in list(range(1200)) + [65535, 65536, (1 << 32) - 1]}
    assert len(seeds) == 4 * 1203 and all(len(s) == 32 for s in seeds)


def test_bench_worker_exceptions_propagate():
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def boom():
        raise ValueError("worker failed")

    with pytest.raises(ValueError):
        bench.run_threads([(boom, ()), ((lambda: None), ())])


def test_bench_plain_headline_runs_only_the_prove_half(monkeypatch):
    """a plain headline run times the prove half and nothing else; --full adds the verify half and the other configurations"""
    import argparse
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    calls = []

    def fake(name):
        def run(args, rank, world, local):
            calls.append((name, args.dump_outputs))
            return {"metric": name, "value": 1.0, "config": {}}
        return run

    for fn, name in (("run_prove", "prove"), ("run_verify", "verify"), ("run_msm", "msm"), ("run_shuffle_sweep", "sweep")):
        monkeypatch.setattr(bench, fn, fake(name))
    args = argparse.Namespace(full=False, headline_only=False, cfg5_logn=22, dump_outputs="out")
    res = bench.run_headline(args, 0, 1, 0)
    assert calls == [("prove", "out")] and "verify" not in res and res["value"] == 1.0
    del calls[:]
    args.full = True
    res = bench.run_headline(args, 0, 1, 0)
    # only the headline's own timed proofs are dumped, not the legs'
    assert calls == [("prove", "out"), ("verify", "out"), ("sweep", None), ("msm", None), ("prove", None), ("prove", None)]
    assert res["verify"]["value"] == 1.0 and "errors" not in res


def test_bench_gpus_flag_spawns_ranks(monkeypatch):
    """`python bench.py --gpus N` without a launcher must start N ranks itself (round 1 silently ran one)"""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 0

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.setattr(bench.sys, "argv", ["bench.py", "--gpus", "4", "--steps", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert "torch.distributed.run" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4" and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "2"]


def test_rust_ffi_is_generated_from_the_header(lib):
    """shim/src/ffi.rs (the Rust `extern "C"` block a maintainer of the reference would bind) is exactly what tools/gen_rust_ffi.py
    makes of include/arkbp.h, and names every exported entry point"""
    import subprocess
    import sys

    gen = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_ffi.py")], capture_output=True, text=True, check=True).stdout
    assert gen == open(os.path.join(ROOT, "shim", "src", "ffi.rs")).read(), "run: python tools/gen_rust_ffi.py > shim/src/ffi.rs"
    assert sorted(re.findall(r"pub fn (bp_\w+)", gen)) == sorted(lib.EXPORTS)


def test_missing_rccl_is_an_error_code_not_a_crash(lib):
    """with no librccl to bind, bp_rccl_unique_id / bp_ctx_rccl_init must return BP_E_HIP with a message (include/arkbp.h)
    — the first version called dlerror() twice and dereferenced the NULL the second call returns.  Own process: the binding is
    resolved once per process."""
    import subprocess
    import sys

    code = (
        "import ctypes as C, sys\n"
        "sys.path.insert(0, %r)\n"
        "from ark_bulletproofs_amd import _lib\n"
        "L = _lib.lib()\n"
        "buf = (C.c_uint8 * 128)()\n"
        "rc = L.bp_rccl_unique_id(buf)\n"
        "msg = L.bp_last_error().decode()\n"
        "print(rc, '|', msg)\n"
        "assert rc == _lib.BP_E_HIP, rc\n"
        "assert 'librccl not found' in msg and 'no-such-librccl' in msg, msg\n"
    ) % ROOT
    env = dict(os.environ, ARKBP_RCCL_LIB="/nonexistent/no-such-librccl.so")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
