"""The host side of batch verification, pinned (no GPU): the dry run of a host-only ctx against tests/golden/vfy_host_staging.json,
recorded before batch_verify_host was split into steps (the file's header names the commit).  Rows and batches: tests/vfy_host_cases.py.

Every row runs three ways — 1 host thread, 8 host threads, and the live replay alone (ARKBP_VFY_NOX8=1 in a fresh child process: the
library reads the switch once) — and gives the recorded (rc, checksum, count, slots) each time; error rows compare rc.  The error rows
also go through bp_r1cs_batch_verify_locate_scenarios with the whole status vector compared: on a host-only ctx that entry point
answers BP_E_NO_DEVICE after its checks and writes no status, which is what the fixture holds (the per-instance statuses of a real
ctx are test_gpu_verify_locate.py's)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import vfy_host_cases as VC  # noqa: E402

E_VERIFICATION, E_GENS_LENGTH, E_FORMAT = -4, -5, -6
EXPECT_RC = {"truncated": E_FORMAT, "off_curve_block0": E_FORMAT, "off_curve_block1": E_FORMAT, "identity_point": E_VERIFICATION,
             "gens_length": E_GENS_LENGTH, "bad_then_truncated": E_FORMAT, "bad_then_off_curve_block1": E_FORMAT}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "vfy_host_staging.json")) as f:
        return json.load(f)


def _nox8_child():
    env = dict(os.environ, ARKBP_VFY_NOX8="1")
    out = subprocess.run([sys.executable, os.path.join(HERE, "vfy_host_cases.py"), "8"], env=env, check=True, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def runs(oracle):
    return {"1 thread": VC.run_all(1, with_locate=True), "8 threads": VC.run_all(8), "live replay only": _nox8_child()}


def test_fixture_header(golden):
    assert len(golden["recorded_at"].split()[0]) == 40 and golden["generators"] == VC.GENS
    for cv in ("0", "1"):
        assert {k: v for k, v in golden["curves"][cv]["err"].items()} == EXPECT_RC


@pytest.mark.parametrize("curve", ["0", "1"])
@pytest.mark.parametrize("how", ["1 thread", "8 threads", "live replay only"])
def test_staging_matches_the_recording(golden, runs, curve, how):
    want, got = golden["curves"][curve], runs[how][curve]
    assert sorted(got["ok"]) == sorted(want["ok"]) and sorted(got["err"]) == sorted(want["err"])
    for name, row in want["ok"].items():
        assert row[0] == 0 and row[2] > 0 and row[3] > 0
        assert got["ok"][name] == row, (name, how)
    for name, rc in want["err"].items():
        assert got["err"][name] == rc, (name, how)


@pytest.mark.parametrize("curve", ["0", "1"])
def test_error_rows_through_locate(golden, runs, curve):
    want, got = golden["curves"][curve]["locate"], runs["1 thread"][curve]["locate"]
    assert sorted(got) == sorted(EXPECT_RC)
    for name in EXPECT_RC:
        assert got[name] == want[name], name
