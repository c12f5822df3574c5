#!/usr/bin/env python3
"""Records tests/golden/vfy_host_staging.json: what the host side of batch verification stages for the batches of
tests/vfy_host_cases.py, as a dry run on a host-only ctx with one host thread.  The file pins the staging of the commit it was
recorded at (named in its header): re-record it only for a change that is MEANT to alter what the host stages.
Run from the repo root, with the library built: python tests/golden/make_vfy_host_staging.py"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vfy_host_cases as VC  # noqa: E402

head = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "ark_bulletproofs_amd", "include"], text=True).strip()
out = {"recorded_at": head + (" (with uncommitted changes to the library)" if dirty else ""), "generators": VC.GENS, "host_threads": 1,
       "rows": "ok: [rc, staging checksum, instances, launch slots]; err: rc; locate: [rc, status per instance]",
       "curves": VC.run_all(1, with_locate=True)}
path = os.path.join(ROOT, "tests", "golden", "vfy_host_staging.json")
with open(path, "w") as f:
    flat = lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]"   # innermost lists on one line  # noqa: E731
    f.write(re.sub(r"\[\s+([^\[\]]*?)\s+\]", flat, json.dumps(out, indent=1)) + "\n")
print("wrote", path)
