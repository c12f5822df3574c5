"""Time of bp_gens_direct_tables_check at the default reach of the direct window tables (gens_derive(8192), gens_direct_tables(8192):
1 GB), per curve, next to the time gens_direct_tables took to BUILD the same tables in the same run.  One warm-up call, then `reps`
calls timed on the host (each ends in the call's own stream wait) with profiling off, then `reps` calls with profiling on for the
HIP-event time of k_dt_check over table 4 (BP_K_DT_CHECK).  Prints one JSON line per curve.
usage: python tools/exp_tables_check.py [count = 8192] [reps = 5]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import ark_bulletproofs_amd as A
from ark_bulletproofs_amd import engine as E

count = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
for curve, name in ((0, "secq256k1"), (1, "zorro")):
    e = A.Engine(curve=curve)
    try:
        e.gens_derive(count)
        one = np.zeros((1, 4), dtype=np.uint64)
        e.pedersen_commit_batch(one, one)            # tables 5 and 6
        t0 = time.perf_counter()
        nbytes = e.gens_direct_tables(count)         # ends in a stream wait
        build_s = time.perf_counter() - t0
        bad, first, checked = e.gens_direct_tables_check()   # warm-up: code objects, the result buffer
        assert bad == [0, 0, 0, 0] and checked[0] == (2 + 2 * count) * 960, (bad, checked)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            e.gens_direct_tables_check()
            wall.append(time.perf_counter() - t0)
        e.set_profiling(True)
        e.reset_profiling()
        for _ in range(reps):
            e.gens_direct_tables_check()
        ms, launches = e.kernel_time(E.K_DT_CHECK)
        e.set_profiling(False)
        assert launches == reps
        print(json.dumps({"curve": name, "generators": count, "table_bytes": nbytes, "entries_checked": checked, "build_ms": round(build_s * 1e3, 3),
                          "check_wall_ms": [round(t * 1e3, 3) for t in wall], "check_wall_ms_median": round(sorted(wall)[reps // 2] * 1e3, 3),
                          "k_dt_check_table4_event_ms_mean": round(ms / launches, 3),
                          "table4_read_GBps_at_kernel_time": round(nbytes / (ms / launches * 1e-3) / 1e9, 1)}), flush=True)
    finally:
        e.close()
