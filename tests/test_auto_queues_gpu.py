"""With nothing set, the library gives job streams hardware queues of their own when it finds the runtime's pool small
(bbs_sign_amd/csrc/queue_policy.hpp, runtime.hpp stream_create): every case is a fresh child process (tests/auto_queues_child.py
-- the setting, and what the library finds when it is loaded, are process-wide) that keeps 8 proof_verify jobs of 70 items in
flight on three streams each -- 24 job streams, more than 16 + 4, so streams with a queue of their own, pooled streams and, in a
small budget, shared streams all occur; 70 items are two wavefronts in the lane-per-item kernels and seven pairing wavefronts
with a ragged tail.  Statuses are compared exactly (every 16th item of one job is corrupted), and what was granted is read from
bbs_runtime_queue_report.  No rate is asserted: the rates are in profiles/auto_queues_ab.log."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (GPU_MAX_HW_QUEUES of the child or None = absent, BBS_DEDICATED_QUEUES or None, torch touches the GPU first,
#  expected effective pool, expected range of dedicated_made)
CASES = {
    "a_pool4_torch_first": ("4", None, True, 4, (1, 16)),
    "b_pool4_switched_off": ("4", "0", True, 4, (0, 0)),
    "c_pool20": ("20", None, True, 20, (0, 0)),
    "d_unset_torch_first": (None, None, True, 4, (1, 16)),
    "e_unset_library_first": (None, None, False, 20, (0, 0)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_auto_dedicated_queues(case):
    pool, setting, torch_first, want_pool, (lo, hi) = CASES[case]
    env = {k: v for k, v in os.environ.items()
           if k not in ("GPU_MAX_HW_QUEUES", "BBS_DEDICATED_QUEUES", "WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if pool is not None:
        env["GPU_MAX_HW_QUEUES"] = pool
    if setting is not None:
        env["BBS_DEDICATED_QUEUES"] = setting
    cmd = [sys.executable, os.path.join(ROOT, "tests", "auto_queues_child.py")] + (["--torch-first"] if torch_first else [])
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(json.dumps(line))
    rep, b = line["report"], line["budget"]
    assert line["statuses_exact"] is True
    assert rep["mode"] == ("auto" if setting is None else int(setting)), rep
    assert rep["effective_pool"] == want_pool, rep
    assert lo <= rep["dedicated_made"] <= hi, rep
    assert rep["pooled_made"] >= 1, rep
    # the one invariant: queues the library has touched stay within the scratch budget, whatever was assumed about the pool
    assert b["total"] >= 8 and rep["dedicated_made"] + min(b["pool"], rep["pooled_made"]) <= b["total"], (rep, b)
    assert b["dedicated_cap"] == max(0, b["total"] - b["pool"]), b
