"""Child process of tests/test_auto_queues_gpu.py (the dedicated-queue setting is process-wide, and what the library finds when it
is loaded -- the variable, the state of the runtime -- can only be arranged in a fresh process).

    python tests/auto_queues_child.py [--torch-first]

--torch-first: torch touches the GPU before the library is loaded, as in any host that uses torch.  Then 8 proof_verify jobs
of 70 items are kept in flight (throughput form: three streams each, 24 job streams beside the context's), L = 4, R = 2,
8-bit tables, every 16th item of job 1 corrupted; prints ONE JSON line: the statuses' verdict, bbs_runtime_queue_report,
bbs_runtime_queue_budget."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JOBS, N, L, R = 8, 70, 4, 2

if "--torch-first" in sys.argv:
    import torch
    torch.zeros(8, device="cuda").sum().item()

from bbs_sign_amd import workload as pc      # noqa: E402

suite, eng, gens, sk = pc.bench_engine("bls12_381", L, None, 8)
eng.set_latency_mode(False)
inputs, expect = [], []
for s in range(JOBS):
    msgs, disclosed, rnds = pc.bench_items(suite, eng, N, L, R, s * N)
    sigs, st = eng.core_sign_batch(msgs)
    assert (st == 1).all()
    proofs, st = eng.core_proof_gen_batch(sigs, msgs, disclosed, rnds)
    assert (st == 1).all()
    want = [1] * N
    if s == 1:
        for i in range(0, N, 16):
            proofs[i].commitments[0] = (proofs[i].commitments[0] + 1) % suite.curve.r
            want[i] = 0
    inputs.append((proofs, [m[:R] for m in msgs], disclosed))
    expect.append(want)
exact = True
for _ in range(2):                            # the second round runs on recycled streams
    jobs = [eng.core_proof_verify_submit(*a) for a in inputs]
    for j, want in zip(jobs, expect):
        j.wait()
        exact = exact and [int(x) for x in j.result] == want
        j.free()
report = eng.queue_report()
t, p, d, sc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
assert eng.lib.bbs_runtime_queue_budget(0, ctypes.byref(t), ctypes.byref(p), ctypes.byref(d), ctypes.byref(sc)) == 0
eng.close()
print(json.dumps({"statuses_exact": exact, "report": report,
                  "budget": {"total": t.value, "pool": p.value, "dedicated_cap": d.value, "scratch_bytes_per_lane": sc.value},
                  "env": {k: os.environ.get(k) for k in ("GPU_MAX_HW_QUEUES", "BBS_DEDICATED_QUEUES")}}))
