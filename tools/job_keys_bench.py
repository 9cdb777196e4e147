#!/usr/bin/env python3
"""Verification under keys that arrive with the job (bbs_*_with_keys_*), on the headline loop's shape: 4096 items per job, 32
messages / 8 disclosed, 16-bit windows, 6 jobs in flight, host buffers, every status checked.  BLS12-381 and BN254,
proof_verify and verify, D = 1 / 16 / 64 / 256 / 1024 / 4096 distinct keys per job (item i under key i mod D).  Prints ONE
JSON line; --out FILE also writes it there.

    python tools/job_keys_bench.py [--curves bls12_381,bn254] [--d 1,16,64,256,1024,4096] [--runs 5] [--out profiles/job_keys_bench.json]

Three legs per (curve, operation, D), items/s, median and [min, max] of --runs runs:
  a_registered   the keyed loop, all D keys registered beforehand: the ceiling
  b_register_per_job   what a caller without the new exports must do: the context's key set replaced by that job's D keys from
                 octets (bbs_ctx_set_public_keys(0) + bbs_ctx_add_public_keys_octets), then the keyed job
  c_with_keys    the new exports: the job prepares its D keys on the device
and `latency_ms_d1`: one job alone, submit to wait, D = 1, legs a and c -- the price of the key stage's one walk.
The workload is generated untimed by ONE context through keyed sign and keyed proof_gen (a signing set of D keys).
"""
import os

os.environ.setdefault("GPU_MAX_HW_QUEUES", "20")
import argparse
import ctypes
import json
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, L, R, INFLIGHT = 4096, 32, 8, 6


def loop(submit, steps, warmup):
    """`submit()` -> job; INFLIGHT outstanding, oldest retired first, every status checked; items/s over `steps`."""
    def run(k):
        pending = []
        for _ in range(k):
            if len(pending) >= INFLIGHT:
                j = pending.pop(0)
                j.wait()
                assert (j.result == 1).all(), np.unique(j.result, return_counts=True)
                j.free()
            pending.append(submit())
        for j in pending:
            j.wait()
            assert (j.result == 1).all(), np.unique(j.result, return_counts=True)
            j.free()
    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return N * steps / (time.perf_counter() - t0)


def stats(v):
    return [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)]


def main():
    global N, L, R
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--d", default="1,16,64,256,1024,4096")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the numbers were taken at")
    ap.add_argument("--lib", default="", help="another build of the library (a dry run through the host twin)")
    ap.add_argument("--batch", type=int, default=N, help="items per job (dry runs)")
    ap.add_argument("--messages", type=int, default=L, help="messages per item (dry runs)")
    ap.add_argument("--disclosed", type=int, default=R, help="disclosed messages per item (dry runs)")
    a = ap.parse_args()
    import parity_cases as pc
    from bbs_sign_amd import Engine, _lib
    from oracle import bbs
    N, L, R = a.batch, a.messages, a.disclosed
    Ds = [int(x) for x in a.d.split(",")]
    out = {"metric": "job_keys_items_per_s_median_min_max", "batch": N, "messages": L, "disclosed": R, "inflight": INFLIGHT,
           "window_bits": 16, "runs": a.runs, "commit": a.commit, "curves": {}}
    for curve in a.curves.split(","):
        suite = bbs.SUITES[curve]
        c = suite.curve
        gens = pc.gens_for(suite, L + 1)

        def ctx(wb=16):
            e = Engine(curve, device=0, window_bits=wb, lib_path=a.lib or None)
            e.set_generators(gens, suite.api_id)
            return e

        maker = ctx(8)
        msgs, disclosed, rnds = pc.bench_items(suite, maker, N, L, R)
        dm = [[msgs[i][j] for j in disclosed[i]] for i in range(N)]
        sks = [bbs.key_gen(suite, bytes([3, k % 256, k // 256] + [7] * 29), b"", b"BBS-SIG-KEYGEN-SALT-") for k in range(max(Ds))]
        st, pks, first = maker.set_secret_keys(sks)
        assert (np.asarray(st) == 1).all() and first == 0
        octs = [bbs.g2_compress(c, k) for k in pks]
        res = {"pv": {}, "vf": {}}
        lat = {}
        for D in Ds:
            kid = np.array([i % D for i in range(N)], dtype=np.uint32)
            sigs, st = maker.core_sign_keyed_batch(kid, msgs)
            assert (st == 1).all()
            proofs, st = maker.core_proof_gen_keyed_batch(kid, sigs, msgs, disclosed, rnds)
            assert (st == 1).all()
            reg, bare = ctx(), ctx()
            assert (reg.set_public_keys(pks[:D]) == 1).all()
            ko = bare._key_octets(octs[:D])
            kst = np.zeros(D, dtype=np.int8)
            first_ix = ctypes.c_uint32(0)
            kip = kid.ctypes.data_as(_lib.c_u32p)
            for op in ("pv", "vf"):
                if op == "pv":
                    n, keep, args = reg._pv_inputs(proofs, dm, disclosed, None, None)
                    name = "bbs_core_proof_verify_%s_submit"
                else:
                    n, keep, args = reg._vf_core_args(sigs, msgs, None)
                    name = "bbs_core_verify_%s_submit"

                def keyed(eng):
                    def submit():
                        j = eng._status_submit(name % "keyed", n, args, kid)
                        j.keep = keep
                        return j
                    return submit

                def per_job():
                    # the key set of THIS job from octets, synchronously on the submitting thread, then the keyed job
                    assert bare.lib.bbs_ctx_set_public_keys(bare.h, 0, None, None, None) == 0
                    assert bare.lib.bbs_ctx_add_public_keys_octets(bare.h, D, ko.ctypes.data_as(_lib.c_u8p), kst.ctypes.data_as(_lib.c_i8p),
                                                                   None, None, ctypes.byref(first_ix)) == 0
                    return keyed(bare)()

                def with_keys():
                    st_ = np.full(N, -128, dtype=np.int8)
                    j = ctypes.c_void_p()
                    rc = getattr(bare.lib, name % "with_keys")(bare.h, n, D, ko.ctypes.data_as(_lib.c_u8p), kip, *args,
                                                               st_.ctypes.data_as(_lib.c_i8p), ctypes.byref(j))
                    assert rc == 0, rc
                    from bbs_sign_amd.engine import Job
                    job = Job(bare, j, n)
                    job.result, job._fixup, job.keep = st_[:n], None, keep
                    return job

                slow = max(3, min(a.steps, int(2.0 / (0.00013 * D + 0.004))))       # leg b: about two seconds per run
                legs = {"a_registered": (keyed(reg), a.steps, INFLIGHT), "b_register_per_job": (per_job, slow, min(3, slow)),
                        "c_with_keys": (with_keys, a.steps, INFLIGHT)}
                row = {}
                for leg, (submit, steps, warm) in legs.items():
                    row[leg] = stats([loop(submit, steps, warm if r == 0 else 1) for r in range(a.runs)])
                res[op][str(D)] = row
                if D == 1:
                    for leg, submit in (("a_registered", keyed(reg)), ("c_with_keys", with_keys)):
                        ms = []
                        for _ in range(a.runs + 1):
                            t0 = time.perf_counter()
                            j = submit()
                            j.wait()
                            ms.append((time.perf_counter() - t0) * 1e3)
                            assert (j.result == 1).all()
                            j.free()
                        lat["%s_%s" % (op, leg)] = [round(x, 3) for x in (statistics.median(ms[1:]), min(ms[1:]), max(ms[1:]))]
            reg.close()
            bare.close()
        maker.close()
        out["curves"][curve] = {"items_per_s": res, "latency_ms_d1": lat}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
