#!/usr/bin/env python3
"""proof_gen under issuer keys that arrive with the job (bbs_core_proof_gen_with_keys_*), on the headline loop's shape: 4096
items per job, 32 messages / 8 disclosed, 16-bit windows, 6 jobs in flight, host buffers, every status checked.  BLS12-381 and
BN254, D = 1 / 16 / 64 / 256 / 1024 / 4096 distinct keys per job (item i under key i mod D).  Prints ONE JSON line; --out FILE
also writes it there.

    python tools/job_keys_gen_bench.py [--curves bls12_381,bn254] [--d 1,16,64,256,1024,4096] [--runs 5] [--out profiles/job_keys_gen_bench.json]

Four legs per (curve, D), items/s, median and [min, max] of --runs runs:
  a_registered        the keyed loop, all D keys registered beforehand: the ceiling
  b_register_per_job  what a caller without the new exports must do: the context's key set replaced by that job's D keys from
                      octets (bbs_ctx_set_public_keys(0) + bbs_ctx_add_public_keys_octets), then the keyed job
  c_with_keys         the new exports, cache off: the job prepares its D keys by the domain-only stage
  d_with_keys_cached  the new exports with bbs_ctx_set_job_key_cache(max(D, 8)), in steady state: every key a hit
`latency_ms_d1`: one job alone, submit to wait, D = 1, legs a and c.
`key_stage_ms`: the key stage alone for 64 and 4096 keys, call to return with the read-back of the entries --
bbs_selftest_key_entries(path = 1), the full stage, against bbs_selftest_key_domain_entries.
The workload is generated untimed by ONE context through keyed sign (a signing set of D keys).
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


def stats(v, nd=1):
    return [round(statistics.median(v), nd), round(min(v), nd), round(max(v), nd)]


def main():
    global N, L, R
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--d", default="1,16,64,256,1024,4096")
    ap.add_argument("--stage", default="64,4096", help="key counts of the key-stage-alone timing")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=18)
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="recorded in the output: the commit the numbers were taken at")
    ap.add_argument("--lib", default="", help="another build of the library (a dry run through the host twin)")
    ap.add_argument("--batch", type=int, default=N, help="items per job (dry runs)")
    ap.add_argument("--messages", type=int, default=L, help="messages per item (dry runs)")
    ap.add_argument("--disclosed", type=int, default=R, help="disclosed messages per item (dry runs)")
    ap.add_argument("--window-bits", type=int, default=16, help="window width of the timed contexts (dry runs)")
    a = ap.parse_args()
    import keyreg_cases as kr
    import parity_cases as pc
    from bbs_sign_amd import Engine, _lib
    from bbs_sign_amd.engine import Job
    from oracle import bbs
    N, L, R = a.batch, a.messages, a.disclosed
    Ds = [int(x) for x in a.d.split(",")]
    stage_ns = [int(x) for x in a.stage.split(",") if x]
    out = {"metric": "job_keys_gen_items_per_s_median_min_max", "batch": N, "messages": L, "disclosed": R, "inflight": INFLIGHT,
           "window_bits": a.window_bits, "runs": a.runs, "commit": a.commit, "curves": {}}
    for curve in a.curves.split(","):
        suite = bbs.SUITES[curve]
        c = suite.curve
        gens = pc.gens_for(suite, L + 1)

        def ctx(wb=a.window_bits):
            e = Engine(curve, device=0, window_bits=wb, lib_path=a.lib or None)
            e.set_generators(gens, suite.api_id)
            return e

        maker = ctx(min(8, a.window_bits))
        msgs, disclosed, rnds = pc.bench_items(suite, maker, N, L, R)
        nk = max(Ds + stage_ns)
        sks = [bbs.key_gen(suite, bytes([3, k % 256, k // 256] + [7] * 29), b"", b"BBS-SIG-KEYGEN-SALT-") for k in range(nk)]
        st, pks, first = maker.set_secret_keys(sks)
        assert (np.asarray(st) == 1).all() and first == 0
        octs = [bbs.g2_compress(c, k) for k in pks]
        res, lat, stage = {}, {}, {}
        for D in Ds:
            kid = np.array([i % D for i in range(N)], dtype=np.uint32)
            sigs, st = maker.core_sign_keyed_batch(kid, msgs)
            assert (st == 1).all()
            reg, bare, cached = ctx(), ctx(), ctx()
            assert (reg.set_public_keys(pks[:D]) == 1).all()
            cached.set_job_key_cache(max(D, 8))
            ko = bare._key_octets(octs[:D])
            kst = np.zeros(D, dtype=np.int8)
            first_ix = ctypes.c_uint32(0)
            # the inputs are marshalled once, untimed; a submit allocates the job's output buffers and calls the export
            n, keep, args = reg._pg_inputs(sigs, msgs, disclosed, rnds, None, None)
            kip = kid.ctypes.data_as(_lib.c_u32p)
            rec = 6 * reg.fpb + 128

            def call(eng, fn, own=()):
                def submit():
                    st_ = np.full(N, -128, dtype=np.int8)
                    pf, cm, cmo = np.zeros(N * rec, dtype=np.uint8), np.zeros(N * L * 32, dtype=np.uint8), np.zeros(N + 1, dtype=np.uint64)
                    j = ctypes.c_void_p()
                    rc = getattr(eng.lib, fn)(eng.h, n, *own, kip, *args, pf.ctypes.data_as(_lib.c_u8p), cm.ctypes.data_as(_lib.c_u8p),
                                              cmo.ctypes.data_as(_lib.c_u64p), st_.ctypes.data_as(_lib.c_i8p), ctypes.byref(j))
                    assert rc == 0, rc
                    job = Job(eng, j, n)
                    job.result, job.keep = st_[:n], (keep, pf, cm, cmo)
                    return job
                return submit

            def keyed(eng):
                return call(eng, "bbs_core_proof_gen_keyed_submit")

            def per_job():
                # the key set of THIS job from octets, synchronously on the submitting thread, then the keyed job
                assert bare.lib.bbs_ctx_set_public_keys(bare.h, 0, None, None, None) == 0
                assert bare.lib.bbs_ctx_add_public_keys_octets(bare.h, D, ko.ctypes.data_as(_lib.c_u8p), kst.ctypes.data_as(_lib.c_i8p),
                                                               None, None, ctypes.byref(first_ix)) == 0
                return keyed(bare)()

            def with_keys(eng):
                return call(eng, "bbs_core_proof_gen_with_keys_submit", (D, ko.ctypes.data_as(_lib.c_u8p)))

            slow = max(3, min(a.steps, int(2.0 / (0.00013 * D + 0.004))))       # leg b: about two seconds per run
            legs = {"a_registered": (keyed(reg), a.steps, INFLIGHT), "b_register_per_job": (per_job, slow, min(3, slow)),
                    "c_with_keys": (with_keys(bare), a.steps, INFLIGHT), "d_with_keys_cached": (with_keys(cached), a.steps, INFLIGHT)}
            row = {}
            for leg, (submit, steps, warm) in legs.items():
                row[leg] = stats([loop(submit, steps, warm if r == 0 else 1) for r in range(a.runs)])
            rep = cached.job_key_cache_report()
            assert rep["misses"] == D and rep["bypassed_jobs"] == 0, rep           # steady state: only the first job missed
            res[str(D)] = row
            if D == 1:
                for leg, submit in (("a_registered", keyed(reg)), ("c_with_keys", with_keys(bare))):
                    ms = []
                    for _ in range(a.runs + 1):
                        t0 = time.perf_counter()
                        j = submit()
                        j.wait()
                        ms.append((time.perf_counter() - t0) * 1e3)
                        assert (j.result == 1).all()
                        j.free()
                    lat[leg] = stats(ms[1:], 3)
            for e in (reg, bare, cached):
                e.close()
        eng = ctx(min(8, a.window_bits))
        for n in stage_ns:
            full, dom = [], []
            for _ in range(a.runs + 1):
                t0 = time.perf_counter()
                _, st1, _ = kr.key_entries(eng, 1, octets=octs[:n])
                t1 = time.perf_counter()
                _, st2 = eng.selftest_key_domain_entries(octs[:n])
                t2 = time.perf_counter()
                assert list(st1) == list(st2) == [1] * n
                full.append((t1 - t0) * 1e3)
                dom.append((t2 - t1) * 1e3)
            stage[str(n)] = {"key_build": stats(full[1:], 3), "key_domain_build": stats(dom[1:], 3)}
        eng.close()
        maker.close()
        out["curves"][curve] = {"items_per_s": res, "latency_ms_d1": lat, "key_stage_ms": stage}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
