#!/usr/bin/env python3
"""The job-local key cache (bbs_ctx_set_job_key_cache) on the headline loop's shape, by the method of tools/job_keys_bench.py:
4096 items per job, 32 messages / 8 disclosed, 16-bit windows, 6 jobs in flight, host buffers, every status checked, median
and [min, max] of --runs runs, every leg in one session.  BLS12-381 and BN254, proof_verify and verify, D = 1 / 16 / 256 / 4096
distinct keys per job (item i under key i mod D).  Prints ONE JSON line; --out FILE also writes it there.

    python tools/job_key_cache_bench.py [--curves bls12_381,bn254] [--d 1,16,256,4096] [--runs 5] [--out profiles/job_key_cache_bench.json]

Legs per (curve, operation, D), items/s:
  a_registered     the keyed loop, all D keys registered beforehand: the ceiling
  c_with_keys      bbs_*_with_keys_*, cache off: one walk of the key stage per job
  d_cache_warm     the same calls, cache on and warm: every key a hit (checked: the loop moves no miss)
  e_new_1_64, e_new_1_8   cache on; every job brings its D recurring keys AND max(1, D / 64) (D / 8) keys the cache does not hold --
                   valid keys no item names, so the items and their statuses are those of the other legs and the key stage walks
                   over the misses alone (checked: every one of them is a miss, no job is bypassed).  The new keys come from a
                   pool of twice the cache's capacity, cycled: a key comes round again only after it has been evicted.
and, for D = 1, one job alone from submit to wait (`latency_ms_d1`): registered, with_keys with the cache off, a hit, a miss;
and `submit_us`: the time the submitting thread spends inside the submit call (the host lookup of n_keys strings is in it) at
the largest D, legs a, c and d.
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


def loop(submit, steps, warmup, spent=None):
    """`submit()` -> job; INFLIGHT outstanding, oldest retired first, every status checked; items/s over `steps`.
    spent: a list that receives the seconds of every timed submit call."""
    def run(k, rec):
        pending = []
        for _ in range(k):
            if len(pending) >= INFLIGHT:
                j = pending.pop(0)
                j.wait()
                assert (j.result == 1).all(), np.unique(j.result, return_counts=True)
                j.free()
            t = time.perf_counter()
            pending.append(submit())
            if rec is not None:
                rec.append(time.perf_counter() - t)
        for j in pending:
            j.wait()
            assert (j.result == 1).all(), np.unique(j.result, return_counts=True)
            j.free()
    run(warmup, None)
    t0 = time.perf_counter()
    run(steps, spent)
    return N * steps / (time.perf_counter() - t0)


def stats(v, digits=1):
    return [round(statistics.median(v), digits), round(min(v), digits), round(max(v), digits)]


def main():
    global N, L, R
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--d", default="1,16,256,4096")
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
    from bbs_sign_amd.engine import Job
    from oracle import bbs
    N, L, R = a.batch, a.messages, a.disclosed
    Ds = [int(x) for x in a.d.split(",")]
    out = {"metric": "job_key_cache_items_per_s_median_min_max", "batch": N, "messages": L, "disclosed": R, "inflight": INFLIGHT,
           "window_bits": 16, "runs": a.runs, "steps": a.steps, "commit": a.commit, "curves": {}}
    u8 = _lib.c_u8p
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
        Dmax = max(Ds)
        cap_of = lambda D: 2 * D + 8                    # the recurring keys, and the strangers of every job in flight, stay pinned
        n_pool = 2 * cap_of(Dmax)                       # the strangers of leg e: valid keys no item names
        sks = [bbs.key_gen(suite, bytes([3, k % 256, (k // 256) % 256, k // 65536] + [7] * 28), b"", b"BBS-SIG-KEYGEN-SALT-") for k in range(Dmax + n_pool)]
        st, pks, first = maker.set_secret_keys(sks[:Dmax])
        assert (np.asarray(st) == 1).all() and first == 0
        octs = [bbs.g2_compress(c, k) for k in pks]
        _, pool, st = maker.sk_to_pk_batch(sks[Dmax:])
        assert (np.asarray(st) == 1).all()
        pool = [bytes(o) for o in pool]
        assert len(set(pool) | set(octs)) == Dmax + n_pool
        res = {"pv": {}, "vf": {}}
        lat, spent_us = {}, {}
        for D in Ds:
            kid = np.array([i % D for i in range(N)], dtype=np.uint32)
            sigs, st = maker.core_sign_keyed_batch(kid, msgs)
            assert (st == 1).all()
            proofs, st = maker.core_proof_gen_keyed_batch(kid, sigs, msgs, disclosed, rnds)
            assert (st == 1).all()
            reg, bare, cach = ctx(), ctx(), ctx()
            assert (reg.set_public_keys(pks[:D]) == 1).all()
            cap = cap_of(D)
            cach.set_job_key_cache(cap)
            ko = bare._key_octets(octs[:D])
            kip = kid.ctypes.data_as(_lib.c_u32p)
            pool_d = pool[:2 * cap]
            turn = [0]                                  # the next stranger of the pool (one cycle through it evicts every one)
            for op in ("pv", "vf"):
                if op == "pv":
                    n, keep, args = reg._pv_inputs(proofs, dm, disclosed, None, None)
                    name = "bbs_core_proof_verify_%s_submit"
                else:
                    n, keep, args = reg._vf_core_args(sigs, msgs, None)
                    name = "bbs_core_verify_%s_submit"

                def keyed():
                    j = reg._status_submit(name % "keyed", n, args, kid)
                    j.keep = keep
                    return j

                def with_keys(eng, octets=ko, n_keys=D):
                    def submit():
                        st_ = np.full(N, -128, dtype=np.int8)
                        j = ctypes.c_void_p()
                        rc = getattr(eng.lib, name % "with_keys")(eng.h, n, n_keys, octets.ctypes.data_as(u8), kip, *args,
                                                                  st_.ctypes.data_as(_lib.c_i8p), ctypes.byref(j))
                        assert rc == 0, rc
                        job = Job(eng, j, n)
                        job.result, job._fixup, job.keep = st_[:n], None, (keep, octets)
                        return job
                    return submit

                def with_new(share):
                    fresh = max(1, D // share)

                    def submit():
                        at = turn[0]
                        turn[0] += fresh
                        new = [pool_d[(at + t) % len(pool_d)] for t in range(fresh)]
                        return with_keys(cach, np.concatenate([ko[:D * len(octs[0])], np.frombuffer(b"".join(new), dtype=np.uint8)]), D + fresh)()
                    return submit, fresh

                row = {}
                spent = {"a": [], "c": [], "d": []}
                row["a_registered"] = stats([loop(keyed, a.steps, INFLIGHT if r == 0 else 1, spent["a"]) for r in range(a.runs)])
                row["c_with_keys"] = stats([loop(with_keys(bare), a.steps, INFLIGHT if r == 0 else 1, spent["c"]) for r in range(a.runs)])
                warm = with_keys(cach)
                j = warm()
                j.wait()
                j.free()
                before = cach.job_key_cache_report()
                row["d_cache_warm"] = stats([loop(warm, a.steps, INFLIGHT if r == 0 else 1, spent["d"]) for r in range(a.runs)])
                after = cach.job_key_cache_report()
                assert after["misses"] == before["misses"] and after["bypassed_jobs"] == before["bypassed_jobs"], (before, after)
                for share in (64, 8):
                    submit, fresh = with_new(share)
                    before = cach.job_key_cache_report()
                    row["e_new_1_%d" % share] = stats([loop(submit, a.steps, INFLIGHT if r == 0 else 1) for r in range(a.runs)])
                    after = cach.job_key_cache_report()
                    jobs = a.runs * a.steps + INFLIGHT + a.runs - 1
                    assert after["misses"] - before["misses"] == jobs * fresh and after["bypassed_jobs"] == before["bypassed_jobs"], (before, after, jobs, fresh)
                    row["e_new_1_%d_keys_per_job" % share] = fresh
                res[op][str(D)] = row
                print("# %s %s D=%d %s" % (curve, op, D, json.dumps(row)), file=sys.stderr, flush=True)
                if D == Dmax:
                    spent_us[op] = {"D": D, **{k: stats([x * 1e6 for x in v]) for k, v in spent.items()}}
                if D == 1:
                    def miss():
                        turn[0] += 1
                        return with_keys(cach, np.frombuffer(pool_d[(turn[0] - 1) % len(pool_d)], dtype=np.uint8).copy(), 1)

                    # (a miss: a key the cache does not hold -- the one item is then under ANOTHER key and must fail, the time is the same)
                    for leg, submit, want in (("a_registered", keyed, 1), ("c_with_keys", with_keys(bare), 1), ("d_hit", warm, 1), ("d_miss", None, 0)):
                        ms = []
                        for _ in range(a.runs + 1):
                            s = submit if submit else miss()
                            t0 = time.perf_counter()
                            j = s()
                            j.wait()
                            ms.append((time.perf_counter() - t0) * 1e3)
                            assert (j.result == want).all()
                            j.free()
                        lat["%s_%s" % (op, leg)] = stats(ms[1:], 3)
            for e in (reg, bare, cach):
                e.close()
        maker.close()
        out["curves"][curve] = {"items_per_s": res, "latency_ms_d1": lat, "submit_us": spent_us}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
