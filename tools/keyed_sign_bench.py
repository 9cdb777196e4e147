#!/usr/bin/env python3
"""Keyed sign (bbs_core_sign_keyed_submit) against the single-key job it is made of.
One device, BLS12-381, 4096 items per job, 32 messages, the library's default windows, the core form (scalars in host buffers;
records and statuses out, every status checked), 16 jobs in flight.  Writes profiles/keyed_sign_bench.json and prints it as ONE
JSON line.

    python tools/keyed_sign_bench.py [--steps 48] [--warmup 16] [--runs 5] [--keys 64] [--parent-lib PATH]

Legs (signatures/s, host-inclusive; [median, min, max] over --runs runs, the legs ALTERNATING run by run):
  a_single_key      bbs_core_sign_submit on a single-key context: the yardstick; its min - max is the spread the others are
                    read against.  With --parent-lib PATH (a build of the library from BEFORE the keyed exports) this leg is
                    ALSO measured on that library, in a child process of its own, as a_single_key_parent.
  b_keyed_k1        keyed, a signing set of one key, the same items
  c_keyed_k64       keyed, 64 keys, item i under key i mod 64
  d_keyed_mixed_k64 the same with bbs_ctx_set_keyed_mixed_lengths on, every item of 32 messages
and the one-off registration time (bbs_ctx_set_secret_keys on a fresh context, generators set) of 64 and of 4096 keys.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE, N, L, INFLIGHT = "bls12_381", 4096, 32, 16
NEW_EXPORTS = ("bbs_ctx_set_secret_keys", "bbs_ctx_add_secret_keys", "bbs_ctx_secret_key_count", "bbs_core_sign_keyed_submit",
               "bbs_core_sign_keyed_batch", "bbs_sign_wire_keyed_submit", "bbs_sign_wire_keyed_batch")


def packed(eng, msgs, key_index=None):
    """(submit, retire) over arguments packed ONCE and output buffers that are reused: only the C call is per step."""
    from bbs_sign_amd import _lib
    from bbs_sign_amd.engine import Job, _ragged_bytes, _u8, _u64
    n = len(msgs)
    ms, mo = eng._scalars(msgs)
    hb, ho = _ragged_bytes([b""] * n)
    rec = 2 * eng.fpb + 32
    ki = None if key_index is None else np.ascontiguousarray(key_index, dtype=np.uint32)
    fn = eng.lib.bbs_core_sign_submit if ki is None else eng.lib.bbs_core_sign_keyed_submit
    head = (eng.h, n) if ki is None else (eng.h, n, ki.ctypes.data_as(_lib.c_u32p))
    spare = []

    def submit():
        bufs = spare.pop() if spare else (np.zeros(n, dtype=np.int8), np.zeros(n * rec, dtype=np.uint8))
        st, out = bufs
        st[:] = -128
        j = ctypes.c_void_p()
        rc = fn(*head, _u8(ms), _u64(mo), _u8(hb), _u64(ho), _u8(out), st.ctypes.data_as(_lib.c_i8p), ctypes.byref(j))
        assert rc == 0, rc
        job = Job(eng, j, n)
        job.bufs, job.keep = bufs, (ms, mo, hb, ho, ki)
        return job

    def retire(job):
        job.wait()
        st = job.bufs[0]
        assert (st == 1).all(), np.unique(st, return_counts=True)
        job.free()
        spare.append(job.bufs)
    return submit, retire


def loop(leg, steps, warmup):
    """INFLIGHT jobs outstanding, the oldest retired first, every status checked; signatures/s over `steps` jobs."""
    submit, retire = leg

    def run(k):
        pending = []
        for _ in range(k):
            if len(pending) >= INFLIGHT:
                retire(pending.pop(0))
            pending.append(submit())
        for j in pending:
            retire(j)
    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return N * steps / (time.perf_counter() - t0)


def measure(a, only=None):
    from bbs_sign_amd import Engine, api
    from oracle import bbs
    suite = bbs.SUITES[CURVE]
    r = suite.curve.r
    gens = api.create_generators(CURVE, L + 1)
    rng = random.Random(1)
    msgs = [[rng.randrange(r) for _ in range(L)] for _ in range(N)]
    K = a.keys
    sks = [rng.randrange(1, r) for _ in range(max(K, 4096))]
    engines = []

    def ctx():
        e = Engine(CURVE, device=0)                 # window_bits=None: the library's default
        e.set_generators(gens, suite.api_id)
        engines.append(e)
        return e
    legs, out = {}, {}
    single = ctx()
    single.set_secret_key(sks[0])
    legs["a_single_key"] = packed(single, msgs)
    if only != "a":
        k1, kk, km = ctx(), ctx(), ctx()
        assert list(k1.set_secret_keys(sks[:1])[0]) == [1]
        t0 = time.perf_counter()
        st = kk.set_secret_keys(sks[:K])[0]
        out["registration_ms_%d_keys" % K] = round((time.perf_counter() - t0) * 1e3, 2)
        assert list(st) == [1] * K
        km.set_keyed_mixed_lengths(True)
        assert list(km.set_secret_keys(sks[:K])[0]) == [1] * K
        reg = ctx()
        t0 = time.perf_counter()
        st = reg.set_secret_keys(sks[:4096])[0]
        out["registration_ms_4096_keys"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert (np.asarray(st) == 1).all()
        engines.remove(reg)
        reg.close()
        kid = np.arange(N, dtype=np.uint32) % K
        legs["b_keyed_k1"] = packed(k1, msgs, np.zeros(N, dtype=np.uint32))
        legs["c_keyed_k%d" % K] = packed(kk, msgs, kid)
        legs["d_keyed_mixed_k%d" % K] = packed(km, msgs, kid)
    got = {k: [] for k in legs}
    for _ in range(a.runs):
        for name, leg in legs.items():
            got[name].append(loop(leg, a.steps, a.warmup))
    out.update({k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in got.items()})
    out["table_bytes_per_context"] = int(single.lib.bbs_ctx_table_bytes(single.h))
    for e in engines:
        e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--only", choices=["a"], default=None, help="measure leg a alone (what --parent-lib runs in its child process)")
    ap.add_argument("--parent-lib", default=None, help="a build of the library without the keyed sign exports: leg a on it too")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_sign_bench.json"))
    a = ap.parse_args()
    if a.only:
        print(json.dumps(measure(a, a.only)))
        return
    out = {"metric": "keyed_sign_signatures_per_s_median_min_max", "curve": CURVE, "batch": N, "messages": L, "inflight": INFLIGHT,
           "window_bits": "library default", "form": "core", "runs": a.runs, "steps": a.steps, "keys": a.keys}
    if a.parent_lib:
        # a process of its own, started before this one touches the device: two builds of the library never share a process
        env = dict(os.environ, BBS_SIGN_AMD_LIB=os.path.abspath(a.parent_lib), BBS_SIGN_AMD_LIB_OPTIONAL=",".join(NEW_EXPORTS))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "a", "--steps", str(a.steps), "--warmup", str(a.warmup),
                            "--runs", str(a.runs)], env=env, stdout=subprocess.PIPE, text=True, check=True)
        out["a_single_key_parent"] = json.loads(r.stdout.strip().splitlines()[-1])["a_single_key"]
    out.update(measure(a))
    ref = out.get("a_single_key_parent", out["a_single_key"])
    out["yardstick"] = "a_single_key_parent" if a.parent_lib else "a_single_key"
    for k in [k for k in out if k[:2] in ("b_", "c_", "d_")]:
        out[k + "_vs_a"] = round(out[k][0] / ref[0], 4)
        out[k + "_outside_a_spread"] = not (ref[1] <= out[k][0] <= ref[2])
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
