#!/usr/bin/env python3
"""Seeded proof_gen (bbs_ctx_set_seeded_random_scalars: the random scalars drawn on the device) against the path that uploads them.
One device, BLS12-381, 4096 proofs per job, 32 messages of which 8 are disclosed, the library's default windows, the wire form
(bbs_proof_gen_wire_submit: signature octets and raw messages in, proof octets and statuses out, every status checked), a
submit loop at 1 and at 16 jobs in flight.  Writes profiles/seeded_gen_bench.json and prints it as ONE JSON line.

    python tools/seeded_gen_bench.py [--steps 48] [--warmup 16] [--runs 5] [--parent-lib PATH] [--draw-trace DIR]

Legs (proofs/s, host-inclusive; [median, min, max] over --runs runs, the legs ALTERNATING run by run), each at both depths:
  a_uploaded        the scalars drawn before the clock starts and uploaded, 928 bytes per item: today's path, the draw not
                    counted; its min - max is the spread the others are read against.  With --parent-lib PATH (a build of the
                    library from BEFORE the switch) this leg is ALSO measured on that library, in a child process of its own.
  b_host_draw       as a, with the draw counted: api.calculate_random_scalars for every item of every job, packed and uploaded
                    -- the rate a caller of the public Python layer gets today
  c_item_seeds      switch on, a 32-byte seed per item (fresh bytes per job, drawn outside the clock as a's scalars are)
  d_job_seed        switch on, one 32-byte seed per job (rnd_off = NULL)
--draw-trace DIR: a child process of this tool runs 8 seeded jobs under `rocprofv3 --kernel-trace` (a run of its own, output in
DIR) and the mean duration of the PgDraw dispatches is reported as pg_draw_kernel_ms_per_job (the stage runs once per upload,
in front of the ingest stage, so bbs_job_stage_times does not list it).
"""
import argparse
import csv
import ctypes
import glob
import json
import os
import random
import secrets
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CURVE, N, L, R, DEPTHS = "bls12_381", 4096, 32, 8, (1, 16)
NEW_EXPORTS = ("bbs_ctx_set_seeded_random_scalars", "bbs_seeded_random_scalars_batch")


def workload(suite, gens, seed=1):
    """N items of L raw messages signed by one issuer (an 8-bit context, untimed), as signature octets; R disclosed indexes."""
    from bbs_sign_amd import Engine
    rng = random.Random(seed)
    sk = rng.randrange(1, suite.curve.r)
    raw = [[b"seeded-bench-%d-%d" % (i, j) for j in range(L)] for i in range(N)]
    disclosed = [sorted(rng.sample(range(L), R)) for _ in range(N)]
    eng = Engine(CURVE, device=0, window_bits=8)
    eng.set_generators(gens, suite.api_id)
    eng.set_secret_key(sk)
    octs, st = eng.sign_wire_batch(raw, [b""] * N)
    assert (np.asarray(st) == 1).all()
    pk = eng.public_key()
    eng.close()
    return pk, (octs, raw, disclosed)


def packed(eng, items, rnd):
    """(submit, retire) over arguments packed ONCE and output buffers that are reused.  rnd() -> (bytes array, offsets or None):
    the random_scalars / rnd_off pair of one job, called inside the clock for every job."""
    from bbs_sign_amd import _lib
    from bbs_sign_amd.engine import Job, _ragged_bytes, _u8, _u64
    octs, raw, disclosed = items
    ob, bad = eng._sig_octets(octs)
    assert not bad
    mb, mbo, mio = eng._raw_msgs(raw)
    di, dio = eng._indexes(disclosed)
    hb, ho = _ragged_bytes([b""] * N)
    pb, po = _ragged_bytes([b""] * N)
    plen = 3 * eng.fpb + 32 * (4 + L - R)
    spare = []

    def submit():
        bufs = spare.pop() if spare else (np.zeros(N, dtype=np.int8), np.zeros(N * plen, dtype=np.uint8), np.zeros(N + 1, dtype=np.uint64))
        st, oc, oo = bufs
        st[:] = -128
        rs, ro = rnd()
        j = ctypes.c_void_p()
        rc = eng.lib.bbs_proof_gen_wire_submit(eng.h, N, _u8(ob), _u8(mb), _u64(mbo), _u64(mio), _u64(di), _u64(dio), _u8(rs), _u64(ro),
                                               _u8(hb), _u64(ho), _u8(pb), _u64(po), _u8(oc), _u64(oo), st.ctypes.data_as(_lib.c_i8p), ctypes.byref(j))
        assert rc == 0, rc
        job = Job(eng, j, N)
        job.bufs, job.keep = bufs, (rs, ro, ob, mb, mbo, mio, di, dio, hb, ho, pb, po)
        return job

    def retire(job):
        job.wait()
        st, _, oo = job.bufs
        assert (st == 1).all() and int(oo[N]) == N * plen, np.unique(st, return_counts=True)
        job.free()
        spare.append(job.bufs)
    return submit, retire


def loop(leg, steps, warmup, depth):
    """`depth` jobs outstanding, the oldest retired first, every status checked; proofs/s over `steps` jobs."""
    submit, retire = leg

    def run(k):
        pending = []
        for _ in range(k):
            if len(pending) >= depth:
                retire(pending.pop(0))
            pending.append(submit())
        for j in pending:
            retire(j)
    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return N * steps / (time.perf_counter() - t0)


def contexts(only=None):
    from bbs_sign_amd import Engine, api
    from bbs_sign_amd.engine import _bytes_arr
    from oracle import bbs
    suite = bbs.SUITES[CURVE]
    gens = api.create_generators(CURVE, L + 1)
    pk, items = workload(suite, gens)
    engines = []

    def ctx(seeded):
        e = Engine(CURVE, device=0)                 # window_bits=None: the library's default
        e.set_generators(gens, suite.api_id)
        e.set_public_key(pk)
        if seeded:
            e.set_seeded_random_scalars(True, suite.api_id + b"SEEDED_RANDOM_SCALARS_")
        engines.append(e)
        return e
    rng = random.Random(2)
    plain = ctx(False)
    pre = plain._scalars([[rng.randrange(1, suite.curve.r) for _ in range(5 + L - R)] for _ in range(N)])
    legs = {"a_uploaded": packed(plain, items, lambda: pre)}
    if only != "a":
        seeded = ctx(True)
        off32 = np.arange(N + 1, dtype=np.uint64) * 32
        legs["b_host_draw"] = packed(plain, items, lambda: plain._scalars([api.calculate_random_scalars(CURVE, 5 + L - R) for _ in range(N)]))
        legs["c_item_seeds"] = packed(seeded, items, lambda: (np.frombuffer(secrets.token_bytes(32 * N), dtype=np.uint8), off32))
        legs["d_job_seed"] = packed(seeded, items, lambda: (_bytes_arr(secrets.token_bytes(32)), None))
    return legs, engines


def measure(a, only=None):
    legs, engines = contexts(only)
    got = {(k, d): [] for k in legs for d in DEPTHS}
    for _ in range(a.runs):
        for d in DEPTHS:
            for name, leg in legs.items():
                # the host draw of leg b takes seconds per job: a fixed, small number of jobs measures it as well
                steps, warmup = (max(2, d // 4), 1) if name == "b_host_draw" else (a.steps, a.warmup)
                got[(name, d)].append(loop(leg, steps, warmup, d))
    out = {"%s_inflight%d" % k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in got.items()}
    out["table_bytes_per_context"] = [int(e.lib.bbs_ctx_table_bytes(e.h)) for e in engines]
    for e in engines:
        e.close()
    return out


def draw_child():
    """8 seeded jobs, one after the other: what --draw-trace runs under the profiler."""
    legs, engines = contexts()
    loop(legs["c_item_seeds"], 8, 0, 1)
    for e in engines:
        e.close()


def draw_trace(outdir):
    """Mean duration of the PgDraw dispatches of draw_child(), in ms, from the profiler's kernel trace."""
    if not shutil.which("rocprofv3"):
        return None, "rocprofv3 not found"
    os.makedirs(outdir, exist_ok=True)
    r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", outdir, "--", sys.executable, os.path.abspath(__file__),
                        "--draw-child"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode:
        return None, "profiler run failed (%d): %s" % (r.returncode, r.stdout[-300:])
    ns = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "PgDraw" in row.get("Kernel_Name", "") and "PgDrawGate" not in row.get("Kernel_Name", ""):
                    ns.append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    if not ns:
        return None, "no PgDraw dispatch in the trace"
    return round(statistics.mean(ns) / 1e6, 4), "%d dispatches, min %.4f max %.4f ms" % (len(ns), min(ns) / 1e6, max(ns) / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=["a"], default=None, help="measure leg a alone (what --parent-lib runs in its child process)")
    ap.add_argument("--parent-lib", default=None, help="a build of the library without the seeded exports: leg a on it too")
    ap.add_argument("--draw-trace", default=None, metavar="DIR", help="PgDraw's kernel time from a profiler run of its own, output in DIR")
    ap.add_argument("--draw-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_gen_bench.json"))
    a = ap.parse_args()
    if a.draw_child:
        draw_child()
        return
    if a.only:
        print(json.dumps(measure(a, a.only)))
        return
    out = {"metric": "seeded_proof_gen_proofs_per_s_median_min_max", "curve": CURVE, "batch": N, "messages": L, "disclosed": R,
           "inflight": list(DEPTHS), "window_bits": "library default", "form": "wire", "runs": a.runs, "steps": a.steps}
    if a.parent_lib:
        # a process of its own, started before this one touches the device: two builds of the library never share a process
        env = dict(os.environ, BBS_SIGN_AMD_LIB=os.path.abspath(a.parent_lib), BBS_SIGN_AMD_LIB_OPTIONAL=",".join(NEW_EXPORTS))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "a", "--steps", str(a.steps), "--warmup", str(a.warmup),
                            "--runs", str(a.runs)], env=env, stdout=subprocess.PIPE, text=True, check=True)
        parent = json.loads(r.stdout.strip().splitlines()[-1])
        for d in DEPTHS:
            out["a_uploaded_parent_inflight%d" % d] = parent["a_uploaded_inflight%d" % d]
    if a.draw_trace:
        out["pg_draw_kernel_ms_per_job"], out["pg_draw_kernel_note"] = draw_trace(a.draw_trace)
    out.update(measure(a))
    out["yardstick"] = "a_uploaded_parent" if a.parent_lib else "a_uploaded"
    for d in DEPTHS:
        ref = out["%s_inflight%d" % (out["yardstick"], d)]
        for k in ("b_host_draw", "c_item_seeds", "d_job_seed"):
            key = "%s_inflight%d" % (k, d)
            out[key + "_vs_a"] = round(out[key][0] / ref[0], 4)
            out[key + "_below_a_spread"] = out[key][0] < ref[1]
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
