#!/usr/bin/env python3
"""Keyed batch verification (bbs_ctx_set_keyed_batch_verification) against the per-item keyed path, on the shape and loop of
tools/keyed_bench.py: BLS12-381, 4096 items per batch, 32 messages / 8 disclosed, 6 batches in flight, host buffers, every
step's statuses checked, 16-bit windows.  Prints ONE JSON line (kept as profiles/keyed_bv_bench.json).

    python tools/keyed_bv_bench.py [--steps 24] [--warmup 6] [--runs 5] [--min-items 64] [--skip-verify] [--legs a,b]

Legs, proof_verify (pv_) and verify (vf_) each, items/s as [off, on]: the switch off (the per-item path, measured in the same
session) against on with min_items_per_key = --min-items (64: groups form in every leg but 512x8, whatever the library's
default is; the value is recorded in the line as "on_min_items"):
  k1        one key                              k16      16 keys, 256 items each, contiguous
  k64       64 keys, 64 items each, contiguous   k64_mix  64 keys, item i under key i mod 64
  512x8     the 64 keys registered 8 times over, 8 items per entry: no group forms, "on" pays the host-side sort alone
  pv_single_bv   a single-key context with bbs_ctx_set_batch_verification on (what k1 "on" is expected to come near)
Break-even, at 64 items per key (K = 64) and 128 items per key (K = 32):
  spread_k64 / spread_k32   the off leg `--runs` times: [median, min, max]
  sweep_k64 / sweep_k32     on with min_items_per_key = 16, 32, 64, 128, 256 (a threshold above the items per key forms no
                            group): items/s each
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import keyed_bench as kb  # noqa: E402  (sets GPU_MAX_HW_QUEUES as that tool does)

N = kb.N
SWEEP = (16, 32, 64, 128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--min-items", type=int, default=64, help="min_items_per_key of the off / on legs (>= 1)")
    ap.add_argument("--skip-verify", action="store_true")
    ap.add_argument("--legs", default="", help="comma-separated subset of k1, k16, k64, k64_mix, 512x8, single_bv, sweep_k64, sweep_k32")
    a = ap.parse_args()
    from bbs_sign_amd import Engine
    legs = set(x for x in a.legs.split(",") if x)
    want = lambda name: not legs or name in legs
    ops = ("pv",) if a.skip_verify else ("pv", "vf")
    out = {"metric": "keyed_batch_verification_items_per_s", "curve": "bls12_381", "batch": N, "messages": kb.L, "disclosed": kb.R,
           "inflight": kb.INFLIGHT, "window_bits": 16, "format": "[off, on]", "on_min_items": a.min_items}
    loads = {}

    def load(K):
        if K not in loads:
            loads[K] = kb.workload(K, 2 + K)
        return loads[K]

    def ctx(gens, api_id, pk=None, keys=None):
        e = Engine("bls12_381", device=0, window_bits=16)
        e.set_generators(gens, api_id)
        if pk is not None:
            e.set_public_key(pk)
        if keys is not None:
            e.set_public_keys(keys)
        return e

    def submitters(e, w, kid, perm=None):
        """{op: submit function} of workload w under key indexes kid (perm: batch item t = workload item perm[t])."""
        _, _, _, _, sigs, msgs, proofs, dm, dis = w
        pick = (lambda x: x) if perm is None else (lambda x: [x[p] for p in perm])
        n, keep, args = e._pv_inputs(pick(proofs), pick(dm), pick(dis), None, None)
        fns = {"pv": kb.packed(e, "bbs_core_proof_verify_keyed_submit", n, args, keep, kid)}
        if "vf" in ops:
            n, keep, args = e._vf_core_args(pick(sigs), pick(msgs), None)
            fns["vf"] = kb.packed(e, "bbs_core_verify_keyed_submit", n, args, keep, kid)
        return fns

    def rate(e, submit, on, min_items=0):
        e.set_keyed_batch_verification(on, None, min_items)
        r = kb.loop(submit, a.steps, a.warmup)
        e.set_keyed_batch_verification(False)
        return round(r, 1)

    def off_on(name, e, fns):
        for op, submit in fns.items():
            out["%s_%s" % (op, name)] = [rate(e, submit, False), rate(e, submit, True, a.min_items)]

    for K, name in ((1, "k1"), (16, "k16"), (64, "k64")):
        if want(name):
            w = load(K)
            e = ctx(w[0], w[1], keys=w[2])
            off_on(name, e, submitters(e, w, np.array(w[3], dtype=np.uint32)))
            e.close()
    if want("k64_mix"):
        w = load(64)
        per = N // 64
        perm = [(t % 64) * per + t // 64 for t in range(N)]
        e = ctx(w[0], w[1], keys=w[2])
        off_on("k64_mix", e, submitters(e, w, np.array(w[3], dtype=np.uint32)[perm], perm))
        e.close()
    if want("512x8"):
        w = load(64)
        e = ctx(w[0], w[1], keys=[w[2][k % 64] for k in range(512)])
        off_on("512x8", e, submitters(e, w, np.array([w[3][i] + 64 * (i % 8) for i in range(N)], dtype=np.uint32)))
        e.close()
    if want("single_bv"):
        w = load(1)
        e = ctx(w[0], w[1], pk=w[2][0])
        n, keep, args = e._pv_inputs(w[6], w[7], w[8], None, None)
        submit = kb.packed(e, "bbs_core_proof_verify_submit", n, args, keep)
        off = round(kb.loop(submit, a.steps, a.warmup), 1)
        e.set_batch_verification(True)
        out["pv_single_bv"] = [off, round(kb.loop(submit, a.steps, a.warmup), 1)]
        e.close()
    for K in (64, 32):
        if not want("sweep_k%d" % K):
            continue
        w = load(K)
        e = ctx(w[0], w[1], keys=w[2])
        for op, submit in submitters(e, w, np.array(w[3], dtype=np.uint32)).items():
            offs = [rate(e, submit, False) for _ in range(a.runs)]
            out["%s_spread_k%d" % (op, K)] = [statistics.median(offs), min(offs), max(offs)]
            out["%s_sweep_k%d" % (op, K)] = {str(m): rate(e, submit, True, m) for m in SWEEP}
        e.close()
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
