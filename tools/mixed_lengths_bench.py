#!/usr/bin/env python3
"""Mixed message counts: one context with bbs_ctx_set_mixed_lengths against the issuer's one-context-per-count routing.
One device, 4096 proof_verify items per list, lengths uniform in 1 .. 32, a quarter of each item's messages disclosed,
16-bit windows, the wire form (proof octets and raw disclosed messages in host buffers, statuses out and checked every
step), 6 lists in flight.  Writes profiles/mixed_lengths_bench.json and prints it as ONE JSON line.

    python tools/mixed_lengths_bench.py [--steps 12] [--warmup 6] [--runs 5] [--curves bls12_381,bn254]

Per curve (items/s, host-inclusive; [median, min, max] over --runs runs, the legs of a pair ALTERNATING run by run):
  a_issuer        bbs_issuer_proof_verify_submit on the list, its 32 contexts warm (today's path)
  b_mixed         bbs_proof_verify_wire_submit on ONE context for 32 messages with the switch on
  c_uniform_on    the same context, a list whose items all have 32 messages, the switch on
  c_uniform_off   the same context and list, the switch off (the price of the new stages on uniform input is c_on / c_off)
  table_bytes     bbs_issuer_table_bytes of the warm issuer against bbs_ctx_table_bytes of the one context
  first_call_s    a cold issuer meeting the 32 lengths in its first call, against the one context's setup (generators by the
                  host, tables, key, per-length prefixes) and its first call
The workload is made untimed by an issuer at 8-bit windows (sign and proof_gen of every item by its own length).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, LMAX, INFLIGHT, WINDOW_BITS = 4096, 32, 6, 16


def workload(curve, lengths, seed):
    """(pk, proof octets, raw disclosed messages, disclosed indexes) of len(lengths) items, item i with lengths[i] messages."""
    import random
    from bbs_sign_amd import Issuer
    from oracle import bbs
    suite = bbs.SUITES[curve]
    rng = random.Random(seed)
    sk = rng.randrange(1, suite.curve.r)
    iss = Issuer(curve, suite.api_id, max_messages=LMAX, window_bits=8)
    iss.set_secret_key(sk)
    raw = [[b"m%d.%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    so, st = iss.sign(raw)
    assert (np.asarray(st) == 1).all()
    disclosed = [sorted(rng.sample(range(l), l // 4)) for l in lengths]
    rnds = [[rng.randrange(1, suite.curve.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, disclosed)]
    po, st = iss.proof_gen(so, raw, disclosed, rnds)
    assert (np.asarray(st) == 1).all()
    iss.close()
    return bbs.sk_to_pk(suite, sk), po, [[raw[i][j] for j in d] for i, d in enumerate(disclosed)], disclosed


def loop(submit, steps, warmup):
    """INFLIGHT lists outstanding, the oldest retired first, every status checked; items/s over `steps` lists."""
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
            assert (j.result == 1).all()
            j.free()
    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return N * steps / (time.perf_counter() - t0)


def alternating(legs, runs, steps, warmup):
    """legs: name -> (prepare, submit).  Every run measures each leg once, in turn; -> name -> [median, min, max]."""
    got = {k: [] for k in legs}
    for _ in range(runs):
        for name, (prepare, submit) in legs.items():
            if prepare:
                prepare()
            got[name].append(loop(submit, steps, warmup))
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in got.items()}


def one_curve(curve, a):
    import random
    from bbs_sign_amd import Engine, Issuer, api
    from oracle import bbs
    suite = bbs.SUITES[curve]
    rng = random.Random(5)
    lengths = [rng.randrange(1, LMAX + 1) for _ in range(N)]
    pk, po, draw, disclosed = workload(curve, lengths, 1)
    pk_u, po_u, draw_u, disclosed_u = workload(curve, [LMAX] * N, 2)
    out = {"lengths_present": len(set(lengths))}
    # ---- (a) the issuer: cold first call, then warm
    iss = Issuer(curve, suite.api_id, max_messages=LMAX, window_bits=WINDOW_BITS)
    iss.set_public_key(pk)
    # (the host buffers of both legs are packed before either clock starts: the two first-call figures cover the library's
    # work alone -- generators on the host, tables, key, prefixes, the call)
    n_a, keep_a, args_a = iss.pack_proof_verify(po, draw, disclosed)
    n_b, keep_b, args_b = n_a, keep_a, args_a       # (bbs_proof_verify_wire_* takes the same eleven arrays in the same order)
    t0 = time.perf_counter()
    st = iss.proof_verify_packed(n_a, args_a)
    cold_issuer = time.perf_counter() - t0
    assert (st == 1).all()
    # ---- (b) the one context: setup and first call
    t0 = time.perf_counter()
    gens = api.create_generators(curve, LMAX + 1)
    t_gens = time.perf_counter() - t0
    eng = Engine(curve, device=0, window_bits=WINDOW_BITS)
    eng.set_generators(gens, suite.api_id)
    eng.set_public_key(pk)
    eng.set_mixed_lengths(True)
    st = eng._status_batch("bbs_proof_verify_wire_batch", n_b, args_b)
    cold_ctx = time.perf_counter() - t0
    assert (st == 1).all()
    out["first_call_s"] = {"issuer_32_new_lengths": round(cold_issuer, 3), "one_context": round(cold_ctx, 3),
                           "one_context_generators_on_host": round(t_gens, 3)}
    out["table_bytes"] = {"issuer": int(iss.table_bytes()), "issuer_contexts": int(iss.context_count()),
                          "one_context": int(eng.lib.bbs_ctx_table_bytes(eng.h))}

    def sub_a():
        j = iss.proof_verify_submit_packed(n_a, args_a)
        j.keep = keep_a
        return j

    def sub_b():
        j = eng._status_submit("bbs_proof_verify_wire_submit", n_b, args_b)
        j.keep = keep_b
        return j
    out.update(alternating({"a_issuer": (None, sub_a), "b_mixed": (None, sub_b)}, a.runs, a.steps, a.warmup))
    out["b_vs_a"] = round(out["b_mixed"][0] / out["a_issuer"][0], 4)
    iss.close()
    # ---- (c) uniform input on the same context (another key: the list is another issuer's), switch on against off
    eng.set_public_key(pk_u)
    n_c, keep_c, args_c = eng._wire_inputs(po_u, draw_u, disclosed_u, None, None)

    def sub_c():
        j = eng._status_submit("bbs_proof_verify_wire_submit", n_c, args_c)
        j.keep = keep_c
        return j
    out.update(alternating({"c_uniform_on": (lambda: eng.set_mixed_lengths(True), sub_c),
                            "c_uniform_off": (lambda: eng.set_mixed_lengths(False), sub_c)}, a.runs, a.steps, a.warmup))
    out["c_on_vs_off"] = round(out["c_uniform_on"][0] / out["c_uniform_off"][0], 4)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_lengths_bench.json"))
    a = ap.parse_args()
    out = {"metric": "mixed_lengths_proof_verify_items_per_s_median_min_max", "batch": N, "lengths": "uniform 1..%d" % LMAX,
           "disclosed": "a quarter", "inflight": INFLIGHT, "window_bits": WINDOW_BITS, "form": "wire", "runs": a.runs, "steps": a.steps}
    for curve in a.curves.split(","):
        out[curve] = one_curve(curve, a)
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
