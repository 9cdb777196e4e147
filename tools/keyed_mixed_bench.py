#!/usr/bin/env python3
"""Keyed jobs of mixed message counts (bbs_ctx_set_keyed_mixed_lengths) against the two constructions it composes.
One device, 4096 proof_verify items per list, 16-bit windows, the wire form (proof octets and raw disclosed messages in host
buffers, statuses out and checked every step), 6 lists in flight.  Writes profiles/keyed_mixed_bench.json and prints it as ONE
JSON line.

    python tools/keyed_mixed_bench.py [--steps 12] [--warmup 6] [--runs 5] [--keys 64] [--curves bls12_381,bn254]

Per curve (items/s, host-inclusive; [median, min, max] over --runs runs, the legs ALTERNATING run by run):
  a_single_mixed    a single-key context with bbs_ctx_set_mixed_lengths on, lengths uniform in 1 .. 32 (the yardstick of b, c)
  b_keyed_mixed_k1  keyed, one key, the new switch on, the same list
  c_keyed_mixed_k64 keyed, 64 keys, item i under key i mod 64, the same lengths (its own list: 64 issuers signed it)
  d_keyed_off_k64   keyed, 64 keys, every item of length 32, the new switch off (the yardstick of e)
  e_keyed_on_k64    the same list and context, the new switch on
  reg_ms            bbs_ctx_add_public_keys_octets of 4096 keys (64 distinct keys repeated) onto an empty set at L = 32, the
                    C call alone, [median, min, max] of 5 in milliseconds, the new switch off and on; the difference is the
                    cost of 4096 x 33 domain midstates on the host threads
  table_bytes       bbs_ctx_table_bytes of that context with the 4096 keys registered, the switch off and on
The workload is made untimed by one issuer at 8-bit windows whose secret key is changed issuer by issuer.
"""
import argparse
import ctypes
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


def workload(curve, lengths, K, seed):
    """Item i with lengths[i] messages, signed and proved by issuer i mod K: (pks, proof octets, raw disclosed messages,
    disclosed indexes)."""
    import random
    from bbs_sign_amd import Issuer
    from oracle import bbs
    suite = bbs.SUITES[curve]
    rng = random.Random(seed)
    n = len(lengths)
    sks = [rng.randrange(1, suite.curve.r) for _ in range(K)]
    raw = [[b"m%d.%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    disclosed = [sorted(rng.sample(range(l), l // 4)) for l in lengths]
    rnds = [[rng.randrange(1, suite.curve.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, disclosed)]
    po = [None] * n
    iss = Issuer(curve, suite.api_id, max_messages=LMAX, window_bits=8)
    for k in range(K):
        idx = list(range(k, n, K))
        iss.set_secret_key(sks[k])
        so, st = iss.sign([raw[i] for i in idx])
        assert (np.asarray(st) == 1).all()
        p, st = iss.proof_gen(so, [raw[i] for i in idx], [disclosed[i] for i in idx], [rnds[i] for i in idx])
        assert (np.asarray(st) == 1).all()
        for t, i in enumerate(idx):
            po[i] = p[t]
    iss.close()
    return [bbs.sk_to_pk(suite, sk) for sk in sks], po, [[raw[i][j] for j in d] for i, d in enumerate(disclosed)], disclosed


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


def packed(eng, fn, items, key_index=None):
    """A submit function over arguments packed ONCE: only the C call is per step."""
    po, draw, disclosed = items
    n, keep, args = eng._wire_inputs(po, draw, disclosed, None, None)

    def submit():
        j = eng._status_submit(fn, n, args, key_index)
        j.keep = keep
        return j
    return submit


def registration(curve, pks, gens, api_id):
    from bbs_sign_amd import Engine, _lib
    from oracle import bbs
    c = bbs.SUITES[curve].curve
    nk = 4096
    octs = [bbs.g2_compress(c, k) for k in pks]
    buf = np.frombuffer(b"".join(octs[k % len(octs)] for k in range(nk)), dtype=np.uint8).copy()
    st = np.zeros(nk, dtype=np.int8)
    first = ctypes.c_uint32(0)
    eng = Engine(curve, device=0, window_bits=8)
    eng.set_generators(gens, api_id)
    out = {"keys": nk, "reg_ms": {}, "table_bytes": {}}
    for name, on in (("off", False), ("on", True)):
        eng.set_public_keys([])
        eng.set_keyed_mixed_lengths(on)
        ms = []
        for _ in range(5):
            eng.set_public_keys([])
            st[:] = 0
            t0 = time.perf_counter()
            rc = eng.lib.bbs_ctx_add_public_keys_octets(eng.h, nk, buf.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p), None, None,
                                                        ctypes.byref(first))
            ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and first.value == 0 and (st == 1).all(), rc
        out["reg_ms"][name] = [round(statistics.median(ms), 2), round(min(ms), 2), round(max(ms), 2)]
        out["table_bytes"][name] = int(eng.lib.bbs_ctx_table_bytes(eng.h))
    out["reg_ms_on_minus_off"] = round(out["reg_ms"]["on"][0] - out["reg_ms"]["off"][0], 2)
    eng.close()
    return out


def one_curve(curve, a):
    import random
    from bbs_sign_amd import Engine, api
    from oracle import bbs
    suite = bbs.SUITES[curve]
    K = a.keys
    rng = random.Random(5)
    lengths = [rng.randrange(1, LMAX + 1) for _ in range(N)]
    pk1, *list1 = workload(curve, lengths, 1, 1)
    pkk, *listk = workload(curve, lengths, K, 2)
    pku, *listu = workload(curve, [LMAX] * N, K, 3)
    gens = api.create_generators(curve, LMAX + 1)
    out = {"lengths_present": len(set(lengths)), "keys": K}

    def ctx():
        e = Engine(curve, device=0, window_bits=WINDOW_BITS)
        e.set_generators(gens, suite.api_id)
        return e
    single, k1, kk, ku = ctx(), ctx(), ctx(), ctx()
    single.set_public_key(pk1[0])
    single.set_mixed_lengths(True)
    k1.set_keyed_mixed_lengths(True)
    k1.set_public_keys(pk1)
    kk.set_keyed_mixed_lengths(True)
    kk.set_public_keys(pkk)
    ku.set_public_keys(pku)
    z = np.zeros(N, dtype=np.uint32)
    kid = np.arange(N, dtype=np.uint32) % K
    fn = "bbs_proof_verify_wire_keyed_submit"
    out.update(alternating({"a_single_mixed": (None, packed(single, "bbs_proof_verify_wire_submit", list1)),
                            "b_keyed_mixed_k1": (None, packed(k1, fn, list1, z)),
                            "c_keyed_mixed_k64": (None, packed(kk, fn, listk, kid))}, a.runs, a.steps, a.warmup))
    sub_u = packed(ku, fn, listu, kid)
    out.update(alternating({"d_keyed_off_k64": (lambda: ku.set_keyed_mixed_lengths(False), sub_u),
                            "e_keyed_on_k64": (lambda: ku.set_keyed_mixed_lengths(True), sub_u)}, a.runs, a.steps, a.warmup))
    out["b_vs_a"] = round(out["b_keyed_mixed_k1"][0] / out["a_single_mixed"][0], 4)
    out["c_vs_a"] = round(out["c_keyed_mixed_k64"][0] / out["a_single_mixed"][0], 4)
    out["e_vs_d"] = round(out["e_keyed_on_k64"][0] / out["d_keyed_off_k64"][0], 4)
    for e in (single, k1, kk, ku):
        e.close()
    out["registration"] = registration(curve, pkk, gens, suite.api_id)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyed_mixed_bench.json"))
    a = ap.parse_args()
    out = {"metric": "keyed_mixed_proof_verify_items_per_s_median_min_max", "batch": N, "lengths": "uniform 1..%d" % LMAX,
           "disclosed": "a quarter", "inflight": INFLIGHT, "window_bits": WINDOW_BITS, "form": "wire", "runs": a.runs, "steps": a.steps}
    for curve in a.curves.split(","):
        out[curve] = one_curve(curve, a)
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
