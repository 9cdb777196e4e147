#!/usr/bin/env python3
"""Mixed message counts on the producing side: one context with bbs_ctx_set_mixed_lengths_gen against the issuer's
one-context-per-count routing, for sign and for proof_gen.  One device, 4096 items per list, lengths uniform in 1 .. 32, a
quarter of each item's messages disclosed (proof_gen), 16-bit windows, the wire forms (raw messages -- and signature octets --
in host buffers, octet strings and statuses out, statuses checked every step), 6 lists in flight.  Writes
profiles/mixed_gen_bench.json and prints it as ONE JSON line.

    python tools/mixed_gen_bench.py [--steps 12] [--warmup 6] [--runs 5] [--curves bls12_381,bn254] [--ops sign,proof_gen]

Per curve and operation (items/s, host-inclusive; [median, min, max] over --runs runs, the legs of a pair ALTERNATING run by
run):
  a_issuer        bbs_issuer_sign_submit / bbs_issuer_proof_gen_submit on the list, its 32 contexts warm (today's path)
  b_mixed         bbs_sign_wire_submit / bbs_proof_gen_wire_submit on ONE context for 32 messages with the switch on
  c_uniform_on    the same context, a list whose items all have 32 messages, the switch on
  c_uniform_off   the same context and list, the switch off (the price of the new stages on uniform input is c_on / c_off,
                  to be read against off_spread = (max - min) / median of the OFF leg in the same session)
  table_bytes     bbs_issuer_table_bytes of the warm issuer against bbs_ctx_table_bytes of the one context
  first_call_s    a cold issuer meeting the 32 lengths in its first call, against the one context's setup (generators by the
                  host, tables, key, per-length prefixes) and its first call
The signatures proof_gen starts from are made untimed by the one context itself (sign_wire_batch with the switch on).
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


class Packed:
    """The flat host buffers of one list (both libraries' entry points take the same arrays in the same order)."""

    def __init__(self, eng, op, raw, sig_octets=None, disclosed=None, rnds=None):
        from bbs_sign_amd.engine import _ragged_bytes, _u8, _u64
        n = len(raw)
        mb, mbo, mio = eng._raw_msgs(raw)
        hb, ho = _ragged_bytes([b""] * n)
        self.n, self.op, self.fpb = n, op, eng.fpb
        if op == "sign":
            self.keep = (mb, mbo, mio, hb, ho)
            self.args = (_u8(mb), _u64(mbo), _u64(mio), _u8(hb), _u64(ho))
            self.out_bytes = n * (eng.fpb + 32)
        else:
            ob, bad = eng._sig_octets(sig_octets)
            assert not bad
            di, dio = eng._indexes(disclosed)
            rs, ro = eng._scalars(rnds)
            pb, po = _ragged_bytes([b""] * n)
            self.keep = (ob, mb, mbo, mio, di, dio, rs, ro, hb, ho, pb, po)
            self.args = (_u8(ob), _u8(mb), _u64(mbo), _u64(mio), _u64(di), _u64(dio), _u8(rs), _u64(ro), _u8(hb), _u64(ho), _u8(pb), _u64(po))
            self.out_bytes = sum(3 * eng.fpb + 32 * (4 + len(m)) for m in raw) + 8

    def outputs(self):
        from bbs_sign_amd import _lib
        from bbs_sign_amd.engine import _u8, _u64
        st = np.full(self.n, -128, dtype=np.int8)
        out = np.zeros(self.out_bytes, dtype=np.uint8)
        if self.op == "sign":
            return st, (out,), (_u8(out), st.ctypes.data_as(_lib.c_i8p))
        off = np.zeros(self.n + 1, dtype=np.uint64)
        return st, (out, off), (_u8(out), _u64(off), st.ctypes.data_as(_lib.c_i8p))


class Pending:
    def __init__(self, lib, wait, free, handle, st, keep):
        self.lib, self._wait, self._free, self.h, self.result, self.keep = lib, wait, free, handle, st, keep

    def wait(self):
        rc = getattr(self.lib, self._wait)(self.h)
        assert rc == 0, (self._wait, rc)

    def free(self):
        getattr(self.lib, self._free)(self.h)


def submitter(lib, handle, fn, wait, free, p):
    def submit():
        st, keep, outs = p.outputs()
        j = ctypes.c_void_p()
        rc = getattr(lib, fn)(handle, p.n, *p.args, *outs, ctypes.byref(j))
        assert rc == 0, (fn, rc)
        return Pending(lib, wait, free, j, st, (keep, p.keep))
    return submit


def batch(lib, handle, fn, p):
    st, keep, outs = p.outputs()
    rc = getattr(lib, fn)(handle, p.n, *p.args, *outs)
    assert rc == 0, (fn, rc)
    assert (st == 1).all(), np.unique(st, return_counts=True)
    return keep


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


def one_op(curve, op, a, sk, lists):
    from bbs_sign_amd import Engine, Issuer, api
    from oracle import bbs
    suite = bbs.SUITES[curve]
    i_fn = "bbs_issuer_sign" if op == "sign" else "bbs_issuer_proof_gen"
    e_fn = "bbs_sign_wire" if op == "sign" else "bbs_proof_gen_wire"
    out = {}
    # ---- (b) the one context first: setup and first call (it also makes the signatures proof_gen starts from)
    t0 = time.perf_counter()
    gens = api.create_generators(curve, LMAX + 1)
    t_gens = time.perf_counter() - t0
    eng = Engine(curve, device=0, window_bits=WINDOW_BITS)
    eng.set_generators(gens, suite.api_id)
    eng.set_secret_key(sk)
    eng.set_mixed_lengths_gen(True)
    setup = time.perf_counter() - t0
    packed = {}
    for name, (raw, disclosed, rnds) in lists.items():
        so = None
        if op == "proof_gen":
            so, st = eng.sign_wire_batch(raw)
            assert (np.asarray(st) == 1).all()
        packed[name] = Packed(eng, op, raw, so, disclosed, rnds)
    t0 = time.perf_counter()
    batch(eng.lib, eng.h, e_fn + "_batch", packed["mixed"])
    cold_ctx = setup + time.perf_counter() - t0
    # ---- (a) the issuer: cold first call, then warm
    iss = Issuer(curve, suite.api_id, max_messages=LMAX, window_bits=WINDOW_BITS)
    iss.set_secret_key(sk)
    t0 = time.perf_counter()
    batch(iss.lib, iss.h, i_fn, packed["mixed"])
    cold_issuer = time.perf_counter() - t0
    out["first_call_s"] = {"issuer_32_new_lengths": round(cold_issuer, 3), "one_context": round(cold_ctx, 3),
                           "one_context_generators_on_host": round(t_gens, 3)}
    out["table_bytes"] = {"issuer": int(iss.table_bytes()), "issuer_contexts": int(iss.context_count()),
                          "one_context": int(eng.lib.bbs_ctx_table_bytes(eng.h))}
    sub_a = submitter(iss.lib, iss.h, i_fn + "_submit", "bbs_issuer_job_wait", "bbs_issuer_job_free", packed["mixed"])
    sub_b = submitter(eng.lib, eng.h, e_fn + "_submit", "bbs_job_wait", "bbs_job_free", packed["mixed"])
    out.update(alternating({"a_issuer": (None, sub_a), "b_mixed": (None, sub_b)}, a.runs, a.steps, a.warmup))
    out["b_vs_a"] = round(out["b_mixed"][0] / out["a_issuer"][0], 4)
    iss.close()
    # ---- (c) uniform input on the same context, switch on against off
    sub_c = submitter(eng.lib, eng.h, e_fn + "_submit", "bbs_job_wait", "bbs_job_free", packed["uniform"])
    out.update(alternating({"c_uniform_on": (lambda: eng.set_mixed_lengths_gen(True), sub_c),
                            "c_uniform_off": (lambda: eng.set_mixed_lengths_gen(False), sub_c)}, a.runs, a.steps, a.warmup))
    off = out["c_uniform_off"]
    out["c_on_vs_off"] = round(out["c_uniform_on"][0] / off[0], 4)
    out["c_off_spread"] = round((off[2] - off[1]) / off[0], 4)
    eng.close()
    return out


def one_curve(curve, a):
    import random
    from oracle import bbs
    suite = bbs.SUITES[curve]
    rng = random.Random(5)
    sk = rng.randrange(1, suite.curve.r)
    lists = {}
    for name, lengths in (("mixed", [rng.randrange(1, LMAX + 1) for _ in range(N)]), ("uniform", [LMAX] * N)):
        raw = [[b"m%d.%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
        disclosed = [sorted(rng.sample(range(l), l // 4)) for l in lengths]
        rnds = [[rng.randrange(1, suite.curve.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, disclosed)]
        lists[name] = (raw, disclosed, rnds)
    return {op: one_op(curve, op, a, sk, lists) for op in a.ops.split(",")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--ops", default="sign,proof_gen")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixed_gen_bench.json"))
    a = ap.parse_args()
    out = {"metric": "mixed_gen_items_per_s_median_min_max", "batch": N, "lengths": "uniform 1..%d" % LMAX,
           "disclosed": "a quarter", "inflight": INFLIGHT, "window_bits": WINDOW_BITS, "form": "wire", "runs": a.runs, "steps": a.steps}
    for curve in a.curves.split(","):
        out[curve] = one_curve(curve, a)
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
