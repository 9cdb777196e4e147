#!/usr/bin/env python3
"""Keyed verification on the headline loop's shape: BLS12-381, 4096 items per batch, 32 messages / 8 disclosed, 6 batches
in flight, host buffers, every step's statuses checked, 16-bit windows in every leg.  Prints ONE JSON line.

    python tools/keyed_bench.py [--steps 24] [--warmup 6] [--keys 64] [--skip-verify]

Legs (items/s, host-inclusive as bench.py's value):
  pv_a_single   a single-key context, the un-keyed bbs_core_proof_verify_submit (the reference leg)
  pv_b_k1       keyed, one key
  pv_c_k64      keyed, 64 keys, items contiguous by key (64 uniform-wavefront runs of 6, 4 mixed items per key)
  pv_d_k64_mix  keyed, 64 keys, item i under key i mod 64 -- the same multiset, so the same pairing order: the sort is
                what makes both layouts equal
  pv_e_mixed_only  keyed, the 64 keys registered 8 times over, 8 items per entry: fewer than 10 items per key, so EVERY
                wavefront takes the mixed body (the worst case of the pairing order)
  vf_*          the same keyed legs for core_verify (and the single-key reference)
  reg_ms        bbs_ctx_set_public_keys for 64 and 4096 keys (the 4096 are the 64 keys repeated: registration cost is per entry)
The workload is generated untimed by 64 single-key contexts at 8-bit windows (sign, proof_gen of their share).

    python tools/keyed_bench.py --reg-only [--lib PATH]

runs only the registration legs, with 1, 16, 64, 256, 1024 and 4096 keys (64 distinct keys repeated), the C call alone (the
records are packed before the clock starts), median of 5 with min and max, in milliseconds:
  set           bbs_ctx_set_public_keys of n keys; also of 4097 and 4112 keys -- the only way to add 1 or 16 keys to a
                4096-key set without bbs_ctx_add_public_keys
  add           bbs_ctx_add_public_keys of n keys onto a 4096-key set (rebuilt, untimed, before every repetition)
  add_octets    bbs_ctx_add_public_keys_octets of the same keys onto a 4096-key set
  stage         bbs_selftest_key_entries path 1 of n keys: the device stage whatever n is, with the read-back of the n entries
                (29 KB each) -- what preparing n keys costs on the device (no call of the library uses the stage yet: this leg
                against `set` is the comparison that decides whether, and from how many keys, it should)
--lib PATH times another build of the library (an older one lacks the add exports: its line has the set legs only).
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


def workload(K, seed):
    """4096 items, item i signed by issuer i * K // N (contiguous): (issuers' pks, owner, sigs, msgs, proofs, dm, disclosed)."""
    import parity_cases as pc
    from oracle import bbs
    suite = bbs.SUITES["bls12_381"]
    gens = pc.gens_for(suite, L + 1)
    sks = [bbs.key_gen(suite, bytes([seed, k % 256, k // 256] + [7] * 29), b"", b"BBS-SIG-KEYGEN-SALT-") for k in range(K)]
    owner = [i * K // N for i in range(N)]
    sigs, proofs, pks = [None] * N, [None] * N, []
    msgs = disclosed = None
    for k in range(K):
        eng = pc.make_engine("bls12_381", gens, suite.api_id, None, sk=sks[k], window_bits=8)
        if msgs is None:
            msgs, disclosed, rnds = pc.bench_items(suite, eng, N, L, R, first_item=seed * N)
        idx = [i for i in range(N) if owner[i] == k]
        s, st = eng.core_sign_batch([msgs[i] for i in idx])
        assert list(st) == [1] * len(idx)
        p, st = eng.core_proof_gen_batch(s, [msgs[i] for i in idx], [disclosed[i] for i in idx], [rnds[i] for i in idx])
        assert list(st) == [1] * len(idx)
        for t, i in enumerate(idx):
            sigs[i], proofs[i] = s[t], p[t]
        pks.append(eng.public_key())
        eng.close()
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(N)]
    return gens, suite.api_id, pks, owner, sigs, msgs, proofs, dm, disclosed


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
            assert (j.result == 1).all()
            j.free()
    run(warmup)
    t0 = time.perf_counter()
    run(steps)
    return N * steps / (time.perf_counter() - t0)


def packed(eng, fn, n, args, keep, key_index=None):
    """A submit function over arguments packed ONCE (as bench.py's serving loop): only the C call is per step."""
    def submit():
        job = eng._status_submit(fn, n, args, key_index)
        job.keep = keep
        return job
    return submit


REG_SIZES = (1, 16, 64, 256, 1024, 4096)
REG_BASE = 4096                                     # the set the add legs append to
REG_NEW_EXPORTS = ("bbs_ctx_add_public_keys", "bbs_ctx_add_public_keys_octets", "bbs_ctx_public_key_count", "bbs_selftest_key_entries",
                   "bbs_selftest_key_entry_bytes")


def reg_only(lib_path):
    """The registration legs (module docstring): one JSON line."""
    if lib_path:
        os.environ["BBS_SIGN_AMD_LIB"] = os.path.abspath(lib_path)
        os.environ["BBS_SIGN_AMD_LIB_OPTIONAL"] = ",".join(REG_NEW_EXPORTS)
    import parity_cases as pc
    from bbs_sign_amd import Engine, _lib
    from oracle import bbs
    suite = bbs.SUITES["bls12_381"]
    c = suite.curve
    gens = pc.gens_for(suite, 5)
    eng = Engine("bls12_381", device=0, window_bits=8)
    eng.set_generators(gens, suite.api_id)
    has_add = hasattr(eng.lib, "bbs_ctx_add_public_keys")
    fpb = eng.fpb
    distinct, q = [], bbs.sk_to_pk(suite, 0x1234567)
    for _ in range(64):
        distinct.append(q)
        q = c.g2_add(q, c.g2)
    recs = [b"".join(int(v).to_bytes(fpb, "little") for v in (k[0][0], k[0][1], k[1][0], k[1][1])) for k in distinct]
    octs = [bbs.g2_compress(c, k) for k in distinct]
    nmax = REG_BASE + 16
    rec_buf = np.frombuffer(b"".join(recs[k % 64] for k in range(nmax)), dtype=np.uint8).copy()
    oct_buf = np.frombuffer(b"".join(octs[k % 64] for k in range(nmax)), dtype=np.uint8).copy()
    ident = np.zeros(nmax, dtype=np.int8)
    st = np.zeros(nmax, dtype=np.int8)
    first = ctypes.c_uint32(0)
    u8, i8 = _lib.c_u8p, _lib.c_i8p

    def timed(call, n, before=None):
        ms = []
        for _ in range(5):
            if before:
                before()
            st[:] = 0
            t0 = time.perf_counter()
            rc = call(n)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and (st[:n] == 1).all(), rc
        return [round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)]

    set_n = lambda n: eng.lib.bbs_ctx_set_public_keys(eng.h, n, rec_buf.ctypes.data_as(u8), ident.ctypes.data_as(i8), st.ctypes.data_as(i8))
    add_n = lambda n: eng.lib.bbs_ctx_add_public_keys(eng.h, n, rec_buf.ctypes.data_as(u8), ident.ctypes.data_as(i8), st.ctypes.data_as(i8),
                                                      ctypes.byref(first))
    add_o = lambda n: eng.lib.bbs_ctx_add_public_keys_octets(eng.h, n, oct_buf.ctypes.data_as(u8), st.ctypes.data_as(i8), None, None,
                                                             ctypes.byref(first))

    def base_set():
        assert set_n(REG_BASE) == 0

    eb = int(eng.lib.bbs_selftest_key_entry_bytes(0)) if has_add else 0
    ent = np.zeros(max(REG_SIZES) * eb + 1, dtype=np.uint8)
    stage_n = lambda n: eng.lib.bbs_selftest_key_entries(eng.h, n, rec_buf.ctypes.data_as(u8), ident.ctypes.data_as(i8), None, 1,
                                                         ent.ctypes.data_as(u8), st.ctypes.data_as(i8), None)

    out = {"metric": "key_registration_ms_median_min_max", "curve": "bls12_381", "lib": lib_path or "product", "has_add": has_add,
           "set": {}, "add": {}, "add_octets": {}, "stage": {}}
    set_n(64)                                           # (first call: the kernel's code object, the pools)
    for n in REG_SIZES + (REG_BASE + 1, REG_BASE + 16):
        out["set"][str(n)] = timed(set_n, n)
    if has_add:
        for n in REG_SIZES:
            out["add"][str(n)] = timed(add_n, n, base_set)
            assert first.value == REG_BASE
            out["add_octets"][str(n)] = timed(add_o, n, base_set)
            out["stage"][str(n)] = timed(stage_n, n)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reg-only", action="store_true", help="only the registration legs (see the module docstring)")
    ap.add_argument("--lib", default="", help="with --reg-only: time this build of the library instead of the product library")
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--keys", type=int, default=64)
    ap.add_argument("--skip-verify", action="store_true")
    ap.add_argument("--legs", default="", help="comma-separated subset of pv_a_single, pv_b_k1, pv_d_k64_mix, ... (profiling runs)")
    a = ap.parse_args()
    if a.reg_only:
        return reg_only(a.lib)
    from bbs_sign_amd import Engine
    K = a.keys
    out = {"metric": "keyed_verify_items_per_s", "curve": "bls12_381", "batch": N, "messages": L, "disclosed": R,
           "inflight": INFLIGHT, "window_bits": 16, "keys": K}
    w1 = workload(1, 1)
    wk = workload(K, 2)
    gens, api_id = w1[0], w1[1]

    legs = set(x for x in a.legs.split(",") if x)

    def run_leg(name, make):
        if not legs or name in legs:
            out[name] = loop(make(), a.steps, a.warmup)

    def ctx(pk=None, keys=None):
        e = Engine("bls12_381", device=0, window_bits=16)
        e.set_generators(gens, api_id)
        if pk is not None:
            e.set_public_key(pk)
        if keys is not None:
            e.set_public_keys(keys)
        return e

    # ---- proof_verify
    _, _, pks1, own1, sig1, msg1, pr1, dm1, dis1 = w1
    _, _, pksk, ownk, sigk, msgk, prk, dmk, disk = wk
    single, k1, kk = ctx(pk=pks1[0]), ctx(keys=pks1), ctx(keys=pksk)
    z = np.zeros(N, dtype=np.uint32)
    kid = np.array(ownk, dtype=np.uint32)
    # interleaved: item t of the batch is item perm[t] of the workload, perm such that key(t) = t mod K
    per = N // K
    perm = [(t % K) * per + t // K for t in range(N)]
    kid_i = kid[perm]
    assert all(kid_i[t] == t % K for t in range(N))
    pvi = lambda e, P, D, X: e._pv_inputs(P, D, X, None, None)
    n, keep, args = pvi(single, pr1, dm1, dis1)
    run_leg("pv_a_single", lambda: packed(single, "bbs_core_proof_verify_submit", n, args, keep))
    n, keep, args = pvi(k1, pr1, dm1, dis1)
    run_leg("pv_b_k1", lambda: packed(k1, "bbs_core_proof_verify_keyed_submit", n, args, keep, z))
    n, keep, args = pvi(kk, prk, dmk, disk)
    run_leg("pv_c_k64", lambda: packed(kk, "bbs_core_proof_verify_keyed_submit", n, args, keep, kid))
    n, keep, args = pvi(kk, [prk[p] for p in perm], [dmk[p] for p in perm], [disk[p] for p in perm])
    run_leg("pv_d_k64_mix", lambda: packed(kk, "bbs_core_proof_verify_keyed_submit", n, args, keep, kid_i))
    # every wavefront mixed: the K keys registered 8 times over (8 * K entries), item i under copy i mod 8 of its key -- 8
    # items per entry, fewer than a wavefront's 10, so the key-uniform body never runs
    kk8 = ctx(keys=[pksk[e % K] for e in range(8 * K)])
    kid8 = np.array([ownk[i] + K * (i % 8) for i in range(N)], dtype=np.uint32)
    n, keep, args = pvi(kk8, prk, dmk, disk)
    run_leg("pv_e_mixed_only", lambda: packed(kk8, "bbs_core_proof_verify_keyed_submit", n, args, keep, kid8))
    # ---- verify
    if not a.skip_verify:
        n, keep, args = single._vf_core_args(sig1, msg1, None)
        run_leg("vf_a_single", lambda: packed(single, "bbs_core_verify_submit", n, args, keep))
        run_leg("vf_b_k1", lambda: packed(k1, "bbs_core_verify_keyed_submit", n, args, keep, z))
        n, keep, args = kk._vf_core_args(sigk, msgk, None)
        run_leg("vf_c_k64", lambda: packed(kk, "bbs_core_verify_keyed_submit", n, args, keep, kid))
        n, keep, args = kk._vf_core_args([sigk[p] for p in perm], [msgk[p] for p in perm], None)
        run_leg("vf_d_k64_mix", lambda: packed(kk, "bbs_core_verify_keyed_submit", n, args, keep, kid_i))
        n, keep, args = kk8._vf_core_args(sigk, msgk, None)
        run_leg("vf_e_mixed_only", lambda: packed(kk8, "bbs_core_verify_keyed_submit", n, args, keep, kid8))
    # ---- registration
    for nk in ((64, 4096) if not legs else ()):
        keys = [pksk[k % K] for k in range(nk)]
        t0 = time.perf_counter()
        st = kk.set_public_keys(keys)
        out["reg_ms_%d" % nk] = round((time.perf_counter() - t0) * 1e3, 2)
        assert (st == 1).all()
    for leg in ("b_k1", "c_k64", "d_k64_mix", "e_mixed_only"):
        for op in ("pv", "vf"):
            if "%s_%s" % (op, leg) in out and "%s_a_single" % op in out:
                out["%s_%s_vs_a" % (op, leg)] = round(out["%s_%s" % (op, leg)] / out["%s_a_single" % op], 4)
    for k, v in list(out.items()):
        if isinstance(v, float) and not k.endswith("_vs_a"):
            out[k] = round(v, 1)
    line = json.dumps(out)
    assert len(line) <= 4096
    print(line)


if __name__ == "__main__":
    main()
