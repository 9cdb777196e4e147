#!/usr/bin/env python3
"""Batched key generation against what a caller had before it.  Prints ONE JSON line per curve.

    python tools/keygen_bench.py [--n 4096] [--repeat 15] [--warmup 3] [--host-n 512] [--curves bls12_381,bn254] [--lib PATH]

Device legs (one synchronous C call each, the arguments packed before the clock starts; median / min / max milliseconds of
`repeat` calls behind `warmup` untimed ones, and keys per second at the median):
  kg_32         bbs_key_gen_batch of n keys: 32-byte key material, empty key info; secret keys, records and octets out
  kg_1024       the same with 1024-byte key material and 1024-byte key info (the reference bench's largest size)
  derive_32     bbs_key_gen_batch with both public-key outputs NULL: the derive stage alone, with its copies
  derive_1024   likewise at 1024 bytes
  sk_to_pk      bbs_sk_to_pk_batch of the n secret keys: the fixed-base stage alone, with its copies
Host legs (what a caller has without the batch call: bbs_key_gen, bbs_ctx_set_secret_key, bbs_ctx_get_public_key per key,
one context per thread), 32-byte key material:
  host_1        one thread, `host-n` keys
  host_16       16 threads, n keys
Every device result is compared with the host's for the keys the host legs made.  --lib PATH times another build of the
library (the other comb window: a build with -DBBS_KG_WB=4).
"""
import argparse
import concurrent.futures as cf
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DST = b"BBS-SIG-KEYGEN-SALT-"


def material(n, size, tag):
    rng = np.random.default_rng(1000 + size + tag)
    return rng.integers(0, 256, size=n * size, dtype=np.uint8)


def run(curve, a):
    from bbs_sign_amd import Engine, _lib
    u8, i8, u64 = _lib.c_u8p, _lib.c_i8p, _lib.c_u64p
    eng = Engine(curve, device=0)
    lib, fpb, n = eng.lib, eng.fpb, a.n
    dst = np.frombuffer(DST, dtype=np.uint8).copy()
    sk = np.zeros(n * 32, dtype=np.uint8)
    pk = np.zeros(n * 4 * fpb, dtype=np.uint8)
    oc = np.zeros(n * 2 * fpb, dtype=np.uint8)
    st = np.zeros(n, dtype=np.int8)
    ident = np.zeros(n, dtype=np.int8)
    p = lambda arr, t=u8: arr.ctypes.data_as(t)

    def timed(call):
        for _ in range(a.warmup):
            assert call() == 0
        ms = []
        for _ in range(a.repeat):
            st[:] = 0
            t0 = time.perf_counter()
            rc = call()                                 # (synchronous: returns behind the stream's synchronisation)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and (st == 1).all(), rc
        med = statistics.median(ms)
        return {"ms": [round(med, 3), round(min(ms), 3), round(max(ms), 3)], "keys_per_s": round(n / med * 1e3, 1)}

    out = {"metric": "key_pairs_per_s", "curve": curve, "n": n, "lib": a.lib or "product", "repeat": a.repeat}
    sk32 = None
    for size in (32, 1024):
        km = material(n, size, 1)
        ki = material(n, size, 2) if size == 1024 else np.zeros(1, dtype=np.uint8)
        kmo = np.arange(n + 1, dtype=np.uint64) * size
        kio = np.arange(n + 1, dtype=np.uint64) * (size if size == 1024 else 0)
        full = lambda: lib.bbs_key_gen_batch(eng.h, n, p(km), p(kmo, u64), p(ki), p(kio, u64), p(dst), len(DST), p(sk), p(pk), p(oc), p(st, i8))
        derive = lambda: lib.bbs_key_gen_batch(eng.h, n, p(km), p(kmo, u64), p(ki), p(kio, u64), p(dst), len(DST), p(sk), None, None, p(st, i8))
        out["kg_%d" % size] = timed(full)
        if size == 32:
            sk32, pk32, km32 = sk.copy(), pk.copy(), km
        out["derive_%d" % size] = timed(derive)
    skb = sk32.copy()
    out["sk_to_pk"] = timed(lambda: lib.bbs_sk_to_pk_batch(eng.h, n, p(skb), p(pk), p(ident, i8), p(oc), p(st, i8)))
    assert (pk == pk32).all() and not ident.any()

    # ---- the host: one context per thread; key k by bbs_key_gen, bbs_ctx_set_secret_key, bbs_ctx_get_public_key
    cid = eng.curve

    def host(keys):
        e = Engine(curve, device=0)
        s, q, inf = np.zeros(32, dtype=np.uint8), np.zeros(4 * fpb, dtype=np.uint8), ctypes.c_int(0)
        got = {}
        for k in keys:
            m = km32[32 * k:32 * (k + 1)]
            assert lib.bbs_key_gen(cid, p(m), 32, None, 0, p(dst), len(DST), p(s)) == 0
            assert lib.bbs_ctx_set_secret_key(e.h, p(s)) == 0 and lib.bbs_ctx_get_public_key(e.h, p(q), ctypes.byref(inf)) == 0
            got[k] = (s.tobytes(), q.tobytes())
        e.close()
        return got

    def check(got):
        for k, (s, q) in got.items():
            assert s == sk32[32 * k:32 * (k + 1)].tobytes() and q == pk32[4 * fpb * k:4 * fpb * (k + 1)].tobytes(), (curve, k)

    host(range(2))
    hn = min(a.host_n, n)
    t0 = time.perf_counter()
    got = host(range(hn))
    out["host_1"] = {"keys": hn, "keys_per_s": round(hn / (time.perf_counter() - t0), 1)}
    check(got)
    T = 16
    with cf.ThreadPoolExecutor(max_workers=T) as ex:
        t0 = time.perf_counter()
        parts = list(ex.map(host, [range(t, n, T) for t in range(T)]))
        out["host_16"] = {"keys": n, "keys_per_s": round(n / (time.perf_counter() - t0), 1)}
    for g in parts:
        check(g)
    out["kg_32_vs_host_16"] = round(out["kg_32"]["keys_per_s"] / out["host_16"]["keys_per_s"], 2)
    out["kg_32_vs_host_1"] = round(out["kg_32"]["keys_per_s"] / out["host_1"]["keys_per_s"], 2)
    eng.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-n", type=int, default=512)
    ap.add_argument("--curves", default="bls12_381,bn254")
    ap.add_argument("--lib", default="", help="time this build of the library instead of the product library")
    a = ap.parse_args()
    if a.lib:
        os.environ["BBS_SIGN_AMD_LIB"] = os.path.abspath(a.lib)
    for curve in a.curves.split(","):
        run(curve, a)


if __name__ == "__main__":
    main()
