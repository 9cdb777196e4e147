"""tests/chain_model.py (the scalar chains of g1.hpp walked on discrete logarithms) tied to the library's host code: for the
inputs of tests/collision_cases.py that fit bbs_selftest_mul3 -- three points, the joint chain of proof_verify's T1, plain and
with the GLV split, both curves -- the entry's result equals the oracle's sum, the model predicts at least one event where the
case aims at that chain, and an ordinary input predicts none.  No GPU: bbs_selftest_mul3 is host code."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

import chain_model as cm
import collision_cases as cc
from oracle.curves import BLS12_381, BN254

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = [(0, "bls12_381"), (1, "bn254")]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def mul3(lib, c, cid, glv, pts, ks):
    fpb = c.fp_bytes

    def rec(P):
        return bytes(2 * fpb) if P is None else P[0].to_bytes(fpb, "little") + P[1].to_bytes(fpb, "little")

    pb = np.frombuffer(b"".join(rec(q) for q in pts), dtype=np.uint8).copy()
    kb = np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in ks), dtype=np.uint8).copy()
    out = np.zeros(2 * fpb, dtype=np.uint8)
    assert lib.bbs_selftest_mul3(cid, glv, _u8(pb), _u8(kb), _u8(out)) == 0
    o = out.tobytes()
    x, y = int.from_bytes(o[:fpb], "little"), int.from_bytes(o[fpb:], "little")
    return None if (x, y) == (0, 0) else (x, y)


def test_digits_sum_back():
    rng = random.Random(1)
    for bits in (256, 128, 64):
        for k in [0, 1, 2, (1 << bits) - 1, (1 << bits) - 2, 1 << (bits - 1)] + [rng.randrange(1 << bits) for _ in range(200)]:
            d = cm.odd_digits(k, bits)                   # (asserts the sum itself)
            assert len(d) == bits // 4 and all(x % 2 and -15 <= x <= 15 for x in d) and d[-1] > 0


@pytest.mark.parametrize("cid,curve", CURVES)
def test_ordinary_inputs_predict_nothing(twin, cid, curve):
    """Unrelated points: no event in any chain (an accidental collision is a 255-bit coincidence)."""
    w = cc.world(curve, twin)
    r = w.r
    rng = random.Random(7 + cid)
    for _ in range(40):
        terms = [(rng.randrange(1, r), rng.randrange(r)) for _ in range(3)]
        for glv in (False, True):
            assert cm.joint(curve, terms, glv, w.lib) == [] and cm.joint(curve, terms[:2], glv, w.lib) == []
            assert cm.comb(curve, terms[:2], glv, w.lib) == [] and cm.comb(curve, [terms[0], terms[1] + (True,)], glv, w.lib) == []
        assert cm.single(curve, *terms[0]) == [] and cm.single_glv(curve, *terms[0], w.lib) == []
    it = w.ordinary("k0", 0)
    assert not any(it.paths.values()), it.paths


@pytest.mark.parametrize("cid,curve", CURVES)
def test_single_chain_r_minus_one(twin, cid, curve):
    """The only canonical scalar in [r - 32, r) that collides in the single chain is r - 1: it cancels at the last digit and
    restarts from the identity for the even-scalar correction."""
    w = cc.world(curve, twin)
    r = w.r
    for k in range(r - 32, r):
        ev = cm.single(curve, 5, k)
        assert ev == ([(63, 0, "cancel"), (64, 0, "from_inf")] if k == r - 1 else []), (hex(k), ev)


@pytest.mark.parametrize("cid,curve", CURVES)
def test_model_against_mul3(twin, cid, curve):
    """T1's three points and scalars of every case and of ordinary items through bbs_selftest_mul3 (the product library's host
    code and the twin's), plain and GLV: the oracle's sum; the model's events where the case aims at T1's chain."""
    from bbs_sign_amd import _lib, build as b
    w = cc.world(curve, twin)
    c = w.c
    libs = [w.lib, _lib.load_library(b.build(twin=False, verbose=False))]
    aimed = 0
    for it in w.cases + [w.ordinary(k, 0) for k in cc.KEYS]:
        p = it.proof
        pts, ks = [p.b_bar, p.a_bar, p.d], [p.challenge, p.e_cap, p.r1_cap]
        want = None
        for q, k in zip(pts, ks):
            want = c.g1_add(want, c.g1_mul(q, k))
        a, g_abar, g_bbar, g_d = w.logs(it)
        for glv in (0, 1):
            ev = cm.joint(curve, list(zip((g_bbar, g_abar, g_d), ks)), bool(glv), w.lib)
            assert (ev.final is None) == (want is None)
            path = "PvT1Chain " + ("glv" if glv else "plain")
            assert ev.kinds() == it.paths[path]
            if it.aims == path:
                assert ev and it.wanted <= ev.kinds(), (it.name, ev)
                aimed += 1
            if it.name == "ordinary":
                assert ev == []
            for lib in libs:
                assert mul3(lib, c, cid, glv, pts, ks) == want, (curve, it.name, glv)
    assert aimed >= 2


@pytest.mark.parametrize("cid,curve", [(0, BLS12_381), (1, BN254)])
def test_repeated_points_take_the_fast_chain(twin, cid, curve):
    """tests/test_f2dot.py::test_joint_multiplication's (P, P, -P) with (5, 7, 12): g1_odd_table fails only for the identity and
    for points of small order, so the repeated points go down the joint chain and meet its branches there -- the model says
    which -- and the sum is the identity."""
    from bbs_sign_amd import _lib
    lib = _lib.load_library(twin)
    name = "bls12_381" if cid == 0 else "bn254"
    P = curve.g1_mul(curve.g1, 123456789)
    for glv in (False, True):
        ev = cm.joint(name, [(1, 5), (1, 7), (curve.r - 1, 12)], glv, lib)
        assert ev.final is None and ev.kinds() & {"dbl", "cancel"}, ev
        assert mul3(lib, curve, cid, int(glv), [P, P, curve.g1_neg(P)], [5, 7, 12]) is None


def test_cases_cover_every_required_cell(twin):
    """Every required cell of the issue is non-empty; the record (cases, searches, coverage per kernel path) is printed."""
    for cid, curve in CURVES:
        w = cc.world(curve, twin)
        cells = {it.cell for it in w.cases}
        assert cells == {"a", "b", "c", "d", "e"} if curve == "bls12_381" else cells == {"b", "c", "d", "e"}
        assert all(it.tries <= cc.CAP for it in w.cases)
        cov = cc.coverage(w)
        need = {"PvT1Chain glv": {"dbl", "cancel"}, "PgFinalize": {"dbl", "cancel"}, "PgVarPart comb glv": {"dbl", "cancel"},
                "PvChallenge identity T1": {"identity"}, "VfVarMul glv": {"cancel"}, "PvVarMul latency glv": {"cancel"},
                "PgVarPart split glv": {"cancel"}}
        if curve == "bls12_381":                     # (BN254 always splits: its plain forms are not on the device)
            need.update({"PvT1Chain plain": {"dbl", "cancel", "from_inf"}, "PgVarPart comb plain": {"dbl", "cancel"},
                         "VfVarMul plain": {"cancel", "from_inf"}, "PgVarPart split plain": {"cancel", "from_inf"},
                         "PvVarMul latency plain": {"cancel", "from_inf"}})
        for path, kinds in need.items():
            assert kinds <= set(cov[path]), (curve, path, cov[path])
        print("\n%s: cases built in %.1f s" % (curve, w.build_seconds))          # (the record: pytest -s shows it)
        for it in w.cases:
            print("  cell %s  key %-10s tries %4d  %-48s -> %s %s" % (it.cell, it.key, it.tries, it.name, it.aims, sorted(it.wanted)))
        for path, kinds in cov.items():
            print("  %-28s %s" % (path, kinds))
