"""The uniform four-product Fp4 half-square of the BLS12-381 cyclotomic squaring (tower.hpp fp4_sqr_part) on the host,
against Python integers: the low half x0^2 + xi x1^2, the high half 2 x0 x1, and the xi form of the high half
xi * 2 x0 x1 that the high lane of the pair (g2, g5) publishes (bbs_selftest_fp4sqr, hi = 0, 1, 1 | 4).  Both the host
twin (bound assertions on) and the product library's host code; exact equality of the canonical bytes."""
import ctypes
import itertools
import os
import random
import sys

import numpy as np
import pytest

from oracle.curves import BLS12_381, BN254

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = 0                      # BBS_CURVE_BLS12_381
NL = 14                      # 28-bit limbs of Fp


@pytest.fixture(scope="module")
def libs():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import _lib, build as b
    return [_lib.load_library(b.build(twin=True, verbose=False)), _lib.load_library(b.build(twin=False, verbose=False))]


def _u8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def _f2mul(x, y, p):
    return ((x[0] * y[0] - x[1] * y[1]) % p, (x[0] * y[1] + x[1] * y[0]) % p)


def _xi(x, p):               # xi = 1 + u
    return ((x[0] - x[1]) % p, (x[0] + x[1]) % p)


def _want(form, a, b, p):
    if form == 0:
        aa, bb = _f2mul(a, a, p), _xi(_f2mul(b, b, p), p)
        return ((aa[0] + bb[0]) % p, (aa[1] + bb[1]) % p)
    t = _f2mul(a, b, p)
    t = (2 * t[0] % p, 2 * t[1] % p)
    return t if form == 1 else _xi(t, p)


def _operands():
    p = BLS12_381.p
    R = 1 << (28 * NL)
    comp = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, R % p]
    quads = set(itertools.product(comp, repeat=4))                           # every component of A and B from the set
    # the same through the INTERNAL representation (x R^-1 is passed, so the Montgomery form is x): all-ones limbs and
    # the largest canonical values inside the column sums, where the xi form's weight-8 imaginary column is tightest
    rinv = pow(R, -1, p)
    top = p.bit_length()
    inner = [x * rinv % p for x in (p - 1, (1 << (top - 1)) - 1, int("0fffffff" * NL, 16) % p)]
    quads |= set(itertools.product(inner, repeat=4))
    rng = random.Random(20381)
    rnd = [tuple(rng.randrange(p) for _ in range(4)) for _ in range(200)]
    for q in rnd[:20]:                                                       # vanishing differences: A = B, A0 = A1, B0 = B1
        quads.add((q[0], q[1], q[0], q[1]))
        quads.add((q[0], q[0], q[2], q[3]))
        quads.add((q[0], q[1], q[2], q[2]))
        quads.add((q[0], q[0], q[2], q[2]))
    return sorted(quads) + rnd


def test_uniform_half_square(libs):
    p, fpb = BLS12_381.p, BLS12_381.fp_bytes
    ops = _operands()
    expected = {form: [_want(form, (q[0], q[1]), (q[2], q[3]), p) for q in ops] for form in (0, 1, 5)}     # once, for both libraries
    bufs = [(np.frombuffer(q[0].to_bytes(fpb, "little") + q[1].to_bytes(fpb, "little"), dtype=np.uint8).copy(),
             np.frombuffer(q[2].to_bytes(fpb, "little") + q[3].to_bytes(fpb, "little"), dtype=np.uint8).copy()) for q in ops]
    out = np.zeros(2 * fpb, dtype=np.uint8)
    for lib in libs:
        for form in (0, 1, 5):
            for q, (ab, bb), want in zip(ops, bufs, expected[form]):
                assert lib.bbs_selftest_fp4sqr(CID, form, _u8(ab), _u8(bb), _u8(out)) == 0
                assert out.tobytes() == want[0].to_bytes(fpb, "little") + want[1].to_bytes(fpb, "little"), (form, [hex(x) for x in q])


def test_xi_form_is_bls_high_one_pass_only(libs):
    """Bit 4 selects the xi form of the high half of the one-pass arm on BLS12-381; every other use is an argument error."""
    fpb = BLS12_381.fp_bytes
    a = np.zeros(2 * fpb, dtype=np.uint8)
    out = np.zeros(2 * fpb, dtype=np.uint8)
    for lib in libs:
        for hi in (4, 6, 7):
            assert lib.bbs_selftest_fp4sqr(CID, hi, _u8(a), _u8(a), _u8(out)) != 0
        b = np.zeros(2 * BN254.fp_bytes, dtype=np.uint8)
        assert lib.bbs_selftest_fp4sqr(1, 5, _u8(b), _u8(b), _u8(out)) != 0
