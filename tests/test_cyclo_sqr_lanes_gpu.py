"""GPU: the cyclotomic squaring of the six-lane pairing code, lane by lane, through the batched Fp12 self-test
(bbs_selftest_f12_batch: ops 10 cyclo_sqr, 11 pow_x, 7 final_exp) against the oracle's big integers, exactly.

On BLS12-381 the two lanes of an Fp4 pair (g_m, g_{m+3}) run one instruction stream with one combine, and lane 5 (the high
half of the pair (g2, g5)) publishes xi times its half because lane 1 is its only reader.  So the inputs single out each pair:
elements that are zero outside one pair (the library maps them into the cyclotomic subgroup itself for ops 10 and 11), next
to the identity, an element of order r, x beside conj(x) and seeded random ones.  (An element supported on one pair is
w^m times an element of the subfield Fp4, so its cyclotomic image is the identity: those items check that each pair's lanes
leave one alone at every position; the dense items -- random, order r, and conj(x), which negates g1, g3, g5 against x --
are the ones that put distinct values through all three pairs, the xi-carrying lane 5 included.)  n = 21: two full wavefronts and a third
with ONE live group, every group position 0..9.  BN254 keeps its two-squarings form and must give what it always gave."""
import os
import random
import sys

import numpy as np
import pytest

from bbs_sign_amd import Engine, _lib
from oracle.curves import CURVES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402

pytestmark = pytest.mark.gpu

N_ITEMS = 21
SENTINEL = 0xA5
PAIRS = ((0, 3), (1, 4), (2, 5))


@pytest.fixture(scope="module", params=["bls12_381", "bn254"])
def ctx(request):
    c = CURVES[request.param]
    eng = Engine(request.param)
    eng.set_public_key(fc.pairing_pk(request.param))
    yield c, eng
    eng.close()


def pair_supported(c, rng, m):
    """dense on the Fp4 pair (g_m, g_{m+3}), zero elsewhere"""
    return [fc.rand_f2(c, rng) if k in (m, m + 3) else fc.Z for k in range(6)]


def items_for(c, op):
    """[(what, x)], N_ITEMS of them.  For final_exp the random ones are the inputs whose oracle values tests/f12_cases.py
    already caches (the oracle needs ~0.3 s per BLS12-381 item); the order of the kinds puts a pair-supported element and
    x beside conj(x) into different wavefronts and the single live group of the third."""
    rng = random.Random(381 + op)
    order_r = fc.final_exp_expected(c, fc.final_exp_inputs(c)[0][1])
    pairs = [("pair (g%d, g%d)" % (m, m + 3), pair_supported(c, rng, m)) for m, _ in PAIRS]
    if op == 7:
        cached = fc.final_exp_inputs(c)
        rnd = [("random", x) for f, x in cached if f == "random"]
        rest = [(f, x) for f, x in cached if f != "random" and x != fc.one()]
    else:
        rnd = [("random", fc.rand_f12(c, rng)) for _ in range(4)]
        rest = [("random", fc.rand_f12(c, rng)) for _ in range(7)]
    x0 = rnd[0][1]
    items = [("identity", fc.one()), ("order r", order_r), ("x", x0), ("conj(x)", c.f12_conj(x0))] + pairs + rnd[1:] + rest
    k = 0
    while len(items) < N_ITEMS - 4:
        items.append(rnd[k % len(rnd)])
        k += 1
    # second and third wavefront: the pairs again in other group positions, conj(x) beside x the other way round
    items = items[:N_ITEMS - 4] + [("conj(x)", c.f12_conj(x0)), ("x", x0), pairs[1], pairs[2]]
    assert len(items) == N_ITEMS and items[20][0] == "pair (g2, g5)"
    return items


def run_batch(eng, c, op, xs):
    n, row = len(xs), 12 * c.fp_bytes
    a = np.frombuffer(b"".join(fc.tower_bytes(c, x) for x in xs), dtype=np.uint8).copy()
    b = np.frombuffer(fc.tower_bytes(c, fc.zero()) * n, dtype=np.uint8).copy()
    od = np.full(n * row, SENTINEL, dtype=np.uint8)
    fl = np.full(n, SENTINEL, dtype=np.uint8)
    rc = eng.lib.bbs_selftest_f12_batch(eng.h, op, n, a.ctypes.data_as(_lib.c_u8p), b.ctypes.data_as(_lib.c_u8p), None, 1, 3,
                                        None, od.ctypes.data_as(_lib.c_u8p), fl.ctypes.data_as(_lib.c_i8p))
    assert rc == 0, (c.name, fc.OPS[op], rc)
    return od.reshape(n, row), fl


@pytest.mark.parametrize("op", [10, 11, 7])
def test_cyclotomic_square_every_pair_every_position(ctx, op):
    c, eng = ctx
    items = items_for(c, op)
    od, fl = run_batch(eng, c, op, [x for _, x in items])
    for i, (what, x) in enumerate(items):
        tag = (c.name, fc.OPS[op], "item %d = wavefront %d group %d" % (i, i // 10, i % 10), what)
        want = fc.expected(c, op, x, fc.zero())
        assert od[i].tobytes() == fc.tower_bytes(c, want), tag
        assert fl[i] == 1, tag
        if op == 10 and what == "identity":
            assert want == [tuple(v) for v in fc.one()], tag


def test_pair_supported_inputs_are_what_they_claim():
    """(no GPU work) each pair-supported element is zero outside its pair and invertible, and the item list reaches every
    group position and leaves one live group in the third wavefront"""
    c = CURVES["bls12_381"]
    rng = random.Random(1)
    for m, h in PAIRS:
        x = pair_supported(c, rng, m)
        assert all((x[k] != fc.Z) == (k in (m, h)) for k in range(6))
        assert fc.in_cyclotomic_subgroup(c, fc.cyclotomic(c, x))
    assert N_ITEMS // 10 == 2 and N_ITEMS % 10 == 1
