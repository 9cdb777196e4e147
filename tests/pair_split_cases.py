"""Items and oracle-side expectations for the pairing self-test (bbs_selftest_pairing_split): no GPU code here.
tests/test_pair_split_hosttwin.py runs them through the one-lane stages of the host twin, tests/test_pair_split_gpu.py through
the latency-form kernels PairMillerHalf and PairFinalDist.

The relation between a Miller value of the library and the oracle's (oracle/curves.py miller_loop).  The library's line is the
oracle's _line up to a factor: in the (c, nl) form the factor of every line lies in Fp, in the unit form every line is further
divided by its c in Fp2.  Squarings, products and the conjugation keep a subfield, so

    library value / miller_loop(P, Q)  is a non-zero element of Fp2   (both forms: w-basis coefficients g1..g5 zero, g0 != 0)
                                       and of Fp in the (c, nl) form  (g0 = (a, 0)),

which the final exponentiation kills.  relation() returns which of the two holds for a value; the host-twin test asserts
what the one-lane code gives, form by form, before the GPU test relies on it."""
import functools
import random

from oracle.curves import CURVES

import f12_cases as fc

Z = (0, 0)
N_TWIN = 23
MILLER_SIZES = (1, 10, 11, 16, 23)      # one group, a full wavefront, one item into the second, the combined checks' 16, ragged
NEGATE_SIZES = (16, 23)
FINAL_SIZES = (1, 10, 16, 23)


# ------------------------------------------------------------------------------------------------ Miller values
@functools.lru_cache(maxsize=None)
def _miller(curve, P, on_pk):
    c = CURVES[curve]
    return tuple(tuple(v) for v in c.miller_loop(P, fc.pairing_pk(curve) if on_pk else c.g2))


def oracle_miller(c, P, pair):
    """miller_loop(P, pk) for pair 0, miller_loop(P, BP2) for pair 1 (P as the kernel uses it: after negate_b)"""
    return [tuple(v) for v in _miller(c.name, P, pair == 0)]


@functools.lru_cache(maxsize=None)
def _relation(curve, value, P, on_pk):
    c = CURVES[curve]
    q = c.f12_mul(list(value), c.f12_inv(list(_miller(curve, P, on_pk))))
    q = [tuple(v) for v in q]
    if q[1:] != [Z] * 5 or q[0] == Z:
        return "none"
    return "Fp" if q[0][1] == 0 else "Fp2"


def relation(c, value, P, pair):
    """'Fp', 'Fp2' (and not Fp) or 'none': where value / miller_loop(P, Q) lies.  Cached by value: an item gives the same
    bytes at every group position, so the division is paid once per (point, key, form)."""
    return _relation(c.name, tuple(tuple(v) for v in value), P, pair == 0)


def neg(c, P):
    """-P for a pair of field elements, on the curve or not (the identity is None)"""
    return None if P is None else (P[0], (-P[1]) % c.p)


def miller_batch(curve, n, rot, negate_b):
    """pk and n items (kind, Pa, Pb as passed to the library, Pb as the kernel uses it, expected status): fc.pairing_batch;
    with negate_b the library is given -Pb, so that the product, and with it the oracle's status, is the pool's."""
    c = CURVES[curve]
    pk, items = fc.pairing_batch(curve, n, rot)
    return pk, [(kind, Pa, neg(c, Pb) if negate_b else Pb, Pb, st) for kind, Pa, Pb, st in items]


def check_miller_rows(c, items, rows, unit, want_relation, tag):
    """rows[i][pair]: 12 * fp_bytes bytes of a processed item.  The oracle relation, and exactly one for an identity slot."""
    one = fc.tower_bytes(c, fc.one())
    for i, (kind, Pa, _, Pb, st) in enumerate(items):
        if st == -41 or rows[i] is None:
            continue
        for pair, P in ((0, Pa), (1, Pb)):
            t = tag + ("item %d = wavefront %d group %d" % (i, i // 10, i % 10), kind, "pair %d" % pair)
            b = bytes(rows[i][pair])
            if P is None:
                assert b == one, t + ("an identity slot gives exactly one",)
                continue
            rel = relation(c, fc.tower_from_bytes(c, b), P, pair)
            assert rel in want_relation, t + ("value / miller_loop in", rel, "expected", want_relation)


# ------------------------------------------------------------------------------------------------ the final stage on given values
FINAL_KINDS = ("inverse", "inverse times Fp6", "inverse times Fp2", "minus inverse", "inverse times order r", "random", "random 2",
               "ones", "single coefficient", "single coefficient 2", "p - 1")


@functools.lru_cache(maxsize=None)
def final_pool(curve):
    """kind -> (g0, g1, expected status): the status of every kind by the oracle, final_exp(g0 g1) == 1 (about 0.2 s each).
    A zero operand is left out: the final exponentiation inverts, no input of the library reaches it with a zero, and the
    reference does not define its result."""
    c = CURVES[curve]
    rng = random.Random(77)
    p = c.p
    r2 = lambda: fc.rand_f2(c, rng)
    x = lambda: fc.rand_f12(c, rng)
    inv = c.f12_inv
    mul = lambda a, b: [tuple(v) for v in c.f12_mul(a, b)]
    pool = {}
    a = x()
    pool["inverse"] = (a, inv(a))
    a = x()
    pool["inverse times Fp6"] = (a, mul(inv(a), [r2(), Z, r2(), Z, r2(), Z]))
    a = x()
    pool["inverse times Fp2"] = (a, mul(inv(a), [r2()] + [Z] * 5))
    a = x()
    pool["minus inverse"] = (a, mul(inv(a), fc.minus_one(c)))
    a = x()
    g = c.pairing(c.g1_mul(c.g1, rng.randrange(1, c.r)), c.g2)
    assert [tuple(v) for v in g] != fc.one() and [tuple(v) for v in c.f12_pow(g, c.r)] == fc.one()
    pool["inverse times order r"] = (a, mul(inv(a), g))
    pool["random"] = (x(), x())
    pool["random 2"] = (x(), x())
    pool["ones"] = (fc.one(), fc.one())
    a = x()
    u = fc.one()
    u[1] = (1, 0)                                        # one + w: in no proper subfield
    pool["single coefficient"] = (a, mul(inv(a), u))
    a = x()
    u = fc.one()
    u[3] = (0, p - 1)                                    # one - i w^3, in Fp4 = Fp2(w^3): killed by (p^6 - 1)(p^2 + 1)
    pool["single coefficient 2"] = (a, mul(inv(a), u))
    pool["p - 1"] = ([(p - 1, p - 1)] * 6, [(p - 1, p - 1)] * 6)
    out = {}
    for kind in FINAL_KINDS:
        g0, g1 = ([tuple(v) for v in e] for e in pool[kind])
        assert g0 != fc.zero() and g1 != fc.zero()
        prod = mul(g0, g1)
        if kind.startswith("single coefficient"):
            assert sum(a != b for a, b in zip(fc.w_to_tower(prod), fc.w_to_tower(fc.one()))) == 1
        out[kind] = (g0, g1, int([tuple(v) for v in c.final_exp(prod)] == fc.one()))
    for kind in ("inverse", "inverse times Fp6", "inverse times Fp2", "minus inverse", "ones"):
        assert out[kind][2] == 1, (curve, kind)
    assert out["inverse times order r"][2] == 0 and out["single coefficient"][2] == 0, curve
    return out


def final_batch(curve, n, rot):
    """n items (kind, g0, g1, expected status), item i of kind FINAL_KINDS[(i + rot) % 11]"""
    pool = final_pool(curve)
    return [(k,) + pool[k] for k in (FINAL_KINDS[(i + rot) % len(FINAL_KINDS)] for i in range(n))]


def final_rotations(n):
    """Rotations that bring every kind into group 0, into group 9 and (n > 20) into the ragged wavefront: all eleven where
    the batch is shorter than the list of kinds, else those that complete the three sets."""
    K = len(FINAL_KINDS)
    if n < K:
        return list(range(K))
    want = {"group 0": set(), "group 9": set(), "ragged": set()}
    chosen = []
    for rot in range(K):
        new = False
        for i in range(n):
            k = (i + rot) % K
            for name, hit in (("group 0", i % 10 == 0), ("group 9", i % 10 == 9), ("ragged", n % 10 != 0 and i // 10 == n // 10)):
                if hit and k not in want[name]:
                    want[name].add(k)
                    new = True
        if new:
            chosen.append(rot)
    return chosen


def miller_in_bytes(c, items):
    return b"".join(fc.tower_bytes(c, g0) + fc.tower_bytes(c, g1) for _, g0, g1, _ in items)
