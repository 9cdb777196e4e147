"""Operands and oracle-side expectations for the six-lane Fp12 self-test (bbs_selftest_f12_batch): no GPU code here.

An element is the oracle's: six Fp2 coefficients g0..g5 over the basis 1, w, .., w^5 (w^6 = xi), each a pair of ints.
The library takes twelve Fp values in tower order; w_to_tower / tower_to_w map between the two.  tests/test_f12_cases.py
checks these builders on the CPU, tests/test_selftest_gpu.py runs them through the device.

The last section builds the G1 point pairs of the pairing-kernel test of the same module (valid, invalid, identity slots, off
the curve) with the oracle's statuses: they are kept here because that test shares the once-per-curve caching and the
CPU-side check of its item arrangement (test_f12_cases.py) with the Fp12 cases."""
import functools
import random

from oracle.curves import CURVES

OPS = {0: "mul", 1: "frob1", 2: "frob2", 3: "frob3", 4: "inv", 5: "conj", 6: "line", 7: "final_exp", 8: "sqr",
       10: "cyclo_sqr", 11: "pow_x", 12: "is_one"}
CYCLOTOMIC_OPS = (10, 11)            # the library maps the operand into the cyclotomic subgroup first
NO_ZERO_OPS = (4, 7, 10, 11)         # the oracle inverts the operand
LIMBS = {"bls12_381": 14, "bn254": 10}            # 28-bit limbs of the internal (Montgomery) representation
Z = (0, 0)


# ------------------------------------------------------------------------------------------------ layouts and bytes
def w_to_tower(g):
    """g0..g5 -> twelve Fp in tower order c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (c0 = (g0, g2, g4), c1 = (g1, g3, g5))"""
    return [v for k in (0, 2, 4, 1, 3, 5) for v in g[k]]


def tower_to_w(t):
    f2 = [(t[2 * k], t[2 * k + 1]) for k in range(6)]
    return [f2[0], f2[3], f2[1], f2[4], f2[2], f2[5]]


def tower_bytes(c, g):
    return b"".join(int(v).to_bytes(c.fp_bytes, "little") for v in w_to_tower(g))


def tower_from_bytes(c, b):
    n = c.fp_bytes
    return tower_to_w([int.from_bytes(b[k * n:(k + 1) * n], "little") for k in range(12)])


# ------------------------------------------------------------------------------------------------ internal representation
def mont_r(c):
    return 1 << (28 * LIMBS[c.name])


def from_internal(c, v):
    """The field element whose Montgomery form is v: x = v R^-1 mod p (x R = v)."""
    return v * pow(mont_r(c), -1, c.p) % c.p


def internal_list(c):
    """Internal representations that put all-ones limb patterns and the largest admissible values into the column sums
    (the list of test_fp4_half_square); p - 1 first."""
    p, top = c.p, c.p.bit_length()
    return [p - 1, (1 << (top - 1)) - 1, (1 << (top - 2)) - 1, 0, 1, int("0fffffff" * LIMBS[c.name], 16) % p, (1 << (top - 1)) + 12345]


def n_lines(c):
    """Entries of a line table: one per doubling, one per addition of the Miller loop (BN254: two Frobenius steps more)."""
    bits = bin(abs(c.x_param) if c.name == "bls12_381" else 6 * c.x_param + 2)[3:]
    return len(bits) + bits.count("1") + (2 if c.name == "bn254" else 0)


# ------------------------------------------------------------------------------------------------ elements
def one():
    return [(1, 0)] + [Z] * 5


def zero():
    return [Z] * 6


def minus_one(c):
    return [(c.p - 1, 0)] + [Z] * 5


def monomial(coef, m):
    return [coef if k == m else Z for k in range(6)]


def rand_f2(c, rng):
    return (rng.randrange(c.p), rng.randrange(c.p))


def rand_f12(c, rng):
    return [rand_f2(c, rng) for _ in range(6)]


def cyclotomic(c, x):
    """x^((p^6 - 1)(p^2 + 1))"""
    t = c.f12_mul(c.f12_conj(x), c.f12_inv(x))
    return c.f12_mul(c.f12_frob(c.f12_frob(t)), t)


def in_cyclotomic_subgroup(c, x):
    """x^(p^4 - p^2 + 1) == 1, by Frobenius maps: x^(p^4) x == x^(p^2)"""
    f2 = c.f12_frob(c.f12_frob(x))
    f4 = c.f12_frob(c.f12_frob(f2))
    return c.f12_mul(f4, x) == f2


def families(c, seed=1):
    """name -> list of elements.  `units` starts with zero (dropped where the oracle is undefined)."""
    rng = random.Random(seed)
    p = c.p
    fam = {}
    fam["units"] = [zero(), one(), minus_one(c)]
    fam["monomials"] = [monomial(co, m) for m in range(6) for co in ((1, 0), (0, 1), (p - 1, p - 1))]
    ints = internal_list(c)
    ext = [[(from_internal(c, v), from_internal(c, v))] * 6 for v in ints if v != 0]       # all twelve coefficients alike
    for _ in range(2):                                                                       # and mixed from the list
        ext.append([(from_internal(c, rng.choice(ints)), from_internal(c, rng.choice(ints))) for _ in range(6)])
    fam["extremes"] = ext
    r = lambda: rand_f2(c, rng)
    fam["subfields"] = [
        [(rng.randrange(1, p), 0)] + [Z] * 5,                   # Fp
        [r()] + [Z] * 5,                                        # Fp2
        [r(), Z, r(), Z, r(), Z],                               # Fp6 = even powers of w
        [Z, r(), Z, r(), Z, r()],                               # w Fp6
    ]
    fam["random"] = [rand_f12(c, rng) for _ in range(6)]
    return fam


def family_items(c, op, seed=1):
    """[(family, element)] for a unary op, zero left out where the oracle is undefined."""
    out = []
    for name, elems in families(c, seed).items():
        for e in elems:
            if e == zero() and op in NO_ZERO_OPS:
                continue
            out.append((name, e))
    return out


def unary_cases(c, op):
    """[(family, x, y)] of every family for op (y is the second operand slot, unused by these ops), plus the neighbours the op
    asks for: x beside inv(x) for the inverse, x beside conj(x) and an element of order r for the cyclotomic ops."""
    items = [(f, x, zero()) for f, x in family_items(c, op)]
    rng = random.Random(100 + op)
    if op == 4:
        for _ in range(2):
            x = rand_f12(c, rng)
            items += [("inverse pair", x, zero()), ("inverse pair", c.f12_inv(x), zero())]
    if op in CYCLOTOMIC_OPS:
        for _ in range(2):
            x = rand_f12(c, rng)
            items += [("conjugate pair", x, zero()), ("conjugate pair", c.f12_conj(x), zero())]
        items.append(("order r", final_exp_expected(c, final_exp_inputs(c)[0][1]), zero()))
    return items


def mul_cases(c):
    """[(family, x, y)]: every cell of the wrap table on its own (w^i w^j), the extremes on both operands at once, each
    family against itself and against dense elements."""
    rng = random.Random(7)
    fam = families(c)
    items = [("monomials", monomial((1, 0), i), monomial((1, 0), j)) for i in range(6) for j in range(6)]
    items += [("monomials", x, rand_f12(c, rng)) for x in fam["monomials"]]
    items += [("monomials", rand_f12(c, rng), x) for x in fam["monomials"][2::3]]
    items += [("extremes", x, x) for x in fam["extremes"]]
    items += [("extremes", x, fam["extremes"][(k + 1) % len(fam["extremes"])]) for k, x in enumerate(fam["extremes"])]
    items += [("units", x, rand_f12(c, rng)) for x in fam["units"]] + [("units", rand_f12(c, rng), x) for x in fam["units"]]
    items += [("units", x, y) for x in fam["units"] for y in fam["units"]]
    items += [("subfields", x, y) for x in fam["subfields"] for y in fam["subfields"]]
    items += [("subfields", x, rand_f12(c, rng)) for x in fam["subfields"]]
    items += [("random", x, rand_f12(c, rng)) for x in fam["random"]]
    return items


def line_points(c, count, seed=9):
    """(x, y) pairs for the line multiplication: random G1 points and arbitrary field pairs of extreme internal representation
    (the operation does not need a curve point)."""
    rng = random.Random(seed)
    ints = [v for v in internal_list(c)]
    pts = [c.g1_mul(c.g1, rng.randrange(1, c.r)) for _ in range(3)]
    pts += [(from_internal(c, c.p - 1), from_internal(c, c.p - 1))]
    pts += [(from_internal(c, a), from_internal(c, b)) for a, b in zip(ints[1:], ints[2:] + ints[:1])]
    return [pts[k % len(pts)] for k in range(count)]


def line_cases(c):
    """[(family, x, y)]: every family as the accumulator; the point sits in the first two values of the second operand."""
    items = family_items(c, 6)
    pts = line_points(c, len(items))
    return [(f, x, [(P[0], P[1])] + [Z] * 5) for (f, x), P in zip(items, pts)]


def final_exp_inputs(c):
    """[(family, x)], twelve per curve: the oracle needs ~0.3 s per item on BLS12-381.  Elements of proper subfields, -1 and
    c w^m must come out exactly one, with every intermediate value of the hard part equal to one."""
    rng = random.Random(21)
    fam = families(c)
    xs = [("random", rand_f12(c, rng)) for _ in range(4)]
    xs += [("units", one()), ("units", minus_one(c))]
    xs += [("subfields", fam["subfields"][2]), ("subfields", fam["subfields"][1]), ("subfields", fam["subfields"][3])]
    xs += [("monomials", monomial((1, 0), 1)), ("monomials", monomial((0, 1), 3))]
    xs += [("extremes", fam["extremes"][0])]
    return xs


@functools.lru_cache(maxsize=None)
def _final_exp(curve, xt):
    c = CURVES[curve]
    r = c.final_exp(list(xt))
    if curve == "bls12_381":                           # the library raises to 3 (p^12 - 1) / r there
        r = c.f12_pow(r, 3)
    return tuple(tuple(v) for v in r)


def final_exp_expected(c, x):
    """The library's final exponentiation of x by the oracle, computed once per element."""
    return list(_final_exp(c.name, tuple(tuple(v) for v in x)))


def cases(c, op):
    """[(family, x, y)] of one op"""
    if op == 0:
        return mul_cases(c)
    if op == 6:
        return line_cases(c)
    if op == 7:
        return [(f, x, zero()) for f, x in final_exp_inputs(c)]
    if op == 12:
        items = [("one" if flag else "single coefficient", x, zero()) for _, x, flag in is_one_cases(c)]
        return items + [(f, x, zero()) for f, x in family_items(c, 12) if x != one()]
    return unary_cases(c, op)


def expected(c, op, x, y):
    """The oracle's value of op (not the line multiplication: its entries are in the library's internal scaling)."""
    if op in CYCLOTOMIC_OPS:
        x = cyclotomic(c, x)
    if op == 0:
        r = c.f12_mul(x, y)
    elif op in (1, 2, 3):
        r = x
        for _ in range(op):
            r = c.f12_frob(r)
    elif op == 4:
        r = c.f12_inv(x)
    elif op == 5:
        r = c.f12_conj(x)
    elif op == 7:
        r = final_exp_expected(c, x)
    elif op in (8, 10):
        r = c.f12_sqr(x)
    elif op == 11:                                    # x^(curve parameter), the sign by conjugation (x unitary)
        r = c.f12_pow(x, abs(c.x_param))
        if c.x_param < 0:
            r = c.f12_conj(r)
    elif op == 12:
        r = x
    else:
        raise ValueError(op)
    return [tuple(v) for v in r]


def is_one_cases(c):
    """[(what, x, expected flag)]: one, and every way of differing from one in a SINGLE one of the twelve Fp coefficients:
    1 where 0 belongs, p - 1, and internal representations that differ from the right one in the lowest / the highest limb
    only."""
    p = c.p
    m1 = mont_r(c) % p                                 # the internal representation of 1
    items = [("one", one(), 1)]
    t1 = w_to_tower(one())
    for k in range(12):
        right = m1 if k == 0 else 0
        variants = [("p - 1", p - 1)]
        if k:
            variants.append(("1 for 0", 1))
        top = 28 * (LIMBS[c.name] - 1)
        low = right ^ 1                                                      # bit 0 of limb 0
        limb = right >> top                                                  # limb N - 1: its lowest set bit cleared, or bit 0 set
        high = right ^ (((limb & -limb) or 1) << top)
        assert low < p and high < p and 0 < (low ^ right) < (1 << 28) and (high ^ right) % (1 << top) == 0 and high != right
        variants += [("lowest limb", from_internal(c, low)), ("highest limb", from_internal(c, high))]
        for what, v in variants:
            t = list(t1)
            assert v != t[k]
            t[k] = v
            items.append(("coefficient %d: %s" % (k, what), tower_to_w(t), 0))
    return items


def position_pool(c, op, count=23):
    """count operands (family, x, y) for the group-position tests: the families interleaved, a different operand in every
    group of a wavefront."""
    byfam = {}
    for f, x, y in cases(c, op):
        byfam.setdefault(f, []).append((f, x, y))
    src = []
    while len(src) < count and any(byfam.values()):
        for f in byfam:
            if byfam[f] and len(src) < count:
                item = byfam[f].pop(0)
                if all(item[1:] != other[1:] for other in src):          # (w^0 is one: families overlap)
                    src.append(item)
    pool = [src[i % len(src)] for i in range(count)]
    for w in range(0, count, 10):
        ops = [(x, y) for _, x, y in pool[w:w + 10]]
        assert all(ops[a] != ops[b] for a in range(len(ops)) for b in range(a)), (op, w)
    return pool


def active_masks(n):
    """name -> n flags: all, only the last group of each wavefront, alternating, none"""
    return {"all": [1] * n, "last group": [1 if (i % 10 == 9 or i == n - 1) else 0 for i in range(n)],
            "alternating": [i & 1 for i in range(n)], "none": [0] * n}


# ------------------------------------------------------------------------------------------------ pairing items
PAIR_KINDS = ("valid", "Pa identity", "off curve", "invalid", "Pb identity", "both identity")


PAIR_SK = 0x1234567


@functools.lru_cache(maxsize=None)
def pairing_pk(curve):
    return CURVES[curve].g2_mul(CURVES[curve].g2, PAIR_SK)


@functools.lru_cache(maxsize=None)
def pairing_pool(curve):
    """kind -> [(Pa, Pb, expected status)] for e(Pa, pk) e(Pb, BP2) == 1 with pk = sk BP2; the statuses of live items from the
    oracle (about 0.35 s each), -41 for a point that is not on the curve."""
    c = CURVES[curve]
    rng = random.Random(55)
    pk, sk = pairing_pk(curve), PAIR_SK
    G = lambda k: c.g1_mul(c.g1, k % c.r)
    pool = {k: [] for k in PAIR_KINDS}
    for _ in range(2):
        a = rng.randrange(1, c.r)
        pool["valid"].append((G(a), c.g1_neg(G(a * sk))))
    a = rng.randrange(1, c.r)
    pool["invalid"] += [(G(a), G(a * sk)), (G(a), c.g1_neg(G(a * sk + 1)))]
    pool["Pa identity"].append((None, G(rng.randrange(1, c.r))))
    pool["Pb identity"].append((G(rng.randrange(1, c.r)), None))
    pool["both identity"].append((None, None))
    x, y = G(rng.randrange(1, c.r))
    good = G(rng.randrange(1, c.r))
    pool["off curve"] += [((x, (y + 1) % c.p), good), (good, (x, (y + 1) % c.p))]
    out = {}
    for kind, items in pool.items():
        out[kind] = []
        for Pa, Pb in items:
            if kind == "off curve":
                assert not (c.g1_is_on_curve(Pa) and c.g1_is_on_curve(Pb))
                st = -41
            else:
                st = int(c.pairing_product_is_one([(Pa, pk), (Pb, c.g2)]))
            out[kind].append((Pa, Pb, st))
    return pk, out


def pairing_kinds(n, rot):
    """Kind of item i = PAIR_KINDS[(i + rot) % 6]: gated (off curve), skipping (identity slots) and full items sit side by
    side, and rot = 0..5 brings every kind to every position."""
    return [PAIR_KINDS[(i + rot) % len(PAIR_KINDS)] for i in range(n)]


def pairing_batch(curve, n, rot):
    """pk and n items (kind, Pa, Pb, expected status)"""
    pk, pool = pairing_pool(curve)
    items = []
    for i, kind in enumerate(pairing_kinds(n, rot)):
        Pa, Pb, st = pool[kind][(i // len(PAIR_KINDS)) % len(pool[kind])]
        items.append((kind, Pa, Pb, st))
    return pk, items
