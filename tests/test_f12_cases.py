"""The operand builders of the six-lane Fp12 self-test (tests/f12_cases.py) checked on the CPU against the oracle: the
GPU tests rely on what these cases are, so what they are is tested here where no GPU is needed."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402
from oracle.curves import CURVES          # noqa: E402

CURVE_NAMES = ["bls12_381", "bn254"]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_monomial_products_fill_the_wrap_table(curve):
    """w^i w^j = xi^[i + j >= 6] w^((i + j) mod 6): each of the 36 pairs has one recognisable non-zero coefficient"""
    c = CURVES[curve]
    for i in range(6):
        for j in range(6):
            want = fc.monomial(c.xi if i + j >= 6 else (1, 0), (i + j) % 6)
            assert c.f12_mul(fc.monomial((1, 0), i), fc.monomial((1, 0), j)) == want, (i, j)
    pairs = [(x, y) for f, x, y in fc.mul_cases(c)[:36]]
    assert pairs == [(fc.monomial((1, 0), i), fc.monomial((1, 0), j)) for i in range(6) for j in range(6)]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_subfield_elements_have_final_exponentiation_one(curve):
    """An element of Fp6 (even coefficients only), -1 and w are killed by the easy part: the device must return exactly one
    for them.  The final_exp inputs hold such elements."""
    c = CURVES[curve]
    fam = fc.families(c)
    inputs = [x for _, x in fc.final_exp_inputs(c)]
    for x in (fam["subfields"][2], fc.minus_one(c), fc.monomial((1, 0), 1)):
        assert x in inputs
        assert fc.final_exp_expected(c, x) == fc.one()
    assert len(inputs) <= 12 and fc.zero() not in inputs
    assert fc.final_exp_expected(c, inputs[0]) != fc.one()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_operands_are_canonical_and_layouts_round_trip(curve):
    c = CURVES[curve]
    seen = set()
    for op in fc.OPS:
        for f, x, y in fc.cases(c, op):
            assert len(x) == len(y) == 6
            assert all(0 <= v < c.p for g in list(x) + list(y) for v in g), (op, f)
            assert fc.tower_to_w(fc.w_to_tower(x)) == [tuple(g) for g in x]
            assert fc.tower_from_bytes(c, fc.tower_bytes(c, x)) == [tuple(g) for g in x]
            if op in fc.NO_ZERO_OPS:
                assert list(x) != fc.zero()
            seen.add(f)
    assert {"units", "monomials", "extremes", "subfields", "random", "inverse pair", "conjugate pair", "order r", "one",
            "single coefficient"} <= seen
    # tower order: c0 = (g0, g2, g4), c1 = (g1, g3, g5)
    g = [(2 * k, 2 * k + 1) for k in range(6)]
    assert fc.w_to_tower(g) == [0, 1, 4, 5, 8, 9, 2, 3, 6, 7, 10, 11]


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_internal_representation_builder(curve):
    """x = v R^-1 mod p has Montgomery form v (x R = v mod p), R = 2^(28 N); the extremes really are the all-(p - 1) element
    and the rest of the list on all twelve coefficients."""
    c = CURVES[curve]
    R = fc.mont_r(c)
    assert R == 1 << (28 * {"bls12_381": 14, "bn254": 10}[curve]) and R > c.p
    ints = fc.internal_list(c)
    assert ints[0] == c.p - 1 and all(0 <= v < c.p for v in ints)
    for v in ints:
        x = fc.from_internal(c, v)
        assert 0 <= x < c.p and x * R % c.p == v
    ext = fc.families(c)["extremes"]
    for e, v in zip(ext, [v for v in ints if v]):
        assert all(co * R % c.p == v for g in e for co in g)
    assert ("extremes", ext[0], ext[0]) in fc.mul_cases(c)          # p - 1 everywhere on both operands at once
    for P in fc.line_points(c, 10)[3:]:
        assert all(co * R % c.p in ints for co in P)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_cyclotomic_map_and_neighbours(curve):
    c = CURVES[curve]
    rng = random.Random(3)
    for x in [fc.rand_f12(c, rng), fc.minus_one(c), fc.families(c)["subfields"][3]]:
        y = fc.cyclotomic(c, x)
        assert fc.in_cyclotomic_subgroup(c, y)
        assert c.f12_mul(y, c.f12_conj(y)) == fc.one()                # unitary: the inverse is the conjugate
        assert c.f12_sqr(y) == fc.expected(c, 10, x, fc.zero())
    assert not fc.in_cyclotomic_subgroup(c, fc.rand_f12(c, rng))
    inv = [x for f, x, _ in fc.cases(c, 4) if f == "inverse pair"]
    assert len(inv) == 4 and all(c.f12_mul(inv[k], inv[k + 1]) == fc.one() for k in (0, 2))
    for op in fc.CYCLOTOMIC_OPS:
        cj = [x for f, x, _ in fc.cases(c, op) if f == "conjugate pair"]
        assert len(cj) == 4 and all(c.f12_conj(cj[k]) == cj[k + 1] for k in (0, 2))
        (gt,) = [x for f, x, _ in fc.cases(c, op) if f == "order r"]
        assert gt != fc.one() and c.f12_pow(gt, c.r) == fc.one()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_is_one_cases_differ_from_one_in_one_coefficient(curve):
    c = CURVES[curve]
    R, top = fc.mont_r(c), 28 * (fc.LIMBS[curve] - 1)
    items = fc.is_one_cases(c)
    assert [flag for _, _, flag in items].count(1) == 1 and items[0][1] == fc.one()
    t1 = fc.w_to_tower(fc.one())
    per_coeff = {k: [] for k in range(12)}
    for what, x, flag in items[1:]:
        t = fc.w_to_tower(x)
        diff = [k for k in range(12) if t[k] != t1[k]]
        assert flag == 0 and len(diff) == 1 and t[diff[0]] < c.p, what
        per_coeff[diff[0]].append((t[diff[0]] * R % c.p) ^ (t1[diff[0]] * R % c.p))     # internal representations, xor
    for k, d in per_coeff.items():
        assert len(d) == (3 if k == 0 else 4), k
        assert any(0 < v < (1 << 28) for v in d), ("lowest limb only", k)
        assert any(v and v % (1 << top) == 0 for v in d), ("highest limb only", k)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_position_pools_and_masks(curve):
    c = CURVES[curve]
    for op in fc.OPS:
        pool = fc.position_pool(c, op)
        assert len(pool) == 23
        assert len({f for f, _, _ in pool}) >= 5, op
    for n in (1, 10, 11, 23):
        m = fc.active_masks(n)
        assert all(len(v) == n for v in m.values())
        assert sum(m["all"]) == n and sum(m["none"]) == 0
        assert [i for i in range(n) if m["last group"][i]] == sorted(set(range(9, n, 10)) | {n - 1})
    assert fc.n_lines(c) == {"bls12_381": 68, "bn254": 102}[curve]          # 63 + 5 ; 64 + 36 + 2


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_pairing_batches_bring_every_kind_to_every_position(curve):
    """(no oracle pairing here: the expected statuses are computed in the GPU test)  kind of item i under rotation rot"""
    n = 23
    at = {}
    for rot in range(6):
        kinds = fc.pairing_kinds(n, rot)
        for i, k in enumerate(kinds):
            at.setdefault(k, set()).add(i)
        # a gated item (off curve) has a skipping and a full neighbour in its wavefront
        assert any(kinds[i] == "off curve" and kinds[i - 1] == "Pa identity" and kinds[i + 1] == "invalid" and (i - 1) // 10 == (i + 1) // 10
                   for i in range(1, n - 1))
    assert all(at[k] == set(range(n)) for k in fc.PAIR_KINDS)
