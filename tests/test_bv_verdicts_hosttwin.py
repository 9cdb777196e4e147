"""The 16 combined checks of batch verification through the TEST-ONLY host twin, both curves, L = 4, R = 2
(tests/bv_verdict_cases.py).  This is where the expectations of tests/test_bv_verdicts_gpu.py are proved right before a GPU
sees them: what the verdict flags and the report are on all-valid jobs, on jobs with failures before the pairing in both job
forms, on forged items and cancelling pairs, and -- for two windows -- that the restatement of the coefficients makes exactly
one chosen window fail.  The twin shares add_batch_combination, RlcPrep / PvChallengeBv and the decision with the product; its
bucket stages are the lane functors, not the cooperative kernel (that one is the GPU tier's)."""
import functools
import os
import sys

import pytest

import bv_verdict_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L, R = 4, 2
N = 20
FORMS = [pytest.param(False, id="throughput"), pytest.param(True, id="latency", marks=pytest.mark.job_form(True))]
FORGED17 = [0, 1, 2, 4, 5, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19]          # the valid ones: 3, 8, 13


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@functools.lru_cache(maxsize=None)
def _scene(curve, twin):
    """(issuer, N valid items): made once per curve, never changed (the cases work on copies)."""
    return vc.make_batch(curve, N, L, R, twin, seed=61)


@functools.lru_cache(maxsize=None)
def _two_key_scene(curve, twin):
    """40 valid items that alternate between two issuers' keys."""
    return vc.make_two_key_batch(curve, [i % 2 for i in range(40)], L, R, twin, seed=67)


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_all_valid(twin, curve, latency):
    iss, base = _scene(curve, twin)
    on, off = vc.engines(iss)
    for n in (1, 3, 4, 5, 17):
        for op in vc.OPS:
            vc.check_all_valid(iss, vc.take(base, range(n)), on, off, op, latency, sample=[n - 1] if n in (1, 17) else ())


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_failures_before_the_pairing(twin, curve, latency):
    iss, base = _scene(curve, twin)
    on, off = vc.engines(iss)
    five = vc.take(base, range(5))
    vc.check_wrong_challenge_scalar(iss, five, on, off, latency, 1)
    vc.check_replaced_abar(iss, five, on, off, latency, 3)
    for op in vc.OPS:
        vc.check_nothing_reaches_the_pairing(iss, vc.take(base, range(3)), on, off, op, latency)


@pytest.mark.parametrize("latency", FORMS)
@pytest.mark.parametrize("curve", vc.CURVES)
def test_forged_items(twin, curve, latency):
    iss, base = _scene(curve, twin)
    on, off = vc.engines(iss)
    five = vc.take(base, range(5))
    for bad in (0, 4, 2):
        batch = five.copy().make_bad([bad])
        for op in vc.OPS:
            vc.check_rejected(iss, batch, on, off, op, {bad}, latency, sample=[bad])


@pytest.mark.parametrize("keyed", [False, True], ids=["single_key", "keyed"])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_repeats_and_cancelling_pairs(twin, curve, keyed):
    iss, base = _scene(curve, twin)
    on, off = vc.keyed_engines(iss) if keyed else vc.engines(iss)
    for op in vc.OPS:
        vc.check_all_valid(iss, vc.repeated(base, 5), on, off, op, keyed=keyed)
    seven = vc.take(base, range(7))
    pair = vc.cancelling(seven, [1], [5], src=1)
    triple = vc.cancelling(seven, [0, 2, 3], [4, 5, 6], src=2)
    for op in vc.OPS:
        vc.check_rejected(iss, pair, on, off, op, {1, 5}, keyed=keyed)
    vc.check_rejected(iss, triple, on, off, "vf", {0, 2, 3, 4, 5, 6}, keyed=keyed)


def test_restated_coefficients():
    """The restatement against itself: digits are bytes, differ between items and jobs, and the nullspace is one."""
    js0, js1 = vc.job_seed(vc.SEED, 0), vc.job_seed(vc.SEED, 1)
    assert js0 != js1 and len(js0) == 32
    assert vc.item_digits(js0, 0) != vc.item_digits(js0, 1) != vc.item_digits(js1, 1)
    r = 2 ** 31 - 1
    rows = [[(3 * i + 7 * j * j + 1) % 256 for j in range(6)] for i in range(4)]
    basis = vc.nullspace_mod(rows, 6, r)
    assert len(basis) >= 2
    for y in basis:
        assert any(y) and all(sum(a * b for a, b in zip(row, y)) % r == 0 for row in rows)


@pytest.mark.parametrize("w", [0, 15])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_exactly_one_window_fails(twin, curve, w):
    """17 forged items among 20 whose errors cancel in every window but w: verdict w alone is 0.  A restatement of the seed
    or the digits that is wrong in any byte cannot produce this."""
    iss, base = _scene(curve, twin)
    on, off = vc.engines(iss)
    vc.check_one_window(iss, base, FORGED17, w, on, off)


@pytest.mark.parametrize("w", [0, 15])
@pytest.mark.parametrize("curve", vc.CURVES)
def test_exactly_one_window_fails_keyed(twin, curve, w):
    """The keyed group form: items alternate between two keys, the 17 forged ones are key 1's (group 1)."""
    iss, base = _two_key_scene(curve, twin)
    vc.check_one_window_keyed(iss, base, list(range(1, 40, 2))[:17], w, group=1)
