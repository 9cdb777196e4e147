"""Valid credentials that collide inside the scalar chains (tests/collision_cases.py) through the TEST-ONLY host twin, both
curves, 4-bit windows: the cases of the GPU tier at n = 23 (the colliding items at positions 0, 9 and 22 of the lone layout):
the twin runs every lane of every stage on one host thread, so it checks the branches' arithmetic, not their divergence."""
import os
import sys

import pytest

import collision_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 23
POS = (0, 9, 22)
SINGLE = [("bls12_381", k) for k in ("one", "minus_one", "glv_dbl", "glv_cancel", "k0")] + [("bn254", k) for k in ("glv_dbl", "glv_cancel", "k0")]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_required_keys(twin):
    for curve in ("bls12_381", "bn254"):
        assert [(c, k) for c, k in SINGLE if c == curve] == [(curve, k) for k in cc.keys_of(cc.world(curve, twin))]


@pytest.mark.parametrize("curve,key", SINGLE)
def test_single_key(twin, curve, key):
    cc.check_single_key(curve, twin, key, N, positions=POS)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve,key", SINGLE)
def test_single_key_latency_form(twin, curve, key):
    cc.check_single_key(curve, twin, key, N, positions=POS)


VOUCHED = ["one", "glv_dbl", "glv_cancel", "k0"]


@pytest.mark.parametrize("key", VOUCHED)
def test_single_key_vouched(twin, key):
    cc.check_single_key("bls12_381", twin, key, N, vouched=True, positions=POS)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("key", VOUCHED)
def test_single_key_vouched_latency_form(twin, key):
    cc.check_single_key("bls12_381", twin, key, N, vouched=True, positions=POS)


@pytest.mark.parametrize("curve,key,vouched", [("bls12_381", "one", False), ("bls12_381", "minus_one", False), ("bls12_381", "k0", False),
                                               ("bls12_381", "glv_dbl", True), ("bls12_381", "glv_cancel", True), ("bls12_381", "k0", True),
                                               ("bn254", "glv_dbl", False), ("bn254", "glv_cancel", False), ("bn254", "k0", False)])
def test_single_key_batch_verification(twin, curve, key, vouched):
    cc.check_single_key(curve, twin, key, N, vouched=vouched, bv=True, positions=POS)


@pytest.mark.parametrize("curve,vouched", [("bls12_381", False), ("bls12_381", True), ("bn254", False)])
def test_keyed(twin, curve, vouched):
    cc.check_keyed(curve, twin, N, vouched=vouched, positions=POS)
