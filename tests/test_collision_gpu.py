"""Valid credentials that collide inside the scalar chains (tests/collision_cases.py) on the GPU, both curves, 8-bit windows,
n = 70 (one full wavefront and a ragged second one), L = 3.  On the device the r == q, r == -q and r == identity branches of
g1j_add_aff are divergent code inside the largest kernels; two layouts per configuration: LONE (colliding items at positions
0, 31, 63, 64 and 69, ordinary valid items everywhere else: one lane of a wavefront diverges) and UNIFORM (positions 0 .. 63 all
colliding items of mixed kinds, the second wavefront ordinary).  Every item: proof_gen's output equals the oracle's proof field
for field, proof_verify and verify give the oracle's verdict (1; 0 for the two tampered neighbours of every batch).

Configurations: throughput and latency job form; BLS12-381 vouched and not; batch verification on (the fused PvChains kernel);
one context per required key; and once through the keyed entries with every key on ONE context."""
import pytest

import collision_cases as cc

pytestmark = pytest.mark.gpu
N = 70
BLS = [("bls12_381", k) for k in ("one", "minus_one", "glv_dbl", "glv_cancel", "k0")]
BN = [("bn254", k) for k in ("glv_dbl", "glv_cancel", "k0")]


def test_required_keys():
    for curve, keys in (("bls12_381", BLS), ("bn254", BN)):
        assert keys == [(curve, k) for k in cc.keys_of(cc.world(curve, None))]


@pytest.mark.parametrize("curve,key", BLS + BN)
def test_single_key(curve, key):
    cc.check_single_key(curve, None, key, N)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve,key", BLS + BN)
def test_single_key_latency_form(curve, key):
    cc.check_single_key(curve, None, key, N)


@pytest.mark.parametrize("curve,key", BLS)
def test_single_key_vouched(curve, key):
    cc.check_single_key(curve, None, key, N, vouched=True)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve,key", BLS)
def test_single_key_vouched_latency_form(curve, key):
    cc.check_single_key(curve, None, key, N, vouched=True)


@pytest.mark.parametrize("curve,key,vouched", [(c, k, False) for c, k in BLS + BN] + [(c, k, True) for c, k in BLS])
def test_single_key_batch_verification(curve, key, vouched):
    cc.check_single_key(curve, None, key, N, vouched=vouched, bv=True)


@pytest.mark.parametrize("curve,vouched", [("bls12_381", False), ("bls12_381", True), ("bn254", False)])
def test_keyed(curve, vouched):
    cc.check_keyed(curve, None, N, vouched=vouched)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve,vouched", [("bls12_381", False), ("bls12_381", True), ("bn254", False)])
def test_keyed_latency_form(curve, vouched):
    cc.check_keyed(curve, None, N, vouched=vouched)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_keyed_batch_verification(curve):
    cc.check_keyed(curve, None, N, bv=True)
