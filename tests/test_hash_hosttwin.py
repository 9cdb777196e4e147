"""Header, ph, message and api_id bytes at every SHA-256 alignment, on the TEST-ONLY host twin: the cover sets of
tests/hash_cases.py (the smallest case lists that visit every branch its path model knows at each site), and the proof
that they are cover sets.  The full sweeps are tests/test_hash_gpu.py (-m gpu)."""
import os
import sys

import pytest

import hash_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.mark.parametrize("curve", CURVES)
def test_model_cover(curve):
    """No library involved: the case lists of both tiers against the path model."""
    hc.check_model_cover(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_sign_domain(twin, curve):
    hc.check_sign_domain(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_proof_domain(twin, curve):
    hc.check_proof_domain(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_challenge(twin, curve):
    hc.check_challenge(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_wire_messages(twin, curve):
    hc.check_wire_messages(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_scalar(twin, curve):
    hc.check_hash_to_scalar(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_dst_too_long(twin, curve):
    hc.check_dst_too_long(curve, twin)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_latency_form(twin, curve):
    """The cover sets of the domain and of the challenge through the latency form of every job."""
    hc.check_sign_domain(curve, twin, every_api_len=False)
    hc.check_challenge(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_lengths(twin, curve):
    hc.check_mixed_lengths(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_two_keys(twin, curve):
    hc.check_keyed(curve, twin)
