"""Keyed sign (bbs_ctx_set_secret_keys, bbs_core_sign_keyed_*, bbs_sign_wire_keyed_*) through the TEST-ONLY host twin, both
curves, 4-bit windows: the cases of tests/keyed_sign_cases.py at the shapes of the GPU tier, except that the long lists have 66
items instead of 130 (one full wavefront and a ragged second one; the positions 0, 63, 64 and 65 still straddle the wavefront
boundary): the twin runs every lane of every stage on one host thread."""
import os
import sys

import pytest

import keyed_sign_cases as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
N = 66


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_export_exists(twin):
    ks.check_export(twin)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length(twin, curve, mixed):
    ks.check_every_key_and_length(curve, twin, n=N, mixed=mixed, python_sample=(1, N - 4) if mixed else ())


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length_latency_form(twin, curve):
    ks.check_every_key_and_length(curve, twin, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(twin, curve):
    ks.check_round_trip(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_registration(twin, curve):
    ks.check_registration(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_overriding_codes(twin, curve):
    ks.check_overriding_codes(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_overriding_dst_too_long(twin, curve):
    ks.check_overriding_dst_too_long(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(twin, curve):
    ks.check_stale_buffers(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_and_lifetime(twin, curve):
    ks.check_setup(curve, twin)


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(twin, curve, which):
    ks.check_prefix_boundaries(curve, twin, which)


def test_reference_vector(twin):
    ks.check_reference_vector(twin)


def test_public_layer(twin):
    ks.check_public_layer(twin)
