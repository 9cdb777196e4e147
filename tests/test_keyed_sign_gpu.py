"""Keyed sign (bbs_ctx_set_secret_keys, bbs_core_sign_keyed_*, bbs_sign_wire_keyed_*) on the GPU, both curves, 8-bit windows:
the cases of tests/keyed_sign_cases.py -- every key and every length in every wavefront through the four exports in both job
forms, with keyed mixed lengths on and off; the round trip through keyed verify on the same context; registration; the codes
that override; stale pooled buffers; set-up and lifetime; prefix boundaries per key; the reference's vector; the public layer."""
import pytest

import keyed_sign_cases as ks

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    ks.check_export(None)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length(curve, mixed):
    ks.check_every_key_and_length(curve, None, n=130, mixed=mixed, python_sample=(125,) if mixed else ())


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length_latency_form(curve):
    ks.check_every_key_and_length(curve, None, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(curve):
    ks.check_round_trip(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_registration(curve):
    ks.check_registration(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_overriding_codes(curve):
    ks.check_overriding_codes(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_overriding_dst_too_long(curve):
    ks.check_overriding_dst_too_long(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(curve):
    ks.check_stale_buffers(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_and_lifetime(curve):
    ks.check_setup(curve, None)


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(curve, which):
    ks.check_prefix_boundaries(curve, None, which)


def test_reference_vector():
    ks.check_reference_vector(None)


def test_public_layer():
    ks.check_public_layer(None)
