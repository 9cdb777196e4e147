"""Keyed proof_gen (bbs_core_proof_gen_keyed_*, bbs_proof_gen_wire_keyed_*) on the GPU, both curves, 8-bit windows: the cases of
tests/keyed_gen_cases.py -- every key and every length in every wavefront through the four exports in both job forms, with
keyed mixed lengths on and off; the item's own key; stale pooled buffers; the structural codes and the key that overrides
them; set-up and lifetime; prefix boundaries; the reference's vector; the public layer."""
import pytest

import keyed_gen_cases as kg

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    kg.check_export(None)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length(curve, mixed):
    kg.check_every_key_and_length(curve, None, n=130, mixed=mixed, python_sample=(128,) if mixed else ())


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length_latency_form(curve):
    kg.check_every_key_and_length(curve, None, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_own_key(curve):
    kg.check_own_key(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(curve):
    kg.check_stale_buffers(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_structural_codes(curve):
    kg.check_structural_codes(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_and_lifetime(curve):
    kg.check_setup(curve, None)


@pytest.mark.parametrize("which", range(3))
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(curve, which):
    kg.check_prefix_boundaries(curve, None, which)


def test_reference_vector():
    kg.check_reference_vector(None)


def test_public_layer():
    kg.check_public_layer(None)
