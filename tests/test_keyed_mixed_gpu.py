"""Keyed jobs of mixed message counts (bbs_ctx_set_keyed_mixed_lengths) on the GPU, both curves, 8-bit windows: the cases of
tests/keyed_mixed_cases.py -- every (key, length) pair through the eight keyed exports in both job forms, the prefix is the
item's own key's and length's, the structural codes per item, stale buffers, the order of set-up, a job keeps what it was
created with, prefix boundaries, the table bytes, the public layer, the reference's vectors."""
import pytest

import keyed_mixed_cases as kx

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    kx.check_export(None)


@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length(curve):
    kx.check_every_key_and_length(curve, None, n=130, python_sample=(129,))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length_latency_form(curve):
    kx.check_every_key_and_length(curve, None, n=23, all_pairs=False)


@pytest.mark.parametrize("curve", CURVES)
def test_own_key_and_length(curve):
    kx.check_own_key_and_length(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_structural_codes(curve):
    kx.check_structural_codes(curve, None, n=130, wire=True)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(curve):
    kx.check_stale_buffers(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_order_of_setup(curve):
    kx.check_order_of_setup(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_job_keeps_what_it_was_created_with(curve):
    kx.check_job_keeps_what_it_was_created_with(curve, None)


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(curve, which):
    kx.check_prefix_boundaries(curve, None, which)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(curve):
    kx.check_table_bytes(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(curve):
    kx.check_public_layer(curve, None)


def test_reference_vectors():
    kx.check_reference_vectors(None)
