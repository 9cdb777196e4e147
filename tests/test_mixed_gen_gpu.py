"""Mixed message counts for sign and proof_gen on one context (bbs_ctx_set_mixed_lengths_gen) on the GPU, both curves, 8-bit
windows: the cases of tests/mixed_gen_cases.py -- every length in every wavefront (core, octets and wire forms; _batch,
_upload and _submit; the latency form), stale pooled buffers, the length is the item's, prefix boundaries, the switch, the
round trip through verification, the reference's vectors on a longer context, the public layer, the issuer's octets."""
import pytest

import mixed_gen_cases as gc

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    gc.check_export(None)


@pytest.mark.parametrize("curve", CURVES)
def test_every_length(curve):
    gc.check_every_length(curve, None, n=130, python_sample=(0, 1, 3, 129))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_length_latency_form(curve):
    gc.check_every_length(curve, None, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(curve):
    gc.check_stale_buffers(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_item_length_defects(curve):
    gc.check_item_length_defects(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(curve):
    gc.check_prefix_boundaries(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_switch(curve):
    gc.check_switch(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(curve):
    gc.check_table_bytes(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(curve):
    gc.check_round_trip(curve, None)


def test_reference_vectors_on_longer_context():
    gc.check_reference_vectors_on_longer_context(None)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(curve):
    gc.check_public_layer(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_against_issuer(curve):
    gc.check_against_issuer(curve, None)
