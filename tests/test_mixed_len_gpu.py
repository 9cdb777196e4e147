"""Mixed message counts on one context (bbs_ctx_set_mixed_lengths) on the GPU, both curves, 8-bit windows: cases 1 - 8 of
tests/mixed_len_cases.py -- every length in every wavefront (core, octets and wire forms; the latency form), the length is
the item's, stale scalars in pooled buffers, prefix boundaries, the job modes, fail closed and misuse, the issuer's statuses,
the public layer."""
import pytest

import mixed_len_cases as mc

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    from bbs_sign_amd import _lib
    lib = _lib.load_library(None)
    assert "bbs_ctx_set_mixed_lengths" in _lib.SIGNATURES and hasattr(lib, "bbs_ctx_set_mixed_lengths")
    assert lib.bbs_ctx_set_mixed_lengths(None, 1) == -100        # BBS_E_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_every_length(curve):
    mc.check_every_length(curve, None, n=130)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_length_latency_form(curve):
    mc.check_every_length(curve, None, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_item_length_defects(curve):
    mc.check_item_length_defects(curve, None, n=130, wire=True)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_scalars(curve):
    mc.check_stale_scalars(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(curve):
    mc.check_prefix_boundaries(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_modes(curve):
    mc.check_modes(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_fail_closed_and_misuse(curve):
    mc.check_fail_closed_and_misuse(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(curve):
    mc.check_table_bytes(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_against_issuer(curve):
    mc.check_against_issuer(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(curve):
    mc.check_public_layer(curve, None)


def test_reference_vectors_on_longer_context():
    mc.check_reference_vectors_on_longer_context(None)
