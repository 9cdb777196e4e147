"""Mixed message counts on one context (bbs_ctx_set_mixed_lengths) through the TEST-ONLY host twin, both curves, 4-bit
windows: cases 1 - 8 of tests/mixed_len_cases.py at the shapes of the GPU tier, except that the lists of cases 1 - 3 have 66
items instead of 130 (one full wavefront and a ragged second one; the defect positions 0, 63, 64 and 65 still straddle the
wavefront boundary): the twin runs every lane of every stage on one host thread."""
import os
import sys

import pytest

import mixed_len_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
N = 66


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_export_exists(twin):
    from bbs_sign_amd import _lib
    lib = _lib.load_library(twin)
    assert "bbs_ctx_set_mixed_lengths" in _lib.SIGNATURES and hasattr(lib, "bbs_ctx_set_mixed_lengths")
    assert lib.bbs_ctx_set_mixed_lengths(None, 1) == -100        # BBS_E_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_every_length(twin, curve):
    mc.check_every_length(curve, twin, n=N, forms=("core", "wire"), python_sample=(0, 1, 3, N - 1))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_length_latency_form(twin, curve):
    mc.check_every_length(curve, twin, n=23, forms=("core", "octets"))


@pytest.mark.parametrize("curve", CURVES)
def test_item_length_defects(twin, curve):
    mc.check_item_length_defects(curve, twin, n=N, positions=(0, 63, 64, 65), python_sample=True)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_scalars(twin, curve):
    mc.check_stale_scalars(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(twin, curve):
    mc.check_prefix_boundaries(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_modes(twin, curve):
    mc.check_modes(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_fail_closed_and_misuse(twin, curve):
    mc.check_fail_closed_and_misuse(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(twin, curve):
    mc.check_table_bytes(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_against_issuer(twin, curve):
    mc.check_against_issuer(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(twin, curve):
    mc.check_public_layer(curve, twin)


def test_reference_vectors_on_longer_context(twin):
    mc.check_reference_vectors_on_longer_context(twin)
