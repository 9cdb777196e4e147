"""Mixed message counts for sign and proof_gen on one context (bbs_ctx_set_mixed_lengths_gen) through the TEST-ONLY host twin,
both curves, 4-bit windows: the cases of tests/mixed_gen_cases.py at the shapes of the GPU tier, except that the long lists
have 66 items instead of 130 (one full wavefront and a ragged second one; the defect positions 0, 63, 64 and 65 still straddle
the wavefront boundary): the twin runs every lane of every stage on one host thread."""
import os
import sys

import pytest

import mixed_gen_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
N = 66


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_export_exists(twin):
    gc.check_export(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_every_length(twin, curve):
    gc.check_every_length(curve, twin, n=N, python_sample=(0, 1, 3, N - 1))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_length_latency_form(twin, curve):
    gc.check_every_length(curve, twin, n=23, forms=("core", "octets"), hows=("batch",))


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(twin, curve):
    gc.check_stale_buffers(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_item_length_defects(twin, curve):
    gc.check_item_length_defects(curve, twin, n=N, positions=(0, 63, 64, 65))


@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(twin, curve):
    gc.check_prefix_boundaries(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_switch(twin, curve):
    gc.check_switch(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(twin, curve):
    gc.check_table_bytes(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_round_trip(twin, curve):
    gc.check_round_trip(curve, twin)


def test_reference_vectors_on_longer_context(twin):
    gc.check_reference_vectors_on_longer_context(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(twin, curve):
    gc.check_public_layer(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_against_issuer(twin, curve):
    gc.check_against_issuer(curve, twin)
