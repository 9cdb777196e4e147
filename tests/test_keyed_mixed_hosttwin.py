"""Keyed jobs of mixed message counts (bbs_ctx_set_keyed_mixed_lengths) through the TEST-ONLY host twin, both curves, 4-bit
windows: the cases of tests/keyed_mixed_cases.py at the shapes of the GPU tier, except that the long lists have 66 items instead
of 130 (one full wavefront and a ragged second one; the defect positions 0, 63, 64 and 65 still straddle the wavefront
boundary; 66 of the 102 (key, length) pairs occur, the GPU tier has all of them): the twin runs every lane of every stage on
one host thread."""
import os
import sys

import pytest

import keyed_mixed_cases as kx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
N = 66
POS = (0, 63, 64, 65)


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_export_exists(twin):
    kx.check_export(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length(twin, curve):
    kx.check_every_key_and_length(curve, twin, n=N, python_sample=(1, N - 1), all_pairs=False)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_key_and_length_latency_form(twin, curve):
    kx.check_every_key_and_length(curve, twin, n=23, all_pairs=False)


@pytest.mark.parametrize("curve", CURVES)
def test_own_key_and_length(twin, curve):
    kx.check_own_key_and_length(curve, twin, n=N, positions=POS)


@pytest.mark.parametrize("curve", CURVES)
def test_structural_codes(twin, curve):
    kx.check_structural_codes(curve, twin, n=N, positions=POS, python_sample=True)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(twin, curve):
    kx.check_stale_buffers(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_order_of_setup(twin, curve):
    kx.check_order_of_setup(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_job_keeps_what_it_was_created_with(twin, curve):
    kx.check_job_keeps_what_it_was_created_with(curve, twin)


@pytest.mark.parametrize("which", range(5))
@pytest.mark.parametrize("curve", CURVES)
def test_prefix_boundaries(twin, curve, which):
    kx.check_prefix_boundaries(curve, twin, which)


@pytest.mark.parametrize("curve", CURVES)
def test_table_bytes(twin, curve):
    kx.check_table_bytes(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_public_layer(twin, curve):
    kx.check_public_layer(curve, twin)


def test_reference_vectors(twin):
    kx.check_reference_vectors(twin)
