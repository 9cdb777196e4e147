"""Seeded random scalars drawn on the device (bbs_ctx_set_seeded_random_scalars, bbs_seeded_random_scalars_batch) through the
TEST-ONLY host twin, both curves, 4-bit windows: the cases of tests/seeded_cases.py at the shapes of the GPU tier, except that the
long lists have 66 items instead of 130 (one full wavefront and a ragged second one): the twin runs every lane of every stage
on one host thread."""
import os
import sys

import pytest

import seeded_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
N = 66


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_export_exists(twin):
    sc.check_export(twin)


def test_reference_vectors(twin):
    sc.check_reference_vectors(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_chain_edges(twin, curve):
    sc.check_chain_edges(curve, twin)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form(twin, curve, mixed):
    sc.check_every_form(curve, twin, n=N, mixed=mixed, python_sample=(1, N - 1))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_latency_form(twin, curve, mixed):
    sc.check_every_form(curve, twin, n=23, mixed=mixed)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_keyed(twin, curve, mixed):
    sc.check_every_form_keyed(curve, twin, n=N, mixed=mixed)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_keyed_latency_form(twin, curve):
    sc.check_every_form_keyed(curve, twin, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_order_of_codes(twin, curve):
    sc.check_order_of_codes(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(twin, curve):
    sc.check_stale_buffers(curve, twin, n=N)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_and_lifetime(twin, curve):
    sc.check_setup(curve, twin)


def test_public_layer(twin):
    sc.check_public_layer(twin)
