"""Seeded random scalars drawn on the device (bbs_ctx_set_seeded_random_scalars, bbs_seeded_random_scalars_batch) on the GPU,
both curves, 8-bit windows: the cases of tests/seeded_cases.py -- the reference's vectors from the mock seed; the edges of the
expand_message chain through the primitive; every proof_gen export and form under per-item seeds and under a job seed, lists
of 130 items (wavefront positions 0, 63, 64, 65, 128, 129), fixed and mixed lengths, single-key and keyed, both job forms;
the order of the codes; stale pooled buffers; set-up and lifetime; the public layer."""
import pytest

import seeded_cases as sc

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


def test_export_exists():
    sc.check_export(None)


def test_reference_vectors():
    sc.check_reference_vectors(None)


@pytest.mark.parametrize("curve", CURVES)
def test_chain_edges(curve):
    sc.check_chain_edges(curve, None)


@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form(curve, mixed):
    sc.check_every_form(curve, None, n=130, mixed=mixed, python_sample=(129,))


@pytest.mark.job_form(True)
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_latency_form(curve, mixed):
    sc.check_every_form(curve, None, n=23, mixed=mixed)


@pytest.mark.parametrize("mixed", [True, False])
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_keyed(curve, mixed):
    sc.check_every_form_keyed(curve, None, n=130, mixed=mixed)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_every_form_keyed_latency_form(curve):
    sc.check_every_form_keyed(curve, None, n=23)


@pytest.mark.parametrize("curve", CURVES)
def test_order_of_codes(curve):
    sc.check_order_of_codes(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_stale_buffers(curve):
    sc.check_stale_buffers(curve, None, n=130)


@pytest.mark.parametrize("curve", CURVES)
def test_setup_and_lifetime(curve):
    sc.check_setup(curve, None)


def test_public_layer():
    sc.check_public_layer(None)
