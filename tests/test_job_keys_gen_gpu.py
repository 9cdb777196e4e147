"""proof_gen under a job-local key set (bbs_*proof_gen*_with_keys_*) on the GPU, both curves: the domain-only key stage alone
and inside a job, the key gate, the prefixes per (key, length), seeded draws, the job-local key cache
(tests/job_keys_gen_cases.py).  The expected bytes come from the keyed twin on an engine whose key set was registered from the
same octets."""
import pytest

import job_keys_gen_cases as jg

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]


def test_exports_declared():
    jg.check_exports(None)


@pytest.mark.parametrize("curve", CURVES)
def test_stage_alone(curve):
    jg.check_stage(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_stage_alone_70_keys(curve):
    """Two wavefronts of the stage: a stand-in lane (refused at 0, 63 and 64, the identity at 65) disturbs no neighbour."""
    jg.check_stage(curve, None, jg.seventy_octets(curve))


@pytest.mark.parametrize("curve", CURVES)
def test_five_keys(curve):
    jg.check_five_keys(curve, None, -41)
    jg.check_five_keys(curve, None, -40, exports=(("wire", False), ("core", True)), oracle=False, round_trip=False)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_latency_form(curve):
    jg.check_five_keys(curve, None, -41, exports=(("core", True), ("wire", True)), oracle=False, round_trip=False)


@pytest.mark.parametrize("curve", CURVES)
def test_same_key_twice_and_counts(curve):
    jg.check_key_twice(curve, None)
    jg.check_counts(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(curve):
    jg.check_run_twice(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(curve):
    jg.check_keyed_mixed(curve, None)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths_latency_form(curve):
    jg.check_keyed_mixed(curve, None, exports=(("core", True), ("wire", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_seeded(curve):
    jg.check_seeded(curve, None)


@pytest.mark.job_form(True)
def test_seeded_latency_form():
    jg.check_seeded("bn254", None, exports=(("wire", True), ("core", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_cache(curve):
    jg.check_cache(curve, None)


def test_arguments():
    jg.check_arguments(None)


@pytest.mark.parametrize("curve", CURVES)
def test_api_register_keys_false(curve):
    jg.check_public_layer(curve, None)
