"""proof_gen under a job-local key set (bbs_*proof_gen*_with_keys_*) through the TEST-ONLY host twin, both curves: the whole
path -- the domain-only key stage, the key gate, prefixes per (key, length), seeded draws, the job-local key cache -- against the
keyed twin on an engine whose key set was registered from the same octets (tests/job_keys_gen_cases.py)."""
import os
import sys

import pytest

import job_keys_gen_cases as jg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_exports_declared(twin):
    jg.check_exports(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_stage_alone(twin, curve):
    jg.check_stage(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_stage_alone_70_keys(twin, curve):
    jg.check_stage(curve, twin, jg.seventy_octets(curve))


@pytest.mark.parametrize("refused_code", [-40, -41])
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys(twin, curve, refused_code):
    jg.check_five_keys(curve, twin, refused_code, oracle=refused_code == -41, round_trip=refused_code == -41)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_latency_form(twin, curve):
    jg.check_five_keys(curve, twin, -41, oracle=False, round_trip=False)


@pytest.mark.parametrize("curve", CURVES)
def test_same_key_twice(twin, curve):
    jg.check_key_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_counts(twin, curve):
    jg.check_counts(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(twin, curve):
    jg.check_run_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(twin, curve):
    jg.check_keyed_mixed(curve, twin)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths_latency_form(twin, curve):
    jg.check_keyed_mixed(curve, twin, exports=(("core", True), ("wire", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_seeded(twin, curve):
    jg.check_seeded(curve, twin)


@pytest.mark.job_form(True)
def test_seeded_latency_form(twin):
    jg.check_seeded("bls12_381", twin, exports=(("wire", True), ("core", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_cache(twin, curve):
    jg.check_cache(curve, twin)


def test_arguments(twin):
    jg.check_arguments(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_api_register_keys_false(twin, curve):
    jg.check_public_layer(curve, twin)
