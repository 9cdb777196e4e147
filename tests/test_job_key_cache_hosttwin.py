"""The job-local key cache (bbs_ctx_set_job_key_cache) through the TEST-ONLY host twin, both curves: lookup by the whole string,
misses prepared and published into their slots, key -> slot translation of the job's words, pins, eviction, bypass, generations
-- every status against the keyed twin on an engine registered from the same octets (tests/job_key_cache_cases.py)."""
import os
import sys

import pytest

import job_key_cache_cases as kcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def test_exports_declared(twin):
    from bbs_sign_amd import _lib
    lib = _lib.load_library(twin)
    header = open(os.path.join(ROOT, "include", "bbs_sign_amd.h")).read()
    for name in ("bbs_ctx_set_job_key_cache", "bbs_ctx_job_key_cache_report", "bbs_job_key_cache_report", "bbs_selftest_job_key_cache_entries"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and ("int %s(" % name) in header, name


@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_twice(twin, curve):
    kcc.check_five_keys_twice(curve, twin)


@pytest.mark.job_form(True)
def test_five_keys_twice_latency_form(twin):
    kcc.check_five_keys_twice("bls12_381", twin, exports=(("pv", "wire", True), ("vf", "core", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_indexes_are_not_slots(twin, curve):
    kcc.check_indexes_are_not_slots(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_key_uniform_wavefronts_read_slots(twin, curve):
    kcc.check_pairing_order(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_same_key_twice_in_one_call(twin, curve):
    kcc.check_key_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_eviction(twin, curve):
    kcc.check_eviction(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_pins_and_bypass(twin, curve):
    kcc.check_pins_and_bypass(curve, twin)


def test_hit_on_a_key_still_being_built(twin):
    kcc.check_hit_while_building("bn254", twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(twin, curve):
    kcc.check_keyed_mixed(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_batch_verification(twin, curve):
    kcc.check_keyed_bv(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_generations(twin, curve):
    kcc.check_generations(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(twin, curve):
    kcc.check_run_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_off_and_arguments(twin, curve):
    kcc.check_off_and_arguments(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_api_key_cache(twin, curve):
    kcc.check_api_key_cache(curve, twin)
