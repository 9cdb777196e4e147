"""The job-local key cache (bbs_ctx_set_job_key_cache) on the GPU, both curves: KeyCachePublish behind the key stage, the
cross-stream wait of a job that hits a key another job is still building, the translated key ids in the pairing order and in
keyed batch verification, eviction, pins, generations (tests/job_key_cache_cases.py).  The expected statuses come from the keyed
twin on an engine whose key set was registered from the same octets."""
import pytest

import job_key_cache_cases as kcc

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
FOUR = tuple((op, form, True) for op in ("pv", "vf") for form in ("core", "wire"))


@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_twice(curve):
    kcc.check_five_keys_twice(curve, None, exports=FOUR)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_twice_latency_form(curve):
    kcc.check_five_keys_twice(curve, None, exports=(("pv", "core", True), ("vf", "wire", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_indexes_are_not_slots(curve):
    kcc.check_indexes_are_not_slots(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_key_uniform_wavefronts_read_slots(curve):
    kcc.check_pairing_order(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_same_key_twice_in_one_call(curve):
    kcc.check_key_twice(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_eviction(curve):
    kcc.check_eviction(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_pins_and_bypass(curve):
    kcc.check_pins_and_bypass(curve, None)


@pytest.mark.parametrize("curve,op,form", [("bls12_381", "pv", "core"), ("bn254", "vf", "wire")])
def test_hit_on_a_key_still_being_built(curve, op, form):
    """Two wavefronts of the key stage; job B is submitted while job A's keys are on their way: B's main stream waits for A's
    event on the device."""
    kcc.check_hit_while_building(curve, None, op, form)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(curve):
    kcc.check_keyed_mixed(curve, None, exports=(("pv", "core", True), ("vf", "wire", True)))


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_batch_verification(curve):
    kcc.check_keyed_bv(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_generations(curve):
    kcc.check_generations(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(curve):
    kcc.check_run_twice(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_off_and_arguments(curve):
    kcc.check_off_and_arguments(curve, None)
