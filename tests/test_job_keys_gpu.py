"""Verification under a job-local key set (bbs_*_with_keys_*) on the GPU, both curves: the key stage inside a job, the key gate,
the prefixes per (key, length) read by real items, keyed batch verification, two wavefronts of keys (tests/job_keys_cases.py).
The expected statuses come from the keyed twin on an engine whose key set was registered from the same octets."""
import numpy as np
import pytest

import job_keys_cases as jk
import keyed_cases as kc

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
FOUR = tuple((op, form, True) for op in ("pv", "vf") for form in ("core", "wire"))


@pytest.mark.parametrize("curve", CURVES)
def test_five_keys(curve):
    jk.check_five_keys(curve, None, -41, exports=FOUR)
    jk.check_five_keys(curve, None, -40, exports=(("pv", "wire", False), ("vf", "core", False)), oracle=False)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_latency_form(curve):
    jk.check_five_keys(curve, None, -41, exports=(("pv", "core", True), ("vf", "wire", True)), oracle=False)


@pytest.mark.parametrize("curve", CURVES)
def test_pairing_order_and_refused_uniform_wavefront(curve):
    jk.check_pairing_order(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_70_items_65_keys(curve):
    """Two wavefronts of the key stage, the second with one lane: key 64 is used by six items, key 63 is refused, key 0 is
    the identity."""
    L, R = 4, 2
    iss = kc.Issuers(curve, 64, L, None, seed=61)
    # job key k: 0 = the identity, 1 .. 62 = issuers 1 .. 62, 63 = refused, 64 = issuer 0
    key_octets = jk.octets_of(curve, [None] + iss.pks[1:63]) + [jk.refused_octets(curve, -41)] + jk.octets_of(curve, [iss.pks[0]])
    owner = list(range(1, 63)) + [5, 7] + [0] * 6
    key_index = list(range(1, 63)) + [0, 63] + [64] * 6
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=13)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=23)
    b = jk.Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)
    ref, kst = jk.registered(iss, key_octets)
    assert kst == [1] * 63 + [-41, 1]
    eng = jk.bare(iss)
    ki = np.array(key_index, dtype=np.uint32)
    for op, form in (("pv", "core"), ("vf", "wire")):
        got = b.run(eng, op, form, ki, key_octets, submit=True, want_keys=kst)
        jk.same(got, b.run(ref, op, form, ki), (curve, op, form))
        assert got[62] == 0 and got[63] == jk.UNKNOWN_KEY and list(got[64:]) == [1, 1, 1, 1, 1, 0], list(got[60:])
        assert all(got[i] == (0 if i % 23 == 0 else 1) for i in range(62))
    ref.close()
    eng.close()


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(curve):
    jk.check_keyed_mixed(curve, None, exports=(("pv", "core", True), ("pv", "wire", False), ("vf", "core", False), ("vf", "wire", True)))


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_batch_verification(curve):
    jk.check_keyed_bv(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(curve):
    jk.check_run_twice(curve, None)
