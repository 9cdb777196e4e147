"""Verification under a job-local key set (bbs_*_with_keys_*) through the TEST-ONLY host twin, both curves: the whole path --
key stage, key gate, prefixes per (key, length), pairing order, keyed batch verification -- against the keyed twin on an
engine whose key set was registered from the same octets (tests/job_keys_cases.py)."""
import os
import sys

import pytest

import job_keys_cases as jk

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
    for op in ("core_verify", "verify_wire", "core_proof_verify", "proof_verify_wire"):
        for tail in ("submit", "batch"):
            assert hasattr(lib, "bbs_%s_with_keys_%s" % (op, tail))
    assert hasattr(lib, "bbs_job_key_statuses") and hasattr(lib, "bbs_selftest_key_len_rows")


@pytest.mark.parametrize("refused_code", [-40, -41])
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys(twin, curve, refused_code):
    jk.check_five_keys(curve, twin, refused_code)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_five_keys_latency_form(twin, curve):
    jk.check_five_keys(curve, twin, -41, oracle=False)


@pytest.mark.parametrize("curve", CURVES)
def test_pairing_order_and_refused_uniform_wavefront(twin, curve):
    jk.check_pairing_order(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_same_key_twice(twin, curve):
    jk.check_key_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_counts(twin, curve):
    jk.check_counts(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_no_key_state_on_the_context(twin, curve):
    jk.check_no_key_state(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_run_twice(twin, curve):
    jk.check_run_twice(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths(twin, curve):
    jk.check_keyed_mixed(curve, twin)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_keyed_mixed_lengths_latency_form(twin, curve):
    jk.check_keyed_mixed(curve, twin, exports=(("pv", "wire", True), ("vf", "core", False)))


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_batch_verification(twin, curve):
    jk.check_keyed_bv(curve, twin)


@pytest.mark.job_form(True)
def test_keyed_batch_verification_latency_form(twin):
    jk.check_keyed_bv("bls12_381", twin)


def test_arguments(twin):
    jk.check_arguments(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_api_register_keys_false(twin, curve):
    """register_keys=False gives the entries of register_keys=True on a mixed list -- two issuers, two counts, one forged item,
    one pk the library refuses -- and leaves the cached engine's key set and index as they were."""
    from bbs_sign_amd import api
    from bbs_sign_amd.api import PublicKey, SecretKey
    import keyed_cases as kc
    sks = [SecretKey(curve, 1000 + k, twin) for k in range(2)]
    pks = [sk.sk_to_pk() for sk in sks]
    bad = PublicKey(curve, kc.OFF_TWIST, twin)
    lists = [[b"a", b"b"], [b"c", b"d", b"e"], [b"f", b"g"], [b"h", b"i", b"j"], [b"k", b"l"]]
    signed = [(sks[i % 2].sign(m, b"hdr%d" % i), b"hdr%d" % i, m) for i, m in enumerate(lists)]
    items = [(pks[i % 2],) + s for i, s in enumerate(signed)]
    items[2] = (items[2][0], items[2][1], items[2][2], [b"forged", b"g"])
    items[4] = (bad,) + items[4][1:]
    want = api.verify_many_issuers(items)
    ie = api._issuer_cache[(curve, 0, twin)]
    index, count = dict(ie.index), ie.eng.public_key_count()
    got = api.verify_many_issuers(items, register_keys=False)
    assert [repr(g) for g in got] == [repr(w) for w in want]
    assert got[0] is True and got[1] is True and got[2] is False and got[3] is True and isinstance(got[4], api.BbsError)
    assert ie.index == index and ie.eng.public_key_count() == count
    # the same through proof_verify
    proofs = []
    for i, (pk, sig, hdr, msgs) in enumerate(items[:4]):
        real = lists[i]
        proofs.append((pks[i % 2], api.proof_gen(pks[i % 2], sig, hdr, b"ph", real, [0]), hdr, b"ph", [msgs[0]], [0]))
    proofs.append((bad,) + proofs[1][1:])
    want = api.proof_verify_many_issuers(proofs)
    got = api.proof_verify_many_issuers(proofs, register_keys=False)
    assert [repr(g) for g in got] == [repr(w) for w in want]
    assert got[1] is True and got[2] is False and isinstance(got[4], api.BbsError)
    assert ie.index == index and ie.eng.public_key_count() == count
