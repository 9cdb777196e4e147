"""Keyed verification on the GPU: both pairing bodies (key-uniform wavefronts and the mixed remainder), the rule that a
keyed status equals the single-key status item by item, both job forms, batch verification switched on (it does not apply
to keyed jobs), core and wire forms (tests/keyed_cases.py)."""
import numpy as np
import pytest

import keyed_cases as kc
from oracle import bbs

pytestmark = pytest.mark.gpu

L, R = 32, 8


def _layout(K, n, interleaved, group_sizes=None):
    if group_sizes:                                   # key k gets group_sizes[k % len] items, contiguous
        owner = []
        k = 0
        while len(owner) < n:
            owner += [k % K] * group_sizes[k % len(group_sizes)]
            k += 1
        return owner[:n]
    return [i % K for i in range(n)] if interleaved else [i * K // n for i in range(n)]


def _run_case(curve, n, K, interleaved, group_sizes=None, batch_verification=False, forms=("core", "wire"), seed=11):
    iss = kc.Issuers(curve, K, L if curve == "bls12_381" else 8, None, seed=seed)
    owner = _layout(K, n, interleaved, group_sizes)
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R if curve == "bls12_381" else 3, seed=seed)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=16)
    key_index = np.array(owner, dtype=np.uint32)
    for i in range(5, n, 37):
        key_index[i] = (owner[i] + 1) % K if K > 1 else 0       # presented under another issuer's key
    if K > 1:
        key_index[3] = K + 7                                   # unknown
    eng, kst = kc.keyed_engine(iss, iss.pks, batch_verification)
    assert list(kst) == [1] * K
    out = {}
    for form in forms:
        run = kc.pv_runner(raw, disclosed, bad_proofs, msgs, headers, phs, form)
        got = run(eng, list(range(n)), key_index)
        want = kc.expected_by_single_key(iss, iss.pks, kst, key_index, run)
        assert np.array_equal(got, want), (form, np.nonzero(got != want)[0][:10])
        out["pv_" + form] = got
        run = kc.vf_runner(curve, raw, sigs, bad_msgs, headers, form)
        got = run(eng, list(range(n)), key_index)
        want = kc.expected_by_single_key(iss, iss.pks, kst, key_index, run)
        assert np.array_equal(got, want), ("verify", form, np.nonzero(got != want)[0][:10])
        out["vf_" + form] = got
    st = out["pv_" + forms[0]]
    ok = [i for i in range(n) if i % 16 and (i - 5) % 37 and i != 3]
    assert all(st[i] == 1 for i in ok)
    assert all(st[i] == 0 for i in range(16, n, 16) if key_index[i] == owner[i])
    if K > 1:
        assert st[3] == kc.UNKNOWN_KEY and all(st[i] == 0 for i in range(5, n, 37) if i % 16)
    # a sample of 64 items against the plain-C oracle with that item's key
    from oracle import c_port
    cp = c_port.port(curve)
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(n)]
    for i in sorted(set(range(0, n, max(1, n // 64))) | {3, 5, 16})[:67]:
        if i >= n or key_index[i] >= K:
            continue
        p = bad_proofs[i]
        op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
        want = cp.core_proof_verify(iss.pks[key_index[i]], op, iss.gens, headers[i], phs[i], dm[i], disclosed[i], iss.api_id)
        assert st[i] == int(want), i
    return iss, eng, key_index, (raw, msgs, disclosed, bad_proofs, headers, phs), out


@pytest.mark.parametrize("K,interleaved", [(1, False), (64, False), (64, True)])
def test_keyed_bls_4096(K, interleaved):
    _run_case("bls12_381", 4096, K, interleaved, forms=("core",) if K == 1 else ("core", "wire"))


def test_keyed_group_sizes():
    # groups of 9, 10, 11, 19, 20, 21 items: wavefronts straddle keys, both pairing bodies run
    _run_case("bls12_381", 600, 24, False, group_sizes=[9, 10, 11, 19, 20, 21])


@pytest.mark.job_form(True)
def test_keyed_latency_form_batch_verification():
    # the latency job form and batch verification switched on: neither changes a keyed status
    _run_case("bls12_381", 300, 7, True, batch_verification=True, forms=("core",))


def test_keyed_bn254():
    _run_case("bn254", 500, 12, True)


def test_keyed_set_replaced_in_flight():
    iss, eng, key_index, (raw, msgs, disclosed, proofs, headers, phs), out = _run_case("bls12_381", 400, 8, True, forms=("core",))
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(len(proofs))]
    jobs = [eng.core_proof_verify_keyed_submit(key_index, proofs, dm, disclosed, headers, phs) for _ in range(3)]
    eng.set_public_keys(iss.pks[::-1])                  # every key moves; the jobs in flight keep the old set
    for j in jobs:
        j.wait()
        assert np.array_equal(j.result, out["pv_core"])
        j.free()
