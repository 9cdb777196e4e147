"""Keyed verification through the TEST-ONLY host twin (both curves): key-set registration, the pairing order and the
per-item key lookup, UNKNOWN_KEY, and the rule that a keyed status equals the single-key status (tests/keyed_cases.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

import keyed_cases as kc
from oracle import bbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L, R = 4, 2


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


def _setup(curve, twin):
    # five registered keys: issuers 0..2, the identity, a point off the twist (refused)
    iss = kc.Issuers(curve, 3, L, twin, seed=41)
    keys = [iss.pks[0], iss.pks[1], None, iss.pks[2], kc.OFF_TWIST]
    # 24 items: owner = signing issuer; key_index = the key the item is presented under
    owner = [i % 3 for i in range(24)]
    to_key = {0: 0, 1: 1, 2: 3}
    key_index = [to_key[o] for o in owner]
    key_index[4] = 0           # a valid item of issuer 1 presented under issuer 0's key
    key_index[7] = 5           # index >= n_keys
    key_index[8] = 4           # the refused key
    key_index[9] = 2           # the identity key
    key_index[10] = 1000       # far out of range
    items = kc.make_items(iss, owner, R, seed=3)
    return iss, keys, owner, np.array(key_index, dtype=np.uint32), items


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_keyed_hosttwin(twin, curve):
    iss, keys, owner, key_index, (raw, msgs, disclosed, sigs, proofs, headers, phs) = _setup(curve, twin)
    n = len(owner)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=6)
    # one malformed item: a disclosed index out of range keeps its existing code
    bad_disclosed = [list(d) for d in disclosed]
    bad_disclosed[13] = [0, L + 3]
    eng, kst = kc.keyed_engine(iss, keys)
    assert list(kst) == [1, 1, 1, 1, -41]
    for form in ("core", "wire"):
        run = kc.pv_runner(raw, bad_disclosed, bad_proofs, msgs, headers, phs, form)
        got = run(eng, list(range(n)), key_index)
        want = kc.expected_by_single_key(iss, keys, kst, key_index, run)
        assert list(got) == list(want), (curve, form, list(got), list(want))
        assert got[7] == got[8] == got[10] == kc.UNKNOWN_KEY
        assert got[1] == 1 and got[0] == 0 and got[4] == 0, (form, list(got))
        assert got[13] < 0 and got[13] != kc.UNKNOWN_KEY
        run = kc.vf_runner(curve, raw, sigs, bad_msgs, headers, form)
        got = run(eng, list(range(n)), key_index)
        want = kc.expected_by_single_key(iss, keys, kst, key_index, run)
        assert list(got) == list(want), (curve, "verify", form, list(got), list(want))
        assert got[1] == 1 and got[0] == 0 and got[4] == 0 and got[7] == kc.UNKNOWN_KEY
    # a few items against the oracle with that item's key
    suite = iss.suite
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(n)]
    st = eng.core_proof_verify_keyed_batch(key_index, bad_proofs, dm, disclosed, headers, phs)
    for i in (1, 2, 4, 6):
        p = bad_proofs[i]
        op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
        want = bbs.core_proof_verify(suite, keys[key_index[i]], op, iss.gens, headers[i], phs[i], dm[i], disclosed[i], iss.api_id)
        assert st[i] == int(want), (curve, i)
    vst = eng.core_verify_keyed_batch(key_index, sigs, bad_msgs, headers)
    for i in (1, 3, 4, 6):
        want = bbs.core_verify(suite, keys[key_index[i]], bbs.Signature(sigs[i].a, sigs[i].e), iss.gens, headers[i],
                               bad_msgs[i], iss.api_id)
        assert vst[i] == int(want), (curve, i)


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_keyed_set_replaced_while_in_flight(twin, curve):
    iss, keys, owner, key_index, (raw, msgs, disclosed, sigs, proofs, headers, phs) = _setup(curve, twin)
    eng, kst = kc.keyed_engine(iss, keys)
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(len(owner))]
    before = eng.core_proof_verify_keyed_batch(key_index, proofs, dm, disclosed, headers, phs)
    job = eng.core_proof_verify_keyed_submit(key_index, proofs, dm, disclosed, headers, phs)
    # the new set moves every key: a job submitted under the old set keeps its results
    assert list(eng.set_public_keys(keys[::-1])) == [-41, 1, 1, 1, 1]
    job.wait()
    assert list(job.result) == list(before)
    job.free()
    after = eng.core_proof_verify_keyed_batch(key_index, proofs, dm, disclosed, headers, phs)
    assert list(after) != list(before)
    # a cleared set, or new generators, leave no key set: keyed calls refuse with BBS_E_STATE
    eng.set_public_keys([])
    with pytest.raises(Exception, match="BBS_E_STATE"):
        eng.core_proof_verify_keyed_batch(key_index, proofs, dm, disclosed, headers, phs)
    eng.set_public_keys(keys)
    eng.set_generators(iss.gens, iss.api_id)
    with pytest.raises(Exception, match="BBS_E_STATE"):
        eng.core_verify_keyed_batch(key_index, sigs, msgs, headers)


def test_keyed_arguments(twin):
    from bbs_sign_amd import Engine, _lib
    curve = "bls12_381"
    iss = kc.Issuers(curve, 1, L, twin, seed=5)
    bare = Engine(curve, lib_path=twin, window_bits=4)
    with pytest.raises(Exception, match="BBS_E_STATE"):          # no generators yet
        bare.set_public_keys([iss.pks[0]])
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    st = np.zeros(1, dtype=np.int8)
    off = np.zeros(2, dtype=np.uint64)
    sig = np.zeros(200, dtype=np.uint8)
    job = ctypes.c_void_p()
    args = (sig.ctypes.data_as(_lib.c_u8p), None, off.ctypes.data_as(_lib.c_u64p), None, off.ctypes.data_as(_lib.c_u64p),
            st.ctypes.data_as(_lib.c_i8p), ctypes.byref(job))
    assert eng.lib.bbs_core_verify_keyed_submit(eng.h, 1, None, *args) == -102        # no key set
    eng.set_public_keys([iss.pks[0]])
    assert eng.lib.bbs_core_verify_keyed_submit(eng.h, 1, None, *args) == -100        # NULL key_index with n > 0
    assert list(eng.core_verify_keyed_batch([], [], [])) == []


def test_keyed_pairing_order_hosttwin(twin):
    # 10, 11 and 9 items under three keys, interleaved in the batch: key-uniform wavefronts (keys 0 and 1) and mixed ones
    # (the remainders 0, 1 and 9 items) -- both halves of the pairing order, and the twin walks the same slot map
    curve = "bls12_381"
    iss = kc.Issuers(curve, 3, L, twin, seed=43)
    counts = [10, 11, 9]
    owner = [k for t in range(11) for k in range(3) if t < counts[k]]
    key_index = np.array(owner, dtype=np.uint32)
    key_index[12] = (owner[12] + 1) % 3                 # another issuer's key
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=5)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=7)
    eng, kst = kc.keyed_engine(iss, iss.pks)
    n = len(owner)
    run = kc.pv_runner(raw, disclosed, bad_proofs, msgs, headers, phs, "core")
    got = run(eng, list(range(n)), key_index)
    want = kc.expected_by_single_key(iss, iss.pks, kst, key_index, run)
    assert list(got) == list(want)
    assert got[12] == 0 and got[0] == 0 and sum(got == 1) == n - 1 - len(range(0, n, 7))
    run = kc.vf_runner(curve, raw, sigs, bad_msgs, headers, "core")
    got = run(eng, list(range(n)), key_index)
    assert list(got) == list(kc.expected_by_single_key(iss, iss.pks, kst, key_index, run))
