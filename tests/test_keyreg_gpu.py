"""Key registration on the GPU: the KeyBuild kernel against the host functions entry by entry at the key counts where its
indexing can go wrong, registration of more than a thousand keys end to end, an append while jobs are in flight, and the
C++ wrapper's append-only key index (tests/keyreg_cases.py, tests/cpp/keyreg_append.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import keyed_cases as kc
import keyreg_cases as kr
from oracle import bbs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, R = 4, 2
N_MAX, BAD_AT, IDENTITY_AT = 129, 17, 63

_reference = {}


def _keys_and_host_entries(curve):
    """129 keys -- valid ones, ONE key outside the subgroup at position 17, the identity at 63 -- and their entries by the
    host functions (path 0), computed once per curve: the entry of a key does not depend on the keys around it."""
    if curve not in _reference:
        c = bbs.SUITES[curve].curve
        iss = kc.Issuers(curve, 1, L, None, seed=23)
        eng = kc.make_engine(curve, iss.gens, iss.api_id, None)
        keys, q = [], iss.pks[0]
        for k in range(N_MAX):
            keys.append(q)
            q = c.g2_add(q, c.g2)                      # sk + 1, sk + 2, ..: distinct keys of order r
        keys[BAD_AT] = kr.off_subgroup_point(curve)
        keys[IDENTITY_AT] = None
        e0, s0, _ = kr.key_entries(eng, 0, keys=keys)
        assert s0 == [kr.NOT_ON_CURVE if k == BAD_AT else 1 for k in range(N_MAX)]
        _reference[curve] = (eng, keys, e0, s0)
    return _reference[curve]


@pytest.mark.parametrize("n", [1, 64, 65, 129])
@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_kernel_entries_equal_host_entries(curve, n):
    # one partial wavefront, one exact, a spill into the next, an odd third; the refused lane and the identity lane stay
    # with their wavefront and must not disturb a neighbour: EVERY entry is compared
    eng, keys, e0, s0 = _keys_and_host_entries(curve)
    e1, s1, _ = kr.key_entries(eng, 1, keys=keys[:n])
    assert s1 == s0[:n]
    wrong = [k for k in range(n) if e1[k] != e0[k]]
    assert not wrong, (curve, n, wrong[:10])
    c = bbs.SUITES[curve].curve
    octs = [bbs.g2_compress(c, k) for k in keys[:n]]
    e2, s2, r2 = kr.key_entries(eng, 1, octets=octs)
    assert s2 == s0[:n]
    wrong = [k for k in range(n) if e2[k] != e0[k] or r2[k] != kr.record(eng.fpb, None if s0[k] != 1 else keys[k])]
    assert not wrong, (curve, n, "octets", wrong[:10])


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_kernel_refusals_and_octet_forms(curve):
    # every kind of refusal and every octet form of tests/test_keyreg_hosttwin.py, through the kernel
    eng = _keys_and_host_entries(curve)[0]
    keys, want = kr.record_cases(curve)
    e0, s0, _ = kr.key_entries(eng, 0, keys=keys)
    e1, s1, _ = kr.key_entries(eng, 1, keys=keys)
    assert s0 == s1 == want and e0 == e1
    octs, want, dec = kr.octet_cases(curve)
    e0, s0, r0 = kr.key_entries(eng, 0, octets=octs)
    e1, s1, r1 = kr.key_entries(eng, 1, octets=octs)
    assert s0 == s1 == want and e0 == e1 and r0 == r1 == [kr.record(eng.fpb, k) for k in dec]


N_KEYS, N_SET = 1030, 1000


def _end_to_end(curve):
    iss = kc.Issuers(curve, 6, L, None, seed=29)
    p = iss.pks
    cycle = [(p[0], 0), (p[1], 1), (kc.OFF_TWIST, None), (p[2], 2), (None, None), (p[3], 3), (p[4], 4), (p[5], 5)]
    keys = [cycle[k % 8][0] for k in range(N_KEYS)]
    eng = kc.make_engine(curve, iss.gens, iss.api_id, None)
    st = list(eng.set_public_keys(keys[:N_SET]))
    c = iss.suite.curve
    # (a point off the twist has no compressed form: its place is taken by an x that no point has, refused with the same status)
    off = bbs.g2_compress(c, (kr.rootless_x(curve), (0, 0)))
    octs = [off if k is kc.OFF_TWIST else bbs.g2_compress(c, k) for k in keys[N_SET:]]
    first, st2, dec = eng.add_public_keys_octets(octs)
    assert first == N_SET and eng.public_key_count() == N_KEYS
    st += list(st2)
    assert st == [1 if cycle[k % 8][0] is not kc.OFF_TWIST else -41 for k in range(N_KEYS)]
    assert dec == [None if k is kc.OFF_TWIST else k for k in keys[N_SET:]]
    # the whole set once more, on a second context, as ONE add by octets of 1030 keys: above any threshold (at most 1024) that
    # may one day send large calls to the kernel
    by_octets = kc.make_engine(curve, iss.gens, iss.api_id, None)
    first, st3, dec3 = by_octets.add_public_keys_octets([off if k is kc.OFF_TWIST else bbs.g2_compress(c, k) for k in keys])
    assert first == 0 and list(st3) == st and dec3 == [None if k is kc.OFF_TWIST else k for k in keys]
    # 40 items: the indexes around the wavefront, set / add and power-of-two boundaries, an identity entry, a refused one, one
    # past the set; the others spread over the set; every 7th item forged
    key_index = [0, 63, 64, 65, 999, 1000, 1023, 1024, 1029, 12, 10, N_KEYS] + [(i * 97 + 5) % N_KEYS for i in range(28)]
    owner = [cycle[k % 8][1] if k < N_KEYS and cycle[k % 8][1] is not None else 0 for k in key_index]
    owner[20] = (owner[20] + 1) % 6                     # an item presented under another issuer's key
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=31)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=7)
    key_index = np.array(key_index, dtype=np.uint32)
    n = len(owner)
    for form in ("core", "wire"):
        for run in (kc.pv_runner(raw, disclosed, bad_proofs, msgs, headers, phs, form), kc.vf_runner(curve, raw, sigs, bad_msgs, headers, form)):
            got = run(eng, list(range(n)), key_index)
            want = kc.expected_by_single_key(iss, keys, st, key_index, run)
            assert list(got) == list(want), (curve, form)
            assert list(run(by_octets, list(range(n)), key_index)) == list(want), (curve, form, "registered from octets")
            assert got[10] == got[11] == kc.UNKNOWN_KEY and got[0] == 0 and got[20] == 0
            assert all(got[i] == 1 for i in (1, 2, 3, 4, 5, 6, 8)), list(got)
    return iss, eng, key_index, (msgs, disclosed, bad_proofs, headers, phs)


def test_registration_end_to_end_bls12_381():
    _end_to_end("bls12_381")


def test_registration_end_to_end_bn254_and_append_in_flight():
    iss, eng, key_index, (msgs, disclosed, proofs, headers, phs) = _end_to_end("bn254")
    # three jobs submitted, then an append, then the waits: the jobs keep the set they were created with
    key_index = key_index.copy()
    key_index[11] = N_KEYS + 1                          # unknown before the append, issuer 1's key after it
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(len(proofs))]
    before = eng.core_proof_verify_keyed_batch(key_index, proofs, dm, disclosed, headers, phs)
    jobs = [eng.core_proof_verify_keyed_submit(key_index, proofs, dm, disclosed, headers, phs) for _ in range(3)]
    first, st = eng.add_public_keys([iss.pks[0], iss.pks[1]])
    assert first == N_KEYS and list(st) == [1, 1]
    for j in jobs:
        j.wait()
        assert np.array_equal(j.result, before)
        j.free()
    after = eng.core_proof_verify_keyed_batch(key_index, proofs, dm, disclosed, headers, phs)
    assert before[11] == kc.UNKNOWN_KEY and after[11] != kc.UNKNOWN_KEY
    assert np.array_equal(np.delete(after, 11), np.delete(before, 11))


def test_cpp_wrapper_appends_gpu():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    lib = b.build(twin=False, verbose=False)
    src = os.path.join(ROOT, "tests", "cpp", "keyreg_append.cpp")
    exe = os.path.join(ROOT, "bbs_sign_amd", "build", "cpp_keyreg_append")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir, libname = os.path.dirname(lib), os.path.basename(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-l:" + libname,
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
