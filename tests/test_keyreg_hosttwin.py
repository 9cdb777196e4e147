"""Key registration through the TEST-ONLY host twin (both curves): the KeyBuild stage against the host functions entry by
entry (bbs_selftest_key_entries), appending to a key set, registration from octets, the arguments, and the C++ wrapper's
append-only key index (tests/cpp/keyreg_append.cpp)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import keyed_cases as kc
import keyreg_cases as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
L, R = 4, 2


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.mark.parametrize("curve", CURVES)
def test_key_entries_stage_equals_host_functions(twin, curve):
    iss = kc.Issuers(curve, 1, L, twin, seed=3)
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    keys, want = kr.record_cases(curve)
    e0, s0, _ = kr.key_entries(eng, 0, keys=keys)
    e1, s1, _ = kr.key_entries(eng, 1, keys=keys)
    assert s0 == want and s1 == want, (s0, s1, want)
    for k in range(len(keys)):
        assert e1[k] == e0[k], (curve, "record", k)
    assert len(set(e0)) == len(set(keys)) - 2          # the three refused keys share one (empty) entry
    octs, want, dec = kr.octet_cases(curve)
    e0, s0, r0 = kr.key_entries(eng, 0, octets=octs)
    e1, s1, r1 = kr.key_entries(eng, 1, octets=octs)
    assert s0 == want and s1 == want, (s0, s1, want)
    for k in range(len(octs)):
        assert e1[k] == e0[k], (curve, "octets", k)
        assert r1[k] == r0[k] == kr.record(eng.fpb, dec[k]), (curve, "decoded record", k)
    # a key by octets and the same key by its record are one entry
    er, _, _ = kr.key_entries(eng, 1, keys=[dec[0], dec[-1]])
    assert er == [e1[0], e1[-1]]
    eng.close()


def _items(curve, twin):
    # five issuers; seven registered keys: issuers 0..2 (set), then issuer 3, a refused key, the identity, issuer 4 (added)
    iss = kc.Issuers(curve, 5, L, twin, seed=47)
    first, second = [iss.pks[0], iss.pks[1], iss.pks[2]], [iss.pks[3], kc.OFF_TWIST, None, iss.pks[4]]
    owner = [i % 5 for i in range(24)]
    to_key = {0: 0, 1: 1, 2: 2, 3: 3, 4: 6}
    key_index = [to_key[o] for o in owner]
    key_index[7] = 3            # a valid item of issuer 2 presented under issuer 3's key
    key_index[10] = 4           # the refused key
    key_index[11] = 5           # the identity key
    key_index[13] = 7           # the first index past the set
    key_index[16] = 1000
    items = kc.make_items(iss, owner, R, seed=11)
    return iss, first, second, owner, np.array(key_index, dtype=np.uint32), items


@pytest.mark.parametrize("curve", CURVES)
def test_append_keeps_indexes_and_verifies(twin, curve):
    iss, first, second, owner, key_index, (raw, msgs, disclosed, sigs, proofs, headers, phs) = _items(curve, twin)
    n = len(owner)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=6)
    eng, st3 = kc.keyed_engine(iss, first)
    assert list(st3) == [1, 1, 1] and eng.public_key_count() == 3
    # a job submitted before the append keeps the set it was created with
    dm = [[msgs[i][j] for j in disclosed[i]] for i in range(n)]
    before = eng.core_proof_verify_keyed_batch(key_index, bad_proofs, dm, disclosed, headers, phs)
    job = eng.core_proof_verify_keyed_submit(key_index, bad_proofs, dm, disclosed, headers, phs)
    first_index, st4 = eng.add_public_keys(second)
    job.wait()
    assert list(job.result) == list(before)
    job.free()
    assert sum(before == kc.UNKNOWN_KEY) > 5           # (keys 3 .. 6 were unknown then)
    assert first_index == 3 and eng.public_key_count() == 7
    whole, st7 = kc.keyed_engine(iss, first + second)
    assert list(st4) == list(st7[3:]) == [1, -41, 1, 1]
    keys = first + second
    for form in ("core", "wire"):
        for run in (kc.pv_runner(raw, disclosed, bad_proofs, msgs, headers, phs, form), kc.vf_runner(curve, raw, sigs, bad_msgs, headers, form)):
            got = run(eng, list(range(n)), key_index)
            assert list(got) == list(kc.expected_by_single_key(iss, keys, st7, key_index, run)), (curve, form)
            assert list(got) == list(run(whole, list(range(n)), key_index)), (curve, form)
            assert got[10] == got[13] == got[16] == kc.UNKNOWN_KEY
            assert got[1] == 1 and got[3] == 1 and got[4] == 1 and got[0] == 0 and got[7] == 0, list(got)
    eng.close()
    whole.close()


@pytest.mark.parametrize("curve", CURVES)
def test_registration_from_octets(twin, curve):
    iss, first, second, owner, key_index, (raw, msgs, disclosed, sigs, proofs, headers, phs) = _items(curve, twin)
    n = len(owner)
    c = iss.suite.curve
    from oracle import bbs
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    off = bbs.g2_compress(c, kr.off_subgroup_point(curve))
    stray = bytearray(bbs.g2_compress(c, None))
    stray[c.fp_bytes] |= 1
    octs = [bbs.g2_compress(c, k) for k in first] + [bbs.g2_compress(c, iss.pks[3]), off, bbs.g2_compress(c, None),
                                                      bbs.g2_compress(c, iss.pks[4]), bytes(stray)]
    first_index, st, keys = eng.add_public_keys_octets(octs)
    one = [kr.from_octets_one(eng, o) for o in octs]
    assert first_index == 0 and eng.public_key_count() == len(octs)
    assert list(st) == [o[0] for o in one] == [1, 1, 1, 1, -41, 1, 1, -40]
    assert keys == first + [iss.pks[3], None, None, iss.pks[4], None]
    # the same keys by their decoded records (a refused key keeps its place)
    rec_eng, rst = kc.keyed_engine(iss, [k if s == 1 else kc.OFF_TWIST for k, s in zip(keys, st)])
    assert [int(x == 1) for x in rst] == [int(x == 1) for x in st]
    for run in (kc.pv_runner(raw, disclosed, proofs, msgs, headers, phs, "core"), kc.vf_runner(curve, raw, sigs, msgs, headers, "wire")):
        got = run(eng, list(range(n)), key_index)
        assert list(got) == list(run(rec_eng, list(range(n)), key_index))
        assert got[0] == 1 and got[4] == 1 and got[7] == 0 and got[10] == kc.UNKNOWN_KEY
    # the public interface: accepted keys as octets_to_public_key gives them, a refused key raises its code
    from bbs_sign_amd import api
    good = [octs[0], octs[5], octs[3]]
    first_index, pks = api.register_public_keys(curve, good, L=2, lib_path=twin)
    assert [p.pk for p in pks] == [api.octets_to_public_key(curve, o, lib_path=twin).pk for o in good]
    assert api.register_public_keys(curve, good[:1], L=2, lib_path=twin)[0] == first_index + 3
    for bad, code in ((off, -41), (bytes(stray), -40), (octs[0][:-1], -42)):
        with pytest.raises(api.BbsError) as e:
            api.register_public_keys(curve, [octs[0], bad], L=2, lib_path=twin)
        with pytest.raises(api.BbsError) as e1:
            api.octets_to_public_key(curve, bad, lib_path=twin)
        assert e.value.status == e1.value.status == code
        if code != -42:                                # (the set has grown by both keys: the exception says where and how)
            assert e.value.statuses == [1, code] and e.value.first_index + 2 == api._engine(curve, 2, lib_path=twin).public_key_count()
    eng.close()
    rec_eng.close()


def test_add_arguments(twin):
    from bbs_sign_amd import Engine, _lib
    curve = "bls12_381"
    iss = kc.Issuers(curve, 2, L, twin, seed=5)
    bare = Engine(curve, lib_path=twin, window_bits=4)
    with pytest.raises(Exception, match="BBS_E_STATE"):          # no generators yet
        bare.add_public_keys([iss.pks[0]])
    with pytest.raises(Exception, match="BBS_E_STATE"):
        bare.add_public_keys_octets([bytes(96)])
    assert bare.public_key_count() == 0
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    buf = np.zeros(4 * eng.fpb, dtype=np.uint8)
    st = np.zeros(1, dtype=np.int8)
    first = ctypes.c_uint32(0)
    u8, i8 = buf.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p)
    lib = eng.lib
    assert lib.bbs_ctx_add_public_keys(eng.h, 1, None, None, i8, ctypes.byref(first)) == -100
    assert lib.bbs_ctx_add_public_keys(eng.h, 1, u8, None, None, ctypes.byref(first)) == -100
    assert lib.bbs_ctx_add_public_keys(eng.h, 1, u8, None, i8, None) == -100
    assert lib.bbs_ctx_add_public_keys(None, 1, u8, None, i8, ctypes.byref(first)) == -100
    assert lib.bbs_ctx_add_public_keys_octets(eng.h, 1, None, i8, None, None, ctypes.byref(first)) == -100
    assert lib.bbs_ctx_add_public_keys_octets(eng.h, 1, u8, None, None, None, ctypes.byref(first)) == -100
    assert lib.bbs_ctx_add_public_keys_octets(eng.h, 1, u8, i8, None, None, None) == -100
    assert lib.bbs_selftest_key_entries(eng.h, 1, None, None, None, 1, u8, i8, None) == -100
    assert lib.bbs_selftest_key_entries(eng.h, 1, u8, None, None, 2, u8, i8, None) == -100
    assert eng.public_key_count() == 0 and lib.bbs_ctx_public_key_count(None) == 0
    # add on an empty set equals set: the same statuses, the same entries serve the same items
    keys = [iss.pks[0], kc.OFF_TWIST, None, iss.pks[1]]
    assert eng.add_public_keys([])[0] == 0 and eng.public_key_count() == 0
    first_index, sa = eng.add_public_keys(keys)
    other, ss = kc.keyed_engine(iss, keys)
    assert first_index == 0 and list(sa) == list(ss) == [1, -41, 1, 1] and eng.public_key_count() == other.public_key_count() == 4
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, [0, 1, 1, 0], R, seed=2)
    ki = np.array([0, 3, 0, 2], dtype=np.uint32)
    assert list(eng.core_verify_keyed_batch(ki, sigs, msgs, headers)) == list(other.core_verify_keyed_batch(ki, sigs, msgs, headers)) == [1, 1, 0, 0]
    # n = 0 reports the size; new generators clear the set
    assert eng.add_public_keys([])[0] == 4
    eng.set_generators(iss.gens, iss.api_id)
    assert eng.public_key_count() == 0
    with pytest.raises(Exception, match="BBS_E_STATE"):
        eng.core_verify_keyed_batch(ki, sigs, msgs, headers)
    assert eng.add_public_keys([iss.pks[1]])[0] == 0 and eng.public_key_count() == 1
    # set still replaces, and n = 0 still clears
    assert list(eng.set_public_keys(keys[:2])) == [1, -41] and eng.public_key_count() == 2
    eng.set_public_keys([])
    assert eng.public_key_count() == 0
    for e in (bare, eng, other):
        e.close()


def test_cpp_wrapper_appends_cpu_twin(twin):
    src = os.path.join(ROOT, "tests", "cpp", "keyreg_append.cpp")
    exe = os.path.join(ROOT, "bbs_sign_amd", "build", "cpp_keyreg_append_twin")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir, libname = os.path.dirname(twin), os.path.basename(twin)
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-l:" + libname,
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
