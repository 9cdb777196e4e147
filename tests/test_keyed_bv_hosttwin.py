"""Keyed batch verification through the TEST-ONLY host twin, both curves, L = 4, R = 2 (tests/keyed_bv_cases.py).

Keys: three issuers, the identity key, one refused key.  9 / 5 / 2 items per issuer, min_items = 4: the first two issuers form
groups (runs of 9 and 5 items, the second starting at position 12 of the bv order), the third stays with the per-item kernel."""
import functools
import os
import random
import sys

import numpy as np
import pytest

import keyed_bv_cases as bv
import keyed_cases as kc
from oracle import bbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

L, R = 4, 2
COUNTS = (9, 5, 2)
TO_KEY = {0: 0, 1: 1, 2: 3}
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@functools.lru_cache(maxsize=None)
def _scene(curve, twin):
    """(issuers, registered keys, the all-valid batch): made once per curve, never changed (tests work on copies)."""
    iss = kc.Issuers(curve, 3, L, twin, seed=47)
    keys = [iss.pks[0], iss.pks[1], None, iss.pks[2], kc.OFF_TWIST]
    owner = bv.interleaved(COUNTS)
    return iss, keys, bv.Batch(iss, owner, [TO_KEY[o] for o in owner], R, seed=9)


def _engine(iss, keys, min_items=4, on=True):
    eng, kst = kc.keyed_engine(iss, keys)
    assert list(kst) == [1, 1, 1, 1, -41]
    if on:
        eng.set_keyed_batch_verification(True, bv.SEED, min_items)
    return eng, kst


def _expected(iss, keys, kst, batch, op):
    return kc.expected_by_single_key(iss, keys, kst, batch.key_index, batch.runner(op))


def test_symbols(twin):
    from bbs_sign_amd import _lib
    bv.check_symbols(_lib.load_library(twin))


@pytest.mark.parametrize("curve", CURVES)
def test_all_valid_and_switch_off(twin, curve):
    iss, keys, batch = _scene(curve, twin)
    eng, kst = _engine(iss, keys)
    off, _ = _engine(iss, keys, on=False)
    for op in ("pv", "vf"):
        want = _expected(iss, keys, kst, batch, op)
        assert list(want) == [1] * batch.n
        for form in ("core", "wire"):
            st, rep, names = batch.run(eng, op, form)
            assert list(st) == list(want), (op, form, list(st))
            assert rep == (2, 2, 14), (op, form, rep)
            assert all(s in names for s in bv.STAGES), names
            # the combination stands in front of the per-item kernel
            assert names.index("keyed_bv_decide") < max(i for i, s in enumerate(names) if s.startswith("pair"))
        st, rep, names = batch.run(off, op)
        assert list(st) == list(want) and rep == (0, 0, 0) and not any(s in names for s in bv.STAGES), (op, rep, names)
    # switched off again on the same engine: the next job is the per-item job
    eng.set_keyed_batch_verification(False)
    st, rep, names = batch.run(eng, "pv")
    assert rep == (0, 0, 0) and not any(s in names for s in bv.STAGES)


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("curve", CURVES)
def test_one_bad_item(twin, curve, where):
    # a digit or a point written at the item index instead of the sorted position gives the bad item weight zero (or
    # another item's weight): its group passes and it is ACCEPTED
    iss, keys, base = _scene(curve, twin)
    run5 = bv.positions_of(base, 1)
    assert len(run5) == 5
    bad = {"first": run5[0], "last": run5[-1], "middle": run5[2]}[where]
    batch = base.copy().make_bad([bad])
    eng, kst = _engine(iss, keys)
    for op in ("pv", "vf"):
        want = _expected(iss, keys, kst, batch, op)
        assert want[bad] == 0 and sum(want == 1) == batch.n - 1, (op, list(want))
        st, rep, _ = batch.run(eng, op)
        assert list(st) == list(want), (op, where, list(st))
        assert rep == (2, 1, 14), (op, where, rep)


@pytest.mark.parametrize("curve", CURVES)
def test_cancelling_pair(twin, curve):
    # two copies of one valid item, tampered to A + T and A - T: their pairing errors are inverse, so equal (or shared)
    # coefficients would let the group pass
    iss, keys, base = _scene(curve, twin)
    run9 = bv.positions_of(base, 0)
    a, b = run9[1], run9[6]
    batch = base.copy().duplicate(a, b).make_bad([a, b], signs=[1, -1])
    eng, kst = _engine(iss, keys)
    st, rep, _ = batch.run(eng, "vf")
    want = _expected(iss, keys, kst, batch, "vf")
    assert list(st) == list(want) and st[a] == 0 and st[b] == 0 and sum(st == 1) == batch.n - 2, list(st)
    assert rep == (2, 1, 14), rep


@pytest.mark.parametrize("curve", CURVES)
def test_gated_out_items_inside_a_group(twin, curve):
    iss, keys, base = _scene(curve, twin)
    run9 = bv.positions_of(base, 0)
    unknown, malformed, mismatch = run9[0], run9[3], run9[8]
    batch = base.copy()
    batch.key_index[unknown] = 7                                   # no such key: BBS_ST_UNKNOWN_KEY, in no group
    batch.disclosed[malformed] = [0, L + 3]                        # a disclosed index out of range
    p = kc.to_engine_proof(batch.proofs[mismatch])
    p.e_cap = (p.e_cap + 1) % iss.suite.curve.r                    # the challenge no longer matches
    batch.proofs[mismatch] = p
    eng, kst = _engine(iss, keys)
    st, rep, _ = batch.run(eng, "pv")
    want = _expected(iss, keys, kst, batch, "pv")
    assert list(st) == list(want), list(st)
    assert st[unknown] == kc.UNKNOWN_KEY and st[malformed] < 0 and st[malformed] != kc.UNKNOWN_KEY and st[mismatch] == 0
    assert sum(st == 1) == batch.n - 3
    assert rep == (2, 2, 13), rep                                  # each keeps its status; neither group is stopped
    st, rep, _ = batch.run(eng, "vf")                              # verify: the unknown key alone
    assert st[unknown] == kc.UNKNOWN_KEY and sum(st == 1) == batch.n - 1 and rep == (2, 2, 13)


@pytest.mark.parametrize("curve", CURVES)
def test_thresholds(twin, curve):
    iss, keys, base = _scene(curve, twin)
    batch = base.copy().make_bad([bv.positions_of(base, 3)[1]])     # a bad item in the two-item key
    eng, kst = _engine(iss, keys, min_items=1)                     # every key is a group, the small one too
    want = {op: _expected(iss, keys, kst, batch, op) for op in ("pv", "vf")}
    for op in ("pv", "vf"):
        st, rep, _ = batch.run(eng, op)
        assert list(st) == list(want[op]) and sum(st == 0) == 1, (op, list(st))
        assert rep == (3, 2, 16), (op, rep)
    eng.set_keyed_batch_verification(True, bv.SEED, 10)            # larger than every count: no groups
    for op in ("pv", "vf"):
        st, rep, names = batch.run(eng, op)
        assert list(st) == list(want[op]) and rep == (0, 0, 0) and not any(s in names for s in bv.STAGES), (op, rep)
    eng.set_keyed_batch_verification(True, bv.SEED, 0)             # the library's default is never below 17
    st, rep, names = batch.run(eng, "vf")
    assert list(st) == list(want["vf"]) and rep == (0, 0, 0) and not any(s in names for s in bv.STAGES)
    eng.set_keyed_batch_verification(True, bv.SEED, 9)             # exactly the largest count: that key alone
    st, rep, _ = batch.run(eng, "pv")
    assert list(st) == list(want["pv"]) and rep == (1, 1, 9), rep


@pytest.mark.parametrize("curve", CURVES)
def test_cnl_line_form(twin, curve):
    iss, keys, base = _scene(curve, twin)
    batch = base.copy().make_bad([bv.positions_of(base, 0)[4]])
    eng, kst = kc.keyed_engine(iss, keys)
    eng.set_unit_lines(False)
    eng.set_keyed_batch_verification(True, bv.SEED, 4)
    for op in ("pv", "vf"):
        st, rep, _ = batch.run(eng, op)
        assert list(st) == list(_expected(iss, keys, kst, batch, op)) and sum(st == 0) == 1, (op, list(st))
        assert rep == (2, 1, 14), (op, rep)


@pytest.mark.parametrize("curve", CURVES)
def test_job_run_twice(twin, curve):
    iss, keys, base = _scene(curve, twin)
    batch = base.copy().make_bad([bv.positions_of(base, 1)[3]])
    eng, kst = _engine(iss, keys)
    for op in ("pv", "vf"):
        job = batch.submit(eng, op)
        job.wait()
        first, rep1 = np.array(job.result), job.bv_report()
        assert list(first) == list(_expected(iss, keys, kst, batch, op)) and rep1 == (2, 1, 14)
        job.run()
        job.wait()
        assert list(job.result) == list(first) and job.bv_report() == rep1
        tot, _ = job.run_timed(2)                                  # the timed runner resets the verdicts as run() does
        assert list(job.status()) == list(first) and job.bv_report() == rep1
        job.free()


@pytest.mark.parametrize("curve", CURVES)
def test_mixed_counts(twin, curve):
    import keyed_mixed_cases as km
    ring = km.Ring(curve, twin, L, K=2, seed=31)
    owner = [0] * 6 + [1] * 5
    lengths = [0, 1, L, L, 1, 0, L, 0, 1, L, L]
    it = km.KItems(ring, owner, lengths, seed=5)
    key_index = list(owner)
    eng = ring.engine()
    off = {op: km.run_keyed(eng, it, op, key_index) for op in ("pv", "vf")}
    eng.set_keyed_batch_verification(True, bv.SEED, 4)
    for op in ("pv", "vf"):
        want = km.expected(ring, it, op, key_index, L)
        ki = np.asarray(key_index, dtype=np.uint32)
        if op == "vf":
            job = eng.core_verify_keyed_submit(ki, it.sigs, it.msgs, it.headers)
        else:
            job = eng.core_proof_verify_keyed_submit(ki, it.proofs, it.dm, it.disclosed, it.headers, it.phs)
        job.wait()
        st, rep = np.array(job.result), job.bv_report()
        job.free()
        assert list(st) == list(off[op]) == [int(x) for x in want] == [1] * it.n, (op, list(st), want)
        assert rep == (2, 2, 11), (op, rep)


@pytest.mark.parametrize("curve", CURVES)
def test_segmented_sums(twin, curve):
    iss, _, _ = _scene(curve, twin)
    c = iss.suite.curve
    rng = random.Random(77)
    sizes = [1, 3, 4, 5, 9]
    n = sum(sizes)
    pts, _ = bv.arithmetic_points(c, n, rng)
    pts[6] = None                                                  # an identity point among the inputs
    digits = [[rng.randrange(256) for _ in range(n)] for _ in range(16)]
    digits[5] = [0] * n                                            # a digit column of all zeros
    digits[9][2] = 255
    groups, first = [], 0
    for s in sizes:
        groups.append((first, s))
        first += s
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    got = eng.segmented_sums(pts, digits, groups)
    assert got == bv.sums_term_by_term(c, pts, digits, groups)
    assert all(row[5] is None for row in got)
    # groups given out of order and overlapping: a group is a run of the input, nothing more
    assert eng.segmented_sums(pts, digits, [groups[4], groups[1], (0, n)])[:2] == [got[4], got[1]]
    with pytest.raises(Exception, match="BBS_E_ARG"):
        eng.segmented_sums(pts, digits, [(n - 1, 2)])


def test_many_issuers_api(twin):
    from bbs_sign_amd import api
    sks = [api.SecretKey("bls12_381", 1000 + k, lib_path=twin) for k in range(2)]
    items = []
    for i in range(7):
        sk = sks[i % 2]
        msgs = [b"m-%d-%d" % (i, j) for j in range(1 + i % 3)]
        sig = sk.sign(msgs, b"hdr")
        items.append((sk.sk_to_pk(), sig, b"hdr" if i != 4 else b"other", msgs))
    plain = api.verify_many_issuers(items)
    assert plain == [i != 4 for i in range(7)]
    assert api.verify_many_issuers(items, batch_verification=True) == plain      # the default threshold: no group in 7 items
    # a threshold of 2: both issuers form groups (4 and 3 items); item 4's pairing fails, so its group is decided one by one
    assert api.verify_many_issuers(items, batch_verification=2) == plain
    ie = api._issuer_engine("bls12_381", 0, twin, 1, [])
    job = ie.eng.verify_wire_keyed_submit([0, 1], [api.signature_to_octets("bls12_381", items[i][1], twin) for i in (0, 1)],
                                          [items[i][3] for i in (0, 1)], [b"hdr", b"hdr"])
    job.wait()
    assert list(job.result) == [1, 1] and job.bv_report() == (0, 0, 0)           # the switch is off again behind the call
    job.free()
    pitems = []
    for i, (pk, sig, hdr, msgs) in enumerate(items):
        if i == 4:
            continue
        proof = api.proof_gen(pk, sig, hdr, b"ph", msgs, [0])
        pitems.append((pk, proof, hdr, b"ph" if i != 2 else b"xx", [msgs[0]], [0]))
    plain = api.proof_verify_many_issuers(pitems)
    assert plain == [i != 2 for i in range(6)]
    assert api.proof_verify_many_issuers(pitems, batch_verification=True) == plain
    assert api.proof_verify_many_issuers(pitems, batch_verification=3) == plain
