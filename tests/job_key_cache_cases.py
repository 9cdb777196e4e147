"""The job-local key cache (bbs_ctx_set_job_key_cache): prepared keys of the bbs_*_with_keys_* jobs kept across jobs.  Shared by
the host-twin tier (tests/test_job_key_cache_hosttwin.py) and the GPU tier (tests/test_job_key_cache_gpu.py); the shapes are
those of tests/job_keys_cases.py (L = 4, R = 2, 12 to 70 items).

The rule that defines correctness is the one of the exports: statuses, key statuses, bv_report and bv_verdicts of a cached job
are those of the same call with the cache off, hence those of the keyed twin on a SECOND engine whose key set was registered
from the same octets (job_keys_cases.registered) -- every expected status here comes from there.  What the cache adds is
counted: hits + misses == n_keys for every cached job, evictions, bypassed jobs."""
import functools
from types import SimpleNamespace

import numpy as np

import job_keys_cases as jk
import keyed_cases as kc
import keyreg_cases as kr
from job_keys_cases import Batch, bare, five_keys, refused_octets, registered, small_batch
from oracle import bbs
from bbs_sign_amd.engine import BbsRuntimeError

UNKNOWN_KEY = jk.UNKNOWN_KEY
COUNTED = ("hits", "misses", "evictions", "bypassed_jobs")
FAR = 99          # a key index no job of these tests has


def cached(iss, capacity, setup=None):
    eng = bare(iss)
    if setup:
        setup(eng)
    eng.set_job_key_cache(capacity)
    return eng


def go(b, eng, op, form, key_index, key_octets, submit=True, keep=False):
    """One with_keys job on `eng`: its statuses, key statuses, and what the context's counters moved by (which is what the
    job's own report says, where the job can be asked)."""
    before = eng.job_key_cache_report()
    r = b.start(eng, op, form, key_index, key_octets, submit)
    out = SimpleNamespace(job=None, kst=None)
    if submit:
        r.wait()
        out.result = np.array(r.result)
        out.kst = [int(x) for x in r.key_statuses()]
        rep = r.key_cache_report()
        if keep:
            out.job = r
        else:
            r.free()
    else:
        out.result = np.array(r)
    after = eng.job_key_cache_report()
    out.d = {k: after[k] - before[k] for k in COUNTED}
    if submit:
        assert (rep["hits"], rep["misses"], rep["bypassed"]) == (out.d["hits"], out.d["misses"], out.d["bypassed_jobs"]), (rep, out.d)
        if not rep["bypassed"] and after["capacity"]:
            assert rep["hits"] + rep["misses"] == len(key_octets)
    return out


def moved(r, hits, misses, evictions=None, bypassed=0):
    assert (r.d["hits"], r.d["misses"], r.d["bypassed_jobs"]) == (hits, misses, bypassed), r.d
    if evictions is not None:
        assert r.d["evictions"] == evictions, r.d


def subset(owner, octets, ids):
    """The job that brings the keys `ids` (of `octets`) in that order: (key_octets, key_index); items of other keys name no key."""
    return [octets[k] for k in ids], np.array([ids.index(o) if o in ids else FAR for o in owner], dtype=np.uint32)


# ---- 2. five keys, twice ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _five(curve, lib_path):
    return five_keys(curve, lib_path, -41)


def check_five_keys_twice(curve, lib_path, exports=jk.EIGHT):
    iss, key_octets, keys, key_index, b = _five(curve, lib_path)
    ref, kst = registered(iss, key_octets)
    assert kst == [1, 1, 1, 1, -41]
    eng = bare(iss)
    for op, form, submit in exports:
        want = b.run(ref, op, form, key_index)
        eng.set_job_key_cache(0)              # (an empty cache for every export)
        eng.set_job_key_cache(8)
        r1 = go(b, eng, op, form, key_index, key_octets, submit)
        moved(r1, 0, 5, 0)
        r2 = go(b, eng, op, form, key_index, key_octets, submit)
        moved(r2, 5, 0, 0)
        for r in (r1, r2):
            jk.same(r.result, want, (curve, op, form, submit))
            assert r.kst is None or r.kst == kst
            assert r.result[7] == r.result[8] == r.result[10] == UNKNOWN_KEY and r.result[1] == 1 and r.result[0] == 0
        assert eng.public_key_count() == 0
        rep = eng.job_key_cache_report()
        assert (rep["capacity"], rep["resident"], rep["pinned"]) == (8, 5, 0) and rep["device_bytes"] > 0
    ref.close()
    eng.close()


# ---- 3. indexes are not slots: the keys in reverse order plus one new key -----------------------------------------------------
def check_indexes_are_not_slots(curve, lib_path):
    iss, key_octets, keys, key_index, b = _five(curve, lib_path)
    eng = cached(iss, 8)
    ref, kst = registered(iss, key_octets)
    for op in ("pv", "vf"):
        moved(go(b, eng, op, "core", key_index, key_octets), 0 if op == "pv" else 5, 5 if op == "pv" else 0)
    ref.close()
    octets2 = key_octets[::-1] + [refused_octets(curve, -40)]
    index2 = np.array([4 - k if k < 5 else k + 10 for k in key_index], dtype=np.uint32)
    ref, kst2 = registered(iss, octets2)
    assert kst2 == kst[::-1] + [-40]
    for t, op in enumerate(("pv", "vf")):
        r = go(b, eng, op, "wire", index2, octets2)
        moved(r, 5 if t == 0 else 6, 1 if t == 0 else 0)
        jk.same(r.result, b.run(ref, op, "wire", index2), (curve, op))
        assert r.kst == kst2
        assert r.result[1] == 1 and r.result[8] == UNKNOWN_KEY
    ref.close()
    eng.close()


# ---- 3b. key-uniform wavefronts: 10 / 11 / 9 items under three keys whose slots are not their indexes --------------------------
@functools.lru_cache(maxsize=None)
def _order(curve, lib_path):
    iss = kc.Issuers(curve, 3, 4, lib_path, seed=43)
    counts = [10, 11, 9]
    owner = [k for t in range(11) for k in range(3) if t < counts[k]]
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, 2, seed=5)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=7)
    return iss, owner, Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)


def check_pairing_order(curve, lib_path):
    """The shape of job_keys_cases.check_pairing_order: keys 0 and 1 fill a key-uniform wavefront each, whose key is read from
    the wave keys.  The first job brings the keys in the order 2, 0, 1 (slots 0, 1, 2), the second in their own order: every
    wave key of the second job differs from its slot."""
    iss, owner, b = _order(curve, lib_path)
    o = jk.octets_of(curve, iss.pks)
    eng = cached(iss, 4)
    for t, ids in enumerate(([2, 0, 1], [0, 1, 2])):
        ko, ki = subset(owner, o, ids)
        ki[12] = (ki[12] + 1) % 3                 # another issuer's key
        ref, kst = registered(iss, ko)
        for op in ("pv", "vf"):
            r = go(b, eng, op, "core", ki, ko)
            moved(r, 3 if (t or op == "vf") else 0, 0 if (t or op == "vf") else 3, 0)
            jk.same(r.result, b.run(ref, op, "core", ki), (curve, op, ids))
            assert sum(r.result == 1) == b.n - 1 - len(range(0, b.n, 7))
        ref.close()
    eng.close()


# ---- 4. the same key twice in one call ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(curve, lib_path, K=3, n=12):
    return small_batch(curve, lib_path, K=K, n=n)


def check_key_twice(curve, lib_path):
    iss, owner, b = _small(curve, lib_path, K=2)
    o = jk.octets_of(curve, iss.pks)
    key_octets = [o[0], o[1], o[0]]
    key_index = np.array([(2 if i % 4 == 0 else 0) if k == 0 else 1 for i, k in enumerate(owner)], dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    eng = cached(iss, 4)
    for t, op in enumerate(("pv", "vf")):
        r = go(b, eng, op, "wire", key_index, key_octets)
        moved(r, 1 if t == 0 else 3, 2 if t == 0 else 0)          # one miss per distinct string
        jk.same(r.result, b.run(ref, op, "wire", key_index), (curve, op))
        assert r.kst == [1, 1, 1]
        assert all(r.result[i] == (0 if i % 5 == 0 else 1) for i in range(b.n))
    assert eng.job_key_cache_report()["resident"] == 2
    ref.close()
    eng.close()


# ---- 5. eviction --------------------------------------------------------------------------------------------------------------
def check_eviction(curve, lib_path, op="pv"):
    iss, owner, b = _small(curve, lib_path, K=5, n=15)
    o = jk.octets_of(curve, iss.pks)
    eng = cached(iss, 4)

    def job(ids):
        ko, ki = subset(owner, o, ids)
        ref, kst = registered(iss, ko)
        r = go(b, eng, op, "core", ki, ko)
        want = b.run(ref, op, "core", ki)
        jk.same(r.result, want, (curve, op, ids))
        assert r.kst == kst == [1] * len(ids)
        assert [i for i in range(b.n) if r.result[i] == UNKNOWN_KEY] == [i for i in range(b.n) if owner[i] not in ids]
        ref.close()
        return r

    moved(job([0, 1, 2]), 0, 3, 0)                # A: three free slots, and freed
    moved(job([3, 4, 0]), 1, 2, 1)                # B: one free slot, one eviction -- not of key 0, which B has just hit
    moved(job([1, 2]), 1, 1, 1)                   # C: B evicted the older of keys 1 and 2: one hit, one miss, one more eviction
    rep = eng.job_key_cache_report()
    assert (rep["resident"], rep["pinned"], rep["evictions"], rep["bypassed_jobs"]) == (4, 0, 2, 0)
    eng.close()


# ---- 6. pins and bypass -------------------------------------------------------------------------------------------------------
def check_pins_and_bypass(curve, lib_path, op="vf"):
    iss, owner, b = _small(curve, lib_path, K=5, n=15)
    o = jk.octets_of(curve, iss.pks)
    eng = cached(iss, 3)
    ko_a, ki_a = subset(owner, o, [0, 1, 2])
    ref_a, _ = registered(iss, ko_a)
    want_a = b.run(ref_a, op, "core", ki_a)
    a = go(b, eng, op, "core", ki_a, ko_a, keep=True)                    # A is not freed: its three slots stay pinned
    moved(a, 0, 3, 0)
    assert eng.job_key_cache_report()["pinned"] == 3
    ko_b, ki_b = subset(owner, o, [3])
    ref_b, _ = registered(iss, ko_b)
    want_b = b.run(ref_b, op, "core", ki_b)
    r = go(b, eng, op, "core", ki_b, ko_b)
    moved(r, 0, 0, 0, bypassed=1)                                        # no slot to be had: the uncached path
    jk.same(r.result, want_b, (curve, "bypassed"))
    assert r.kst == [1] and eng.job_key_cache_report()["bypassed_jobs"] == 1
    jk.same(a.result, want_a, (curve, "A"))
    a.job.run()                                                          # A again, after the bypassed job: its slots are as they were
    a.job.wait()
    jk.same(a.job.result, want_a, (curve, "A again"))
    a.job.free()
    assert eng.job_key_cache_report()["pinned"] == 0
    r = go(b, eng, op, "core", ki_b, ko_b)
    moved(r, 0, 1, 1)                                                    # now a miss, with an eviction
    jk.same(r.result, want_b, (curve, "after A.free()"))
    ko_c, ki_c = subset(owner, o, [0, 1, 2, 3])                          # more keys than slots
    ref_c, _ = registered(iss, ko_c)
    r = go(b, eng, op, "core", ki_c, ko_c)
    moved(r, 0, 0, 0, bypassed=1)
    jk.same(r.result, b.run(ref_c, op, "core", ki_c), (curve, "n_keys > capacity"))
    for e in (ref_a, ref_b, ref_c, eng):
        e.close()


# ---- 7. a hit on a key still being built: 70 items, 65 keys ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seventy(curve, lib_path):
    """The shape of test_70_items_65_keys: job key 0 = the identity, 1 .. 62 = issuers 1 .. 62, 63 = refused, 64 = issuer 0."""
    iss = kc.Issuers(curve, 64, 4, lib_path, seed=61)
    key_octets = jk.octets_of(curve, [None] + iss.pks[1:63]) + [refused_octets(curve, -41)] + jk.octets_of(curve, [iss.pks[0]])
    owner = list(range(1, 63)) + [5, 7] + [0] * 6
    key_index = np.array(list(range(1, 63)) + [0, 63] + [64] * 6, dtype=np.uint32)
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, 2, seed=13)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=23)
    return iss, key_octets, key_index, Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)


def stranger_octets(curve, count):
    """`count` distinct strings no issuer has: whatever the decoder makes of them, the cache keeps them under their own bytes."""
    fpb = 48 if curve == "bls12_381" else 32
    out = []
    for t in range(count):
        body = bytes((37 * t + 11 * j + 5) % 256 for j in range(2 * fpb - 2))
        out.append(bytes([0x80 | (t % 32), t % 256]) + body)
    assert len(set(out)) == count
    return out


def check_hit_while_building(curve, lib_path, op="pv", form="core"):
    iss, key_octets, key_index, b = _seventy(curve, lib_path)
    ref, kst = registered(iss, key_octets)
    assert kst == [1] * 63 + [-41, 1]
    want = b.run(ref, op, form, key_index)
    ref.close()
    eng = cached(iss, 128)
    ja = b.start(eng, op, form, key_index, key_octets, submit=True)
    jb = b.start(eng, op, form, key_index, key_octets, submit=True)      # at once: A's keys are on their way, not there
    jb.wait()
    ja.wait()
    assert jb.key_cache_report() == {"hits": 65, "misses": 0, "bypassed": 0}
    assert ja.key_cache_report() == {"hits": 0, "misses": 65, "bypassed": 0}
    for j in (jb, ja):
        jk.same(j.result, want, (curve, op, form))
        assert [int(x) for x in j.key_statuses()] == kst
    assert want[62] == 0 and want[63] == UNKNOWN_KEY and list(want[64:]) == [1, 1, 1, 1, 1, 0]
    assert eng.job_key_cache_report()["pinned"] == 65
    ja.free()
    jb.free()
    # a third job evicts some of them, a fourth brings them back: slots stop following the order of the keys
    strangers = stranger_octets(curve, 80)
    far = np.full(b.n, 80, dtype=np.uint32)
    r = go(b, eng, op, form, far, strangers)
    moved(r, 0, 80, 80 - (128 - 65))
    jk.same(r.result, [UNKNOWN_KEY] * b.n, (curve, "strangers"))
    ref_s, kst_s = registered(iss, strangers)
    assert r.kst == kst_s
    ref_s.close()
    r = go(b, eng, op, form, key_index, key_octets)
    moved(r, 65 - 17, 17, 17)
    jk.same(r.result, want, (curve, op, form, "fourth job"))
    assert r.kst == kst
    # every resident string: what the cache holds against the key stage alone, byte for byte
    resident = list(key_octets)
    for s in strangers:
        try:
            eng.selftest_job_key_cache_entries([s])
            resident.append(s)
        except BbsRuntimeError as e:
            assert e.rc == -102, e
    assert len(resident) == 128 == eng.job_key_cache_report()["resident"]
    got_e, got_st, _ = eng.selftest_job_key_cache_entries(resident)
    want_e, want_st, _ = kr.key_entries(eng, 1, octets=resident)
    assert [int(x) for x in got_st] == [int(x) for x in want_st]
    assert got_e == want_e
    eng.close()


# ---- 8. mixed counts -------------------------------------------------------------------------------------------------------------
def check_keyed_mixed(curve, lib_path, L=4, exports=(("pv", "wire", True), ("vf", "core", True))):
    import keyed_mixed_cases as kmc
    ring = kmc.Ring(curve, lib_path, L, K=3)
    lengths = [0, 1, L - 1, L] * 3
    owner = [(i // 4 + i) % 3 for i in range(len(lengths))]
    it = kmc.KItems(ring, owner, lengths, seed=7)
    key_octets = jk.octets_of(curve, ring.keys[:3]) + [refused_octets(curve, -41), bbs.g2_compress(bbs.SUITES[curve].curve, None)]
    key_index = list(owner)
    key_index[5] = ring.REFUSED
    key_index[6] = ring.IDENTITY
    key_index[7] = (owner[7] + 1) % 3
    ref = ring.bare()
    ref.set_keyed_mixed_lengths(True)
    _, kst, _ = ref.add_public_keys_octets(key_octets)
    kst = [int(x) for x in kst]
    assert kst == [1, 1, 1, -41, 1]
    eng = ring.bare()
    eng.set_keyed_mixed_lengths(True)
    b = Batch(curve, it.raw, it.msgs, it.disclosed, it.sigs, it.proofs, it.headers, it.phs)
    b.dm = it.dm
    b.args = lambda e, op, form: jk._mixed_args(kmc, it, e, op, form)
    for op, form, submit in exports:
        want = b.run(ref, op, form, key_index)
        eng.set_job_key_cache(0)
        eng.set_job_key_cache(8)
        r1 = go(b, eng, op, form, key_index, key_octets, submit)
        r2 = go(b, eng, op, form, key_index, key_octets, submit)
        moved(r1, 0, 5, 0)
        moved(r2, 5, 0, 0)                        # the second run: all hits
        for r in (r1, r2):
            jk.same(r.result, want, (curve, op, form, submit))
            assert r.kst is None or r.kst == kst
            assert r.result[5] == UNKNOWN_KEY and r.result[0] == 1 and r.result[3] == 1 and r.result[7] == 0, list(r.result)
    # the rows the cache holds against the functions registration uses
    _, st, rows = eng.selftest_job_key_cache_entries(key_octets, rows=True)
    rows_host, st_host = eng.selftest_key_len_rows(key_octets, 0)
    assert [int(x) for x in st] == [int(x) for x in st_host] == kst
    assert rows == rows_host
    assert eng.job_key_cache_report()["device_bytes"] >= 8 * (L + 1) * 368
    ref.close()
    eng.close()


# ---- 9. keyed batch verification ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bv(curve, lib_path):
    iss = kc.Issuers(curve, 3, 4, lib_path, seed=53)
    owner = [i % 3 for i in range(18)]
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, 2, seed=9)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=100)        # item 0 (key 0) forged, nothing else
    return iss, owner, Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)


def check_keyed_bv(curve, lib_path):
    iss, owner, b = _bv(curve, lib_path)
    o = jk.octets_of(curve, iss.pks[:2]) + [refused_octets(curve, -41)]
    seed = bytes(range(32))
    on = lambda e: e.set_keyed_batch_verification(True, seed, 4)
    eng = cached(iss, 8, on)
    plain = bare(iss)              # the same calls with the cache off
    on(plain)
    first = True
    for order in ([0, 1, 2], [2, 1, 0]):          # the job's keys as given, then permuted: groups follow the job's numbering
        key_octets = [o[k] for k in order]
        key_index = np.array([order.index(k) for k in owner], dtype=np.uint32)
        ref, kst = registered(iss, key_octets, on)
        assert kst == [1 if k < 2 else -41 for k in order]
        accepted = [g for g, k in enumerate(order) if k < 2]             # the groups the keyed twin forms, in its order
        for op in ("pv", "vf"):
            jr = b.start(ref, op, "core", key_index, submit=True)
            jr.wait()
            jo = b.start(plain, op, "core", key_index, key_octets, submit=True)
            jo.wait()
            assert jr.bv_report() == (2, 2 if op == "pv" else 1, 12)
            for run in ("miss", "hit"):
                r = go(b, eng, op, "core", key_index, key_octets, keep=True)
                if first:
                    moved(r, 0, 3)
                    first = False
                else:
                    moved(r, 3, 0)
                jk.same(r.result, jr.result, (curve, op, order, run))
                assert list(r.result) == [0] + [1, UNKNOWN_KEY, 1] * 5 + [1, UNKNOWN_KEY]
                assert r.kst == kst
                assert r.job.bv_report() == jr.bv_report()
                v = list(r.job.bv_verdicts())
                assert v == list(jo.bv_verdicts()) and len(v) == 48          # the same call with the cache off
                assert [x for g in accepted for x in v[16 * g:16 * g + 16]] == list(jr.bv_verdicts())      # and the keyed twin
                failing = [g for g in range(3) if 0 in v[16 * g:16 * g + 16] and order[g] < 2]
                assert failing == ([order.index(0)] if op == "vf" else [])
                r.job.free()
            jr.free()
            jo.free()
        ref.close()
    eng.close()
    plain.close()


# ---- 10. generations -------------------------------------------------------------------------------------------------------------
def check_generations(curve, lib_path):
    iss, owner, b = _small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks[:2]) + [refused_octets(curve, -40)]
    key_index = np.array(owner, dtype=np.uint32)

    def twin(setup=None, api_id=None):
        e = kc.make_engine(iss.curve, iss.gens, iss.api_id if api_id is None else api_id, iss.lib_path, window_bits=iss.wb)
        if setup:
            setup(e)
        _, st, _ = e.add_public_keys_octets(list(key_octets))
        assert [int(x) for x in st] == [1, 1, -40]
        return e

    def job(eng, ref, op, hits, misses, what):
        r = go(b, eng, op, "core", key_index, key_octets)
        moved(r, hits, misses, 0)
        jk.same(r.result, b.run(ref, op, "core", key_index), (curve, op, what))
        assert r.kst == [1, 1, -40]
        return r

    eng = cached(iss, 8)
    ref = twin()
    r = job(eng, ref, "pv", 0, 3, "first")
    assert sum(r.result == 1) > 0
    job(eng, ref, "vf", 3, 0, "populated")
    # a job uploaded before a change of form and waited for after it: it keeps the generation it was planned in
    early = b.start(eng, "pv", "core", key_index, key_octets, submit=True)
    eng.set_keyed_mixed_lengths(True)
    mixed = twin(lambda e: e.set_keyed_mixed_lengths(True))
    job(eng, mixed, "pv", 0, 3, "keyed mixed lengths on")            # rows are kept now: a new, empty generation
    job(eng, mixed, "vf", 3, 0, "keyed mixed lengths on, again")
    early.wait()
    jk.same(early.result, b.run(ref, "pv", "core", key_index), (curve, "uploaded before the change"))
    assert [int(x) for x in early.key_statuses()] == [1, 1, -40] and early.key_cache_report() == {"hits": 3, "misses": 0, "bypassed": 0}
    early.free()
    mixed.close()
    eng.set_keyed_mixed_lengths(False)
    job(eng, ref, "pv", 0, 3, "keyed mixed lengths off again")
    # the line form
    eng.set_unit_lines(False)
    plain_lines = twin(lambda e: e.set_unit_lines(False))
    job(eng, plain_lines, "vf", 0, 3, "(c, nl) lines")
    job(eng, plain_lines, "pv", 3, 0, "(c, nl) lines, again")
    plain_lines.close()
    eng.set_unit_lines(True)
    job(eng, ref, "vf", 0, 3, "unit lines again")
    ref.close()
    # other generators' api_id: every prefix differs, no credential of the batch verifies
    other = iss.api_id + b"OTHER_"
    eng.set_generators(iss.gens, other)
    ref2 = twin(api_id=other)
    r = job(eng, ref2, "pv", 0, 3, "another api_id")
    assert sum(r.result == 1) == 0
    job(eng, ref2, "vf", 3, 0, "another api_id, again")
    ref2.close()
    assert eng.job_key_cache_report()["resident"] == 3 and eng.job_key_cache_report()["pinned"] == 0
    eng.close()


# ---- 11. run twice ---------------------------------------------------------------------------------------------------------------
def check_run_twice(curve, lib_path):
    iss, owner, b = _small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks[:2]) + [refused_octets(curve, -40)]
    key_index = np.array(owner, dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    assert kst == [1, 1, -40]
    eng = cached(iss, 4)
    for op in ("pv", "vf"):
        want = b.run(ref, op, "core", key_index)
        job = b.start(eng, op, "core", key_index, key_octets, submit=True)
        job.wait()
        jk.same(job.result, want, (curve, op, "first run"))
        assert list(job.key_statuses()) == kst
        before = eng.job_key_cache_report()
        job.run()
        job.wait()
        jk.same(job.result, want, (curve, op, "second run"))
        assert list(job.key_statuses()) == kst
        assert eng.job_key_cache_report() == before               # a run looks nothing up
        job.free()
    ref.close()
    eng.close()


# ---- 12. off, and the argument errors ---------------------------------------------------------------------------------------------
def check_off_and_arguments(curve, lib_path):
    import ctypes
    from bbs_sign_amd import _lib
    iss, owner, b = _small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks)
    key_index = np.array(owner, dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    want = b.run(ref, "vf", "core", key_index)
    eng = bare(iss)
    zero = {"capacity": 0, "resident": 0, "pinned": 0, "hits": 0, "misses": 0, "evictions": 0, "bypassed_jobs": 0, "device_bytes": 0}
    assert eng.job_key_cache_report() == zero                    # off by default
    r = go(b, eng, "vf", "core", key_index, key_octets)
    moved(r, 0, 0, 0)
    jk.same(r.result, want, (curve, "off by default"))
    eng.set_job_key_cache(4)
    assert eng.job_key_cache_report() == dict(zero, capacity=4)  # nothing is allocated before the first cached job
    moved(go(b, eng, "vf", "core", key_index, key_octets), 0, 3, 0)
    moved(go(b, eng, "vf", "core", key_index, key_octets), 3, 0, 0)
    assert eng.job_key_cache_report()["resident"] == 3 and eng.job_key_cache_report()["device_bytes"] > 0
    eng.set_job_key_cache(0)                                     # drops the cache; the counters stay
    assert eng.job_key_cache_report() == dict(zero, hits=3, misses=3)
    r = go(b, eng, "vf", "core", key_index, key_octets)
    moved(r, 0, 0, 0)
    jk.same(r.result, want, (curve, "off again"))
    assert r.kst == kst
    try:
        eng.selftest_job_key_cache_entries(key_octets[:1])
        raise AssertionError("the cache is off")
    except BbsRuntimeError as e:
        assert e.rc == -102, e
    # the argument errors
    lib = eng.lib
    assert lib.bbs_ctx_set_job_key_cache(None, 4) == -100
    assert lib.bbs_ctx_set_job_key_cache(eng.h, 0xFFFFFFF1) == -100
    assert lib.bbs_ctx_set_job_key_cache(eng.h, 0xFFFFFFF0) == 0 and lib.bbs_ctx_set_job_key_cache(eng.h, 0) == 0
    assert lib.bbs_ctx_job_key_cache_report(None, None, None, None, None, None, None, None, None) == -100
    assert lib.bbs_ctx_job_key_cache_report(eng.h, None, None, None, None, None, None, None, None) == 0
    assert lib.bbs_job_key_cache_report(None, None, None, None) == -100
    j = b.start(eng, "vf", "core", key_index, key_octets, submit=True)
    j.wait()
    assert lib.bbs_job_key_cache_report(j.h, None, None, None) == 0
    j.free()
    ref_job = b.start(ref, "vf", "core", key_index, submit=True)          # a keyed job: no key set of its own
    ref_job.wait()
    h = ctypes.c_uint32(7)
    assert lib.bbs_job_key_cache_report(ref_job.h, ctypes.byref(h), None, None) == -102
    ref_job.free()
    pk = np.frombuffer(key_octets[0], dtype=np.uint8).copy()
    st = np.zeros(1, dtype=np.int8)
    assert lib.bbs_selftest_job_key_cache_entries(None, 1, pk.ctypes.data_as(_lib.c_u8p), pk.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p), None) == -100
    assert lib.bbs_selftest_job_key_cache_entries(eng.h, 1, None, pk.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p), None) == -100
    ref.close()
    eng.close()


# ---- 13. api.verify_many_issuers(..., register_keys=False, key_cache=8) -------------------------------------------------------------
def check_api_key_cache(curve, lib_path):
    from bbs_sign_amd import api
    from bbs_sign_amd.api import PublicKey, SecretKey
    # (the keys of test_job_keys_hosttwin's api test, in its order: the process-wide cached engine other api tests index by
    # position stays what they expect)
    sks = [SecretKey(curve, 1000 + k, lib_path) for k in range(2)]
    pks = [sk.sk_to_pk() for sk in sks]
    bad = PublicKey(curve, kc.OFF_TWIST, lib_path)
    lists = [[b"a", b"b"], [b"c", b"d", b"e"], [b"f", b"g"], [b"h", b"i", b"j"], [b"k", b"l"]]
    signed = [(sks[i % 2].sign(m, b"hdr%d" % i), b"hdr%d" % i, m) for i, m in enumerate(lists)]
    items = [(pks[i % 2],) + s for i, s in enumerate(signed)]
    items[2] = (items[2][0], items[2][1], items[2][2], [b"forged", b"g"])
    items[4] = (bad,) + items[4][1:]
    want = api.verify_many_issuers(items)
    ie = api._issuer_cache[(curve, 0, lib_path)]
    index, count = dict(ie.index), ie.eng.public_key_count()
    before = ie.eng.job_key_cache_report()
    for call in range(2):
        got = api.verify_many_issuers(items, register_keys=False, key_cache=8)
        assert [repr(g) for g in got] == [repr(w) for w in want]
        assert got[0] is True and got[1] is True and got[2] is False and got[3] is True and isinstance(got[4], api.BbsError)
    rep = ie.eng.job_key_cache_report()
    assert rep["capacity"] == 8 and rep["misses"] - before["misses"] == 3 and rep["hits"] - before["hits"] == 3, rep
    assert ie.index == index and ie.eng.public_key_count() == count
    proofs = []
    for i, (pk, sig, hdr, msgs) in enumerate(items[:4]):
        proofs.append((pks[i % 2], api.proof_gen(pks[i % 2], sig, hdr, b"ph", lists[i], [0]), hdr, b"ph", [msgs[0]], [0]))
    proofs.append((bad,) + proofs[1][1:])
    want = api.proof_verify_many_issuers(proofs)
    got = api.proof_verify_many_issuers(proofs, register_keys=False, key_cache=8)
    assert [repr(g) for g in got] == [repr(w) for w in want]
    assert ie.eng.job_key_cache_report()["hits"] - rep["hits"] == 3          # the same three strings, the same engine: all hits
    got = api.verify_many_issuers(items, register_keys=False)                 # key_cache=0: the cache is switched off again
    assert [repr(g) for g in got] == [repr(w) for w in api.verify_many_issuers(items)]
    assert ie.eng.job_key_cache_report()["capacity"] == 0
