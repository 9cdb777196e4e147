"""proof_gen under a job-local key set (bbs_core_proof_gen_with_keys_*, bbs_proof_gen_wire_with_keys_*): the issuer keys arrive
with the job as compressed octets, the job prepares their domain midstates on the device (stages_key.hpp KeyDomainBuild) and
releases them.  Shared by the host-twin tier (tests/test_job_keys_gen_hosttwin.py) and the GPU tier
(tests/test_job_keys_gen_gpu.py); the shapes are those of tests/job_keys_cases.py (L = 4, R = 2).

The rule that defines correctness: status AND output bytes are, bit for bit, what the keyed twin (bbs_*proof_gen*_keyed_*)
returns on a context with the same generators, api_id, switches and random scalars or seeds whose key set was registered from
the same octets (bbs_ctx_add_public_keys_octets).  Every expected value therefore comes from a SECOND engine,
job_keys_cases.registered(), running the keyed export -- never from the code under test; a few items are also checked against
the pure-Python oracle with the item's key, and against verification."""
import ctypes
import random
from types import SimpleNamespace

import numpy as np

import job_keys_cases as jk
import job_key_cache_cases as jc
import keyed_cases as kc
import keyreg_cases as kr
from bbs_sign_amd import _lib
from oracle import bbs

UNKNOWN_KEY = jk.UNKNOWN_KEY
EXPORTS = tuple("bbs_%s_with_keys_%s" % (op, tail) for op in ("core_proof_gen", "proof_gen_wire") for tail in ("submit", "batch"))
FOUR = tuple((form, submit) for form in ("core", "wire") for submit in (False, True))


def check_exports(lib_path):
    lib = _lib.load_library(lib_path)
    for name in EXPORTS + ("bbs_selftest_key_domain_entries",):
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name


# ---- one proof_gen call in every form; the result is everything the library wrote ----------------------------------------------
class Gen:
    """The inputs of one proof_gen batch: signatures, messages (scalars and raw bytes), disclosed indexes, headers, phs."""

    def __init__(self, curve, sigs, msgs, raw, disclosed, headers, phs, sig_octets):
        self.curve, self.n = curve, len(sigs)
        self.sigs, self.msgs, self.raw, self.disclosed, self.headers, self.phs = sigs, msgs, raw, disclosed, headers, phs
        self.sig_octets = sig_octets

    def start(self, eng, form, rnds, key_index, key_octets=None, submit=False):
        """The keyed export (key_octets None) or the with_keys export of that form -> what the call returns."""
        own = {} if key_octets is None else {"key_octets": list(key_octets)}
        how = "keyed" if key_octets is None else "with_keys"
        tail = "submit" if submit else "batch"
        if form == "core":
            a = (key_index, self.sigs, self.msgs, self.disclosed, rnds, self.headers, self.phs)
            fn = "bbs_core_proof_gen_%s_%s" % (how, tail)
            return eng._pg_core_keyed_submit(fn, *a, **own) if submit else eng._pg_core_keyed(fn, *a, **own)
        a = (self.sig_octets, self.raw, self.disclosed, rnds, self.headers, self.phs)
        f = getattr(eng, "proof_gen_wire_%s_%s" % (how, tail))
        return f(key_index, *a) if key_octets is None else f(list(key_octets), key_index, *a)

    def run(self, eng, form, rnds, key_index, key_octets=None, submit=False, want_keys=None, keep=False):
        """-> SimpleNamespace(st, out): the statuses and, byte for byte, the output -- core: (records, commitments, offsets);
        wire: the octet strings (their lengths are the offsets)."""
        r = self.start(eng, form, rnds, key_index, key_octets, submit)
        res = SimpleNamespace(job=None, rep=None)
        if submit:
            r.wait()
            res.st = [int(x) for x in r.result]
            if form == "core":
                res.out = tuple(x.tobytes() for x in r.raw)
                res.proofs = r.output()[0]
            else:
                res.out = tuple(r.output()[0])
            if key_octets is not None:
                res.kst = [int(x) for x in r.key_statuses()]
                res.rep = r.key_cache_report()
                if want_keys is not None:
                    assert res.kst == list(want_keys), (res.kst, want_keys)
            if keep:
                res.job = r
            else:
                r.free()
        elif form == "core":
            n, st, pf, cm, cmo = r
            res.st = [int(x) for x in st[:n]]
            res.out = (pf.tobytes(), cm.tobytes(), cmo.tobytes())
            res.proofs = eng._dec_proofs(pf, cm, cmo, st, n)
        else:
            res.st = [int(x) for x in r[1]]
            res.out = tuple(r[0])
        return res


def same(got, want, what):
    assert got.st == want.st, (what, "statuses", got.st, want.st)
    assert got.out == want.out, (what, "bytes")


def no_output(g, form, i, fpb):
    """Item i of a result has no output: a zero record (core) or no octet string (wire)."""
    if form == "wire":
        return g.out[i] == b""
    rec = 6 * fpb + 128
    return g.out[0][i * rec:(i + 1) * rec] == bytes(rec) and g.proofs[i] is None


def gen_of(b, iss):
    """The proof_gen inputs of a job_keys_cases.Batch: its signatures, the messages they were made over, its disclosed indexes
    (one of them malformed), and random scalars of our own."""
    rng = random.Random(97)
    r = iss.suite.curve.r
    rnds = [[rng.randrange(1, r) for _ in range(5 + iss.L - len(b.disclosed[i]))] for i in range(b.n)]
    raw = [[b"item-%d-msg-%d-3" % (i, j) for j in range(iss.L)] for i in range(b.n)]      # (kc.make_items, seed = 3: not the forged ones)
    return Gen(b.curve, b.sigs, b.pm, raw, b.disclosed, b.headers, b.phs, [kc.sig_octets(b.curve, s) for s in b.sigs]), rnds


# ---- the stage alone -------------------------------------------------------------------------------------------------------------
def check_stage(curve, lib_path, octets=None):
    """bbs_selftest_key_domain_entries against bbs_selftest_key_entries(path = 0): equal statuses, the `hash` part of every entry
    byte for byte, the `tab` part that of a table-less entry."""
    iss = kc.Issuers(curve, 1, 4, lib_path, seed=5)
    eng = jk.bare(iss)
    want_st = None
    if octets is None:
        octets, want_st, _ = kr.octet_cases(curve)
    want_e, st0, _ = kr.key_entries(eng, 0, octets=octets)
    got_e, got_st = eng.selftest_key_domain_entries(octets)
    assert [int(x) for x in got_st] == [int(x) for x in st0]
    if want_st is not None:
        assert [int(x) for x in st0] == want_st
    hb = int(eng.lib.bbs_selftest_hash_ctx_bytes())
    eb = int(eng.lib.bbs_selftest_key_entry_bytes(eng.curve))
    # a KeyEntry is its line table, then its HashCtx.  The table of a key without one: what the host path writes for a refused
    # string (no lines, the identity flag set) -- the same bytes for every refused string
    refused = [k for k in range(len(octets)) if st0[k] != 1]
    no_table = want_e[refused[0]][:eb - hb]
    assert all(want_e[k][:eb - hb] == no_table for k in refused) and no_table.count(b"\x01") == 1 and sum(no_table) == 1
    for k in range(len(octets)):
        assert got_e[k][eb - hb:] == want_e[k][eb - hb:], (curve, "hash part of key", k)
        assert got_e[k][:eb - hb] == no_table, (curve, "table part of key", k)
    # an accepted key's midstate is its own; a refused key's is the one every entry starts from
    ok = [k for k in range(len(octets)) if st0[k] == 1]
    assert len({got_e[k][eb - hb:] for k in ok}) == len({octets[k] for k in ok})
    assert len({got_e[k][eb - hb:] for k in refused}) == 1
    eng.close()


def seventy_octets(curve):
    """70 strings, two wavefronts of the stage: refused strings at 0, 63 and 64, the identity at 65, valid keys elsewhere."""
    c = bbs.SUITES[curve].curve
    octs = jk.octets_of(curve, kr.valid_keys(curve, 70, seed=71))
    octs[0] = jk.refused_octets(curve, -41)
    octs[63] = jk.refused_octets(curve, -40)
    octs[64] = bbs.g2_compress(c, kr.off_subgroup_point(curve))
    octs[65] = bbs.g2_compress(c, None)
    return octs


# ---- five keys -------------------------------------------------------------------------------------------------------------------
def check_five_keys(curve, lib_path, refused_code, exports=FOUR, oracle=True, round_trip=True):
    iss, key_octets, keys, key_index, b = jk.five_keys(curve, lib_path, refused_code)
    g, rnds = gen_of(b, iss)
    ref, kst = jk.registered(iss, key_octets)
    assert kst == [1, 1, 1, 1, refused_code]
    eng = jk.bare(iss)
    got = {}
    for form, submit in exports:
        want = g.run(ref, form, rnds, key_index)
        r = g.run(eng, form, rnds, key_index, key_octets, submit, want_keys=kst)
        same(r, want, (curve, form, submit))
        for i in (7, 8, 10):
            assert r.st[i] == UNKNOWN_KEY and no_output(r, form, i, eng.fpb), (form, i)
        # item 13 discloses an index out of range under a good key: its own code
        assert r.st[13] < 0 and r.st[13] != UNKNOWN_KEY and no_output(r, form, 13, eng.fpb)
        assert [i for i in range(g.n) if r.st[i] != 1] == [7, 8, 10, 13], r.st
        got[form] = r
    assert eng.public_key_count() == 0
    # the same malformed item under a bad key: the unknown key wins
    bad_index = np.array(key_index)
    bad_index[13] = 4
    r = g.run(eng, exports[0][0], rnds, bad_index, key_octets)
    same(r, g.run(ref, exports[0][0], rnds, bad_index), (curve, "item 13 under the refused key"))
    assert r.st[13] == UNKNOWN_KEY
    if oracle and "core" in got:       # a few items against the oracle with that item's key (9: the identity key)
        for i in (1, 4, 9):
            want = bbs.core_proof_gen(iss.suite, keys[key_index[i]], bbs.Signature(b.sigs[i].a, b.sigs[i].e), b.headers[i], iss.gens,
                                      b.phs[i], b.pm[i], b.disclosed[i], iss.api_id, rnds[i])
            p = got["core"].proofs[i]
            assert (p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge) == \
                   (want.a_bar, want.b_bar, want.d, want.e_cap, want.r1_cap, want.r3_cap, list(want.commitments), want.challenge), (curve, i)
    if round_trip and "core" in got:
        # the proofs verify under the same octets exactly where proof_gen gave 1 and the item's key was the signer's
        r = got["core"]
        idx = [i for i in range(g.n) if r.st[i] == 1]
        dm = [[b.pm[i][j] for j in b.disclosed[i]] for i in idx]
        vst = eng.core_proof_verify_with_keys_batch(key_octets, key_index[idx], [r.proofs[i] for i in idx], dm,
                                                    [b.disclosed[i] for i in idx], [b.headers[i] for i in idx], [b.phs[i] for i in idx])
        signer = {0: 0, 1: 1, 2: 3}      # issuer -> its key of this job (five_keys)
        want_v = [1 if key_index[i] == signer[i % 3] else 0 for i in idx]
        assert [int(x) for x in vst] == want_v, (list(vst), want_v)
        assert r.st[4] == 1 and want_v[idx.index(4)] == 0 and r.st[9] == 1 and want_v[idx.index(9)] == 0
    ref.close()
    eng.close()


# ---- the same string twice, counts, run twice ------------------------------------------------------------------------------------
def small(curve, lib_path, K=3, n=12):
    iss, owner, b = jk.small_batch(curve, lib_path, K=K, n=n)
    g, rnds = gen_of(b, iss)
    raw = [[b"item-%d-msg-%d-47" % (i, j) for j in range(iss.L)] for i in range(b.n)]      # (small_batch makes its items with seed 47)
    g.raw = raw
    return iss, owner, g, rnds


def check_key_twice(curve, lib_path):
    iss, owner, g, rnds = small(curve, lib_path, K=2)
    o = jk.octets_of(curve, iss.pks)
    key_octets = [o[0], o[1], o[0]]
    key_index = np.array([(2 if i % 4 == 0 else 0) if k == 0 else 1 for i, k in enumerate(owner)], dtype=np.uint32)
    ref, kst = jk.registered(iss, key_octets)
    eng = jk.bare(iss)
    for form in ("core", "wire"):
        r = g.run(eng, form, rnds, key_index, key_octets, submit=True, want_keys=[1, 1, 1])
        same(r, g.run(ref, form, rnds, key_index), (curve, form))
        assert r.st == [1] * g.n
    ref.close()
    eng.close()


def check_counts(curve, lib_path):
    iss, owner, g, rnds = small(curve, lib_path, K=1, n=4)
    eng = jk.bare(iss)
    key_index = np.zeros(g.n, dtype=np.uint32)
    for form, submit in FOUR:
        r = g.run(eng, form, rnds, key_index, [], submit, want_keys=[])            # n_keys = 0, n > 0
        assert r.st == [UNKNOWN_KEY] * g.n and all(no_output(r, form, i, eng.fpb) for i in range(g.n)), (form, submit)
    o = jk.octets_of(curve, iss.pks)
    for keys in (o, []):                                                             # n = 0
        proofs, st = eng.core_proof_gen_with_keys_batch(keys, [], [], [], [], [])
        assert proofs == [] and list(st) == []
        octs, st = eng.proof_gen_wire_with_keys_batch(keys, [], [], [], [], [])
        assert octs == [] and list(st) == []
    eng.close()


def check_run_twice(curve, lib_path):
    iss, owner, g, rnds = small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks[:2]) + [jk.refused_octets(curve, -40)]
    key_index = np.array(owner, dtype=np.uint32)
    ref, kst = jk.registered(iss, key_octets)
    assert kst == [1, 1, -40]
    want = g.run(ref, "core", rnds, key_index)
    eng = jk.bare(iss)
    r = g.run(eng, "core", rnds, key_index, key_octets, submit=True, want_keys=kst, keep=True)
    same(r, want, (curve, "first run"))
    assert r.job.device_bytes() > 0
    r.job.run()
    r.job.wait()
    again = SimpleNamespace(st=[int(x) for x in r.job.result], out=tuple(x.tobytes() for x in r.job.raw))
    same(again, want, (curve, "second run"))
    assert [int(x) for x in r.job.key_statuses()] == kst
    assert [i for i in range(g.n) if again.st[i] == UNKNOWN_KEY] == [i for i in range(g.n) if owner[i] == 2]
    r.job.free()
    ref.close()
    eng.close()


# ---- keyed mixed lengths: counts 0 .. L under three keys ----------------------------------------------------------------------
def check_keyed_mixed(curve, lib_path, L=4, exports=FOUR):
    import keyed_gen_cases as kg
    import keyed_mixed_cases as kmc
    import mixed_len_cases as mc
    ring = kmc.Ring(curve, lib_path, L, K=3)
    lengths = list(range(L + 1)) * 3
    owner = [(i // 4 + i) % 3 for i in range(len(lengths))]
    it = kmc.KItems(ring, owner, lengths, seed=7)
    rnds = kg.rnds_of(it, seed=7)
    g = Gen(curve, it.sigs, it.msgs, it.raw, it.disclosed, it.headers, it.phs, [mc.sig_octets(it.w, s) for s in it.sigs])
    key_octets = jk.octets_of(curve, ring.keys[:3]) + [jk.refused_octets(curve, -41), bbs.g2_compress(bbs.SUITES[curve].curve, None)]
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
    for form, submit in exports:
        want = g.run(ref, form, rnds, key_index)
        r = g.run(eng, form, rnds, key_index, key_octets, submit, want_keys=kst)
        same(r, want, (curve, form, submit))
        assert r.st[5] == UNKNOWN_KEY and [i for i in range(g.n) if r.st[i] != 1] == [5], r.st
    # the rows the job built are those of the stages bbs_selftest_key_len_rows runs, against the functions registration uses
    rows_host, st_host = eng.selftest_key_len_rows(key_octets, 0)
    rows_dev, st_dev = eng.selftest_key_len_rows(key_octets, 1)
    assert list(st_host) == list(st_dev) == kst
    assert rows_host == rows_dev
    ref.close()
    eng.close()


# ---- seeded random scalars -------------------------------------------------------------------------------------------------------
def check_seeded(curve, lib_path, exports=(("core", True), ("wire", False))):
    iss, owner, g, _ = small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks[:2]) + [jk.refused_octets(curve, -41)]
    key_index = np.array(owner, dtype=np.uint32)
    dst = iss.api_id + b"SEEDED_RANDOM_SCALARS_"
    on = lambda e: e.set_seeded_random_scalars(True, dst)
    ref, kst = jk.registered(iss, key_octets, on)
    eng = jk.bare(iss)
    on(eng)
    seeds = [b"seed-%d" % i * (1 + i % 3) for i in range(g.n)]
    for what, rnds in (("per-item seeds", seeds), ("job seed", bytes(range(32)))):
        for form, submit in exports:
            r = g.run(eng, form, rnds, key_index, key_octets, submit, want_keys=kst)
            same(r, g.run(ref, form, rnds, key_index), (curve, what, form))
            refused = [i for i in range(g.n) if owner[i] == 2]
            assert [i for i in range(g.n) if r.st[i] != 1] == refused and all(r.st[i] == UNKNOWN_KEY for i in refused)
            assert all(no_output(r, form, i, eng.fpb) for i in refused)
    ref.close()
    eng.close()


# ---- the job-local key cache -----------------------------------------------------------------------------------------------------
def counted(eng, fn):
    before = eng.job_key_cache_report()
    out = fn()
    after = eng.job_key_cache_report()
    return out, {k: after[k] - before[k] for k in jc.COUNTED}


def check_cache(curve, lib_path):
    iss, owner, g, rnds = small(curve, lib_path)
    key_octets = jk.octets_of(curve, iss.pks)
    key_index = np.array(owner, dtype=np.uint32)
    ref, kst = jk.registered(iss, key_octets)
    want = g.run(ref, "core", rnds, key_index)
    off = jk.bare(iss)
    same(g.run(off, "core", rnds, key_index, key_octets), want, (curve, "cache off"))
    eng = jc.cached(iss, 8)
    # job 1: three misses; job 2: three hits, the bytes of the cache-off call
    for hits, misses in ((0, 3), (3, 0)):
        r, d = counted(eng, lambda: g.run(eng, "core", rnds, key_index, key_octets, submit=True, want_keys=kst))
        assert (d["hits"], d["misses"], d["bypassed_jobs"]) == (hits, misses, 0), d
        assert r.rep == {"hits": hits, "misses": misses, "bypassed": 0}
        same(r, want, (curve, "cached", hits))
    # whole slots: what the proof_gen job published is the full entry, table included ...
    got_e, got_st, _ = eng.selftest_job_key_cache_entries(key_octets)
    want_e, want_st, _ = kr.key_entries(eng, 0, octets=key_octets)
    assert [int(x) for x in got_st] == [int(x) for x in want_st] == kst
    assert got_e == want_e
    # ... so a verify job with the same octets hits all three, with the statuses of the cache-off call
    b = jk.small_batch(curve, lib_path)[2]
    v_off = b.run(off, "pv", "core", key_index, key_octets)
    rv = jc.go(b, eng, "pv", "core", key_index, key_octets)
    jc.moved(rv, 3, 0)
    jk.same(rv.result, v_off, (curve, "verify after proof_gen"))
    assert sum(rv.result == 1) > 0
    eng.close()
    # the other direction: slots a verify job published serve a proof_gen job
    eng = jc.cached(iss, 8)
    jc.moved(jc.go(b, eng, "vf", "core", key_index, key_octets), 0, 3)
    r, d = counted(eng, lambda: g.run(eng, "wire", rnds, key_index, key_octets, submit=True, want_keys=kst))
    assert (d["hits"], d["misses"]) == (3, 0), d
    same(r, g.run(ref, "wire", rnds, key_index), (curve, "proof_gen after verify"))
    eng.close()
    # capacity 2, three keys: bypassed and counted, the twin's bytes (the uncached path: the domain-only stage)
    eng = jc.cached(iss, 2)
    r, d = counted(eng, lambda: g.run(eng, "core", rnds, key_index, key_octets, submit=True, want_keys=kst))
    assert (d["hits"], d["misses"], d["bypassed_jobs"]) == (0, 0, 1) and r.rep == {"hits": 0, "misses": 0, "bypassed": 1}
    same(r, want, (curve, "bypassed"))
    eng.close()
    # two jobs back to back with the same new keys: the second hits slots the first is still publishing
    eng = jc.cached(iss, 8)
    ja = g.start(eng, "core", rnds, key_index, key_octets, submit=True)
    jb = g.start(eng, "core", rnds, key_index, key_octets, submit=True)
    jb.wait()
    ja.wait()
    assert ja.key_cache_report() == {"hits": 0, "misses": 3, "bypassed": 0}
    assert jb.key_cache_report() == {"hits": 3, "misses": 0, "bypassed": 0}
    for j in (jb, ja):
        got = SimpleNamespace(st=[int(x) for x in j.result], out=tuple(x.tobytes() for x in j.raw))
        same(got, want, (curve, "back to back"))
        assert [int(x) for x in j.key_statuses()] == kst
        j.free()
    for e in (eng, off, ref):
        e.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def check_arguments(lib_path):
    from bbs_sign_amd import Engine
    curve = "bls12_381"
    iss, owner, g, rnds = small(curve, lib_path, K=1, n=1)
    eng = jk.bare(iss)
    n, keep, args = eng._pg_inputs(g.sigs, g.msgs, g.disclosed, rnds, g.headers, g.phs)
    short = eng._pg_inputs(g.sigs, g.msgs, g.disclosed, [rnds[0][:-1]], g.headers, g.phs)
    st = np.zeros(1, dtype=np.int8)
    pf = np.zeros(6 * eng.fpb + 128, dtype=np.uint8)
    cm = np.zeros(32 * iss.L, dtype=np.uint8)
    cmo = np.zeros(2, dtype=np.uint64)
    ki = np.zeros(1, dtype=np.uint32)
    pk = np.frombuffer(jk.octets_of(curve, iss.pks)[0], dtype=np.uint8).copy()
    job = ctypes.c_void_p()
    out = (pf.ctypes.data_as(_lib.c_u8p), cm.ctypes.data_as(_lib.c_u8p), cmo.ctypes.data_as(_lib.c_u64p), st.ctypes.data_as(_lib.c_i8p),
           ctypes.byref(job))
    kip, pkp = ki.ctypes.data_as(_lib.c_u32p), pk.ctypes.data_as(_lib.c_u8p)
    f = eng.lib.bbs_core_proof_gen_with_keys_submit
    assert f(eng.h, 1, 1, None, kip, *args, *out) == -100                  # NULL pk_octets with n_keys > 0
    assert f(eng.h, 1, 1, pkp, None, *args, *out) == -100                  # NULL key_index with n > 0
    assert f(eng.h, 1, 0xFFFFFFF1, pkp, kip, *args, *out) == -100          # n_keys > 0xFFFFFFF0
    assert f(eng.h, 1, 1, pkp, kip, *short[2], *out) == -100               # a wrong number of random scalars
    no_gens = Engine(curve, lib_path=lib_path, window_bits=4)
    assert no_gens.lib.bbs_core_proof_gen_with_keys_submit(no_gens.h, 1, 1, pkp, kip, *args, *out) == -102      # BBS_E_STATE
    assert f(eng.h, 1, 1, pkp, kip, *args, *out) == 0                      # and the call itself is fine
    j = _job_of(eng, job, 1)
    j.wait()
    assert int(st[0]) == 1
    j.free()
    no_gens.close()
    eng.close()


def _job_of(eng, handle, n):
    from bbs_sign_amd.engine import Job
    return Job(eng, handle, n)


# ---- the public layer ------------------------------------------------------------------------------------------------------------
def check_public_layer(curve, lib_path):
    """register_keys=False gives the entries of register_keys=True on a mixed list -- two issuers, two counts, one pk the library
    refuses -- and leaves the cached engine's key set and index as they were; key_cache=4 gives the same entries."""
    from bbs_sign_amd import api
    from bbs_sign_amd.api import PublicKey, SecretKey
    sks = [SecretKey(curve, 2000 + k, lib_path) for k in range(2)]
    pks = [sk.sk_to_pk() for sk in sks]
    bad = PublicKey(curve, kc.OFF_TWIST, lib_path)
    lists = [[b"a", b"b"], [b"c", b"d", b"e"], [b"f", b"g"], [b"h", b"i", b"j"], [b"k", b"l"]]
    rng = random.Random(5)
    r = bbs.SUITES[curve].curve.r
    items = []
    for i, m in enumerate(lists):
        hdr = b"hdr%d" % i
        sig = sks[i % 2].sign(m, hdr)
        items.append((pks[i % 2], sig, hdr, b"ph", m, [0], [rng.randrange(1, r) for _ in range(5 + len(m) - 1)]))
    items[4] = (bad,) + items[4][1:]
    want = api.proof_gen_many_issuers(items)
    ie = api._issuer_cache[(curve, 0, lib_path)]
    index, count = dict(ie.index), ie.eng.public_key_count()
    for kw in ({"register_keys": False}, {"register_keys": False, "key_cache": 4}, {"register_keys": False, "key_cache": 4}):
        got = api.proof_gen_many_issuers(items, **kw)
        assert [repr(x) for x in got] == [repr(w) for w in want], kw
        assert ie.index == index and ie.eng.public_key_count() == count
    assert isinstance(want[4], api.BbsError) and not any(isinstance(w, api.BbsError) for w in want[:4])
    rep = ie.eng.job_key_cache_report()
    assert rep["capacity"] == 4 and rep["hits"] >= 3
    for i in range(4):             # and the proofs are proofs
        assert api.proof_verify(pks[i % 2], want[i], items[i][2], b"ph", [lists[i][0]], [0]) is True
    ie.eng.set_job_key_cache(0)
