"""Verification under a job-local key set (bbs_*_with_keys_*): the keys arrive with the job as compressed octets, the job
prepares them on the device and releases them.  Shared by the host-twin tier (tests/test_job_keys_hosttwin.py) and the GPU
tier (tests/test_job_keys_gpu.py).

The rule that defines correctness: the statuses are, bit for bit, what the keyed twin returns on a context with the same
generators, api_id and switches whose key set was registered from the same octets (bbs_ctx_add_public_keys_octets), given the
same key_index and items.  The expected statuses therefore come from a SECOND engine, `registered()`; a few items are also
checked against the pure-Python oracle with the item's key."""
import numpy as np

import keyed_cases as kc
import keyreg_cases as kr
from oracle import bbs
from parity_cases import make_engine

UNKNOWN_KEY = kc.UNKNOWN_KEY


def octets_of(curve, keys):
    c = bbs.SUITES[curve].curve
    return [bbs.g2_compress(c, k) for k in keys]


def refused_octets(curve, code):
    """A string registration refuses with `code`: -40 an x >= p, -41 an x no point of the twist has."""
    octs, want, _ = kr.octet_cases(curve)
    c = bbs.SUITES[curve].curve
    if code == -41:
        return bbs.g2_compress(c, (kr.rootless_x(curve), (0, 0)))
    # (octet_cases: the string whose first coordinate on the wire is p)
    k = 5 if c.name == "bls12_381" else 4
    assert want[k] == -40
    return octs[k]


def bare(iss):
    """An engine with generators and NOTHING else: no public key, no key set."""
    return make_engine(iss.curve, iss.gens, iss.api_id, iss.lib_path, window_bits=iss.wb)


def registered(iss, key_octets, setup=None):
    """The engine of the rule: the same generators, api_id and switches, its key set registered from the same octets."""
    eng = bare(iss)
    if setup:
        setup(eng)
    _, st, _ = eng.add_public_keys_octets(list(key_octets))
    return eng, [int(x) for x in st]


class Batch:
    """One list of items and how it is presented: run(eng, op, form, ...) calls the keyed export (key_octets None) or the
    with_keys export of that operation and form, batch or submit."""

    def __init__(self, curve, raw, msgs, disclosed, sigs, proofs, headers, phs, proof_msgs=None, sig_msgs=None):
        self.curve, self.n = curve, len(sigs)
        self.raw, self.disclosed, self.sigs, self.proofs, self.headers, self.phs = raw, disclosed, sigs, proofs, headers, phs
        self.pm = msgs if proof_msgs is None else proof_msgs      # the messages the proofs disclose
        self.sm = msgs if sig_msgs is None else sig_msgs          # the messages the signatures are checked with
        # (a disclosed index out of range -- a malformed item -- discloses a zero message)
        self.dm = [[self.pm[i][j] if j < len(self.pm[i]) else 0 for j in disclosed[i]] for i in range(self.n)]

    def args(self, eng, op, form):
        if op == "pv":
            if form == "core":
                return (self.proofs, self.dm, self.disclosed, self.headers, self.phs)
            R = [[self.raw[i][j] if j < len(self.raw[i]) else b"" for j in self.disclosed[i]] for i in range(self.n)]
            return (eng.proofs_to_octets_batch(self.proofs), R, self.disclosed, self.headers, self.phs)
        if form == "core":
            return (self.sigs, self.sm, self.headers)
        return ([kc.sig_octets(self.curve, s) for s in self.sigs], self.raw, self.headers)

    def start(self, eng, op, form, key_index, key_octets=None, submit=False):
        name = {"pv": {"core": "core_proof_verify", "wire": "proof_verify_wire"},
                "vf": {"core": "core_verify", "wire": "verify_wire"}}[op][form]
        fn = getattr(eng, "%s_%s_%s" % (name, "keyed" if key_octets is None else "with_keys", "submit" if submit else "batch"))
        a = self.args(eng, op, form)
        return fn(key_index, *a) if key_octets is None else fn(list(key_octets), key_index, *a)

    def run(self, eng, op, form, key_index, key_octets=None, submit=False, want_keys=None):
        r = self.start(eng, op, form, key_index, key_octets, submit)
        if not submit:
            return np.array(r)
        r.wait()
        out = np.array(r.result)
        if want_keys is not None:
            assert list(r.key_statuses()) == list(want_keys)
        r.free()
        return out


EIGHT = tuple((op, form, submit) for op in ("pv", "vf") for form in ("core", "wire") for submit in (False, True))


def same(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))


# ---- the keyed test's shape: 24 items, five keys (three issuers, the identity encoding, one refused key) -----------------------
def five_keys(curve, lib_path, refused_code, L=4, R=2, window_bits=None):
    iss = kc.Issuers(curve, 3, L, lib_path, seed=41, window_bits=window_bits)
    key_octets = octets_of(curve, [iss.pks[0], iss.pks[1], None, iss.pks[2]]) + [refused_octets(curve, refused_code)]
    keys = [iss.pks[0], iss.pks[1], None, iss.pks[2], None]
    owner = [i % 3 for i in range(24)]
    to_key = {0: 0, 1: 1, 2: 3}
    key_index = [to_key[o] for o in owner]
    key_index[4] = 0           # a valid item of issuer 1 presented under issuer 0's key
    key_index[7] = 5           # index >= n_keys
    key_index[8] = 4           # the refused key
    key_index[9] = 2           # the identity key
    key_index[10] = 1000       # far out of range
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=3)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=6)
    bad_disclosed = [list(d) for d in disclosed]
    bad_disclosed[13] = [0, L + 3]       # one malformed item: a disclosed index out of range keeps its own code
    b = Batch(curve, raw, msgs, bad_disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)
    return iss, key_octets, keys, np.array(key_index, dtype=np.uint32), b


def check_five_keys(curve, lib_path, refused_code, exports=EIGHT, oracle=True, window_bits=None):
    iss, key_octets, keys, key_index, b = five_keys(curve, lib_path, refused_code, window_bits=window_bits)
    ref, kst = registered(iss, key_octets)
    assert kst == [1, 1, 1, 1, refused_code]
    eng = bare(iss)
    got = {}
    for op, form, submit in exports:
        want = b.run(ref, op, form, key_index)
        g = b.run(eng, op, form, key_index, key_octets, submit, want_keys=kst)
        same(g, want, (curve, op, form, submit))
        assert g[7] == g[8] == g[10] == UNKNOWN_KEY
        assert g[1] == 1 and g[0] == 0 and g[4] == 0, (op, form, list(g))
        if op == "pv":
            assert g[13] < 0 and g[13] != UNKNOWN_KEY
        got[(op, form)] = g
    assert eng.public_key_count() == 0
    if oracle:        # a few items against the oracle with that item's key
        suite = iss.suite
        if ("pv", "core") in got:
            for i in (1, 2, 4, 6):
                p = b.proofs[i]
                op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
                want = bbs.core_proof_verify(suite, keys[key_index[i]], op, iss.gens, b.headers[i], b.phs[i], b.dm[i], b.disclosed[i], iss.api_id)
                assert got[("pv", "core")][i] == int(want), (curve, i)
        if ("vf", "core") in got:
            for i in (1, 3, 4, 6):
                want = bbs.core_verify(suite, keys[key_index[i]], bbs.Signature(b.sigs[i].a, b.sigs[i].e), iss.gens, b.headers[i],
                                       b.sm[i], iss.api_id)
                assert got[("vf", "core")][i] == int(want), (curve, i)
    ref.close()
    eng.close()


# ---- pairing order: 10 / 11 / 9 items under three keys, interleaved; again with the 10-item key replaced by a refused one ------
def check_pairing_order(curve, lib_path, L=4, R=2, window_bits=None):
    iss = kc.Issuers(curve, 3, L, lib_path, seed=43, window_bits=window_bits)
    counts = [10, 11, 9]
    owner = [k for t in range(11) for k in range(3) if t < counts[k]]
    key_index = np.array(owner, dtype=np.uint32)
    key_index[12] = (owner[12] + 1) % 3                 # another issuer's key
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=5)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=7)
    b = Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)
    good = octets_of(curve, iss.pks)
    eng = bare(iss)
    for key_octets, code in ((good, 1), ([refused_octets(curve, -41)] + good[1:], -41)):
        ref, kst = registered(iss, key_octets)
        assert kst == [code, 1, 1]
        for op in ("pv", "vf"):
            want = b.run(ref, op, "core", key_index)
            got = b.run(eng, op, "core", key_index, key_octets, submit=True, want_keys=kst)
            same(got, want, (curve, op, code))
            if code != 1:      # a key-uniform wavefront whose key is refused: every one of its items, and nothing else
                assert [i for i in range(b.n) if got[i] == UNKNOWN_KEY] == [i for i in range(b.n) if key_index[i] == 0]
            else:
                assert sum(got == 1) == b.n - 1 - len(range(0, b.n, 7))
        ref.close()
    eng.close()


# ---- the same key twice, counts, no key state, run twice -----------------------------------------------------------------------
def small_batch(curve, lib_path, K=3, n=12, L=4, R=2, every=5, seed=47, window_bits=None):
    iss = kc.Issuers(curve, K, L, lib_path, seed=seed, window_bits=window_bits)
    owner = [i % K for i in range(n)]
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, R, seed=seed)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=every)
    return iss, owner, Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)


def check_key_twice(curve, lib_path):
    iss, owner, b = small_batch(curve, lib_path, K=2)
    o = octets_of(curve, iss.pks)
    key_octets = [o[0], o[1], o[0]]
    key_index = np.array([(2 if i % 4 == 0 else 0) if k == 0 else 1 for i, k in enumerate(owner)], dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    eng = bare(iss)
    for op in ("pv", "vf"):
        got = b.run(eng, op, "wire", key_index, key_octets, submit=True, want_keys=[1, 1, 1])
        same(got, b.run(ref, op, "wire", key_index), (curve, op))
        assert all(got[i] == (0 if i % 5 == 0 else 1) for i in range(b.n))
    ref.close()
    eng.close()


def check_counts(curve, lib_path):
    iss, owner, b = small_batch(curve, lib_path, K=1, n=4)
    eng = bare(iss)
    key_index = np.zeros(b.n, dtype=np.uint32)
    for op, form, submit in EIGHT:
        got = b.run(eng, op, form, key_index, [], submit, want_keys=[])      # n_keys = 0, n > 0
        same(got, [UNKNOWN_KEY] * b.n, (op, form, submit))
    o = octets_of(curve, iss.pks)
    assert list(eng.core_verify_with_keys_batch(o, [], [], [])) == []         # n = 0
    assert list(eng.proof_verify_wire_with_keys_batch(o, [], [], [], [])) == []
    assert list(eng.core_verify_with_keys_batch([], [], [], [])) == []
    eng.close()


def check_no_key_state(curve, lib_path):
    iss, owner, b = small_batch(curve, lib_path)
    key_octets = octets_of(curve, iss.pks[::-1])                 # the job's indexes are not the registered set's
    key_index = np.array([2 - k for k in owner], dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    want = {op: b.run(ref, op, "core", key_index) for op in ("pv", "vf")}
    # a context with NO public key and NO key set serves the call
    eng = bare(iss)
    for op in ("pv", "vf"):
        same(b.run(eng, op, "core", key_index, key_octets), want[op], (curve, op, "bare"))
    eng.close()
    # a context WITH a registered set serves it, and its set and the statuses of a keyed call are what they were
    eng = bare(iss)
    eng.set_public_keys(iss.pks)
    own_index = np.array(owner, dtype=np.uint32)
    before = {op: b.run(eng, op, "core", own_index) for op in ("pv", "vf")}
    for op in ("pv", "vf"):
        same(b.run(eng, op, "core", key_index, key_octets), want[op], (curve, op, "registered"))
    assert eng.public_key_count() == 3
    for op in ("pv", "vf"):
        same(b.run(eng, op, "core", own_index), before[op], (curve, op, "keyed call afterwards"))
    eng.close()
    ref.close()


def check_run_twice(curve, lib_path, window_bits=None):
    iss, owner, b = small_batch(curve, lib_path, window_bits=window_bits)
    key_octets = octets_of(curve, iss.pks[:2]) + [refused_octets(curve, -40)]
    key_index = np.array(owner, dtype=np.uint32)
    ref, kst = registered(iss, key_octets)
    assert kst == [1, 1, -40]
    eng = bare(iss)
    for op in ("pv", "vf"):
        want = b.run(ref, op, "core", key_index)
        job = b.start(eng, op, "core", key_index, key_octets, submit=True)
        job.wait()
        same(job.result, want, (curve, op, "first run"))
        assert list(job.key_statuses()) == kst
        job.run()
        job.wait()
        same(job.result, want, (curve, op, "second run"))
        assert list(job.key_statuses()) == kst
        job.free()
    ref.close()
    eng.close()


# ---- keyed mixed lengths: items of counts 0, 1, L - 1, L under three keys --------------------------------------------------------
def check_keyed_mixed(curve, lib_path, L=4, exports=EIGHT):
    import keyed_mixed_cases as kmc
    ring = kmc.Ring(curve, lib_path, L, K=3)
    lengths = [0, 1, L - 1, L] * 3
    owner = [(i // 4 + i) % 3 for i in range(len(lengths))]
    it = kmc.KItems(ring, owner, lengths, seed=7)
    key_octets = octets_of(curve, ring.keys[:3]) + [refused_octets(curve, -41), bbs.g2_compress(bbs.SUITES[curve].curve, None)]
    key_index = list(owner)
    key_index[5] = ring.REFUSED
    key_index[6] = ring.IDENTITY
    key_index[7] = (owner[7] + 1) % 3
    ref = ring.bare()
    ref.set_keyed_mixed_lengths(True)
    _, kst, _ = ref.add_public_keys_octets(key_octets)
    assert list(kst) == [1, 1, 1, -41, 1]
    eng = ring.bare()
    eng.set_keyed_mixed_lengths(True)
    b = Batch(curve, it.raw, it.msgs, it.disclosed, it.sigs, it.proofs, it.headers, it.phs)
    b.dm = it.dm
    b.args = lambda e, op, form: _mixed_args(kmc, it, e, op, form)
    for op, form, submit in exports:
        want = b.run(ref, op, form, key_index)
        got = b.run(eng, op, form, key_index, key_octets, submit, want_keys=list(kst))
        same(got, want, (curve, op, form, submit))
        assert got[5] == UNKNOWN_KEY and got[0] == 1 and got[3] == 1 and got[7] == 0, list(got)
    # the prefixes per (key, length): the job's stages against the functions registration uses, byte for byte
    rows_host, st_host = eng.selftest_key_len_rows(key_octets, 0)
    rows_dev, st_dev = eng.selftest_key_len_rows(key_octets, 1)
    assert list(st_host) == list(st_dev) == list(kst)
    assert rows_host == rows_dev
    assert len({r for k in (0, 1, 2, 4) for r in rows_host[k]}) == 4 * (L + 1)        # every accepted (key, length) its own prefix
    assert len(set(rows_host[3])) == 1                                              # a refused key: rows as they start out
    ref.close()
    eng.close()


def _mixed_args(kmc, it, eng, op, form):
    import mixed_len_cases as mc
    if op == "vf":
        if form == "core":
            return (it.sigs, it.msgs, it.headers)
        return ([mc.sig_octets(it.w, s) for s in it.sigs], it.raw, it.headers)
    if form == "core":
        return (it.proofs, it.dm, it.disclosed, it.headers, it.phs)
    return (eng.proofs_to_octets_batch(it.proofs), it.draw, it.disclosed, it.headers, it.phs)


# ---- keyed batch verification: min_items_per_key = 4; a key with a forged item, a clean key, a refused key (all items gated) ---
def check_keyed_bv(curve, lib_path, window_bits=None):
    iss = kc.Issuers(curve, 3, 4, lib_path, seed=53, window_bits=window_bits)
    owner = [i % 3 for i in range(18)]
    raw, msgs, disclosed, sigs, proofs, headers, phs = kc.make_items(iss, owner, 2, seed=9)
    raw, bad_proofs, bad_msgs = kc.corrupt(iss, raw, sigs, proofs, msgs, every=100)        # item 0 (key 0) forged, nothing else
    b = Batch(curve, raw, msgs, disclosed, sigs, bad_proofs, headers, phs, sig_msgs=bad_msgs)
    key_octets = octets_of(curve, iss.pks[:2]) + [refused_octets(curve, -41)]
    key_index = np.array(owner, dtype=np.uint32)
    seed = bytes(range(32))
    on = lambda e: e.set_keyed_batch_verification(True, seed, 4)
    ref, kst = registered(iss, key_octets, on)
    assert kst == [1, 1, -41]
    eng_on, eng_off = bare(iss), bare(iss)
    on(eng_on)
    for op in ("pv", "vf"):
        off = b.run(eng_off, op, "core", key_index, key_octets)
        jr = b.start(ref, op, "core", key_index, submit=True)
        jr.wait()
        job = b.start(eng_on, op, "core", key_index, key_octets, submit=True)
        job.wait()
        same(job.result, off, (curve, op, "switch on against switch off"))
        same(job.result, jr.result, (curve, op, "against the keyed twin"))
        assert list(job.result) == [0] + [1, UNKNOWN_KEY, 1] * 5 + [1, UNKNOWN_KEY]
        # (a forged proof fails its challenge and never reaches the combination: both groups pass; a forged signature fails
        # the pairing: its key's group fails and its items get their own products)
        assert jr.bv_report() == (2, 2 if op == "pv" else 1, 12)
        assert job.bv_report() == jr.bv_report()
        assert list(job.key_statuses()) == kst
        v = job.bv_verdicts()              # 16 per group the host planned: keys 0 and 1, and the refused key's
        assert len(v) == 48 and list(v[16:32]) == [1] * 16 and (0 in list(v[:16])) == (op == "vf")
        jr.free()
        job.free()
    for e in (ref, eng_on, eng_off):
        e.close()


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def check_arguments(lib_path):
    import ctypes
    from bbs_sign_amd import Engine, _lib
    curve = "bls12_381"
    iss = kc.Issuers(curve, 1, 4, lib_path, seed=5)
    st = np.zeros(1, dtype=np.int8)
    off = np.zeros(2, dtype=np.uint64)
    sig = np.zeros(200, dtype=np.uint8)
    ki = np.zeros(1, dtype=np.uint32)
    pk = np.frombuffer(octets_of(curve, iss.pks)[0], dtype=np.uint8).copy()
    job = ctypes.c_void_p()
    args = (sig.ctypes.data_as(_lib.c_u8p), None, off.ctypes.data_as(_lib.c_u64p), None, off.ctypes.data_as(_lib.c_u64p),
            st.ctypes.data_as(_lib.c_i8p), ctypes.byref(job))
    kip, pkp = ki.ctypes.data_as(_lib.c_u32p), pk.ctypes.data_as(_lib.c_u8p)
    no_gens = Engine(curve, lib_path=lib_path, window_bits=4)
    assert no_gens.lib.bbs_core_verify_with_keys_submit(no_gens.h, 1, 1, pkp, kip, *args) == -102     # BBS_E_STATE: no generators
    eng = bare(iss)
    f = eng.lib.bbs_core_verify_with_keys_submit
    assert f(eng.h, 1, 1, None, kip, *args) == -100                  # NULL pk_octets with n_keys > 0
    assert f(eng.h, 1, 1, pkp, None, *args) == -100                  # NULL key_index with n > 0
    assert f(eng.h, 1, 0xFFFFFFF1, pkp, kip, *args) == -100          # n_keys > 0xFFFFFFF0
    eng.set_mixed_lengths(True)                                      # the single-key switch alone: as the keyed twins
    assert f(eng.h, 1, 1, pkp, kip, *args) == -102
    eng.set_mixed_lengths(False)
    # bbs_job_key_statuses: BBS_E_STATE for a job without a key set of its own
    eng.set_public_keys(iss.pks)
    j = eng.core_verify_keyed_submit([], [], [])
    j.wait()
    cnt = ctypes.c_size_t(0)
    out = np.zeros(4, dtype=np.int8)
    assert eng.lib.bbs_job_key_statuses(j.h, out.ctypes.data_as(_lib.c_i8p), 4, ctypes.byref(cnt)) == -102
    j.free()
    no_gens.close()
    eng.close()
