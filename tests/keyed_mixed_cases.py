"""Keyed jobs of mixed message counts (bbs_ctx_set_keyed_mixed_lengths).  Shared by the host-twin tier
(tests/test_keyed_mixed_hosttwin.py) and the GPU tier (tests/test_keyed_mixed_gpu.py).

The rule that defines correctness: item i, presented under key k_i with its own count l_i, gets bit for bit the status a
single-key context made with generators[0 .. l_i] and key k_i gives that item alone; an unknown index or a refused key gives
BBS_ST_UNKNOWN_KEY whatever else is wrong with the item.

Expected values: mixed_len_cases.expect_pv / expect_vf (the reference's order of the structural codes, the plain-C oracle
with (pk_{k_i}, gens[: l_i + 1]) for the verdicts) looked at through the world of the PRESENTED key; second witness:
fixed-length single-key contexts of the same library; a handful of items through the pure-Python oracle.

Worlds with different seeds share generators and differ in key: a Ring is K of them plus one refused key (off the twist)
and the identity key, registered behind the valid ones."""
import copy
import functools
import random

import numpy as np

import mixed_len_cases as mc
from keyed_cases import OFF_TWIST, UNKNOWN_KEY
from mixed_len_cases import Items, World, same
from oracle import bbs
from parity_cases import gens_for, make_engine

HASHCTX_BYTES = 32 + 8 + 64 + 4 + 256 + 4            # HashCtx of stages_common.hpp: 368, no padding


@functools.lru_cache(maxsize=None)
def shared_gens(curve, count):
    """The generators World would make (they do not depend on the key or the api_id of the world): made once per session."""
    return tuple(gens_for(bbs.SUITES[curve], count))


class Ring:
    """K valid keys (worlds 0 .. K - 1, the same generators and api_id), then the refused key, then the identity key."""

    def __init__(self, curve, lib_path, L, K=3, api_id=None, seed=21):
        self.curve, self.lib_path, self.L, self.K = curve, lib_path, L, K
        w0 = World(curve, lib_path, L, seed=seed, api_id=api_id, gens=list(shared_gens(curve, L + 1)))
        self.worlds = [w0] + [World(curve, lib_path, L, seed=seed + k, api_id=w0.api_id, gens=w0.gens) for k in range(1, K)]
        assert len({w.pk for w in self.worlds}) == K
        self.keys = [w.pk for w in self.worlds] + [OFF_TWIST, None]
        self.REFUSED, self.IDENTITY = K, K + 1
        self.key_status = [1] * K + [-41, 1]
        self.gens, self.api_id = w0.gens, w0.api_id

    def bare(self):
        return make_engine(self.curve, self.gens, self.api_id, self.lib_path)

    def engine(self, on=True):
        eng = self.bare()
        if on:
            eng.set_keyed_mixed_lengths(True)
        assert list(eng.set_public_keys(self.keys)) == self.key_status
        return eng

    def identity_world(self):
        w = copy.copy(self.worlds[0])
        w.pk = None
        return w


class KItems(Items):
    """Items of several issuers in one list: item i was signed (and proved) by world owner[i] with lengths[i] messages.  The
    fields are those of mixed_len_cases.Items, so plant(), copy() and run() of that module take it as it is."""

    def __init__(self, ring, owner, lengths, seed=3, disclosed=None, headers=None):
        n = len(owner)
        self.ring, self.w, self.n = ring, ring.worlds[0], n
        self.owner, self.lengths = list(owner), list(lengths)
        self.forced = {}
        fields = ("raw", "msgs", "headers", "phs", "disclosed", "sigs", "proofs", "dm", "draw")
        for f in fields:
            setattr(self, f, [None] * n)
        for k in sorted(set(owner)):
            idx = [i for i in range(n) if owner[i] == k]
            part = Items(ring.worlds[k], [lengths[i] for i in idx], seed=seed + k,
                         disclosed=None if disclosed is None else [disclosed[i] for i in idx],
                         headers=None if headers is None else [headers[i] for i in idx])
            for f in fields:
                for t, i in enumerate(idx):
                    getattr(self, f)[i] = getattr(part, f)[t]


def under(it, world):
    """The same list looked at by the expectation functions of mixed_len_cases with `world`'s key (it: a KItems or the Items
    its copy() returns)."""
    v = copy.copy(it)
    v.w = world
    return v


def expected(ring, it, op, key_index, L, base=None, changed=None):
    """Statuses of the rule.  The identity key's items are left to the single-key witness (identity_witness): None here."""
    f = mc.expect_pv if op == "pv" else mc.expect_vf
    views = [under(it, w) for w in ring.worlds]
    out = [None] * it.n if base is None else list(base)
    for i in (range(it.n) if changed is None else changed):
        k = int(key_index[i])
        if k >= len(ring.keys) or ring.key_status[k] != 1:
            out[i] = UNKNOWN_KEY
        elif k == ring.IDENTITY:
            out[i] = None
        else:
            out[i] = f(views[k], i, L)
    return out


def identity_witness(ring, it, op, idx):
    """What a single-key context with the identity key (mixed lengths on) gives the items idx."""
    w = ring.identity_world()
    eng = w.mixed()
    got = mc.run(eng, it, op, "core", list(idx))
    eng.close()
    return [int(x) for x in got]


def run_keyed(eng, it, op, key_index, form="core", submit=False, idx=None):
    idx = list(range(it.n)) if idx is None else idx
    ki = np.asarray([key_index[i] for i in idx], dtype=np.uint32)
    H = [it.headers[i] for i in idx]
    if op == "vf":
        S, M = [it.sigs[i] for i in idx], [it.msgs[i] for i in idx]
        if form == "core":
            r = eng.core_verify_keyed_submit(ki, S, M, H) if submit else eng.core_verify_keyed_batch(ki, S, M, H)
        else:
            octs, R = [mc.sig_octets(it.w, s) for s in S], [it.raw[i] for i in idx]
            r = eng.verify_wire_keyed_submit(ki, octs, R, H) if submit else eng.verify_wire_keyed_batch(ki, octs, R, H)
    else:
        P, D, X, Ph = [it.proofs[i] for i in idx], [it.dm[i] for i in idx], [it.disclosed[i] for i in idx], [it.phs[i] for i in idx]
        if form == "core":
            r = eng.core_proof_verify_keyed_submit(ki, P, D, X, H, Ph) if submit else eng.core_proof_verify_keyed_batch(ki, P, D, X, H, Ph)
        else:
            octs, R = eng.proofs_to_octets_batch(P), [it.draw[i] for i in idx]
            r = eng.proof_verify_wire_keyed_submit(ki, octs, R, X, H, Ph) if submit else eng.proof_verify_wire_keyed_batch(ki, octs, R, X, H, Ph)
    if not submit:
        return r
    r.wait()
    out = np.array(r.result)
    r.free()
    return out


EIGHT = tuple((op, form, submit) for op in ("pv", "vf") for form in ("core", "wire") for submit in (False, True))


# ---- case 1: the export -----------------------------------------------------------------------------------------------------
def check_export(lib_path):
    from bbs_sign_amd import _lib
    lib = _lib.load_library(lib_path)
    assert "bbs_ctx_set_keyed_mixed_lengths" in _lib.SIGNATURES and hasattr(lib, "bbs_ctx_set_keyed_mixed_lengths")
    assert lib.bbs_ctx_set_keyed_mixed_lengths(None, 1) == -100        # BBS_E_ARG


# ---- case 2: every (key, length) ------------------------------------------------------------------------------------------
def check_every_key_and_length(curve, lib_path=None, n=130, L=33, K=3, exports=EIGHT, python_sample=(), all_pairs=True):
    ring = Ring(curve, lib_path, L, K)
    owner = [i % K for i in range(n)]
    lengths = [i % (L + 1) for i in range(n)]
    if all_pairs:
        assert len(set(zip(owner, lengths))) == K * (L + 1)
        assert all(owner.count(k) >= 10 for k in range(K))            # key-uniform and mixed pairing wavefronts
    it = KItems(ring, owner, lengths)
    if n >= 66:
        assert any(any(j >= 32 for j in d) for d in it.disclosed) and any(d == [] for d in it.disclosed)
    eng = ring.engine()
    want = {op: expected(ring, it, op, owner, L) for op in ("pv", "vf")}
    for op, form, submit in exports:
        assert want[op] == [1] * n, (curve, op, want[op])
        same(run_keyed(eng, it, op, owner, form, submit), want[op], (curve, op, form, "submit" if submit else "batch"))
    eng.close()
    for op in sorted({e[0] for e in exports}):
        # second witness: every key's items through fixed-length single-key contexts of that key
        for k in range(K):
            idx = [i for i in range(n) if owner[i] == k]
            part = copy.copy(under(it, ring.worlds[k]))
            for f in ("raw", "msgs", "headers", "phs", "disclosed", "sigs", "proofs", "dm", "draw", "lengths"):
                setattr(part, f, [getattr(it, f)[i] for i in idx])
            part.n = len(idx)
            same(mc.witness_fixed(part, op), [1] * len(idx), (curve, op, "fixed-length contexts of key", k))
        for i in python_sample:
            mc.check_python_oracle_sample(under(it, ring.worlds[owner[i]]), op, [i], want[op])


# ---- cases 3 and 4: the prefix is the item's own key's and own length's; structural codes per item ------------------------
@functools.lru_cache(maxsize=4)
def defect_base(curve, lib_path, n, L, K, positions):
    ring = Ring(curve, lib_path, L, K)
    owner = [i % K for i in range(n)]
    lengths = [3 + (i * 7) % (L - 3) for i in range(n)]                  # 3 .. L - 1: every defect fits every position
    rng = random.Random(9)
    disclosed = [[0] if i in positions else mc.disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
    it = KItems(ring, owner, lengths, disclosed=disclosed)
    base = {op: expected(ring, it, op, owner, L) for op in ("pv", "vf")}
    assert base["pv"] == base["vf"] == [1] * n
    return ring, owner, it, base


def check_own_key_and_length(curve, lib_path=None, n=130, L=33, K=3, positions=(0, 63, 64, 129)):
    ring, owner, base_it, base = defect_base(curve, lib_path, n, L, K, tuple(positions))
    eng = ring.engine()
    # the same items under the next valid key: every one is false, none an error
    rotated = [(k + 1) % K for k in owner]
    for op in ("pv", "vf"):
        want = expected(ring, base_it, op, rotated, L)
        assert want == [0] * n, (curve, op, want)
        same(run_keyed(eng, base_it, op, rotated), want, (curve, op, "rotated keys"))
    # one message (verify) / one commitment (proof_verify) fewer: decided under l - 1, false
    for op in ("pv", "vf"):
        it = base_it.copy()
        for p in positions:
            assert mc.plant(it, p, "minus_one", op), p
        want = expected(ring, it, op, owner, L, base[op], positions)
        assert all(want[p] == 0 for p in positions)
        for form in ("core", "wire"):
            same(run_keyed(eng, it, op, owner, form), want, (curve, op, form, "presented with l - 1"))
        # second witness: a single-key context of the item's key and PRESENTED length
        p = positions[1]
        count = len(it.proofs[p].commitments) + len(it.disclosed[p]) if op == "pv" else len(it.msgs[p])
        f = ring.worlds[owner[p]].fixed(count)
        same(mc.run(f, it, op, "core", [p]), [0], (curve, op, "fixed-length context", p))
        f.close()
    eng.close()


def check_structural_codes(curve, lib_path=None, n=130, L=33, K=3, positions=(0, 63, 64, 129), wire=False, python_sample=False):
    ring, owner, base_it, base = defect_base(curve, lib_path, n, L, K, tuple(positions))
    eng = ring.engine()
    for op, defects in (("pv", mc.PV_DEFECTS), ("vf", mc.VF_DEFECTS)):
        for kind, code in defects:
            if kind == "minus_one":
                continue                                   # check_own_key_and_length
            it = base_it.copy()
            for p in positions:
                assert mc.plant(it, p, kind, op), (kind, p)
            want = expected(ring, it, op, owner, L, base[op], positions)
            assert all(want[p] == code for p in positions), (op, kind, [want[p] for p in positions])
            forms = ("core", "wire") if wire and kind not in ("noncanonical", "off_curve") else ("core",)
            for form in forms:
                same(run_keyed(eng, it, op, owner, form), want, (curve, op, kind, form))
            if python_sample and kind in ("index_eq_l", "messages_ne_indexes", "forged"):
                p = positions[0]
                mc.check_python_oracle_sample(under(it, ring.worlds[owner[p]]), op, [p], want)
        # l = L + 1 (-1), keys that are not there (outside the set, the refused key), both at once (the key decides), and
        # the identity key
        it = base_it.copy()
        p_long, p_out, p_ref, p_both, p_id = positions[0], positions[1], positions[2], positions[3], 1
        for p in (p_long, p_both):
            l = it.lengths[p]
            if op == "pv":
                it.proofs[p].commitments.extend([7] * (L + 1 - l))
            else:
                it.msgs[p].extend([5] * (L + 1 - l)); it.raw[p].extend([b"extra"] * (L + 1 - l))
        key_index = list(owner)
        key_index[p_out], key_index[p_ref], key_index[p_both], key_index[p_id] = 1000, ring.REFUSED, len(ring.keys), ring.IDENTITY
        changed = (p_long, p_out, p_ref, p_both, p_id)
        want = expected(ring, it, op, key_index, L, base[op], changed)
        assert (want[p_long], want[p_out], want[p_ref], want[p_both]) == (-1, UNKNOWN_KEY, UNKNOWN_KEY, UNKNOWN_KEY)
        want[p_id] = identity_witness(ring, it, op, [p_id])[0]
        for form in ("core", "wire") if wire else ("core",):
            same(run_keyed(eng, it, op, key_index, form), want, (curve, op, "-1 and unknown keys", form))
    eng.close()


# ---- case 5: stale buffers --------------------------------------------------------------------------------------------------
def check_stale_buffers(curve, lib_path=None, n=130, L=33, K=3):
    ring = Ring(curve, lib_path, L, K)
    owner = [i % K for i in range(n)]
    full = KItems(ring, owner, [L] * n, seed=5)
    short = KItems(ring, owner, [(0, 1, L - 1)[(i // K) % 3] for i in range(n)], seed=6)
    eng = ring.engine()
    for op in ("pv", "vf"):
        want = expected(ring, short, op, owner, L)
        assert want == [1] * n
        same(run_keyed(eng, full, op, owner), [1] * n, (curve, op, "full"))
        same(run_keyed(eng, short, op, owner), want, (curve, op, "short after full"))
        same(run_keyed(eng, full, op, owner), [1] * n, (curve, op, "full again"))
    eng.close()


# ---- cases 6 and 7: order of set-up; a job keeps what it was created with ---------------------------------------------------
def small_list(curve, lib_path, L, K, n=None):
    ring = Ring(curve, lib_path, L, K)
    n = n or 2 * K * 2
    owner = [i % K for i in range(n)]
    lengths = [(i * 5 + i // K) % (L + 1) for i in range(n)]
    it = KItems(ring, owner, lengths)
    it.proofs[2].e_cap = (it.proofs[2].e_cap + 1) % ring.worlds[0].c.r           # one forged item
    it.sigs[2] = type(it.sigs[2])(it.sigs[2].a, (it.sigs[2].e + 1) % ring.worlds[0].c.r)
    return ring, owner, it


def key_octets(ring, pk):
    from bbs_sign_amd import api
    return api.public_key_to_octets(api.PublicKey(ring.curve, pk, ring.lib_path))


def check_order_of_setup(curve, lib_path=None, L=6):
    K = 4
    ring, owner, it = small_list(curve, lib_path, L, K)
    assert set(owner) == set(range(K)) and len(set(it.lengths)) >= 4
    keys = ring.keys[:K]
    want = {op: expected(ring, it, op, owner, L) for op in ("pv", "vf")}
    assert want["pv"] == want["vf"] == [0 if i == 2 else 1 for i in range(it.n)]

    def route(r):
        eng = ring.bare()
        if r in (1, 3, 4):
            eng.set_keyed_mixed_lengths(True)
        if r in (1, 2):
            assert list(eng.set_public_keys(keys)) == [1] * K
        if r == 2:
            eng.set_keyed_mixed_lengths(True)
        if r in (3, 4):
            assert list(eng.set_public_keys(keys[:2])) == [1, 1]
            if r == 4:
                eng.set_keyed_mixed_lengths(False)
                eng.set_keyed_mixed_lengths(True)
            first, st, _ = eng.add_public_keys_octets([key_octets(ring, pk) for pk in keys[2:]])
            assert first == 2 and list(st) == [1, 1]
        return eng
    for r in (1, 2, 3, 4):
        eng = route(r)
        for op in ("pv", "vf"):
            same(run_keyed(eng, it, op, owner), want[op], (curve, op, "route", r))
        if r == 4:
            # other generators: the key set is gone, every index is unknown
            other = bbs.synthetic_generators(ring.worlds[0].suite, L + 1, b"keyed-mixed-other-generators")
            eng.set_generators(other, ring.api_id)
            assert eng.public_key_count() == 0
            for op in ("pv", "vf"):
                same(run_keyed(eng, it, op, owner), [UNKNOWN_KEY] * it.n, (curve, op, "after set_generators"))
        eng.close()


def check_job_keeps_what_it_was_created_with(curve, lib_path=None, L=6):
    import pytest
    K = 3
    ring, owner, it = small_list(curve, lib_path, L, K)
    want = {op: expected(ring, it, op, owner, L) for op in ("pv", "vf")}
    eng = ring.bare()
    eng.set_keyed_mixed_lengths(True)
    eng.set_public_keys(ring.keys[:K])
    P, D, X = it.proofs, it.dm, it.disclosed
    held = eng.core_proof_verify_keyed_submit(np.asarray(owner, dtype=np.uint32), P, D, X, it.headers, it.phs)
    held_v = eng.core_verify_keyed_submit(np.asarray(owner, dtype=np.uint32), it.sigs, it.msgs, it.headers)
    eng.add_public_keys([ring.worlds[0].pk])           # a new set and new rows: the jobs hold the old ones
    eng.set_keyed_mixed_lengths(False)                 # the context lets go of the rows
    eng.set_public_keys(ring.keys[:K][::-1])           # and of the set
    for job, op in ((held, "pv"), (held_v, "vf")):
        job.wait()
        same(job.result, want[op], (curve, op, "held job"))
        job.run()                                      # again, from the prefixes and keys only the job still holds
        same(job.status(), want[op], (curve, op, "held job, second run"))
        job.free()
    eng.set_public_keys(ring.keys[:K])
    # the new switch off, the single-key switch on: BBS_E_STATE, as before
    eng.set_mixed_lengths(True)
    for op in ("pv", "vf"):
        with pytest.raises(Exception, match="BBS_E_STATE"):
            run_keyed(eng, it, op, owner)
    # both on: the keyed jobs take mixed counts whatever the single-key switch says
    eng.set_keyed_mixed_lengths(True)
    for op in ("pv", "vf"):
        same(run_keyed(eng, it, op, owner), want[op], (curve, op, "both switches on"))
    # both off: a keyed job is a fixed-length one
    eng.set_keyed_mixed_lengths(False)
    eng.set_mixed_lengths(False)
    fixed = [want["pv"][i] if it.lengths[i] == L else -1 for i in range(it.n)]
    assert 1 in fixed and -1 in fixed
    for op in ("pv", "vf"):
        same(run_keyed(eng, it, op, owner), fixed, (curve, op, "both switches off"))
    # single-key jobs never look at the new switch
    eng.set_keyed_mixed_lengths(True)
    eng.set_public_key(ring.worlds[0].pk)
    mine = [i for i in range(it.n) if owner[i] == 0]
    same(mc.run(eng, it, "pv", "core", mine), [(0 if i == 2 else 1) if it.lengths[i] == L else -1 for i in mine], (curve, "single-key job"))
    eng.close()


# ---- case 8: prefix boundaries ----------------------------------------------------------------------------------------------
BOUNDARY_ENDS = (0, 1, 55, 56, 63)
# api_id lengths m for which the domain prefix of SOME length l <= 8 ends 55, 56, 63, 0 and 1 bytes into a SHA-256 block
# (prefix_bytes: 216 + 48 l + m on BLS12-381, 168 + 32 l + m on BN254; both hit these ends at l = 0, 4, 8 -- BN254 at every even l)
BOUNDARY_API_ID_LENS = {"bls12_381": (31, 32, 39, 40, 41), "bn254": (15, 16, 23, 24, 25)}


def check_prefix_boundaries(curve, lib_path=None, which=0, L=8):
    """check_prefix_boundaries of mixed_len_cases per key, K = 2: api_id number `which` of BOUNDARY_API_ID_LENS[curve] (one per
    test case, so that a case stays short).  Together the five put the end of the domain prefix 0, 1, 55, 56 and 63 bytes into
    a SHA-256 block for some length (asserted, for the whole set and for this api_id's own end); every length 0 .. L occurs
    under both keys with headers of 0, 55, 56 and 64 bytes."""
    lens = BOUNDARY_API_ID_LENS[curve]
    K = 2
    hl = (0, 55, 56, 64)
    ends = {m: {mc.prefix_bytes(curve, l, m) % 64 for l in range(L + 1)} for m in lens}
    assert set(BOUNDARY_ENDS) <= set().union(*ends.values()), ends
    m = lens[which]
    assert sorted(BOUNDARY_ENDS)[(which + 2) % 5] in ends[m], (m, ends[m])        # lens is ordered 55, 56, 63, 0, 1
    aid = bytes(65 + k % 26 for k in range(m))
    ring = Ring(curve, lib_path, L, K, api_id=aid)
    lengths = [l for l in range(L + 1) for _ in hl for _ in range(K)]
    owner = [k for l in range(L + 1) for _ in hl for k in range(K)]
    it = KItems(ring, owner, lengths, headers=[bytes([7 + l]) * h for l in range(L + 1) for h in hl for _ in range(K)])
    eng = ring.engine()
    for op in ("pv", "vf"):
        want = expected(ring, it, op, owner, L)
        assert want == [1] * it.n, (curve, m, want)
        same(run_keyed(eng, it, op, owner), want, (curve, op, m))
    eng.close()


# ---- case 9: table bytes ----------------------------------------------------------------------------------------------------
def check_table_bytes(curve, lib_path=None, L=7):
    """One row of L + 1 prefixes per key of the set, refused keys included, while the switch is on."""
    ring = Ring(curve, lib_path, L, 3)
    tb = lambda e: int(e.lib.bbs_ctx_table_bytes(e.h))
    eng = ring.bare()
    off = tb(eng)
    eng.set_public_keys(ring.keys)
    nk = len(ring.keys)
    assert tb(eng) == off                                  # (the key set itself was never counted)
    eng.set_keyed_mixed_lengths(True)
    assert tb(eng) == off + nk * (L + 1) * HASHCTX_BYTES, (tb(eng), off)
    eng.add_public_keys([ring.worlds[0].pk, OFF_TWIST])
    assert tb(eng) == off + (nk + 2) * (L + 1) * HASHCTX_BYTES
    eng.set_mixed_lengths(True)                            # the single-key switch counts its own L + 1 only with a key
    assert tb(eng) == off + (nk + 2) * (L + 1) * HASHCTX_BYTES
    eng.set_mixed_lengths(False)
    eng.set_keyed_mixed_lengths(False)
    assert tb(eng) == off
    eng.set_keyed_mixed_lengths(True)
    eng.set_public_keys([])
    assert tb(eng) == off
    eng.set_public_keys(ring.keys[:2])
    assert tb(eng) == off + 2 * (L + 1) * HASHCTX_BYTES
    eng.set_generators(ring.gens[:4], ring.api_id)         # the set is dropped with the generators
    assert tb(eng) == tb_of(ring, 3)
    eng.close()


def tb_of(ring, L):
    e = make_engine(ring.curve, ring.gens[:L + 1], ring.api_id, ring.lib_path)
    t = int(e.lib.bbs_ctx_table_bytes(e.h))
    e.close()
    return t


# ---- case 10: the public layer ----------------------------------------------------------------------------------------------
def check_public_layer(curve, lib_path=None):
    from bbs_sign_amd import BbsError, Signature, api
    suite = bbs.SUITES[curve]
    rng = random.Random(99)
    sks = [api.SecretKey(curve, rng.randrange(1, suite.curve.r), lib_path) for _ in range(3)]
    pks = [sk.sk_to_pk() for sk in sks]
    lengths = [0, 1, 2, 3, 4, 5, 6, 2, 3]
    n = len(lengths)
    who = [i % 3 for i in range(n)]
    msgs = [[b"issuers-%d-%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    headers = [b"h%d" % i for i in range(n)]
    sigs = [sks[who[i]].sign(msgs[i], headers[i]) for i in range(n)]
    vitems = [(pks[who[i]], sigs[i], headers[i], msgs[i]) for i in range(n)]
    vitems[7] = (pks[(who[7] + 1) % 3], sigs[7], headers[7], msgs[7])                      # another issuer's key: false
    vitems[8] = (pks[who[8]], Signature(sigs[8].a, suite.curve.r), headers[8], msgs[8])   # e = r: cannot be written as octets
    disclosed = [sorted(rng.sample(range(l), l // 2)) for l in lengths]
    proofs = [api.proof_gen(pks[who[i]], sigs[i], headers[i], b"ph", msgs[i], disclosed[i]) for i in range(n)]
    pitems = [(pks[who[i]], proofs[i], headers[i], b"ph", [msgs[i][j] for j in disclosed[i]], disclosed[i]) for i in range(n)]
    pitems[7] = (pks[(who[7] + 1) % 3],) + pitems[7][1:]
    bad = copy.copy(proofs[8])
    bad.e_cap = suite.curve.r                                                              # not a canonical scalar: no octets
    pitems[8] = (pks[who[8]], bad) + pitems[8][2:]

    def one(f, *a):
        try:
            return f(*a)
        except BbsError as e:
            return e

    def check(many, single, items):
        got = many(items)
        for i, item in enumerate(items):
            want = one(single, *item)
            if isinstance(want, BbsError):
                assert isinstance(got[i], BbsError) and got[i].status == want.status, (curve, i, got[i], want)
            else:
                assert got[i] is want, (curve, i, got[i], want)
        if len(items) == n:
            assert [g is True for g in got[:7]] == [True] * 7 and got[7] is False and isinstance(got[8], BbsError), got
        else:
            assert all(g is True for g in got), got
    v_single = lambda pk, *a: pk.verify(*a)
    p_single = lambda pk, *a: api.proof_verify(pk, *a)
    check(api.verify_many_issuers, v_single, vitems)
    check(api.proof_verify_many_issuers, p_single, pitems)
    assert api.verify_many_issuers([]) == [] and api.proof_verify_many_issuers([]) == []
    ie = api._issuer_cache[(curve, 0, lib_path)]
    assert ie.L == 6 and ie.eng.public_key_count() == 3
    check(api.verify_many_issuers, v_single, vitems[:4])
    assert api._issuer_cache[(curve, 0, lib_path)] is ie and ie.eng.public_key_count() == 3      # a key is registered once
    # a longer item: the engine is rebuilt with its keys, and still answers the first list
    long_msgs = [b"long-%d" % j for j in range(8)]
    long_item = (pks[1], sks[1].sign(long_msgs, b"hl"), b"hl", long_msgs)
    assert api.verify_many_issuers([long_item]) == [True]
    ie8 = api._issuer_cache[(curve, 0, lib_path)]
    assert ie8 is not ie and ie8.L == 8 and ie8.eng.public_key_count() == 3
    check(api.verify_many_issuers, v_single, vitems)
    check(api.proof_verify_many_issuers, p_single, pitems)
    assert api._issuer_cache[(curve, 0, lib_path)] is ie8 and ie8.eng.public_key_count() == 3
    # a key the library refuses (the documented divergence from the one-item form): its item is BBS_ST_UNKNOWN_KEY, the others
    # stand; the refused key takes an index of its own
    off = api.PublicKey(curve, OFF_TWIST, lib_path)
    got = api.verify_many_issuers([vitems[1], (off,) + vitems[2][1:], vitems[3]])
    assert got[0] is True and got[2] is True and isinstance(got[1], BbsError) and got[1].status == UNKNOWN_KEY, got
    assert ie8.eng.public_key_count() == 4
    api.clear_caches()
    assert not api._issuer_cache


# ---- case 11: the reference's vectors ---------------------------------------------------------------------------------------
def check_reference_vectors(lib_path=None, L=5):
    """The reference's signature and proof vectors (one message: src/tests/test_vector.rs:163-260, the bytes
    mixed_len_cases.check_reference_vectors_on_longer_context uses) through the keyed path of a context made for L messages,
    the vector's key at index 1 behind a decoy."""
    from bbs_sign_amd import api
    curve = "bls12_381"
    H = bytes.fromhex
    pk = api.octets_to_public_key(curve, H(
        "a820f230f6ae38503b86c70dc50b61c58a77e45c39ab25c0652bbaa8fa136f2851bd4781c9dcde39fc9d1d52c9e60268"
        "061e7d7632171d91aa8d460acee0e96f1e7c4cfb12d3ff9ab5d5dc91c277db75c845d649ef3c4f63aebc364cd55ded0c"), lib_path)
    m1 = H("9872ad089e452c7b6e283dfac2a80d58e8d0ff71cc4d5e310a1debdda4a45f02")
    header = H("11223344556677889900aabbccddeeff")
    ph = H("bed231d880675ed101ead304512e043ade9958dd0241ea70b4b3957fba941501")
    sig = H("84773160b824e194073a57493dac1a20b667af70cd2352d8af241c77658da5253aa8458317cca0eae615690d55b1f271"
            "64657dcafee1d5c1973947aa70e2cfbb4c892340be5969920d0916067b4565a0")
    proof = H("94916292a7a6bade28456c601d3af33fcf39278d6594b467e128a3f83686a104ef2b2fcf72df0215eeaf69262ffe8194a19fab31a82ddbe06908985abc4c9825788b8a1610942d12b7f5debbea8985296361206dbace7af0cc834c80f33e0aadaeea5597befbb651827b5eed5a66f1a959bb46cfd5ca1a817a14475960f69b32c54db7587b5ee3ab665fbd37b506830a49f21d592f5e634f47cee05a025a2f8f94e73a6c15f02301d1178a92873b6e8634bafe4983c3e15a663d64080678dbf29417519b78af042be2b3e1c4d08b8d520ffab008cbaaca5671a15b22c239b38e940cfeaa5e72104576a9ec4a6fad78c532381aeaa6fb56409cef56ee5c140d455feeb04426193c57086c9b6d397d9418")
    suite = bbs.SUITES[curve]
    decoy = bbs.sk_to_pk(suite, 12345)
    eng = make_engine(curve, api.create_generators(curve, L + 1, lib_path), suite.api_id, lib_path)
    eng.set_keyed_mixed_lengths(True)
    assert list(eng.set_public_keys([decoy, pk.pk])) == [1, 1]
    assert list(eng.verify_wire_keyed_batch([1, 0, 1], [sig] * 3, [[m1], [m1], [m1, b""]], [header] * 3)) == [1, 0, 0]
    assert list(eng.proof_verify_wire_keyed_batch([1, 0, 1], [proof] * 3, [[m1]] * 3, [[0]] * 3, [header] * 3, [ph, ph, ph + b"x"])) == [1, 0, 0]
    eng.close()
    assert api.verify_many_issuers([(pk, api.octets_to_signature(curve, sig, lib_path), header, [m1])]) == [True]
    assert api.proof_verify_many_issuers([(pk, api.octets_to_proof(curve, proof, lib_path), header, ph, [m1], [0])]) == [True]
