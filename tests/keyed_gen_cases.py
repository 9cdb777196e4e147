"""Keyed proof_gen (bbs_core_proof_gen_keyed_*, bbs_proof_gen_wire_keyed_*).  Shared by the host-twin tier
(tests/test_keyed_gen_hosttwin.py) and the GPU tier (tests/test_keyed_gen_gpu.py).

The rule that defines correctness: item i, presented with key index k_i and its own message count l_i, gets the status AND the
output bytes a single-key context with key k_i (made with generators[0 .. l_i] in the mixed form) gives that item alone; an
index at or beyond the set's size, or one naming a refused key, gives BBS_ST_UNKNOWN_KEY and no output, whatever else is wrong
with the item.

Expected values: the plain-C restatement of the oracle for EVERY item (core_proof_gen with (pk_{k_i}, generators[: l_i + 1]);
there is no pairing in proof_gen), a handful of items through the pure-Python oracle, and as second witness single-key contexts
of the same library, one per key.  Everything is compared as octet strings, b"" for an item that failed."""
import functools
import random
import types

import numpy as np
import pytest

from keyed_cases import OFF_TWIST, UNKNOWN_KEY
from keyed_mixed_cases import KItems, Ring
from mixed_gen_cases import proof_octets, random_scalars_of, same_bytes
from mixed_len_cases import Items, World, disclosed_for, lengths_mod, prefix_bytes, same, sig_octets
from oracle import bbs
from parity_cases import make_engine

FOUR = tuple((form, submit) for form in ("core", "wire") for submit in (False, True))
EXPORTS = ("bbs_core_proof_gen_keyed_submit", "bbs_core_proof_gen_keyed_batch", "bbs_proof_gen_wire_keyed_submit",
           "bbs_proof_gen_wire_keyed_batch")


def rnds_of(it, seed=3, disclosed_given=False):
    """The random scalars KItems drew for its proofs: one mixed_len_cases.Items per owner k, made with seed + k."""
    out = [None] * it.n
    for k in sorted(set(it.owner)):
        idx = [i for i in range(it.n) if it.owner[i] == k]
        part = types.SimpleNamespace(lengths=[it.lengths[i] for i in idx], disclosed=[it.disclosed[i] for i in idx], w=it.ring.worlds[k])
        for i, x in zip(idx, random_scalars_of(part, seed + k, disclosed_given)):
            out[i] = x
    return out


def key_of(ring, k):
    """(accepted, public key) of key index k of the ring's set."""
    if k >= len(ring.keys) or ring.key_status[k] != 1:
        return False, None
    return True, ring.keys[k]


def want_keyed(ring, it, key_index, rnds, eng, L, idx=None, python=False):
    """(octet strings, statuses) of the rule for VALID items (no structural defect but l > L), through the C port -- or, with
    python = True, through the pure-Python oracle."""
    idx = list(range(it.n)) if idx is None else idx
    w = ring.worlds[0]
    st, proofs = [], []
    for i in idx:
        ok, pk = key_of(ring, int(key_index[i]))
        l = len(it.msgs[i])
        if not ok or l > L:
            st.append(1 if ok and l <= L else (UNKNOWN_KEY if not ok else -1))
            proofs.append(None)
            continue
        sig = bbs.Signature(it.sigs[i].a, it.sigs[i].e)
        if python:
            p = bbs.core_proof_gen(w.suite, pk, sig, it.headers[i], ring.gens[:l + 1], it.phs[i], it.msgs[i], it.disclosed[i], ring.api_id, rnds[i])
        else:
            p = w.cp.core_proof_gen(pk, sig, it.headers[i], ring.gens[:l + 1], it.phs[i], it.msgs[i], sorted(it.disclosed[i]), ring.api_id, rnds[i])
        assert len(p.commitments) == l - len(it.disclosed[i])
        st.append(1)
        proofs.append(p)
    return proof_octets(eng, proofs), st


def run_keyed(eng, it, rnds, key_index, form="core", submit=False, idx=None):
    """Every export ends as (octet strings, statuses)."""
    idx = list(range(it.n)) if idx is None else idx
    ki = np.asarray([key_index[i] for i in idx], dtype=np.uint32)
    S, M, D = [it.sigs[i] for i in idx], [it.msgs[i] for i in idx], [it.disclosed[i] for i in idx]
    X, H, P = [rnds[i] for i in idx], [it.headers[i] for i in idx], [it.phs[i] for i in idx]
    if form == "wire":
        octs, R = [sig_octets(it.w, s) for s in S], [it.raw[i] for i in idx]
        if not submit:
            return eng.proof_gen_wire_keyed_batch(ki, octs, R, D, X, H, P)
        job = eng.proof_gen_wire_keyed_submit(ki, octs, R, D, X, H, P)
        job.wait()
        out = job.output()
        job.free()
        return out
    if submit:
        job = eng.core_proof_gen_keyed_submit(ki, S, M, D, X, H, P)
        job.wait()
        proofs, st = job.output()
        job.free()
    else:
        proofs, st = eng.core_proof_gen_keyed_batch(ki, S, M, D, X, H, P)
    for t, i in enumerate(idx):
        if proofs[t] is not None:              # exactly l - r commitments are delivered
            assert len(proofs[t].commitments) == len(it.msgs[i]) - len(it.disclosed[i]), (i, len(proofs[t].commitments))
    return proof_octets(eng, proofs), st


def single_key_witness(ring, it, rnds, key_index, mixed=True, idx=None, api_id=None, form="core"):
    """Second witness: the items of every accepted key through a single-key context of that key (bbs_ctx_set_public_key; the
    producing side's mixed lengths on or off as the keyed job's).  Unknown keys: (UNKNOWN_KEY, b"")."""
    from mixed_gen_cases import run_proof
    idx = list(range(it.n)) if idx is None else idx
    out, st = {i: b"" for i in idx}, {i: UNKNOWN_KEY for i in idx}
    for k in sorted({int(key_index[i]) for i in idx}):
        ok, pk = key_of(ring, k)
        if not ok:
            continue
        mine = [i for i in idx if int(key_index[i]) == k]
        eng = make_engine(ring.curve, ring.gens, ring.api_id if api_id is None else api_id, ring.lib_path, pk=pk)
        eng.set_mixed_lengths_gen(mixed)
        o, s = run_proof(eng, it, rnds, form, mine)
        eng.close()
        for t, i in enumerate(mine):
            out[i], st[i] = o[t], int(s[t])
    return [out[i] for i in idx], [st[i] for i in idx]


def spread(n):
    """The four positions of a list of n items that straddle the wavefront boundary where it has one."""
    return (0, 63, 64, n - 1) if n > 65 else (0, n // 3, n // 2, n - 1)


# ---- the exports ------------------------------------------------------------------------------------------------------------
def check_export(lib_path=None):
    from bbs_sign_amd import Engine, _lib
    lib = _lib.load_library(lib_path)
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("core_proof_gen_keyed_batch", "core_proof_gen_keyed_submit", "proof_gen_wire_keyed_batch", "proof_gen_wire_keyed_submit"):
        assert callable(getattr(Engine, name))
    from bbs_sign_amd import api
    assert api.proof_gen_many_issuers([]) == []


# ---- case 1: every key and every length in every wavefront ------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def every_base(curve, lib_path, n, L, K, mixed):
    ring = Ring(curve, lib_path, L, K)
    owner = [i % K for i in range(n)]
    it = KItems(ring, owner, lengths_mod(n) if mixed else [L] * n)
    return ring, owner, it, rnds_of(it)


def check_every_key_and_length(curve, lib_path=None, n=130, L=33, K=3, mixed=True, exports=FOUR, python_sample=()):
    ring, owner, it, rnds = every_base(curve, lib_path, n, L, K, mixed)
    pos = spread(n)
    key_index = list(owner)
    # refused and unknown items on both sides of the wavefront boundary; the identity key is an accepted key
    key_index[pos[0]], key_index[pos[1]], key_index[pos[2]], key_index[pos[3]] = ring.REFUSED, len(ring.keys), 0xFFFFFFFF, ring.REFUSED
    ident = [i for i in range(n) if i % 11 == 5 and i not in pos]
    for i in ident:
        key_index[i] = ring.IDENTITY
    assert ident and set(owner) == set(range(K))
    if mixed:
        assert 0 in it.lengths and (n < 36 or L + 1 in it.lengths) and (n < 70 or all(l in it.lengths for l in range(L + 2)))
    eng = ring.engine(on=mixed)
    want = want_keyed(ring, it, key_index, rnds, eng, L)
    assert [want[1][p] for p in pos] == [UNKNOWN_KEY] * 4 and all(want[1][i] == 1 for i in ident if it.lengths[i] <= L)
    assert all(s == (UNKNOWN_KEY if i in pos else (1 if it.lengths[i] <= L else -1)) for i, s in enumerate(want[1]))
    # the proofs the fixed-length single-key contexts of every item's owner made (KItems): the items presented under their owner
    mine = [i for i in range(n) if key_index[i] == owner[i] and it.lengths[i] <= L]
    made = proof_octets(eng, [it.proofs[i] for i in mine])
    assert made == [want[0][i] for i in mine], (curve, "fixed-length contexts against the C port")
    fpb = ring.worlds[0].c.fp_bytes
    for form, submit in exports:
        got = run_keyed(eng, it, rnds, key_index, form, submit)
        same_bytes(got, want, (curve, form, "submit" if submit else "batch", "mixed" if mixed else "fixed"))
        for i in range(n):
            l, r = it.lengths[i], len(it.disclosed[i])
            assert len(got[0][i]) == (3 * fpb + 32 * (4 + l - r) if want[1][i] == 1 else 0), (curve, form, i)
    eng.close()
    same_bytes(single_key_witness(ring, it, rnds, key_index, mixed), want, (curve, "single-key contexts, one per key"))
    if python_sample:
        assert all(want[1][i] == 1 for i in python_sample)
        e = ring.bare()
        py = want_keyed(ring, it, key_index, rnds, e, L, list(python_sample), python=True)
        e.close()
        same_bytes(py, ([want[0][i] for i in python_sample], [want[1][i] for i in python_sample]), (curve, "python oracle"))


# ---- case 2: the item's own key, not a neighbour's --------------------------------------------------------------------------
def check_own_key(curve, lib_path=None, n=130, L=33, K=3):
    """The same items with key_index moved to the next valid key: the bytes are the oracle's under THAT key and differ from
    those under the owner's.  What proof_verify then says about them on the same context is the oracle's verdict under the
    presented key (a proof derived under a key that did not sign is a well-formed proof that does not verify: the domain enters
    B, and the signature is over the owner's B); the proofs derived under the owners' keys verify."""
    ring, owner, it, rnds = every_base(curve, lib_path, n, L, K, True)
    idx = [i for i in range(n) if it.lengths[i] <= L][:2 * 64 + 2 if n > 65 else n]
    rotated = [(k + 1) % K for k in owner]
    eng = ring.engine()
    own = want_keyed(ring, it, owner, rnds, eng, L, idx)
    want = want_keyed(ring, it, rotated, rnds, eng, L, idx)
    assert all(s == 1 for s in want[1]) and all(a != b for a, b in zip(own[0], want[0]))
    for form in ("core", "wire"):
        same_bytes(run_keyed(eng, it, rnds, rotated, form, idx=idx), want, (curve, form, "rotated keys"))
    same_bytes(single_key_witness(ring, it, rnds, rotated, True, idx), want, (curve, "single-key contexts of the presented keys"))
    # proof_verify of what came out, on the same context, under the presented key
    cp = ring.worlds[0].cp
    sample = idx[:6] + idx[-6:]
    R, X = [it.draw[i] for i in sample], [it.disclosed[i] for i in sample]
    H, Ph = [it.headers[i] for i in sample], [it.phs[i] for i in sample]
    for keys, octs in ((owner, own[0]), (rotated, want[0])):
        po = [octs[idx.index(i)] for i in sample]
        verdict = []
        for i, o in zip(sample, po):
            p = eng.proofs_from_octets_batch([o])[0][0]
            l = it.lengths[i]
            op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge)
            verdict.append(int(cp.core_proof_verify(ring.keys[keys[i]], op, ring.gens[:l + 1], it.headers[i], it.phs[i], it.dm[i], it.disclosed[i], ring.api_id)))
        if keys is owner:
            assert verdict == [1] * len(sample), (curve, verdict)
        ki = np.asarray([keys[i] for i in sample], dtype=np.uint32)
        same(eng.proof_verify_wire_keyed_batch(ki, po, R, X, H, Ph), verdict, (curve, "proof_verify of the derived proofs", keys is owner))
    eng.close()


# ---- case 3: stale pooled buffers -------------------------------------------------------------------------------------------
def check_stale_buffers(curve, lib_path=None, n=130, L=33, K=3):
    """A job of full-length items under key 0, then a job of short items under key 2 on the same context: the pools hand the
    second job the first one's fscal, fscal2, msgs, mtilde and out_mhat."""
    ring = Ring(curve, lib_path, L, K)
    full = KItems(ring, [0] * n, [L] * n, seed=5)
    short = KItems(ring, [2] * n, [i % 3 for i in range(n)], seed=6)
    assert all(m != 0 for ms in full.msgs for m in ms)
    rf, rs = rnds_of(full, 5), rnds_of(short, 6)
    eng = ring.engine()
    wf, ws = want_keyed(ring, full, full.owner, rf, eng, L), want_keyed(ring, short, short.owner, rs, eng, L)
    for form in ("core", "wire"):
        same_bytes(run_keyed(eng, full, rf, full.owner, form), wf, (curve, form, "full"))
        same_bytes(run_keyed(eng, short, rs, short.owner, form), ws, (curve, form, "short after full"))
    eng.close()
    fresh = ring.engine()
    same_bytes(run_keyed(fresh, short, rs, short.owner), ws, (curve, "a fresh context"))
    fresh.close()


# ---- case 4: structural codes keep their order, the key overrides -----------------------------------------------------------
@functools.lru_cache(maxsize=4)
def defect_base(curve, lib_path, n, L, K):
    ring = Ring(curve, lib_path, L, K)
    pos = spread(n)
    owner = [i % K for i in range(n)]
    lengths = [3 + (i * 7) % (L - 3) for i in range(n)]                  # 3 .. L - 1: every defect fits every position
    rng = random.Random(9)
    disclosed = [[0] if i in pos else disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
    it = KItems(ring, owner, lengths, disclosed=disclosed)
    return ring, owner, it, rnds_of(it, disclosed_given=True)


DEFECTS = (("too_long", -1), ("more_indexes_than_messages", -2), ("index_in_l_L", -3), ("duplicate", -4), ("r2_zero", -21),
           ("message_not_canonical", -40))


def planted(base, rnds0, kind, pos, L):
    it, rnds = base.copy(), [list(x) for x in rnds0]
    r = it.w.c.r
    for p in pos:
        l = base.lengths[p]
        if kind == "too_long":                 # l = L + 1
            it.msgs[p] = it.msgs[p] + [5] * (L + 1 - l)
            it.raw[p] = it.raw[p] + [b"extra"] * (L + 1 - l)
            rnds[p] = rnds[p] + [7] * (L + 1 - l)
        elif kind == "more_indexes_than_messages":     # r > l
            it.disclosed[p] = list(range(l)) + [0]
            rnds[p] = rnds[p][:5]
        elif kind == "index_in_l_L":           # a disclosed index in [l, L): in range for the context, not for the item
            it.disclosed[p] = [0, l]
            rnds[p] = rnds[p][:5 + l - 2]
        elif kind == "duplicate":
            it.disclosed[p] = [0, 0]
            rnds[p] = rnds[p][:5 + l - 2]
        elif kind == "r2_zero":                # proof_gen.rs:346: the inverse of r2 = 0
            rnds[p][1] = 0
        elif kind == "message_not_canonical":
            it.msgs[p] = it.msgs[p][:-1] + [r]
    return it, rnds


def check_structural_codes(curve, lib_path=None, n=130, L=33, K=3):
    """Every structural code of proof_gen at the four positions, statuses AND bytes against the single-key mixed-gen contexts of
    the items' keys; two of the four positions then name a key that is not there (beyond the set, refused): BBS_ST_UNKNOWN_KEY
    overrides the code.  (-20 is sign's alone, src/sign.rs:129: proof_gen cannot give it.  -23 is a property of the context's
    api_id, not of an item: below, on contexts with api_ids of 240 and 252 bytes.)"""
    ring, owner, base, rnds0 = defect_base(curve, lib_path, n, L, K)
    pos = spread(n)
    key_index = list(owner)
    key_index[pos[1]], key_index[pos[2]] = len(ring.keys), ring.REFUSED
    eng = ring.engine()
    for kind, code in DEFECTS:
        it, rnds = planted(base, rnds0, kind, pos, L)
        forms = ("core",) if kind == "message_not_canonical" else ("core", "wire")      # the wire form hashes its messages
        for form in forms:
            wit = single_key_witness(ring, it, rnds, owner, True, form=form)
            assert [wit[1][p] for p in pos] == [code] * 4 and all(s == 1 for i, s in enumerate(wit[1]) if i not in pos), (curve, kind, form)
            assert all(wit[0][p] == b"" for p in pos)
            want = (list(wit[0]), list(wit[1]))
            for p in (pos[1], pos[2]):
                want[1][p] = UNKNOWN_KEY
            same_bytes(run_keyed(eng, it, rnds, key_index, form), want, (curve, kind, form))
    eng.close()
    # -23: the DST of msg_to_scalars (240 bytes of api_id; wire form, items with messages) and of the domain hash (252; every item)
    for m, form in ((240, "wire"), (252, "core")):
        aid = b"x" * m
        e = make_engine(curve, ring.gens, aid, lib_path)
        e.set_keyed_mixed_lengths(True)
        assert list(e.set_public_keys(ring.keys)) == ring.key_status
        wit = single_key_witness(ring, base, rnds0, owner, True, api_id=aid, form=form)
        assert set(wit[1]) == {-23}, (curve, m, sorted(set(wit[1])))
        want = (list(wit[0]), list(wit[1]))
        for p in (pos[1], pos[2]):
            want[1][p] = UNKNOWN_KEY
        same_bytes(run_keyed(e, base, rnds0, key_index, form), want, (curve, "-23", m, form))
        e.close()


# ---- case 5: set-up and lifetime --------------------------------------------------------------------------------------------
def small_list(curve, lib_path, L, K, n=None):
    ring = Ring(curve, lib_path, L, K)
    n = n or 4 * K
    owner = [i % K for i in range(n)]
    lengths = [(i * 5 + i // K) % (L + 1) for i in range(n)]
    it = KItems(ring, owner, lengths)
    return ring, owner, it, rnds_of(it)


def check_setup(curve, lib_path=None, L=6):
    from bbs_sign_amd import Engine, _lib
    import parity_cases as pc
    K = 3
    ring, owner, it, rnds = small_list(curve, lib_path, L, K)
    n = it.n
    assert len(set(it.lengths)) >= 4 and L in it.lengths
    ref = ring.engine()
    want = want_keyed(ring, it, owner, rnds, ref, L)
    assert want[1] == [1] * n
    same_bytes(run_keyed(ref, it, rnds, owner), want, (curve, "reference context"))
    full = [i for i in range(n) if it.lengths[i] == L]
    only_L = ([want[0][i] if i in full else b"" for i in range(n)], [1 if i in full else -1 for i in range(n)])

    def refused(eng, code, key_index=owner, rn=rnds):
        for form, submit in FOUR:
            with pytest.raises(Exception, match=code):
                run_keyed(eng, it, rn, key_index, form, submit)

    # without generators
    e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
    refused(e, "BBS_E_STATE")
    e.close()
    # without a key set while the keyed switch is off; an empty set with the switch on
    e = ring.bare()
    refused(e, "BBS_E_STATE")
    e.set_keyed_mixed_lengths(True)
    for form, submit in FOUR:
        same_bytes(run_keyed(e, it, rnds, owner, form, submit), ([b""] * n, [UNKNOWN_KEY] * n), (curve, "no set, switch on", form, submit))
    e.set_public_keys([])
    same_bytes(run_keyed(e, it, rnds, owner), ([b""] * n, [UNKNOWN_KEY] * n), (curve, "an empty set, switch on"))
    e.close()
    # the producing side's single-key switch on and the keyed switch off: BBS_E_STATE; both on: mixed counts; both off: l = L only
    e = ring.engine(on=False)
    same_bytes(run_keyed(e, it, rnds, owner), only_L, (curve, "both switches off"))
    e.set_mixed_lengths_gen(True)
    refused(e, "BBS_E_STATE")
    e.set_keyed_mixed_lengths(True)
    same_bytes(run_keyed(e, it, rnds, owner), want, (curve, "both switches on"))
    e.set_mixed_lengths_gen(False)
    e.set_mixed_lengths(True)                       # the verifying side's single-key switch is not looked at
    same_bytes(run_keyed(e, it, rnds, owner), want, (curve, "the verifying switch"))
    e.set_mixed_lengths(False)
    # NULL key_index; a wrong count of random scalars, whatever the item's key; n = 0
    nn, keep, args = e._pg_inputs(it.sigs, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    st = np.zeros(n, dtype=np.int8)
    pf, cm, cmo = np.zeros(n * (6 * e.fpb + 128), dtype=np.uint8), np.zeros(32 * sum(it.lengths) + 32, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    outs = (pf.ctypes.data_as(_lib.c_u8p), cm.ctypes.data_as(_lib.c_u8p), cmo.ctypes.data_as(_lib.c_u64p), st.ctypes.data_as(_lib.c_i8p))
    assert e.lib.bbs_core_proof_gen_keyed_batch(e.h, n, None, *args, *outs) == -100
    ki = np.asarray(owner, dtype=np.uint32)
    assert e.lib.bbs_core_proof_gen_keyed_batch(e.h, n, ki.ctypes.data_as(_lib.c_u32p), *args, *outs[:3], None) == -100
    assert e.lib.bbs_core_proof_gen_keyed_batch(e.h, 0, None, *args, *outs) == 0               # n = 0: nothing is read
    assert e.lib.bbs_core_proof_gen_keyed_batch(None, n, ki.ctypes.data_as(_lib.c_u32p), *args, *outs) == -100
    for form, submit in FOUR:
        assert run_keyed(e, it, rnds, owner, form, submit, idx=[])[0] == []
    for p, k in ((0, owner[0]), (n - 1, len(ring.keys)), (1, ring.REFUSED)):
        bad = [list(x) for x in rnds]
        bad[p] = bad[p] + [1]
        ki2 = list(owner)
        ki2[p] = k
        refused(e, "BBS_E_ARG", ki2, bad)
    same_bytes(run_keyed(e, it, rnds, owner), want, (curve, "after the refused calls"))
    # an unrelated single public key set on the context: the same bytes
    e.set_public_key(World(curve, lib_path, L, seed=77, api_id=ring.api_id, gens=ring.gens).pk)
    same_bytes(run_keyed(e, it, rnds, owner), want, (curve, "an unrelated single key"))
    # the identity key is an accepted key
    ki3 = [ring.IDENTITY] * n
    wi = want_keyed(ring, it, ki3, rnds, e, L)
    assert wi[1] == [1] * n and all(a != b for a, b in zip(wi[0], want[0]))
    same_bytes(run_keyed(e, it, rnds, ki3, "wire"), wi, (curve, "identity key"))
    # a job keeps what it was created with: the key set, the rows per (key, length), the generators' tables
    for form in ("core", "wire"):
        ki = np.asarray(owner, dtype=np.uint32)
        if form == "core":
            held = e.core_proof_gen_keyed_submit(ki, it.sigs, it.msgs, it.disclosed, rnds, it.headers, it.phs)
        else:
            held = e.proof_gen_wire_keyed_submit(ki, [sig_octets(it.w, s) for s in it.sigs], it.raw, it.disclosed, rnds, it.headers, it.phs)
        e.add_public_keys([ring.worlds[0].pk])             # a new set and new rows: the job holds the old ones
        e.set_keyed_mixed_lengths(False)                   # the context lets go of the rows
        e.set_public_keys(ring.keys[:K][::-1])             # and of the set
        if form == "wire":
            e.set_generators(bbs.synthetic_generators(ring.worlds[0].suite, L + 1, b"keyed-gen-other-generators"), ring.api_id)
        held.wait()
        out = held.output()
        held.free()
        if form == "core":
            out = (proof_octets(e, out[0]), out[1])
        same_bytes(out, want, (curve, "held job", form))
        if form == "core":
            e.set_keyed_mixed_lengths(True)
            assert list(e.set_public_keys(ring.keys)) == ring.key_status
    assert e.public_key_count() == 0                       # (the generators took the key set with them)
    e.close()
    ref.close()
    # any order of generators, registration and the switch ends in the same bytes
    keys = ring.keys[:K]
    for route in (1, 2, 3, 4):
        e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
        if pc.LATENCY_MODE is not None:
            e.set_latency_mode(pc.LATENCY_MODE)
        if route == 4:
            e.set_keyed_mixed_lengths(True)                # the switch before the generators
        e.set_generators(ring.gens, ring.api_id)
        if route in (1, 3):
            e.set_keyed_mixed_lengths(True)
        if route in (1, 2, 4):
            assert list(e.set_public_keys(keys)) == [1] * K
        if route == 2:
            e.set_keyed_mixed_lengths(True)
        if route == 3:
            assert list(e.set_public_keys(keys[:1])) == [1]
            e.set_keyed_mixed_lengths(False)
            e.set_keyed_mixed_lengths(True)
            first, st2 = e.add_public_keys(keys[1:])
            assert first == 1 and list(st2) == [1] * (K - 1)
        same_bytes(run_keyed(e, it, rnds, owner), want, (curve, "route", route))
        e.close()


# ---- case 6: prefix boundaries ----------------------------------------------------------------------------------------------
def check_prefix_boundaries(curve, lib_path=None, which=0, L=8):
    """Header and api_id lengths that put the end of `key octets || count || generators || api_id` on, one before and one after
    a SHA-256 block edge for two different lengths at least (the api_ids of mixed_gen_cases.check_prefix_boundaries, one per test
    case), under two keys, with headers of 0, 55, 56 and 64 bytes."""
    lens = (39, 40, 41) if curve == "bls12_381" else (23, 24, 25)
    K = 2
    hl = (0, 55, 56, 64)
    ends = {m: {l: prefix_bytes(curve, l, m) % 64 for l in range(L + 1)} for m in lens}
    for e in (63, 0, 1):
        assert any(sum(1 for l in ends[m] if ends[m][l] == e) >= 2 for m in lens), (e, ends)
    m = lens[which]
    assert sum(1 for l in ends[m] if ends[m][l] == (63, 0, 1)[which]) >= 2, (m, ends[m])
    ring = Ring(curve, lib_path, L, K, api_id=bytes(65 + k % 26 for k in range(m)))
    lengths = [l for l in range(L + 1) for _ in hl for _ in range(K)]
    owner = [k for l in range(L + 1) for _ in hl for k in range(K)]
    it = KItems(ring, owner, lengths, headers=[bytes([7 + l]) * h for l in range(L + 1) for h in hl for _ in range(K)])
    rnds = rnds_of(it)
    eng = ring.engine()
    want = want_keyed(ring, it, owner, rnds, eng, L)
    assert want[1] == [1] * it.n
    same_bytes(run_keyed(eng, it, rnds, owner), want, (curve, m))
    eng.close()


# ---- case 7: the reference's vector -----------------------------------------------------------------------------------------
def check_reference_vector(lib_path=None, L=5):
    """The BLS12-381 proof vector of src/tests/test_vector.rs:199-260 derived as a keyed item of one message on a context made
    for L messages, the vector's key registered behind two others."""
    from bbs_sign_amd import api
    curve = "bls12_381"
    S = bbs.BLS_SUITE
    H = bytes.fromhex
    pk = api.octets_to_public_key(curve, H(
        "a820f230f6ae38503b86c70dc50b61c58a77e45c39ab25c0652bbaa8fa136f2851bd4781c9dcde39fc9d1d52c9e60268"
        "061e7d7632171d91aa8d460acee0e96f1e7c4cfb12d3ff9ab5d5dc91c277db75c845d649ef3c4f63aebc364cd55ded0c"), lib_path)
    m1 = H("9872ad089e452c7b6e283dfac2a80d58e8d0ff71cc4d5e310a1debdda4a45f02")
    header = H("11223344556677889900aabbccddeeff")
    ph = H("bed231d880675ed101ead304512e043ade9958dd0241ea70b4b3957fba941501")
    sig = H("84773160b824e194073a57493dac1a20b667af70cd2352d8af241c77658da5253aa8458317cca0eae615690d55b1f271"
            "64657dcafee1d5c1973947aa70e2cfbb4c892340be5969920d0916067b4565a0")
    proof = "94916292a7a6bade28456c601d3af33fcf39278d6594b467e128a3f83686a104ef2b2fcf72df0215eeaf69262ffe8194a19fab31a82ddbe06908985abc4c9825788b8a1610942d12b7f5debbea8985296361206dbace7af0cc834c80f33e0aadaeea5597befbb651827b5eed5a66f1a959bb46cfd5ca1a817a14475960f69b32c54db7587b5ee3ab665fbd37b506830a49f21d592f5e634f47cee05a025a2f8f94e73a6c15f02301d1178a92873b6e8634bafe4983c3e15a663d64080678dbf29417519b78af042be2b3e1c4d08b8d520ffab008cbaaca5671a15b22c239b38e940cfeaa5e72104576a9ec4a6fad78c532381aeaa6fb56409cef56ee5c140d455feeb04426193c57086c9b6d397d9418"
    rnd = bbs.mocked_calculate_random_scalars(S, 5)
    eng = make_engine(curve, api.create_generators(curve, L + 1, lib_path), S.api_id, lib_path)
    eng.set_keyed_mixed_lengths(True)
    assert list(eng.set_public_keys([bbs.sk_to_pk(S, 12345), bbs.sk_to_pk(S, 54321), pk.pk])) == [1, 1, 1]
    po, st = eng.proof_gen_wire_keyed_batch([2, 0, 7], [sig] * 3, [[m1]] * 3, [[0]] * 3, [rnd] * 3, [header] * 3, [ph] * 3)
    assert list(st) == [1, 1, UNKNOWN_KEY] and po[0].hex() == proof and po[1] and po[1].hex() != proof and po[2] == b""
    msg = eng.hash_to_scalar_batch([m1], S.api_id + b"MAP_MSG_TO_SCALAR_AS_HASH_")
    s = eng.signatures_from_octets_batch([sig])[0][0]
    proofs, st = eng.core_proof_gen_keyed_batch([2], [s], [[msg[0]]], [[0]], [rnd], [header], [ph])
    assert list(st) == [1] and eng.proofs_to_octets_batch(proofs)[0].hex() == proof
    eng.close()
    got = api.proof_gen_many_issuers([(pk, api.octets_to_signature(curve, sig, lib_path), header, ph, [m1], [0], rnd)])
    assert api.proof_to_octets(curve, got[0], lib_path).hex() == proof
    api.clear_caches()


# ---- case 8: the public layer -----------------------------------------------------------------------------------------------
def check_public_layer(lib_path=None):
    """api.proof_gen_many_issuers over 12 items of 3 issuers per curve, counts 0 .. 6, both curves in one list."""
    from bbs_sign_amd import BbsError, Signature, api
    from parity_cases import proof_eq
    rng = random.Random(99)
    lengths = [0, 1, 2, 3, 4, 5, 6, 2, 3, 4, 1, 5]
    items, pv = [], []
    for curve in ("bls12_381", "bn254"):
        r = bbs.SUITES[curve].curve.r
        sks = [api.SecretKey(curve, rng.randrange(1, r), lib_path) for _ in range(3)]
        pks = [sk.sk_to_pk() for sk in sks]
        for i, l in enumerate(lengths[:6] if curve == "bn254" else lengths[6:] + lengths[:6]):
            msgs = [b"gen-issuers-%d-%d" % (i, j) for j in range(l)]
            h = b"h%d" % i
            sig = sks[i % 3].sign(msgs, h)
            d = sorted(rng.sample(range(l), l // 2))
            items.append((pks[i % 3], sig, h, b"ph%d" % i, msgs, d, [rng.randrange(1, r) for _ in range(5 + l - len(d))]))
    n = len(items)
    assert n == 18 and {it[0].curve for it in items} == {"bls12_381", "bn254"}
    bad_sig, refused = 4, 9
    items[bad_sig] = (items[bad_sig][0], Signature(items[bad_sig][1].a, bbs.SUITES["bls12_381"].curve.r)) + items[bad_sig][2:]   # e = r: no octets
    items[refused] = (api.PublicKey(items[refused][0].curve, OFF_TWIST, lib_path),) + items[refused][1:]
    got = api.proof_gen_many_issuers(items)
    assert len(api._issuer_cache) == 2                     # one engine, one device call, per curve
    for i, item in enumerate(items):
        if i == refused:
            assert isinstance(got[i], BbsError) and got[i].status == UNKNOWN_KEY, got[i]
            continue
        try:
            want = api.proof_gen(*item)
        except BbsError as e:
            assert isinstance(got[i], BbsError) and got[i].status == e.status, (i, got[i], e)
            continue
        assert proof_eq(got[i], want), i
    assert isinstance(got[bad_sig], BbsError) and got[bad_sig].status == -40
    ok = [i for i in range(n) if i not in (bad_sig, refused)]
    assert all(not isinstance(got[i], BbsError) for i in ok)
    verdicts = api.proof_verify_many_issuers([(items[i][0], got[i], items[i][2], items[i][3], [items[i][4][j] for j in items[i][5]], items[i][5]) for i in ok])
    assert verdicts == [True] * len(ok), verdicts
    assert len(api._issuer_cache) == 2 and all(ie.eng.public_key_count() <= 4 for ie in api._issuer_cache.values())     # keys registered once
    # random scalars drawn by the call where an item brings none: the proofs verify
    drawn = api.proof_gen_many_issuers([items[i][:6] for i in ok[:5]])
    assert api.proof_verify_many_issuers([(items[i][0], p, items[i][2], items[i][3], [items[i][4][j] for j in items[i][5]], items[i][5])
                                          for i, p in zip(ok[:5], drawn)]) == [True] * 5
    api.clear_caches()
