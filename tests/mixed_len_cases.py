"""Mixed message counts on one context (bbs_ctx_set_mixed_lengths).  Shared by the host-twin tier
(tests/test_mixed_len_hosttwin.py) and the GPU tier (tests/test_mixed_len_gpu.py).

The rule that defines correctness: item i, whose own count is l_i (verify: its messages; proof_verify: its commitments +
disclosed indexes), gets exactly the status a context made with generators[0 .. l_i] gives that item alone.

Expected values (expect_pv / expect_vf): the structural verdicts in the reference's order (proof_verify_init,
src/proof_verify.rs:139-150: -3, -6, -1 -- here only for l_i > L -- and the duplicate panic -22), the range and on-curve
verdicts the ABI documents (-40, -41; planted by construction), and for everything else the oracle's boolean, computed with
generators[: l_i + 1] by its plain-C restatement (oracle/c: pairings in pure Python take seconds each); a sample of items of
every kind also goes through the pure-Python oracle (check_python_oracle_sample).  Second witness: fixed-length contexts of
the same library, one per length (witness_fixed)."""
import random

import numpy as np

from bbs_sign_amd import Proof, Signature
from oracle import bbs, c_port
from parity_cases import gens_for, make_engine

VARIANT_CODE = {"InvalidDisclosedIndex": -3, "InvalidIndicesAndMessagesLength": -6, "InvalidMessageAndGeneratorsLength": -1}
FORMS = ("core", "octets", "wire")


class World:
    """One ciphersuite, one key, generators for L messages (and with them for every shorter count)."""

    def __init__(self, curve, lib_path, L, seed=7, api_id=None, gens=None):
        self.curve, self.lib_path, self.L = curve, lib_path, L
        self.suite = bbs.SUITES[curve]
        self.c = self.suite.curve
        self.api_id = self.suite.api_id if api_id is None else api_id
        self.gens = gens if gens is not None else gens_for(self.suite, L + 1)
        rng = random.Random(seed)
        self.sk = rng.randrange(1, self.c.r)
        self.pk = bbs.sk_to_pk(self.suite, self.sk)
        self.cp = c_port.port(curve)

    def signer(self, l):
        return make_engine(self.curve, self.gens[:l + 1], self.api_id, self.lib_path, sk=self.sk)

    def fixed(self, l, pk="own"):
        return make_engine(self.curve, self.gens[:l + 1], self.api_id, self.lib_path, pk=self.pk if pk == "own" else pk)

    def mixed(self, L=None, on=True):
        eng = make_engine(self.curve, self.gens[:(self.L if L is None else L) + 1], self.api_id, self.lib_path, pk=self.pk)
        eng.set_mixed_lengths(on)
        return eng


class Items:
    """A list of items, each of its own length: signatures and proofs made by fixed-length contexts of that length."""

    def __init__(self, w, lengths, seed=3, headers=None, disclosed=None):
        rng = random.Random(seed)
        c = w.c
        n = len(lengths)
        self.w, self.n, self.lengths = w, n, list(lengths)
        self.raw = [[b"item-%d-msg-%d-%d" % (i, j, seed) for j in range(l)] for i, l in enumerate(lengths)]
        h = w.fixed(0)
        flat = h.hash_to_scalar_batch([m for r in self.raw for m in r], w.api_id + b"MAP_MSG_TO_SCALAR_AS_HASH_") if sum(lengths) else []
        h.close()
        self.msgs, at = [], 0
        for l in lengths:
            self.msgs.append(list(flat[at:at + l]))
            at += l
        self.headers = list(headers) if headers is not None else [bytes([i % 251]) * (i % 5) for i in range(n)]
        self.phs = [bytes([i % 13]) * (i % 3) for i in range(n)]
        self.disclosed = [list(d) for d in disclosed] if disclosed is not None else [disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
        self.sigs, self.proofs = [None] * n, [None] * n
        self.forced = {}                    # item -> -40 / -41 planted by a defect
        rnds = [[rng.randrange(1, c.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, self.disclosed)]
        for l in sorted(set(lengths)):
            if l > w.L:
                continue
            idx = [i for i in range(n) if lengths[i] == l]
            eng = w.signer(l)
            s, st = eng.core_sign_batch([self.msgs[i] for i in idx], [self.headers[i] for i in idx])
            assert list(st) == [1] * len(idx)
            p, st = eng.core_proof_gen_batch(s, [self.msgs[i] for i in idx], [self.disclosed[i] for i in idx], [rnds[i] for i in idx],
                                             [self.headers[i] for i in idx], [self.phs[i] for i in idx])
            assert list(st) == [1] * len(idx)
            for t, i in enumerate(idx):
                self.sigs[i], self.proofs[i] = s[t], p[t]
            eng.close()
        for i in range(n):                  # longer than the context: a zero signature / proof of that shape (decided -1 at ingest)
            if self.sigs[i] is None:
                self.sigs[i] = Signature(w.gens[0], 1)
                self.proofs[i] = Proof(w.gens[0], w.gens[0], w.gens[0], 1, 1, 1, [1] * (lengths[i] - len(self.disclosed[i])), 1)
        self.dm = [[self.msgs[i][j] for j in self.disclosed[i]] for i in range(n)]
        self.draw = [[self.raw[i][j] for j in self.disclosed[i]] for i in range(n)]

    def copy(self):
        o = Items.__new__(Items)
        o.__dict__.update(self.__dict__)
        for k in ("raw", "msgs", "disclosed", "dm", "draw"):
            setattr(o, k, [list(x) for x in getattr(self, k)])
        o.headers, o.phs = list(self.headers), list(self.phs)
        o.sigs = [Signature(s.a, s.e) for s in self.sigs]
        o.proofs = [Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge) for p in self.proofs]
        o.forced = dict(self.forced)
        return o


def disclosed_for(i, l, rng):
    """Disclosed sets that include none, all, index l - 1, and an index >= 32 where l allows."""
    kind = i % 5
    if l == 0 or kind == 0:
        return []
    if kind == 1:
        return list(range(l))
    if kind == 2:
        return [l - 1]
    if kind == 3 and l > 32:
        return sorted({0, 32, l - 1})
    return sorted(rng.sample(range(l), rng.randrange(1, l + 1)))


# ---- expected values -------------------------------------------------------------------------------------------------------
def expect_pv(it, i, L):
    w = it.w
    p, dm, di = it.proofs[i], it.dm[i], it.disclosed[i]
    l = len(p.commitments) + len(di)
    if any(j >= l for j in di):
        return -3
    if len(dm) != len(di):
        return -6
    if l > L:
        return -1
    if len(set(di)) != len(di):
        return -22
    if i in it.forced:
        return it.forced[i]
    op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
    return int(w.cp.core_proof_verify(w.pk, op, w.gens[:l + 1], it.headers[i], it.phs[i], dm, di, w.api_id))


def expect_vf(it, i, L):
    w = it.w
    l = len(it.msgs[i])
    if l > L:
        return -1
    if i in it.forced:
        return it.forced[i]
    return int(w.cp.core_verify(w.pk, bbs.Signature(it.sigs[i].a, it.sigs[i].e), w.gens[:l + 1], it.headers[i], it.msgs[i], w.api_id))


def expected(it, op, L, base=None, changed=None):
    """Statuses of the rule for the whole list; with `base` (the expected statuses of the list before `changed` was edited)
    only the changed items are recomputed."""
    f = expect_pv if op == "pv" else expect_vf
    if base is None:
        return [f(it, i, L) for i in range(it.n)]
    out = list(base)
    for i in changed:
        out[i] = f(it, i, L)
    return out


def check_python_oracle_sample(it, op, idx, got):
    """The pure-Python oracle, called with generators[: l + 1], on a few items."""
    w = it.w
    for i in idx:
        try:
            if op == "pv":
                p, di = it.proofs[i], it.disclosed[i]
                l = len(p.commitments) + len(di)
                op_ = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
                want = int(bbs.core_proof_verify(w.suite, w.pk, op_, w.gens[:l + 1], it.headers[i], it.phs[i], it.dm[i], di, w.api_id))
            else:
                l = len(it.msgs[i])
                want = int(bbs.core_verify(w.suite, w.pk, bbs.Signature(it.sigs[i].a, it.sigs[i].e), w.gens[:l + 1], it.headers[i],
                                           it.msgs[i], w.api_id))
        except bbs.BbsError as e:
            want = VARIANT_CODE[e.variant]
        except bbs.BbsPanic:
            want = -22
        assert int(got[i]) == want, (w.curve, op, i, int(got[i]), want)


# ---- running a list through a context --------------------------------------------------------------------------------------
def sig_octets(w, s):
    return bbs.g1_compress(w.c, s.a) + int(s.e).to_bytes(32, "big")


def run(eng, it, op, form="core", idx=None, submit=False):
    idx = list(range(it.n)) if idx is None else idx
    H = [it.headers[i] for i in idx]
    if op == "vf":
        S, M = [it.sigs[i] for i in idx], [it.msgs[i] for i in idx]
        if form == "core":
            return eng.core_verify_submit(S, M, H) if submit else eng.core_verify_batch(S, M, H)
        octs = [sig_octets(it.w, s) for s in S]
        if form == "octets":
            return eng.verify_octets_submit(octs, M, H) if submit else eng.verify_octets_batch(octs, M, H)
        return eng.verify_wire_batch(octs, [it.raw[i] for i in idx], H)
    P, D, X, Ph = [it.proofs[i] for i in idx], [it.dm[i] for i in idx], [it.disclosed[i] for i in idx], [it.phs[i] for i in idx]
    if form == "core":
        return eng.core_proof_verify_submit(P, D, X, H, Ph) if submit else eng.core_proof_verify_batch(P, D, X, H, Ph)
    octs = eng.proofs_to_octets_batch(P)
    if form == "octets":
        return eng.proof_verify_octets_batch(octs, D, X, H, Ph)
    R = [it.draw[i] for i in idx]
    return eng.proof_verify_wire_submit(octs, R, X, H, Ph) if submit else eng.proof_verify_wire_batch(octs, R, X, H, Ph)


def witness_fixed(it, op, form="core", pk="own"):
    """Second witness: every item through a fixed-length context of ITS length (same library, key, api_id)."""
    w = it.w
    out = np.full(it.n, -1, dtype=np.int8)
    count = [len(it.proofs[i].commitments) + len(it.disclosed[i]) if op == "pv" else len(it.msgs[i]) for i in range(it.n)]
    for l in sorted(set(count)):
        if l > w.L:
            continue
        idx = [i for i in range(it.n) if count[i] == l]
        eng = w.fixed(l, pk)
        out[idx] = run(eng, it, op, form, idx)
        eng.close()
    return out


def same(got, want, what):
    got, want = [int(x) for x in got], [int(x) for x in want]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, (what, bad[:10], [got[i] for i in bad[:10]], [want[i] for i in bad[:10]])


# ---- defects (case 2) ------------------------------------------------------------------------------------------------------
def off_curve(w, p):
    return (p[0], (p[1] + 1) % w.c.p)


def plant(it, i, kind, op):
    """Edits item i in place; returns False where the item cannot take the defect (too short)."""
    w = it.w
    r = w.c.r
    l = it.lengths[i]
    if op == "vf":
        s = it.sigs[i]
        if kind == "minus_one":
            if l < 1:
                return False
            it.msgs[i].pop(); it.raw[i].pop()
        elif kind == "plus_one":
            if l + 1 > w.L:
                return False
            it.msgs[i].append(5); it.raw[i].append(b"extra")
        elif kind == "forged":
            if l < 1:
                return False
            it.msgs[i][0] = (it.msgs[i][0] + 1) % r; it.raw[i][0] = b"forged"
        elif kind == "noncanonical":
            it.sigs[i] = Signature(s.a, r); it.forced[i] = -40
        elif kind == "off_curve":
            it.sigs[i] = Signature(off_curve(w, s.a), s.e); it.forced[i] = -41
        else:
            return False
        return True
    p = it.proofs[i]
    if kind == "minus_one":
        if not p.commitments or any(j >= l - 1 for j in it.disclosed[i]):
            return False
        p.commitments.pop()
    elif kind == "plus_one":
        if l + 1 > w.L:
            return False
        p.commitments.append(7)
    elif kind == "index_eq_l":
        if l >= w.L or not p.commitments:
            return False
        it.disclosed[i] = it.disclosed[i] + [l]
        it.dm[i].append(3); it.draw[i].append(b"x")
        p.commitments.pop()                    # the count stays l: index l is out of range for THIS item, not for the context
    elif kind == "duplicate":
        if not it.disclosed[i] or not p.commitments:
            return False
        it.disclosed[i] = it.disclosed[i] + [it.disclosed[i][0]]
        it.dm[i].append(it.dm[i][0]); it.draw[i].append(it.draw[i][0])
        p.commitments.pop()
    elif kind == "messages_ne_indexes":
        it.dm[i].append(1); it.draw[i].append(b"y")
    elif kind == "forged":
        if not it.dm[i]:
            p.e_cap = (p.e_cap + 1) % r
        else:
            it.dm[i][0] = (it.dm[i][0] + 1) % r; it.draw[i][0] = b"forged"
    elif kind == "noncanonical":
        p.r1_cap = r; it.forced[i] = -40
    elif kind == "off_curve":
        p.d = off_curve(w, p.d); it.forced[i] = -41
    else:
        return False
    return True


PV_DEFECTS = (("minus_one", 0), ("plus_one", 0), ("index_eq_l", -3), ("duplicate", -22), ("messages_ne_indexes", -6), ("forged", 0),
              ("noncanonical", -40), ("off_curve", -41))
VF_DEFECTS = (("minus_one", 0), ("plus_one", 0), ("forged", 0), ("noncanonical", -40), ("off_curve", -41))


def lengths_mod(n, mod=35):
    return [i % mod for i in range(n)]


def case_lengths(n, L):
    """l_i = i mod 35; the list always holds the lengths 0, L + 1 and L + 2 (the last two are decided -1)."""
    ls = lengths_mod(n)
    if L + 1 not in ls:
        ls[-2] = L + 1
    if L + 2 not in ls:
        ls[-1] = L + 2
    return ls


# ---- case 1: every length in every wavefront ------------------------------------------------------------------------------
def check_every_length(curve, lib_path=None, n=130, L=33, forms=FORMS, python_sample=()):
    w = World(curve, lib_path, L)
    it = Items(w, case_lengths(n, L))
    assert 0 in it.lengths and L + 1 in it.lengths and L + 2 in it.lengths
    if n >= 70:
        assert any(any(j >= 32 for j in d) for d in it.disclosed) and any(d == [] for d in it.disclosed)
    eng = w.mixed()
    for op in ("vf", "pv"):
        want = expected(it, op, L)
        assert all(want[i] == (-1 if it.lengths[i] > L else 1) for i in range(n)), want
        for form in forms:
            same(run(eng, it, op, form), want, (curve, op, form))
        same(witness_fixed(it, op), want, (curve, op, "fixed-length contexts"))
        check_python_oracle_sample(it, op, python_sample, want)
    eng.close()


# ---- case 2: the length is the item's, not the context's ------------------------------------------------------------------
def check_item_length_defects(curve, lib_path=None, n=130, L=33, positions=(0, 63, 64, 129), wire=False, python_sample=False):
    w = World(curve, lib_path, L)
    lengths = [3 + (i * 7) % (L - 3) for i in range(n)]                  # 3 .. L - 1: every defect fits every position
    rng = random.Random(9)
    disclosed = [[0] if i in positions else disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
    base = Items(w, lengths, disclosed=disclosed)
    eng = w.mixed()
    for op, defects in (("pv", PV_DEFECTS), ("vf", VF_DEFECTS)):
        base_want = expected(base, op, L)
        assert base_want == [1] * n
        for kind, code in defects:
            it = base.copy()
            for p in positions:
                assert plant(it, p, kind, op), (kind, p)
            want = expected(it, op, L, base_want, positions)
            assert all(want[p] == code for p in positions), (op, kind, [want[p] for p in positions])
            forms = ("core", "wire") if wire and kind not in ("noncanonical", "off_curve") else ("core",)
            for form in forms:
                got = run(eng, it, op, form)
                same(got, want, (curve, op, kind, form))
                assert all(got[q] == 1 for p in positions for q in (p - 1, p + 1) if 0 <= q < n and q not in positions)
            # second witness: a fixed-length context of the PRESENTED length decides the same
            count = [len(it.proofs[p].commitments) + len(it.disclosed[p]) if op == "pv" else len(it.msgs[p]) for p in positions]
            for p, l in zip(positions[:2], count[:2]):
                f = w.fixed(l)
                same(run(f, it, op, "core", [p]), [code], (curve, op, kind, "fixed", p))
                f.close()
            if python_sample and kind in ("minus_one", "index_eq_l", "messages_ne_indexes", "forged"):
                check_python_oracle_sample(it, op, positions[:1], want)
    eng.close()


# ---- case 3: stale scalars ------------------------------------------------------------------------------------------------
def check_stale_scalars(curve, lib_path=None, n=130, L=33):
    w = World(curve, lib_path, L)
    full = Items(w, [L] * n, seed=5)
    short = Items(w, [(0, 1, L - 1)[i % 3] for i in range(n)], seed=6)
    eng = w.mixed()
    for op in ("pv", "vf"):
        same(run(eng, full, op), [1] * n, (curve, op, "full"))
        want = expected(short, op, L)
        assert want == [1] * n
        same(run(eng, short, op), want, (curve, op, "short after full"))
    # an uploaded job, run twice: the second run reads the scalars the first one wrote, and the same prefixes
    job = eng.core_proof_verify_upload(short.proofs, short.dm, short.disclosed, short.headers, short.phs)
    for _ in range(2):
        job.run()
        same(job.status(), [1] * n, (curve, "re-run"))
    job.free()
    eng.close()


# ---- case 4: prefix boundaries --------------------------------------------------------------------------------------------
def prefix_bytes(curve, l, api_id_len):
    """Z_pad (64) || compress(pk) || I2OSP(l, 8) || compress(Q1) || compress(H_1 .. H_l) || api_id (Ctx::domain_midstate)."""
    return (216 + 48 * l if curve == "bls12_381" else 168 + 32 * l) + api_id_len


def check_prefix_boundaries(curve, lib_path=None, L=8):
    suite = bbs.SUITES[curve]
    lens = (39, 40) if curve == "bls12_381" else (23, 24)
    on, before = set(), set()
    for m in lens:
        on |= {l for l in range(L + 1) if prefix_bytes(curve, l, m) % 64 == 0}
        before |= {l for l in range(L + 1) if prefix_bytes(curve, l, m) % 64 == 63}
    assert on and before, (on, before)
    hl = (0, 55, 56, 64)
    for aid in [suite.api_id] + [bytes(65 + k % 26 for k in range(m)) for m in lens]:
        w = World(curve, lib_path, L, api_id=aid)
        lengths = [l for l in range(L + 1) for _ in hl]
        it = Items(w, lengths, headers=[bytes([7 + l]) * h for l in range(L + 1) for h in hl])
        eng = w.mixed()
        for op in ("pv", "vf"):
            want = expected(it, op, L)
            assert want == [1] * it.n, (curve, len(aid), want)
            same(run(eng, it, op), want, (curve, op, len(aid)))
        eng.close()


# ---- case 5: modes --------------------------------------------------------------------------------------------------------
def check_modes(curve, lib_path=None, n=23, L=8):
    w = World(curve, lib_path, L)
    c = w.c
    lengths = [i % (L + 1) for i in range(n)]
    it = Items(w, lengths)
    off = w.mixed()
    on = w.mixed()
    on.set_batch_verification(True, bytes(range(32)))
    for op in ("pv", "vf"):
        same(run(off, it, op), [1] * n, (curve, op))
        same(run(on, it, op), [1] * n, (curve, op, "batch verification"))
    # one pairing-only failure (a self-consistent proof of a forged signature): the combined check fails, the fallback decides
    bad = it.copy()
    k = 5
    bad.sigs[k] = Signature(c.g1_add(it.sigs[k].a, c.g1), it.sigs[k].e)
    rng = random.Random(2)
    s = w.signer(lengths[k])
    fp, st = s.core_proof_gen_batch([bad.sigs[k]], [it.msgs[k]], [it.disclosed[k]], [[rng.randrange(1, c.r) for _ in range(5 + lengths[k] - len(it.disclosed[k]))]],
                                    [it.headers[k]], [it.phs[k]])
    s.close()
    assert list(st) == [1]
    bad.proofs[k] = fp[0]
    for op in ("pv", "vf"):
        want = expected(bad, op, L, [1] * n, [k])
        assert want[k] == 0
        same(run(off, bad, op), want, (curve, op, "pairing-only failure"))
        same(run(on, bad, op), want, (curve, op, "pairing-only failure, batch verification"))
    on.close()
    tree = w.mixed()
    tree.set_fixed_base_tree(True)
    same(run(tree, bad, "pv"), expected(bad, "pv", L, [1] * n, [k]), (curve, "fixed-base tree"))
    tree.close()
    if curve == "bls12_381":
        sub = w.mixed()
        sub.set_points_in_subgroup(True)
        for op in ("pv", "vf"):
            same(run(sub, bad, op), run(off, bad, op), (curve, op, "points in subgroup"))
        sub.close()
    # the switch goes off again on the same context: a short item is -1 again
    off.set_mixed_lengths(False)
    for op in ("pv", "vf"):
        same(run(off, it, op), [1 if l == L else -1 for l in lengths], (curve, op, "switched off"))
    off.set_mixed_lengths(True)
    # another key, then other generators, with the switch on: the statuses follow the new data
    w2 = World(curve, lib_path, L, seed=8)
    it2 = Items(w2, lengths, seed=4)
    off.set_public_key(w2.pk)
    for op in ("pv", "vf"):
        same(run(off, it2, op), [1] * n, (curve, op, "new key"))
        same(run(off, it, op), [0] * n, (curve, op, "old key's items"))
        same(witness_fixed(it, op, pk=w2.pk), [0] * n, (curve, op, "old key's items, fixed-length contexts"))
    L3 = L - 2
    w3 = World(curve, lib_path, L3, seed=8, gens=bbs.synthetic_generators(w.suite, L3 + 1, b"mixed-lengths-other-generators"))
    it3 = Items(w3, [i % (L3 + 1) for i in range(n)], seed=4)
    off.set_generators(w3.gens, w3.api_id)
    for op in ("pv", "vf"):
        same(run(off, it3, op), [1] * n, (curve, op, "new generators"))
        same(run(off, it2, op), [-1 if l > L3 else 0 for l in lengths], (curve, op, "old generators' items"))
    off.close()


# ---- case 6: fail closed and misuse ---------------------------------------------------------------------------------------
def check_fail_closed_and_misuse(curve, lib_path=None, L=5):
    import pytest
    w = World(curve, lib_path, L)
    lengths = [0, 1, L, 3, L, 2]
    it = Items(w, lengths)
    n = it.n
    eng = w.mixed()
    for job in (eng.core_proof_verify_upload(it.proofs, it.dm, it.disclosed, it.headers, it.phs),
                eng.core_verify_upload(it.sigs, it.msgs, it.headers)):
        with pytest.raises(Exception, match="BBS_E_STATE"):       # uploaded, never run: nothing to report
            job.status()
        job.run()
        same(job.status(), [1] * n, (curve, "uploaded job"))
        job.free()
    # keyed entry points on a switched-on context: BBS_E_STATE, nothing enqueued
    eng.set_public_keys([w.pk])
    kidx = np.zeros(n, dtype=np.uint32)
    octs = eng.proofs_to_octets_batch(it.proofs)
    so = [sig_octets(w, s) for s in it.sigs]
    keyed = [lambda: eng.core_proof_verify_keyed_batch(kidx, it.proofs, it.dm, it.disclosed, it.headers, it.phs),
             lambda: eng.core_proof_verify_keyed_submit(kidx, it.proofs, it.dm, it.disclosed, it.headers, it.phs),
             lambda: eng.proof_verify_wire_keyed_batch(kidx, octs, it.draw, it.disclosed, it.headers, it.phs),
             lambda: eng.proof_verify_wire_keyed_submit(kidx, octs, it.draw, it.disclosed, it.headers, it.phs),
             lambda: eng.core_verify_keyed_batch(kidx, it.sigs, it.msgs, it.headers),
             lambda: eng.core_verify_keyed_submit(kidx, it.sigs, it.msgs, it.headers),
             lambda: eng.verify_wire_keyed_batch(kidx, so, it.raw, it.headers),
             lambda: eng.verify_wire_keyed_submit(kidx, so, it.raw, it.headers)]
    for f in keyed:
        with pytest.raises(Exception, match="BBS_E_STATE"):
            f()
    eng.set_mixed_lengths(False)
    L_items = [i for i in range(n) if lengths[i] == L]
    same(eng.core_verify_keyed_batch(kidx[:len(L_items)], [it.sigs[i] for i in L_items], [it.msgs[i] for i in L_items],
                                     [it.headers[i] for i in L_items]), [1] * len(L_items), (curve, "keyed, switch off"))
    eng.close()
    # sign and proof_gen do not look at the switch: -1 for l != L, the same output for l = L
    plain = w.signer(L)
    mixed = w.signer(L)
    mixed.set_mixed_lengths(True)
    rng = random.Random(12)
    rnds = [[rng.randrange(1, w.c.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, it.disclosed)]
    want_st = [1 if l == L else -1 for l in lengths]
    sa, st_a = plain.core_sign_batch(it.msgs, it.headers)
    sb, st_b = mixed.core_sign_batch(it.msgs, it.headers)
    same(st_a, want_st, "sign"); same(st_b, want_st, "sign, switch on")
    for i in L_items:
        assert (sa[i].a, sa[i].e) == (sb[i].a, sb[i].e) == (it.sigs[i].a, it.sigs[i].e)
    sig_in = [it.sigs[i] if lengths[i] == L else it.sigs[L_items[0]] for i in range(n)]
    pa, st_a = plain.core_proof_gen_batch(sig_in, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    pb, st_b = mixed.core_proof_gen_batch(sig_in, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    same(st_a, want_st, "proof_gen"); same(st_b, want_st, "proof_gen, switch on")
    from parity_cases import proof_eq
    for i in L_items:
        assert proof_eq(pa[i], pb[i])
    plain.close(); mixed.close()


def check_table_bytes(curve, lib_path=None, L=7):
    """bbs_ctx_table_bytes counts the L + 1 per-length prefixes while the switch is on (and key and generators are set)."""
    HASHCTX_BYTES = 32 + 8 + 64 + 4 + 256 + 4            # HashCtx of stages_common.hpp: 368, no padding
    w = World(curve, lib_path, L)
    eng = make_engine(curve, w.gens, w.api_id, lib_path, pk=w.pk)
    tb = lambda e: int(e.lib.bbs_ctx_table_bytes(e.h))
    off = tb(eng)
    eng.set_mixed_lengths(True)
    assert tb(eng) == off + (L + 1) * HASHCTX_BYTES, (tb(eng), off)
    eng.set_generators(w.gens[:4], w.api_id)              # L = 3 now: the prefixes follow the generators
    on3 = tb(eng)
    eng.set_mixed_lengths(False)
    assert on3 == tb(eng) + 4 * HASHCTX_BYTES
    eng.set_generators(w.gens, w.api_id)
    assert tb(eng) == off
    eng.close()
    nokey = make_engine(curve, w.gens, w.api_id, lib_path)    # no key: no prefixes to count
    before = tb(nokey)
    nokey.set_mixed_lengths(True)
    assert tb(nokey) == before
    nokey.close()


# ---- case 7: against the issuer -------------------------------------------------------------------------------------------
def check_against_issuer(curve, lib_path=None, n=96, max_l=12):
    from bbs_sign_amd import Engine, Issuer, api
    suite = bbs.SUITES[curve]
    c = suite.curve
    rng = random.Random(77)
    sk = rng.randrange(1, c.r)
    pk = bbs.sk_to_pk(suite, sk)
    wb = 4 if lib_path else 8
    iss = Issuer(curve, suite.api_id, lib_path=lib_path, max_messages=max_l, window_bits=wb)
    iss.set_secret_key(sk)
    lengths = [i % (max_l + 1) for i in range(n)]
    raw = [[b"issuer-item-%d-%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    headers = [bytes([i % 7]) * (i % 4) for i in range(n)]
    phs = [bytes([i % 5]) * (i % 3) for i in range(n)]
    so, st = iss.sign(raw, headers)
    assert list(st) == [1] * n
    disclosed = [disclosed_for(i, l, rng) if l < 3 else sorted({0} | set(rng.sample(range(l - 1), rng.randrange(0, l - 1)))) for i, l in enumerate(lengths)]
    rnds = [[rng.randrange(1, c.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, disclosed)]
    po, st = iss.proof_gen(so, raw, disclosed, rnds, headers, phs)
    assert list(st) == [1] * n
    draw = [[raw[i][j] for j in disclosed[i]] for i in range(n)]
    # the defects of case 2 as they look on the wire (an off-curve point cannot be written as octets: -41 has no wire form)
    vraw = [list(r) for r in raw]
    rb = int(c.r).to_bytes(32, "big")
    fpb = c.fp_bytes
    cand = [i for i in range(n) if 4 <= lengths[i] < max_l and len(disclosed[i]) < lengths[i] - 1]
    t = iter(cand)
    planted = {}
    i = next(t); po[i] = po[i][:-64] + po[i][-32:]; planted[i] = 0                        # presented with l - 1
    i = next(t); po[i] = po[i][:-32] + bytes(31) + b"\x07" + po[i][-32:]; planted[i] = 0   # presented with l + 1
    i = next(t); disclosed[i] = disclosed[i] + [lengths[i]]; draw[i].append(b"x"); po[i] = po[i][:-64] + po[i][-32:]; planted[i] = -3
    i = next(t); disclosed[i] = disclosed[i] + [disclosed[i][0]]; draw[i].append(draw[i][0]); po[i] = po[i][:-64] + po[i][-32:]; planted[i] = -22
    i = next(t); draw[i].append(b"y"); planted[i] = -6
    i = next(t); draw[i][0] = b"forged"; planted[i] = 0
    i = next(t); po[i] = po[i][:3 * fpb + 32] + rb + po[i][3 * fpb + 64:]; planted[i] = -40
    j = next(t); vraw[j].pop(); k = next(t); vraw[k].append(b"extra"); m = next(t); vraw[m][0] = b"forged"
    q = next(t); so[q] = so[q][:fpb] + rb
    long_i = max_l                                    # an item of max_l messages presented with one commitment more: above the limit
    assert lengths[long_i] == max_l and long_i not in planted
    po[long_i] = po[long_i][:-32] + bytes(31) + b"\x07" + po[long_i][-32:]
    got_iss = [int(x) for x in iss.proof_verify(po, draw, disclosed, headers, phs)]
    got_iss_v = [int(x) for x in iss.verify(so, vraw, headers)]
    iss.close()
    eng = Engine(curve, lib_path=lib_path, window_bits=wb)
    import parity_cases as pc
    if pc.LATENCY_MODE is not None:
        eng.set_latency_mode(pc.LATENCY_MODE)
    eng.set_generators(api.create_generators(curve, max_l + 1, lib_path), suite.api_id)
    eng.set_public_key(pk)
    eng.set_mixed_lengths(True)
    got = [int(x) for x in eng.proof_verify_wire_batch(po, draw, disclosed, headers, phs)]
    got_v = [int(x) for x in eng.verify_wire_batch(so, vraw, headers)]
    eng.close()
    assert got == got_iss, [(i, got[i], got_iss[i]) for i in range(n) if got[i] != got_iss[i]]
    assert got_v == got_iss_v, [(i, got_v[i], got_iss_v[i]) for i in range(n) if got_v[i] != got_iss_v[i]]
    for i, code in planted.items():
        assert got[i] == code, (i, got[i], code)
    assert got[long_i] == got_iss[long_i] == -1
    assert all(got[i] == 1 for i in range(n) if i not in planted and i != long_i)
    assert (got_v[j], got_v[k], got_v[m], got_v[q]) == (0, 0, 0, -40), (got_v[j], got_v[k], got_v[m], got_v[q])
    assert all(got_v[i] == 1 for i in range(n) if i not in (j, k, m, q))


# ---- case 8: the public layer ---------------------------------------------------------------------------------------------
def check_public_layer(curve, lib_path=None):
    from bbs_sign_amd import BbsError, api
    suite = bbs.SUITES[curve]
    rng = random.Random(88)
    sk = api.SecretKey(curve, rng.randrange(1, suite.curve.r), lib_path)
    pk = sk.sk_to_pk()
    lengths = [0, 1, 2, 3, 4, 5, 2, 3]
    msgs = [[b"public-%d-%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    headers = [b"h%d" % i for i in range(len(lengths))]
    sigs = [sk.sign(m, h) for m, h in zip(msgs, headers)]
    vitems = [(s, h, m) for s, h, m in zip(sigs, headers, msgs)]
    vitems[6] = (sigs[6], headers[6], [b"forged"] + msgs[6][1:])
    vitems[7] = (Signature(sigs[7].a, suite.curve.r), headers[7], msgs[7])            # e = r: not a canonical scalar
    disclosed = [sorted(rng.sample(range(l), l // 2)) for l in lengths]
    proofs = [api.proof_gen(pk, s, h, b"ph", m, d) for s, h, m, d in zip(sigs, headers, msgs, disclosed)]
    pitems = [(p, h, b"ph", [m[j] for j in d], d) for p, h, m, d in zip(proofs, headers, msgs, disclosed)]
    pitems[6] = (proofs[6], headers[6], b"another ph", pitems[6][3], disclosed[6])
    pitems[7] = (proofs[7], headers[7], b"ph", pitems[7][3] + [b"x"], disclosed[7] + [lengths[7] + 1])    # index out of range

    def one(f, *a):
        try:
            return f(*a)
        except BbsError as e:
            return e
    for many, single, items in ((api.verify_many, pk.verify, vitems), (lambda p, its: api.proof_verify_many(p, its), lambda *a: api.proof_verify(pk, *a), pitems)):
        got = many(pk, items)
        for i, item in enumerate(items):
            want = one(single, *item)
            if isinstance(want, BbsError):
                assert isinstance(got[i], BbsError) and got[i].status == want.status, (curve, i, got[i], want)
            else:
                assert got[i] is want, (curve, i, got[i], want)
        assert [g is True for g in got[:6]] == [True] * 6 and got[6] is False and isinstance(got[7], BbsError)
    assert api.verify_many(pk, []) == [] and api.proof_verify_many(pk, []) == []
    # one copy of the tables per key: a shorter list reuses the engine made for the longest list seen, a longer one replaces it
    e5 = api._mixed_engine(pk, 5)
    assert api._mixed_engine(pk, 3) is e5 and api._mixed_engine(pk, 0) is e5
    assert api.verify_many(pk, vitems[:3]) == [True] * 3 and api._mixed_engine(pk, 2) is e5
    e7 = api._mixed_engine(pk, 7)
    assert e7 is not e5 and api._mixed_engine(pk, 5) is e7
    assert sum(1 for k in api._eng_cache if k[0] == "mixed" and k[2] == curve and k[3] == tuple(map(tuple, pk.pk))) == 1


def check_reference_vectors_on_longer_context(lib_path=None, L=5):
    """The reference's signature and proof vectors (one message: src/tests/test_vector.rs:163-260, as tests/parity_cases.py
    check_kat_vectors has them) verify as items of a context made for more messages."""
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
    eng = api._mixed_engine(pk, L)
    assert list(eng.verify_wire_batch([sig, sig], [[m1], [m1, b""]], [header, header])) == [1, 0]
    assert list(eng.proof_verify_wire_batch([proof, proof], [[m1], [m1]], [[0], [0]], [header, header], [ph, ph + b"x"])) == [1, 0]
    got = api.verify_many(pk, [(api.octets_to_signature(curve, sig, lib_path), header, [m1]),
                               (api.octets_to_signature(curve, sig, lib_path), header, [m1] * 4)])
    assert got == [True, False]
    got = api.proof_verify_many(pk, [(api.octets_to_proof(curve, proof, lib_path), header, ph, [m1], [0])])
    assert got == [True]
