"""Valid credentials whose points collide inside the scalar chains (g1.hpp: the r == q, r == -q and r == identity branches of
g1j_add_aff, and the same branches of g1j_add_i where proof_gen's split form adds partial sums).  Shared by the host-twin tier
(tests/test_collision_hosttwin.py) and the GPU tier (tests/test_collision_gpu.py).

A test that owns the secret key knows every point of an item as a multiple of B: A = a B with a = 1 / (sk + e), D = r2 B,
Abar = a r1 r2 B, Bbar = sk Abar.  tests/chain_model.py walks the chains on these logarithms and says which step takes which
branch; the builders below choose keys, e, the prover's random scalars and the presentation header so that a VALID item
enters a named branch of a named kernel path, and ASSERT the model's prediction, so a case that stops colliding fails
loudly.  Right or wrong is decided by the oracle alone: proof_gen's output equals the oracle's proof field for field; a valid
proof has status 1 only if T1 and T2 were exact (the challenge hashes them), a valid signature only if e A - B was.

Everything: L = 3 messages, indexes 0 and 2 disclosed, generators from gens_for.  The cells (the issue's letters):
  a  T1's joint chain, plain (BLS12-381 not vouched): sk = 1 (Bbar == Abar, "dbl") and sk = r - 1 (Bbar == -Abar, "cancel" then
     "from_inf"); the presentation header is searched until the top digits of c and e^ agree.
  b  T1's joint chain, GLV (BN254; BLS12-381 vouched): sk = +-d2 / (d0 + d1 lambda) for guessed top digits of c's halves and
     of e^'s low half; the presentation header is searched.
  c  the single chain with k = r - 1: a signature with e = r - 1 through verify; a proof of it with r1 r2 = 1 through
     proof_gen's split form (the scalar of e r1 r2 A is r - 1); and a proof whose e^ = r - 1 (e~ chosen after c, r1~ moved so
     that T1 stays) through PvVarMul.  No proof with r3^ = r - 1: T2 holds r3~, so the challenge moves with it.  In the GLV
     form of the single chain -- the only form BN254 has -- r - 1 enters nothing (its halves are 0 and lambda + 1, or -1 and
     0); k = 0 does (a cancellation in the correction round, the product is the identity), so e = 0 and e^ = 0 are cases too.
  d  proof_gen's split form, the additions of partial sums in pg_finalize_item: e = -sk / 2 (r1r2 B == -(e r1r2 A): "dbl"),
     r1~ = e~ r1 a (T1's parts equal: "dbl"), r1~ = -e~ r1 a (T1 THE IDENTITY: "cancel"; the proof is valid, its verification
     ends T1's chain at the identity and takes g1j_to_aff2 and the compressed-point hash through their identity paths.  On
     BN254 the oracle's encoding of the identity is marked "unpinned" in oracle/bbs.py: the expectation there is the oracle's
     alone).
  e  proof_gen's comb (throughput form), the two-term combs of Bbar and T1: r1 is searched, the colliding digit of e r1r2's
     first piece guessed, round 0's collision solved for a, e = 1 / a - sk; kept if the model confirms.  Plain comb on
     BLS12-381, GLV comb on BN254 and on vouched BLS12-381.  The families a = +-1 (A == +-B) are included whatever they enter.
A search may try at most CAP presentation headers / candidates per case; one that needs more is a failure of the builder."""
import functools
import random
import time

import chain_model as cm
from bbs_sign_amd import Signature, _lib
from oracle import bbs, c_port
from parity_cases import gens_for, make_engine, proof_eq, to_engine_proof

L = 3
DISCLOSED = [0, 2]
UNDISCLOSED = [1]
CAP = 5000
LONE = (0, 31, 63, 64, 69)
ORDINARY_POOL = 8            # distinct ordinary items per key; a batch repeats them
KEYS = ("one", "minus_one", "glv_dbl", "glv_cancel", "k0", "k1")
# guessed top digits (d0, d1, d2) of cell b: the halves are below 2^127.4 (BLS12-381) / 2^127 (BN254), so the top digits of
# their 128-bit recodings run over 1 .. 11 / 1 .. 7 and the small ones are the frequent ones
GLV_GUESS = {"bls12_381": (3, 3, 3), "bn254": (1, 1, 1)}


class Item:
    """One valid item: a credential (key, header, messages, signature) and a proof of it, both the oracle's."""

    def __init__(self, **kw):
        self.name = self.cell = self.aims = None
        self.wanted = frozenset()
        self.tries = 0
        self.__dict__.update(kw)


class CWorld:
    def __init__(self, curve, lib_path):
        t0 = time.time()
        self.curve, self.lib_path = curve, lib_path
        self.suite = bbs.SUITES[curve]
        self.c = self.suite.curve
        self.r = self.c.r
        self.api_id = self.suite.api_id
        self.gens = gens_for(self.suite, L + 1)
        self.cp = c_port.port(curve)
        self.lib = _lib.load_library(lib_path)
        self.lam = cm.glv_lambda(curve, self.lib)
        assert (self.lam * self.lam + self.lam + 1) % self.r == 0
        r, lam = self.r, self.lam
        rng = random.Random(20260 + len(curve))
        d0, d1, d2 = GLV_GUESS[curve]
        solved = d2 * pow(d0 + d1 * lam, -1, r) % r
        self.sks = {"one": 1, "minus_one": r - 1, "glv_dbl": solved, "glv_cancel": r - solved,
                    "k0": rng.randrange(2, r - 1), "k1": rng.randrange(2, r - 1)}
        self.pks = {k: self.cp.sk_to_pk(s) for k, s in self.sks.items()}
        assert self.pks["k0"] == bbs.sk_to_pk(self.suite, self.sks["k0"]) and self.pks["one"] == self.c.g2
        self.rng = rng
        self.cases = []
        self.build_cases()
        self._ordinary = {}
        self.build_seconds = time.time() - t0

    def ordinary(self, key, j):
        if (key, j) not in self._ordinary:
            self._ordinary[key, j] = self.ordinary_item(key, j)
        return self._ordinary[key, j]

    # ---- credentials and proofs, all through the oracle ----------------------------------------------------------------
    def credential(self, key, tag, e=None):
        msgs = [bbs.hash_to_scalar(self.c, b"collision-%s-%d" % (tag, j), b"COLLISION_TEST_MSG_") for j in range(L)]
        header = b"hdr-" + tag
        sk = self.sks[key]
        if e is None:
            return msgs, header, self.cp.core_sign(sk, self.gens, header, msgs, self.api_id)
        domain = bbs.calculate_domain(self.suite, self.pks[key], self.gens[0], self.gens[1:], header, self.api_id)
        B = self.cp.g1_msm_plain([self.suite.p1, self.gens[0]] + self.gens[1:], [1, domain] + msgs)
        assert B == bbs.compute_b(self.suite, self.gens, domain, msgs)
        return msgs, header, bbs.Signature(self.c.g1_mul(B, pow(sk + e, -1, self.r)), e % self.r)

    def scalars(self):
        return [self.rng.randrange(1, self.r) for _ in range(5 + len(UNDISCLOSED))]

    def init(self, key, msgs, header, sig, rs):
        return bbs.proof_init(self.suite, self.pks[key], sig, self.gens, rs, header, msgs, UNDISCLOSED, self.api_id)

    def finish(self, init, msgs, sig, rs, ph):
        c = bbs.proof_challenge_calculate(self.suite, init, [msgs[i] for i in DISCLOSED], DISCLOSED, ph, self.api_id)
        return bbs.proof_finalize(self.suite, init, c, sig.e, rs, [msgs[i] for i in UNDISCLOSED])

    def item(self, key, msgs, header, sig, rs, ph, proof=None, **kw):
        """The oracle's proof (twice: proof_init .. proof_finalize in Python and core_proof_gen of the C port) and verdicts."""
        if proof is None:
            proof = self.finish(self.init(key, msgs, header, sig, rs), msgs, sig, rs, ph)
        pk = self.pks[key]
        again = self.cp.core_proof_gen(pk, sig, header, self.gens, ph, msgs, DISCLOSED, self.api_id, rs)
        assert proof_eq(proof, again), ("the two oracles disagree", kw.get("name"))
        dm = [msgs[i] for i in DISCLOSED]
        assert self.cp.core_proof_verify(pk, proof, self.gens, header, ph, dm, DISCLOSED, self.api_id) is True, kw.get("name")
        assert self.cp.core_verify(pk, sig, self.gens, header, msgs, self.api_id) is True, kw.get("name")
        it = Item(key=key, msgs=msgs, header=header, sig=sig, rs=list(rs), ph=ph, proof=proof, dm=dm, **kw)
        it.paths = self.paths(it)
        return it

    def ordinary_item(self, key, j):
        """A valid item under `key` that enters no branch anywhere (under the keys 1 and r - 1 Bbar == +-Abar for every item,
        so there the presentation header is searched the other way round)."""
        msgs, header, sig = self.credential(key, b"ord-%s-%d" % (key.encode(), j))
        rs = self.scalars()
        for t in range(CAP):
            ph = b"ph-ord" + str(t).encode()
            proof = self.cp.core_proof_gen(self.pks[key], sig, header, self.gens, ph, msgs, DISCLOSED, self.api_id, rs)
            it = Item(key=key, msgs=msgs, header=header, sig=sig, rs=rs, ph=ph, proof=proof, dm=[msgs[i] for i in DISCLOSED],
                      name="ordinary", cell="-")
            it.paths = self.paths(it)
            if not any(it.paths.values()):
                break
        else:
            raise AssertionError("no ordinary item under key %s" % key)
        assert self.cp.core_proof_verify(self.pks[key], proof, self.gens, header, ph, it.dm, DISCLOSED, self.api_id) is True
        return it

    # ---- the model ------------------------------------------------------------------------------------------------------
    def logs(self, it):
        r = self.r
        a = pow(self.sks[it.key] + it.sig.e, -1, r)
        r1, r2 = it.rs[0], it.rs[1]
        g_abar = a * r1 * r2 % r
        return a, g_abar, self.sks[it.key] * g_abar % r, r2

    def vscal(self, it):
        """pg_scalars_item's v[0 .. 6]."""
        r = self.r
        r1, r2, et, r1t, r3t = it.rs[:5]
        r1r2 = r1 * r2 % r
        return [r2, r1r2, r2 * r1t % r, r2 * r3t % r, r1r2, r1r2 * it.sig.e % r, r1r2 * et % r]

    def paths(self, it):
        """kernel path -> the kinds of events the model predicts for the item there."""
        cv, lib, r = self.curve, self.lib, self.r
        a, g_abar, g_bbar, g_d = self.logs(it)
        p = it.proof
        t1 = [(g_bbar, p.challenge), (g_abar, p.e_cap), (g_d, p.r1_cap)]
        var = t1 + [(g_d, p.r3_cap)]
        v = self.vscal(it)
        out = {}
        for glv, tag in ((False, "plain"), (True, "glv")):
            one = (lambda g, k: cm.single_glv(cv, g, k, lib)) if glv else (lambda g, k: cm.single(cv, g, k))
            j = cm.joint(cv, t1, glv, lib)
            out["PvT1Chain " + tag] = j.kinds()
            out["PvVarMul r3^ " + tag] = one(g_d, p.r3_cap).kinds()
            out["PvVarMul latency " + tag] = set().union(*(one(g, k).kinds() for g, k in var))
            out["VfVarMul " + tag] = one(a, it.sig.e).kinds()
            combs = ([(1, v[0])], [(a, v[4])], [(1, v[1]), (a, v[5], True)], [(1, v[2]), (a, v[6])], [(1, v[3])])
            out["PgVarPart comb " + tag] = set().union(*(cm.comb(cv, t, glv, lib).kinds() for t in combs))
            out["PgVarPart split " + tag] = set().union(*(one(1 if k < 4 else a, v[k]).kinds() for k in range(7)))
        s = cm.two_sum(cv, g_bbar * p.challenge, g_abar * p.e_cap)
        s2 = cm.two_sum(cv, s.final or 0, g_d * p.r1_cap)
        out["PvChallenge sum"] = s.kinds() | s2.kinds()
        out["PvChallenge identity T1"] = {"identity"} if j.final is None else set()
        out["PgFinalize"] = cm.two_sum(cv, v[1], -a * v[5]).kinds() | cm.two_sum(cv, a * v[6], v[2]).kinds()
        return out

    def case(self, it, cell, name, aims, wanted, tries=0):
        it.cell, it.name, it.aims, it.wanted, it.tries = cell, name, aims, frozenset(wanted), tries
        assert it.wanted <= it.paths[aims], ("the case no longer collides", self.curve, name, aims, sorted(it.paths[aims]))
        assert tries <= CAP
        self.cases.append(it)
        return it

    # ---- the cells ------------------------------------------------------------------------------------------------------
    def search_ph(self, key, tag, aims, wanted, rs=None, e=None):
        """Cells a and b: proof_init once, then presentation headers b"ph" + counter until T1's chain enters `wanted`."""
        msgs, header, sig = self.credential(key, tag, e)
        rs = rs or self.scalars()
        init = self.init(key, msgs, header, sig, rs)
        a, g_abar, g_bbar, g_d = self.logs(Item(key=key, sig=sig, rs=rs))
        for t in range(1, CAP + 1):
            ph = b"ph" + str(t).encode()
            p = self.finish(init, msgs, sig, rs, ph)
            ev = cm.joint(self.curve, [(g_bbar, p.challenge), (g_abar, p.e_cap), (g_d, p.r1_cap)], aims.endswith("glv"), self.lib)
            if wanted <= ev.kinds():
                return self.item(key, msgs, header, sig, rs, ph, proof=p), t
        raise AssertionError("%s %s: no presentation header among %d enters %s" % (self.curve, tag, CAP, sorted(wanted)))

    def build_cases(self):
        r = self.r
        bls = self.curve == "bls12_381"
        # a
        if bls:
            it, t = self.search_ph("one", b"a-dbl", "PvT1Chain plain", {"dbl"})
            self.case(it, "a", "T1 plain, Bbar == Abar", "PvT1Chain plain", {"dbl"}, t)
            it, t = self.search_ph("minus_one", b"a-cancel", "PvT1Chain plain", {"cancel", "from_inf"})
            self.case(it, "a", "T1 plain, Bbar == -Abar", "PvT1Chain plain", {"cancel", "from_inf"}, t)
        # b
        for key, kind in (("glv_dbl", "dbl"), ("glv_cancel", "cancel")):
            it, t = self.search_ph(key, b"b-" + kind.encode(), "PvT1Chain glv", {kind})
            self.case(it, "b", "T1 GLV, solved key, " + kind, "PvT1Chain glv", {kind}, t)
        # c
        sk = self.sks["k0"]
        msgs, header, sig = self.credential("k0", b"c-e", e=r - 1)
        rs = self.scalars()
        rs[0] = pow(rs[1], -1, r)                                    # r1 r2 = 1: the scalar of (e r1 r2) A is r - 1
        it = self.item("k0", msgs, header, sig, rs, b"ph-c")
        assert self.vscal(it)[5] == r - 1
        self.case(it, "c", "e = r - 1 (verify; proof_gen with r1 r2 = 1)", "VfVarMul plain", {"cancel", "from_inf"})
        assert {"cancel", "from_inf"} <= it.paths["PgVarPart split plain"]
        for target, name, aims, wanted in ((r - 1, "e^ = r - 1 (proof_verify)", "PvVarMul latency plain", {"cancel", "from_inf"}),
                                           (0, "e^ = 0 (proof_verify)", "PvVarMul latency glv", {"cancel"})):
            msgs, header, sig = self.credential("k0", b"c-ecap-%d" % (target != 0))
            rs = self.scalars()
            p0 = self.finish(self.init("k0", msgs, header, sig, rs), msgs, sig, rs, b"ph-c2")
            a = pow(sk + sig.e, -1, r)
            t1_log = (rs[2] * a * rs[0] + rs[3]) * rs[1] % r               # T1 = e~ Abar + r1~ D
            rs[2] = (target - sig.e * p0.challenge) % r                  # e^ = e~ + e c = the target
            rs[3] = (t1_log * pow(rs[1], -1, r) - rs[2] * a * rs[0]) % r   # ... and T1, hence c, stays
            it = self.item("k0", msgs, header, sig, rs, b"ph-c2")
            assert it.proof.e_cap == target and it.proof.challenge == p0.challenge
            self.case(it, "c", name, aims, wanted)
            assert target or "cancel" in it.paths["PvVarMul latency plain"]
        # (k = r - 1 enters nothing in the GLV form of the single chain -- its halves are 0 and lambda + 1, or -1 and 0 -- and
        # BN254 has no other form; k = 0 does: the sum is the identity, reached by a cancellation in the correction round)
        msgs, header, sig = self.credential("k0", b"c-e0", e=0)
        it = self.item("k0", msgs, header, sig, self.scalars(), b"ph-c0")
        self.case(it, "c", "e = 0 (verify, proof_gen)", "VfVarMul glv", {"cancel"})
        assert "cancel" in it.paths["VfVarMul plain"] and "cancel" in it.paths["PgVarPart split glv"] and "cancel" in it.paths["PgVarPart split plain"]
        # d
        e = (-sk * pow(2, -1, r)) % r
        msgs, header, sig = self.credential("k0", b"d-bbar", e=e)
        it = self.item("k0", msgs, header, sig, self.scalars(), b"ph-d1")
        self.case(it, "d", "e = -sk / 2: Bbar's parts equal", "PgFinalize", {"dbl"})
        for sign, kind, name in ((1, "dbl", "r1~ = e~ r1 a: T1's parts equal"), (-1, "cancel", "r1~ = -e~ r1 a: T1 the identity")):
            msgs, header, sig = self.credential("k0", b"d-t1-" + kind.encode())
            rs = self.scalars()
            rs[3] = sign * rs[2] * rs[0] * pow(sk + sig.e, -1, r) % r
            it = self.item("k0", msgs, header, sig, rs, b"ph-d2")
            self.case(it, "d", name, "PgFinalize", {kind})
            if sign < 0:
                init = self.init("k0", msgs, header, sig, rs)
                assert init.points[3] is None and it.paths["PvChallenge identity T1"] and "cancel" in it.paths["PvT1Chain plain"]
                assert "cancel" in it.paths["PgVarPart comb plain"] and "cancel" in it.paths["PgVarPart comb glv"]
        # e
        for glv in ([False, True] if bls else [True]):
            for kind in ("dbl", "cancel"):
                for part in (2, 3):
                    self.comb_case(glv, kind, part)
        for sign in (1, -1):
            msgs, header, sig = self.credential("k0", b"e-family-%d" % (sign + 1), e=(sign - sk) % r)
            assert pow(sk + sig.e, -1, r) == sign % r                 # a = +-1
            it = self.item("k0", msgs, header, sig, self.scalars(), b"ph-e-family")
            self.case(it, "e", "A == %sB" % ("" if sign > 0 else "-"), "PgVarPart comb " + ("plain" if bls else "glv"), set())

    def comb_case(self, glv, kind, part):
        """Cell e on the comb of Bbar (part 2: terms (B, r1 r2), (A, e r1 r2, neg)) or of T1 (part 3: (B, r1~ r2), (A, e~ r1 r2)):
        the scalar of B is drawn, the top digit of the first piece of A's scalar guessed, round 0 solved for a; the model decides."""
        r, cv, lib = self.r, self.curve, self.lib
        sk = self.sks["k0"]
        aims = "PgVarPart comb " + ("glv" if glv else "plain")
        guess = 7
        rs = self.scalars()
        tries = 0
        while tries < CAP:
            rs[0 if part == 2 else 3] = self.rng.randrange(1, r)
            rs[2] = self.rng.randrange(1, r)
            kb = (rs[0] if part == 2 else rs[3]) * rs[1] % r
            first = self.round0(kb, glv)                            # round 0's sum over B's four pieces
            for a in (first * pow(guess, -1, r) % r, -first * pow(guess, -1, r) % r):
                tries += 1
                e = (pow(a, -1, r) - sk) % r
                ka = rs[0] * rs[1] * (e if part == 2 else rs[2]) % r
                ev = cm.comb(cv, [(1, kb), (a, ka, part == 2)], glv, lib)
                if any(rd == 0 and k == kind for rd, _, k in ev):
                    msgs, header, sig = self.credential("k0", b"e-%s-%d-%d" % (kind.encode(), glv, part), e=e)
                    it = self.item("k0", msgs, header, sig, rs, b"ph-e")
                    name = "comb of %s, %s, round 0, %s" % ("Bbar" if part == 2 else "T1", "GLV" if glv else "plain", kind)
                    return self.case(it, "e", name, aims, {kind}, tries)
        raise AssertionError("%s: no comb candidate among %d enters %s" % (cv, CAP, kind))

    def round0(self, k, glv):
        M = (1 << 64) - 1
        if glv:
            h0, h1, n0, n1, lam = cm.halves(self.curve, k, self.lib)
            pieces = [(1, h0 & M, n0), (1 << 64, h0 >> 64, n0), (lam, h1 & M, n1), (lam << 64, h1 >> 64, n1)]
        else:
            pieces = [(1 << (64 * j), (k >> (64 * j)) & M, False) for j in range(4)]
        return sum((-1 if n else 1) * cm.odd_digits(p, 64)[15] * b for b, p, n in pieces) % self.r


@functools.lru_cache(maxsize=4)
def world(curve, lib_path=None):
    """Built once per curve (and library) per session."""
    return CWorld(curve, lib_path)


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def layout(w, kind, n, keys, positions=LONE):
    """n items.  lone: the cases of `keys` one by one at `positions` (cycling; a layout per round until every case was placed),
    ordinary valid items of the same keys everywhere else.  uniform: positions 0 .. 63 (or the first n - n // 4) all colliding
    items of mixed kinds, the rest ordinary.  Returns a list of lists of items."""
    cases = [it for it in w.cases if it.key in keys]
    assert cases, keys
    def ordinary(i):
        return w.ordinary(keys[i % len(keys)], (i // len(keys)) % ORDINARY_POOL)

    if kind == "uniform":
        full = min(64, n - max(n // 4, 1))
        return [[cases[i % len(cases)] if i < full else ordinary(i) for i in range(n)]]
    out = []
    for at in range(0, len(cases), len(positions)):
        chunk = [cases[(at + t) % len(cases)] for t in range(len(positions))]
        out.append([chunk[positions.index(i)] if i in positions else ordinary(i) for i in range(n)])
    return out


def tamper_spots(items):
    """Two ordinary neighbours of a batch (scalar + 1), expected 0."""
    spots = [i for i, it in enumerate(items) if it.name == "ordinary"][:2]
    assert len(spots) == 2
    return spots


# ---- running ------------------------------------------------------------------------------------------------------------------
def configure(eng, vouched=False, bv=False):
    eng.set_points_in_subgroup(bool(vouched))
    if bv:
        eng.set_batch_verification(True, bytes(range(32)))
    return eng


def check_items(w, eng, items, what, key_index=None, sign_sks=None):
    """proof_gen's output equals the oracle's proof; proof_verify and verify give the oracle's verdict (1 for every built item,
    0 for the two tampered neighbours)."""
    n = len(items)
    r = w.r
    sigs = [Signature(it.sig.a, it.sig.e) for it in items]
    msgs = [it.msgs for it in items]
    H, PH = [it.header for it in items], [it.ph for it in items]
    disc = [DISCLOSED] * n
    rnds = [it.rs for it in items]
    if key_index is None:
        proofs, st = eng.core_proof_gen_batch(sigs, msgs, disc, rnds, H, PH)
    else:
        proofs, st = eng.core_proof_gen_keyed_batch(key_index, sigs, msgs, disc, rnds, H, PH)
    assert [int(x) for x in st] == [1] * n, (what, "proof_gen", [int(x) for x in st])
    bad = [(i, items[i].name) for i in range(n) if not proof_eq(proofs[i], items[i].proof)]
    assert not bad, (what, "proof_gen differs from the oracle", bad)
    spots = tamper_spots(items)
    want = [0 if i in spots else 1 for i in range(n)]
    pv = [to_engine_proof(it.proof) for it in items]
    pv[spots[0]].e_cap = (pv[spots[0]].e_cap + 1) % r
    pv[spots[1]].r1_cap = (pv[spots[1]].r1_cap + 1) % r
    dm = [it.dm for it in items]
    vs = list(sigs)
    for s in spots:
        vs[s] = Signature(sigs[s].a, (sigs[s].e + 1) % r)
    if key_index is None:
        got_pv = eng.core_proof_verify_batch(pv, dm, disc, H, PH)
        got_vf = eng.core_verify_batch(vs, msgs, H)
    else:
        got_pv = eng.core_proof_verify_keyed_batch(key_index, pv, dm, disc, H, PH)
        got_vf = eng.core_verify_keyed_batch(key_index, vs, msgs, H)
    for got, op in ((got_pv, "proof_verify"), (got_vf, "verify")):
        got = [int(x) for x in got]
        wrong = [(i, items[i].name, got[i]) for i in range(n) if got[i] != want[i]]
        assert not wrong, (what, op, wrong)
    if sign_sks is not None:                   # the credentials' own signatures (e is the hash's): sign under every key of the batch
        out, st = eng.core_sign_keyed_batch(key_index, msgs, H)
        assert [int(x) for x in st] == [1] * n, (what, "sign")
        for i in (0, n // 2, n - 1) + tuple(i for i, it in enumerate(items) if it.key in ("one", "minus_one", "glv_dbl", "glv_cancel"))[:8]:
            s = w.cp.core_sign(sign_sks[key_index[i]], w.gens, H[i], msgs[i], w.api_id)
            assert (out[i].a, out[i].e) == (s.a, s.e), (what, "sign", i)


def keys_of(w):
    return [k for k in KEYS if any(it.key == k for it in w.cases)]


def check_single_key(curve, lib_path, key, n, vouched=False, bv=False, positions=LONE):
    """One context per required key: the lone and the uniform layout of that key's cases."""
    w = world(curve, lib_path)
    eng = configure(make_engine(curve, w.gens, w.api_id, lib_path, pk=w.pks[key]), vouched, bv)
    for kind in ("lone", "uniform"):
        for items in layout(w, kind, n, [key], positions):
            check_items(w, eng, items, (curve, key, kind, "vouched" if vouched else "", "bv" if bv else ""))
    eng.close()


def check_keyed(curve, lib_path, n, vouched=False, bv=False, positions=LONE):
    """Every key on ONE context (1, r - 1, the solved keys, two ordinary keys): all cases share a batch."""
    w = world(curve, lib_path)
    eng = configure(make_engine(curve, w.gens, w.api_id, lib_path), vouched, bv)
    eng.set_keyed_mixed_lengths(True)
    st, pks, first = eng.set_secret_keys([w.sks[k] for k in KEYS])
    assert [int(x) for x in st] == [1] * len(KEYS) and pks == [w.pks[k] for k in KEYS]
    sks = [w.sks[k] for k in KEYS]
    for kind in ("lone", "uniform"):
        for items in layout(w, kind, n, list(KEYS), positions):
            ki = [KEYS.index(it.key) for it in items]
            assert kind != "uniform" or len({it.key for it in items[:min(n, 64)]}) >= 3
            check_items(w, eng, items, (curve, "keyed", kind), key_index=ki, sign_sks=sks)
    eng.close()


def coverage(w):
    """kernel path -> sorted event kinds over the committed cases (for the record; printed by tests/test_chain_model.py -s)."""
    cov = {}
    for it in w.cases:
        for path, kinds in it.paths.items():
            cov.setdefault(path, set()).update(kinds)
    return {p: sorted(k) for p, k in sorted(cov.items())}
