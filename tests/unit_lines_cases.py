"""Line tables in the unit form and in the (c, nl) form (bbs_ctx_set_unit_lines).  Shared by tests/test_unit_lines.py (host
twin) and tests/test_unit_lines_gpu.py.

The entries are read through bbs_selftest_key_entries (tests/keyreg_cases.py): a KeyEntry starts with its LineTable --
MAX_LINES entries of (c, nl), each an Fp2 of two Montgomery values in 28-bit limbs, one limb per 32-bit word -- followed by
n_lines, q_is_identity and unit.  The entries of the unit form are the plain residues of 1/c and nl/c (pairing.hpp)."""
import random

from bbs_sign_amd import Signature
from oracle import bbs

import keyed_cases as kc
import keyreg_cases as kr
from parity_cases import to_engine_proof

MAX_LINES = 128
LIMBS = {"bls12_381": 14, "bn254": 10}
N_ITEMS = 21                      # three pairing wavefronts of ten six-lane groups
FORGED = (0, 9, 10, 20)           # first and last group of a wavefront, first of the next, the last item
IDENTITY = 5                      # the item whose Abar (proof) / A (signature) is the identity
L, R = 3, 1


def parse_table(curve, entry):
    """(lines [(c, nl)] as oracle Fp2 values, n_lines, q_is_identity, unit) of a KeyEntry's bytes."""
    c = bbs.SUITES[curve].curve
    n = LIMBS[curve]
    rinv = pow(1 << (28 * n), -1, c.p)

    def fe(off):
        v = 0
        for j in range(n):
            limb = int.from_bytes(entry[off + 4 * j:off + 4 * j + 4], "little")
            assert limb < (1 << 28), "an entry is stored as its representative in [0, p): normal limbs"
            v |= limb << (28 * j)
        assert v < c.p
        return v * rinv % c.p

    tail = MAX_LINES * 16 * n
    n_lines, ident, unit = (int.from_bytes(entry[tail + 4 * k:tail + 4 * k + 4], "little") for k in range(3))
    if unit:
        rinv = 1                  # the unit form stores the plain residues of 1/c and nl/c
    lines = []
    for s in range(n_lines):
        o = s * 16 * n
        lines.append(((fe(o), fe(o + 4 * n)), (fe(o + 8 * n), fe(o + 12 * n))))
    return lines, n_lines, ident, unit


def table_keys(curve, seed=11):
    """the generator (its table is the context's BP2 table) and three random keys"""
    return [bbs.SUITES[curve].curve.g2] + kr.valid_keys(curve, 3, seed)


def check_tables(eng, curve, paths=(0,)):
    """Both forms of every table: nl_unit * c == nl and cinv_unit * c == 1 entry by entry, the flags, and the switch back."""
    c = bbs.SUITES[curve].curve
    keys = table_keys(curve)
    first = None
    for path in paths:
        eng.set_unit_lines(True)
        eu, su, _ = kr.key_entries(eng, path, keys=keys)
        eng.set_unit_lines(False)
        eo, so, _ = kr.key_entries(eng, path, keys=keys)
        eng.set_unit_lines(True)
        again, _, _ = kr.key_entries(eng, path, keys=keys)
        assert su == so == [1] * len(keys)
        assert again == eu, (curve, path, "the unit form again after the (c, nl) form")
        if first is None:
            first = (eu, eo)
        else:
            assert (eu, eo) == first, (curve, "the stage and the host functions, both forms, byte for byte")
        for k in range(len(keys)):
            lu, nu, iu, uu = parse_table(curve, eu[k])
            lo, no, io, uo = parse_table(curve, eo[k])
            assert (nu, iu, uu) == (no, 0, 1) and (io, uo) == (0, 0) and nu == {"bls12_381": 68, "bn254": 102}[curve], (curve, k)
            assert eu[k][len(eu[k]) - 368:] == eo[k][len(eo[k]) - 368:], (curve, k, "the midstate does not depend on the form")
            for s in range(nu):
                (cinv, nlc), (cc, nl) = lu[s], lo[s]
                assert c.f2_mul(cinv, cc) == (1, 0), (curve, "key", k, "line", s, "cinv_unit * c == 1")
                assert c.f2_mul(nlc, cc) == nl, (curve, "key", k, "line", s, "nl_unit * c == nl")
    return first


class Items:
    """N_ITEMS items of `owners` issuers (item i by issuer i mod owners): valid, except that the items FORGED carry a
    signature whose e is off by one -- for proof_verify a proof GENERATED from that signature, so that its challenge holds
    and only the pairing product tells -- and that item IDENTITY has the identity for A / Abar.  `want_vf` / `want_pv` are
    the oracle's verdicts under the item's issuer key, computed once."""

    def __init__(self, curve, lib_path, owners, seed, window_bits=None):
        self.iss = iss = kc.Issuers(curve, owners, L, lib_path, seed, window_bits)
        suite, c = iss.suite, iss.suite.curve
        rng = random.Random(seed)
        n = N_ITEMS
        self.owner = [i % owners for i in range(n)]
        self.msgs = [[rng.randrange(c.r) for _ in range(L)] for _ in range(n)]
        self.headers = [bytes([i % 251]) * (i % 5) for i in range(n)]
        self.phs = [bytes([i % 13]) * (i % 3) for i in range(n)]
        self.disclosed = [sorted(rng.sample(range(L), R)) for _ in range(n)]
        rnds = [[rng.randrange(1, c.r) for _ in range(5 + L - R)] for _ in range(n)]
        self.sigs, self.proofs = [None] * n, [None] * n
        for k in range(owners):
            idx = [i for i in range(n) if self.owner[i] == k]
            eng = iss.signer(k)
            s, st = eng.core_sign_batch([self.msgs[i] for i in idx], [self.headers[i] for i in idx])
            assert list(st) == [1] * len(idx)
            s = [Signature(x.a, (x.e + 1) % c.r) if i in FORGED else x for i, x in zip(idx, s)]
            p, st = eng.core_proof_gen_batch(s, [self.msgs[i] for i in idx], [self.disclosed[i] for i in idx], [rnds[i] for i in idx],
                                             [self.headers[i] for i in idx], [self.phs[i] for i in idx])
            assert list(st) == [1] * len(idx)
            for t, i in enumerate(idx):
                self.sigs[i], self.proofs[i] = s[t], to_engine_proof(p[t])
            eng.close()
        self.sigs[IDENTITY] = Signature(None, self.sigs[IDENTITY].e)
        self.proofs[IDENTITY].a_bar = None
        self.dm = [[self.msgs[i][j] for j in self.disclosed[i]] for i in range(n)]
        self.want_vf, self.want_pv = [], []
        for i in range(n):
            pk = iss.pks[self.owner[i]]
            self.want_vf.append(int(bbs.core_verify(suite, pk, bbs.Signature(self.sigs[i].a, self.sigs[i].e), iss.gens, self.headers[i],
                                                    self.msgs[i], iss.api_id)))
            p = self.proofs[i]
            op = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge)
            self.want_pv.append(int(bbs.core_proof_verify(suite, pk, op, iss.gens, self.headers[i], self.phs[i], self.dm[i],
                                                          self.disclosed[i], iss.api_id)))
        bad = set(FORGED) | {IDENTITY}
        assert self.want_vf == self.want_pv == [0 if i in bad else 1 for i in range(n)], (curve, self.want_vf, self.want_pv)

    def verify(self, eng, key_index=None):
        if key_index is None:
            return list(eng.core_verify_batch(self.sigs, self.msgs, self.headers))
        return list(eng.core_verify_keyed_batch(key_index, self.sigs, self.msgs, self.headers))

    def proof_verify(self, eng, key_index=None):
        if key_index is None:
            return list(eng.core_proof_verify_batch(self.proofs, self.dm, self.disclosed, self.headers, self.phs))
        return list(eng.core_proof_verify_keyed_batch(key_index, self.proofs, self.dm, self.disclosed, self.headers, self.phs))


_items = {}


def items(curve, lib_path, owners, window_bits=None):
    key = (curve, lib_path, owners, window_bits)
    if key not in _items:
        _items[key] = Items(curve, lib_path, owners, seed=101 + owners, window_bits=window_bits)
    return _items[key]


def check_single_key(curve, lib_path, window_bits=None):
    """verify and proof_verify of the 21 items under the context's one key, in both line forms: the oracle's statuses"""
    it = items(curve, lib_path, 1, window_bits)
    eng = it.iss.verifier(it.iss.pks[0])
    for unit in (True, False, True):
        eng.set_unit_lines(unit)
        assert it.verify(eng) == it.want_vf, (curve, "verify", "unit" if unit else "(c, nl)")
        assert it.proof_verify(eng) == it.want_pv, (curve, "proof_verify", "unit" if unit else "(c, nl)")
    eng.close()


def check_keyed(curve, lib_path, window_bits=None):
    """One keyed job over two keys, item i under key i mod 2: on a context in the unit form, on the same context switched to
    the (c, nl) form with its key set in place, and on a context that was switched before its keys were registered."""
    it = items(curve, lib_path, 2, window_bits)
    keys = list(it.iss.pks)
    eng, st = kc.keyed_engine(it.iss, keys)
    assert list(st) == [1, 1]
    assert it.verify(eng, it.owner) == it.want_vf and it.proof_verify(eng, it.owner) == it.want_pv, (curve, "unit")
    eng.set_unit_lines(False)
    assert it.verify(eng, it.owner) == it.want_vf and it.proof_verify(eng, it.owner) == it.want_pv, (curve, "switched to (c, nl)")
    eng.close()
    eng = kc.make_engine(curve, it.iss.gens, it.iss.api_id, lib_path, window_bits=window_bits)
    eng.set_unit_lines(False)
    assert list(eng.set_public_keys(keys)) == [1, 1]
    assert it.verify(eng, it.owner) == it.want_vf and it.proof_verify(eng, it.owner) == it.want_pv, (curve, "registered in (c, nl)")
    eng.set_unit_lines(True)
    assert it.verify(eng, it.owner) == it.want_vf and it.proof_verify(eng, it.owner) == it.want_pv, (curve, "switched to unit")
    eng.close()
