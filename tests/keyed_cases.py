"""Keyed verification (bbs_ctx_set_public_keys, bbs_*_keyed_*): one context, many issuer keys.  Shared by the host-twin
tier (tests/test_keyed_hosttwin.py) and the GPU tier (tests/test_keyed_gpu.py).

The rule that defines correctness: an item whose key index names an accepted key gets, byte for byte, the status the
un-keyed form gives on a single-key context with that key; an unknown index or a refused key gives BBS_ST_UNKNOWN_KEY."""
import random

import numpy as np

from bbs_sign_amd import Proof
from oracle import bbs
from parity_cases import gens_for, make_engine, to_engine_proof

UNKNOWN_KEY = -44


OFF_TWIST = ((1, 2), (3, 4))      # a G2 record that is not on the twist: bbs_ctx_set_public_key refuses it


class Issuers:
    """K issuers of one ciphersuite: secret keys, public keys; engines that sign as one of them or verify under one key."""

    def __init__(self, curve, K, L, lib_path, seed, window_bits=None):
        self.curve, self.L, self.lib_path, self.wb = curve, L, lib_path, window_bits
        self.suite = bbs.SUITES[curve]
        self.api_id = self.suite.api_id
        self.gens = gens_for(self.suite, L + 1)
        rng = random.Random(seed)
        self.sks = [rng.randrange(1, self.suite.curve.r) for _ in range(K)]
        self.pks = [bbs.sk_to_pk(self.suite, sk) for sk in self.sks]

    def signer(self, k):
        return make_engine(self.curve, self.gens, self.api_id, self.lib_path, sk=self.sks[k], window_bits=self.wb)

    def verifier(self, pk):
        return make_engine(self.curve, self.gens, self.api_id, self.lib_path, pk=pk, window_bits=self.wb)


def make_items(iss, owner, R, seed):
    """Item i signed (and proved) by issuer owner[i]: (raw messages, msgs, disclosed, signatures, proofs, headers, phs)."""
    rng = random.Random(seed)
    c = iss.suite.curve
    n, L = len(owner), iss.L
    # messages as raw bytes (the wire forms hash them on the device) and their scalars (the core forms)
    raw = [[b"item-%d-msg-%d-%d" % (i, j, seed) for j in range(L)] for i in range(n)]
    h = iss.verifier(None)
    flat = h.hash_to_scalar_batch([m for r in raw for m in r], iss.api_id + b"MAP_MSG_TO_SCALAR_AS_HASH_")
    msgs = [flat[i * L:(i + 1) * L] for i in range(n)]
    disclosed = [sorted(rng.sample(range(L), R)) for _ in range(n)]
    rnds = [[rng.randrange(1, c.r) for _ in range(5 + L - R)] for _ in range(n)]
    headers = [bytes([i % 251]) * (i % 5) for i in range(n)]
    phs = [bytes([i % 13]) * (i % 3) for i in range(n)]
    sigs, proofs = [None] * n, [None] * n
    for k in sorted(set(owner)):
        idx = [i for i in range(n) if owner[i] == k]
        eng = iss.signer(k)
        s, st = eng.core_sign_batch([msgs[i] for i in idx], [headers[i] for i in idx])
        assert list(st) == [1] * len(idx)
        p, st = eng.core_proof_gen_batch(s, [msgs[i] for i in idx], [disclosed[i] for i in idx], [rnds[i] for i in idx],
                                         [headers[i] for i in idx], [phs[i] for i in idx])
        assert list(st) == [1] * len(idx)
        for t, i in enumerate(idx):
            sigs[i], proofs[i] = s[t], p[t]
        eng.close()
    h.close()
    return raw, msgs, disclosed, sigs, proofs, headers, phs


def corrupt(iss, raw, sigs, proofs, msgs, every):
    """Every `every`-th item forged (proof: e^ + 1; signature: its first message changed, raw and scalar form)."""
    c = iss.suite.curve
    proofs = [to_engine_proof(p) if not isinstance(p, Proof) else Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap,
                                                                        list(p.commitments), p.challenge) for p in proofs]
    msgs = [list(m) for m in msgs]
    raw = [list(r) for r in raw]
    for i in range(0, len(proofs), every):
        proofs[i].e_cap = (proofs[i].e_cap + 1) % c.r
        msgs[i][0] = (msgs[i][0] + 1) % c.r
        raw[i][0] = b"forged"
    return raw, proofs, msgs


def expected_by_single_key(iss, keys, key_status, key_index, run_one):
    """Statuses of the rule: per accepted key, its items through a single-key context (run_one(eng, items) -> statuses)."""
    n = len(key_index)
    want = np.full(n, UNKNOWN_KEY, dtype=np.int8)
    for k in sorted(set(int(x) for x in key_index)):
        if k >= len(keys) or key_status[k] != 1:
            continue
        idx = [i for i in range(n) if key_index[i] == k]
        eng = iss.verifier(keys[k])
        want[idx] = run_one(eng, idx)
    return want


def keyed_engine(iss, keys, batch_verification=False):
    eng = make_engine(iss.curve, iss.gens, iss.api_id, iss.lib_path, window_bits=iss.wb)
    st = eng.set_public_keys(keys)
    if batch_verification:
        eng.set_batch_verification(True, bytes(range(32)))
    return eng, st


def sig_octets(curve, s):
    c = bbs.SUITES[curve].curve
    return bbs.g1_compress(c, s.a) + int(s.e).to_bytes(32, "big")


def pv_runner(raw, disclosed, proofs, msgs, headers, phs, form):
    """run(eng, idx, key_index=None): proof_verify of the items idx, core form or wire form, keyed when key_index is given."""
    # (a disclosed index out of range -- a malformed item -- discloses a zero message)
    dm = [[msgs[i][j] if j < len(msgs[i]) else 0 for j in disclosed[i]] for i in range(len(proofs))]

    def run(eng, idx, key_index=None):
        P = [proofs[i] for i in idx]
        D = [dm[i] for i in idx]
        X = [disclosed[i] for i in idx]
        H = [headers[i] for i in idx]
        Ph = [phs[i] for i in idx]
        if form == "core":
            if key_index is None:
                return eng.core_proof_verify_batch(P, D, X, H, Ph)
            return eng.core_proof_verify_keyed_batch(key_index, P, D, X, H, Ph)
        octs = eng.proofs_to_octets_batch(P)
        R = [[raw[i][j] if j < len(raw[i]) else b"" for j in disclosed[i]] for i in idx]
        if key_index is None:
            return eng.proof_verify_wire_batch(octs, R, X, H, Ph)
        return eng.proof_verify_wire_keyed_batch(key_index, octs, R, X, H, Ph)
    return run


def vf_runner(curve, raw, sigs, msgs, headers, form):
    def run(eng, idx, key_index=None):
        S = [sigs[i] for i in idx]
        M = [msgs[i] for i in idx]
        H = [headers[i] for i in idx]
        if form == "core":
            if key_index is None:
                return eng.core_verify_batch(S, M, H)
            return eng.core_verify_keyed_batch(key_index, S, M, H)
        octs = [sig_octets(curve, s) for s in S]
        R = [raw[i] for i in idx]
        if key_index is None:
            return eng.verify_wire_batch(octs, R, H)
        return eng.verify_wire_keyed_batch(key_index, octs, R, H)
    return run
