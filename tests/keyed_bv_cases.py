"""Keyed batch verification (bbs_ctx_set_keyed_batch_verification): combined pairing checks per issuer key.  Shared by the
host-twin tier (tests/test_keyed_bv_hosttwin.py) and the GPU tier (tests/test_keyed_bv_gpu.py).

The rule that defines correctness: with the switch on every status is what the switch-off job gives (and so the single-key
status of tests/keyed_cases.py), and bbs_job_bv_report tells which groups were decided by their 16 combined checks.

A BAD item is one that reaches the pairing step and fails there: a valid signature whose A is replaced by A + T (T = the
group's generator), and for proof_verify a proof DERIVED by proof_gen from such a signature, so that its challenge matches.
"""
import random

import numpy as np

import keyed_cases as kc
from bbs_sign_amd import Signature

SEED = bytes(range(1, 33))
STAGES = ("keyed_rlc_prep", "keyed_pip_windows", "keyed_pip_group_sums", "keyed_rlc_pairing", "keyed_bv_decide")


def tampered(iss, sig, sign=1):
    """A + T (sign = 1) or A - T: still in the subgroup, no longer a signature."""
    c = iss.suite.curve
    return Signature(c.g1_add(sig.a, c.g1 if sign > 0 else c.g1_neg(c.g1)), sig.e)


class Batch:
    """Items of several issuers: owner[i] signed item i, which is presented under key_index[i]."""

    def __init__(self, iss, owner, key_index, R, seed):
        self.iss, self.owner, self.R, self.n = iss, list(owner), R, len(owner)
        self.key_index = np.array(key_index, dtype=np.uint32)
        self.raw, self.msgs, self.disclosed, self.sigs, self.proofs, self.headers, self.phs = (
            list(x) for x in kc.make_items(iss, owner, R, seed))
        rng = random.Random(seed + 1)
        self.rnds = [[rng.randrange(1, iss.suite.curve.r) for _ in range(5 + iss.L - R)] for _ in range(self.n)]

    def copy(self):
        b = Batch.__new__(Batch)
        b.__dict__.update(self.__dict__)
        for f in ("owner", "raw", "msgs", "disclosed", "sigs", "proofs", "headers", "phs", "rnds"):
            setattr(b, f, list(getattr(self, f)))
        b.key_index = self.key_index.copy()
        return b

    def make_bad(self, positions, signs=None):
        """The items at `positions` become bad items (signs: +1 / -1 per position, default +1)."""
        by_owner = {}
        for t, i in enumerate(positions):
            self.sigs[i] = tampered(self.iss, self.sigs[i], 1 if signs is None else signs[t])
            by_owner.setdefault(self.owner[i], []).append(i)
        for k, idx in by_owner.items():
            eng = self.iss.signer(k)
            p, st = eng.core_proof_gen_batch([self.sigs[i] for i in idx], [self.msgs[i] for i in idx], [self.disclosed[i] for i in idx],
                                             [self.rnds[i] for i in idx], [self.headers[i] for i in idx], [self.phs[i] for i in idx])
            assert list(st) == [1] * len(idx)
            for t, i in enumerate(idx):
                self.proofs[i] = p[t]
            eng.close()
        return self

    def duplicate(self, src, dst):
        """Item dst becomes a copy of item src (same issuer, same everything)."""
        for f in ("owner", "raw", "msgs", "disclosed", "sigs", "proofs", "headers", "phs", "rnds"):
            getattr(self, f)[dst] = getattr(self, f)[src]
        self.key_index[dst] = self.key_index[src]
        return self

    def dm(self):
        return [[self.msgs[i][j] if j < len(self.msgs[i]) else 0 for j in self.disclosed[i]] for i in range(self.n)]

    def runner(self, op, form="core"):
        if op == "pv":
            return kc.pv_runner(self.raw, self.disclosed, self.proofs, self.msgs, self.headers, self.phs, form)
        return kc.vf_runner(self.iss.curve, self.raw, self.sigs, self.msgs, self.headers, form)

    def submit(self, eng, op, form="core"):
        """The keyed job of the whole batch in its submit form (not yet waited for)."""
        if op == "pv":
            if form == "core":
                return eng.core_proof_verify_keyed_submit(self.key_index, self.proofs, self.dm(), self.disclosed, self.headers, self.phs)
            octs = eng.proofs_to_octets_batch(self.proofs)
            R = [[self.raw[i][j] if j < len(self.raw[i]) else b"" for j in self.disclosed[i]] for i in range(self.n)]
            return eng.proof_verify_wire_keyed_submit(self.key_index, octs, R, self.disclosed, self.headers, self.phs)
        if form == "core":
            return eng.core_verify_keyed_submit(self.key_index, self.sigs, self.msgs, self.headers)
        return eng.verify_wire_keyed_submit(self.key_index, [kc.sig_octets(self.iss.curve, s) for s in self.sigs], self.raw, self.headers)

    def run(self, eng, op, form="core"):
        """-> (statuses, bv_report, stage names) of one keyed job."""
        job = self.submit(eng, op, form)
        job.wait()
        out = np.array(job.result), job.bv_report(), job.stage_names()
        job.free()
        return out


def interleaved(counts):
    """Owners of sum(counts) items, issuer k owning counts[k] of them, round robin."""
    return [k for t in range(max(counts)) for k in range(len(counts)) if t < counts[k]]


def positions_of(batch, key):
    """The items presented under `key`, in batch order: the group's run in the bv order."""
    return [i for i in range(batch.n) if batch.key_index[i] == key]


def check_symbols(lib):
    from bbs_sign_amd import _lib
    for name in ("bbs_ctx_set_keyed_batch_verification", "bbs_job_bv_report", "bbs_selftest_segmented_sums"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.bbs_ctx_set_keyed_batch_verification(None, 1, None, 0) == -100      # BBS_E_ARG
    assert lib.bbs_job_bv_report(None, None, None, None) == -100


# ---- the segmented sums alone ---------------------------------------------------------------------------------------------
def arithmetic_points(c, n, rng):
    """n distinct subgroup points P_i = (s0 + i * d) G with their scalars: one addition each."""
    s0, d = rng.randrange(1, c.r), rng.randrange(1, c.r)
    P, D = c.g1_mul(c.g1, s0), c.g1_mul(c.g1, d)
    pts, sc = [], []
    for i in range(n):
        pts.append(P)
        sc.append((s0 + i * d) % c.r)
        P = c.g1_add(P, D)
    return pts, sc


def sums_by_scalars(c, scalars, digits, groups):
    """sum_i digits[w][i] * P_i per (group, window) for P_i = scalars[i] * G: one multiplication of the generator by the
    integer combination, in the oracle's big-integer arithmetic."""
    out = []
    for first, count in groups:
        row = []
        for w in range(16):
            k = sum(int(digits[w][i]) * scalars[i] for i in range(first, first + count)) % c.r
            row.append(c.g1_mul(c.g1, k) if k else None)
        out.append(row)
    return out


def sums_term_by_term(c, points, digits, groups):
    """The same sums as the definition reads: every product digit * P_i by the oracle, added up."""
    out = []
    for first, count in groups:
        row = []
        for w in range(16):
            acc = None
            for i in range(first, first + count):
                if digits[w][i] and points[i] is not None:
                    acc = c.g1_add(acc, c.g1_mul(points[i], int(digits[w][i])))
            row.append(acc)
        out.append(row)
    return out
