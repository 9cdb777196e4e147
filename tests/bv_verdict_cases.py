"""The 16 combined checks of batch verification, observed (bbs_job_bv_verdicts / bbs_job_bv_report).  Shared by the host-twin
tier (tests/test_bv_verdicts_hosttwin.py), where every expectation is proved on the CPU first, and the GPU tier
(tests/test_bv_verdicts_gpu.py).

The statuses of a batch-verification job are right whatever its combination computed: a combined check that fails sends the
pending items to the per-item kernel.  So the statuses cannot tell a passing combination from a silent fallback, and these
cases look at the verdict flags themselves:
  * an all-valid job has all 16 verdicts at 1 -- a combination that is wrong in the failing direction shows here;
  * a job with an item whose pairing product is not 1 has a verdict that is not 1, and the statuses of the switch-off job;
  * one_window_job builds a job in which exactly ONE chosen window fails, from the coefficients restated in Python: the
    decision must read that verdict, and that window's digit row must be the one the restatement says.

Items: one issuer, L messages of which R are disclosed (tests/keyed_cases.py make_items); a FORGED item is
keyed_bv_cases.tampered (A + T, and for proof_verify a proof derived from it, so that only the pairing decides)."""
import hashlib
import random

import keyed_bv_cases as bv
import keyed_cases as kc
import parity_cases as pc
from bbs_sign_amd import Proof, Signature
from oracle import bbs, c_port

SEED = bytes(range(1, 33))
ONES = [1] * 16
OPS = ("pv", "vf")
CURVES = ["bls12_381", "bn254"]


# ---- items and jobs ---------------------------------------------------------------------------------------------------------
def make_batch(curve, n, L, R, lib_path, seed, window_bits=None):
    """n valid items of one issuer (a keyed_bv_cases.Batch whose every item names key 0)."""
    iss = kc.Issuers(curve, 1, L, lib_path, seed, window_bits)
    return iss, bv.Batch(iss, [0] * n, [0] * n, R, seed)


def take(batch, idx):
    """The items idx of a batch, in that order, as a batch of their own."""
    b = batch.copy()
    for f in ("owner", "raw", "msgs", "disclosed", "sigs", "proofs", "headers", "phs", "rnds"):
        setattr(b, f, [getattr(batch, f)[i] for i in idx])
    b.key_index = batch.key_index[list(idx)].copy()
    b.n = len(idx)
    return b


def engines(iss, seed=SEED):
    """(batch verification on, off): single-key contexts under the issuer's key, in the job form of the running test."""
    on, off = iss.verifier(iss.pks[0]), iss.verifier(iss.pks[0])
    on.set_batch_verification(True, seed)
    return on, off


def keyed_engines(iss, seed=SEED):
    """The same pair as keyed contexts whose key set is the one key; every key forms a group."""
    on, kst = kc.keyed_engine(iss, iss.pks)
    off, _ = kc.keyed_engine(iss, iss.pks)
    assert list(kst) == [1]
    on.set_keyed_batch_verification(True, seed, 1)
    return on, off


class Run:
    def __init__(self, job):
        job.wait()
        self.st = [int(s) for s in job.result]
        self.verdicts = [int(v) for v in job.bv_verdicts()]
        self.report = job.bv_report()
        self.names = job.stage_names()
        job.free()


def run(eng, batch, op, keyed=False):
    """One core-form job of the whole batch -> its statuses, verdict flags, report and stage names."""
    if keyed:
        return Run(batch.submit(eng, op))
    if op == "pv":
        return Run(eng.core_proof_verify_submit(batch.proofs, batch.dm(), batch.disclosed, batch.headers, batch.phs))
    return Run(eng.core_verify_submit(batch.sigs, batch.msgs, batch.headers))


def check_form(r, op, latency):
    """The job had the form the test asked for: proof_verify's combination has a stage of its own (rlc_prep) in the latency
    form only -- in the throughput form the challenge stage prepares it."""
    assert pc.LATENCY_MODE is latency
    if op == "pv":
        assert ("rlc_prep" in r.names) == bool(latency), r.names


def oracle_sample(iss, batch, st, op, sample):
    cp = c_port.port(iss.curve)
    dm = batch.dm()
    for i in sample:
        if op == "pv":
            p = batch.proofs[i]
            want = cp.core_proof_verify(iss.pks[0], bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge),
                                        iss.gens, batch.headers[i], batch.phs[i], dm[i], batch.disclosed[i], iss.api_id)
        else:
            want = cp.core_verify(iss.pks[0], bbs.Signature(batch.sigs[i].a, batch.sigs[i].e), iss.gens, batch.headers[i], batch.msgs[i],
                                  iss.api_id)
        assert st[i] == int(want), (iss.curve, op, i, st[i], want)


# ---- B1: all valid ----------------------------------------------------------------------------------------------------------
def check_all_valid(iss, batch, on, off, op, latency=False, keyed=False, sample=()):
    r, o = run(on, batch, op, keyed), run(off, batch, op, keyed)
    tag = (iss.curve, op, batch.n, latency, keyed)
    assert o.verdicts == [] and o.report == (0, 0, 0), tag
    assert r.st == o.st == [1] * batch.n, tag
    assert r.verdicts == ONES, tag + (r.verdicts,)
    assert r.report == (1, 1, batch.n), tag + (r.report,)
    if not keyed:
        check_form(r, op, latency)
    oracle_sample(iss, batch, r.st, op, sample)


# ---- B2: failures before the pairing ----------------------------------------------------------------------------------------
def _edit_proof(batch, i, **fields):
    p = batch.proofs[i]
    q = Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge)
    for k, v in fields.items():
        setattr(q, k, v)
    batch.proofs[i] = q


def check_wrong_challenge_scalar(iss, base, on, off, latency, i):
    """proof_verify, item i's challenge scalar + 1: the challenge check fails, the proof's points are untouched and their
    pairing product is 1 -- whether the item is part of the combination (latency form) or not, all 16 verdicts stay 1."""
    c = iss.suite.curve
    batch = base.copy()
    _edit_proof(batch, i, challenge=(batch.proofs[i].challenge + 1) % c.r)
    r, o = run(on, batch, "pv"), run(off, batch, "pv")
    check_form(r, "pv", latency)
    assert r.st == o.st == [0 if k == i else 1 for k in range(batch.n)], (iss.curve, latency, r.st, o.st)
    assert r.verdicts == ONES and r.report == (1, 1, batch.n), (iss.curve, latency, r.verdicts, r.report)
    oracle_sample(iss, batch, r.st, "pv", [i])


def check_replaced_abar(iss, base, on, off, latency, i):
    """proof_verify, item i's Abar replaced by Abar + T: the challenge no longer matches AND the pairing product is not 1.
    Throughput form: the combination follows the challenge stage and leaves the item out -- all verdicts 1.  Latency form:
    the combination runs beside the challenge stage over the structurally valid items -- the item is in it and a verdict
    fails.  Status 0 in both forms, every other item accepted."""
    c = iss.suite.curve
    batch = base.copy()
    _edit_proof(batch, i, a_bar=c.g1_add(batch.proofs[i].a_bar, c.g1))
    r, o = run(on, batch, "pv"), run(off, batch, "pv")
    check_form(r, "pv", latency)
    assert r.st == o.st == [0 if k == i else 1 for k in range(batch.n)], (iss.curve, latency, r.st, o.st)
    if latency:
        assert r.verdicts != ONES and r.report == (1, 0, batch.n), (iss.curve, r.verdicts, r.report)
    else:
        assert r.verdicts == ONES and r.report == (1, 1, batch.n), (iss.curve, r.verdicts, r.report)
    oracle_sample(iss, batch, r.st, "pv", [i])


def check_nothing_reaches_the_pairing(iss, base, on, off, op, latency):
    """Every item decided before the pairing -- Abar / A moved off the curve, which the ingest stage refuses in both job
    forms: both sums of every window are empty, the 16 products are e(O, W) e(O, BP2) = 1, and nothing is pending behind them.
    (The identity for A would not do: such an item reaches the pairing step and fails THERE, src/verify.rs.)"""
    c = iss.suite.curve
    batch = base.copy()
    for i in range(batch.n):
        if op == "pv":
            x, y = batch.proofs[i].a_bar
            _edit_proof(batch, i, a_bar=(x, (y + 1) % c.p))
        else:
            x, y = batch.sigs[i].a
            batch.sigs[i] = Signature((x, (y + 1) % c.p), batch.sigs[i].e)
    r, o = run(on, batch, op), run(off, batch, op)
    check_form(r, op, latency)
    assert r.st == o.st and all(s < 0 for s in r.st), (iss.curve, op, latency, r.st, o.st)
    assert r.verdicts == ONES and r.report == (1, 1, batch.n), (iss.curve, op, latency, r.verdicts, r.report)


# ---- B3 / B4: forged items, repeats, cancelling pairs -----------------------------------------------------------------------
def check_rejected(iss, batch, on, off, op, bad, latency=False, keyed=False, sample=()):
    """`batch` holds items whose pairing product is not 1 at `bad`: a verdict fails, the report says so, and the statuses are
    the switch-off job's -- exactly the bad items rejected."""
    r, o = run(on, batch, op, keyed), run(off, batch, op, keyed)
    tag = (iss.curve, op, batch.n, sorted(bad), latency, keyed)
    assert o.st == [0 if k in bad else 1 for k in range(batch.n)], tag + (o.st,)
    assert r.st == o.st, tag + ([k for k in range(batch.n) if r.st[k] != o.st[k]][:8],)
    assert len(r.verdicts) == 16 and r.verdicts != ONES and set(r.verdicts) <= {0, 1}, tag + (r.verdicts,)
    assert r.report == (1, 0, batch.n), tag + (r.report,)
    if not keyed:
        check_form(r, op, latency)
    oracle_sample(iss, batch, r.st, op, sample)


def repeated(base, n, src=0):
    """n copies of item src."""
    return take(base, [src] * n)


def cancelling(base, plus, minus, src):
    """The items `plus` and `minus` become copies of item src with A + T and A - T: the errors of their pairing products are
    inverse to each other, so equal coefficients would cancel them."""
    batch = base.copy()
    for i in list(plus) + list(minus):
        if i != src:
            batch.duplicate(src, i)
    return batch.make_bad(list(plus) + list(minus), signs=[1] * len(plus) + [-1] * len(minus))


# ---- B5: exactly one window fails -------------------------------------------------------------------------------------------
def job_seed(ctx_seed, counter):
    """runtime.hpp next_rlc_seed: SHA-256(context seed || counter).  The context keeps its 32 seed bytes as eight
    little-endian words and the hash absorbs words big-endian: every group of four bytes goes in reversed."""
    words = b"".join(ctx_seed[4 * k:4 * k + 4][::-1] for k in range(8))
    return hashlib.sha256(words + counter.to_bytes(8, "big")).digest()


def item_digits(jseed, i):
    """pippenger.hpp RlcPrep: digit w of item i is byte (w & 3) of word w >> 2 of SHA-256(job seed || I2OSP(i, 8)), counted
    from the word's low end -- h[w >> 2] >> 8 * (w & 3) with the digest's words big-endian."""
    h = hashlib.sha256(jseed + i.to_bytes(8, "big")).digest()
    return [h[4 * (w >> 2) + 3 - (w & 3)] for w in range(16)]


def nullspace_mod(rows, ncols, r):
    """A basis of { y : rows . y = 0 mod r } (r prime), by Gauss-Jordan elimination."""
    m = [[v % r for v in row] for row in rows]
    pivots, rk = [], 0
    for col in range(ncols):
        p = next((k for k in range(rk, len(m)) if m[k][col]), None)
        if p is None:
            continue
        m[rk], m[p] = m[p], m[rk]
        inv = pow(m[rk][col], -1, r)
        m[rk] = [v * inv % r for v in m[rk]]
        for k in range(len(m)):
            if k != rk and m[k][col]:
                f = m[k][col]
                m[k] = [(a - f * b) % r for a, b in zip(m[k], m[rk])]
        pivots.append(col)
        rk += 1
        if rk == len(m):
            break
    basis = []
    for free in (c for c in range(ncols) if c not in pivots):
        y = [0] * ncols
        y[free] = 1
        for k, pc_ in enumerate(pivots):
            y[pc_] = -m[k][free] % r
        basis.append(y)
    return basis


def one_window_job(iss, base, positions, w, ctx_seed=SEED, rng_seed=1):
    """A verify job in which exactly window w's combined check fails.  The items at `positions` (17 of them) become
    A_i + x_i T.  Item i then contributes e(T, BP2)^(x_i (sk + e_i)) to the product e(A, W) e(e A - B, BP2) of the
    signature equation, and window v's combined product is e(T, BP2)^(sum_i d_i[v] y_i) with y_i = x_i (sk + e_i): y is
    taken from the nullspace of the 15 digit rows v != w, with every y_i != 0 (every item is a real forgery) and row w's
    sum != 0.  (Keyed jobs: the forged items are all of ONE key, sk is that key's, and the coefficient of an item is still
    that of its index in the job, whatever its place in the key's run.)  The job must be the FIRST of its context after set_batch_verification(True, ctx_seed): counter 0.
    -> (batch, expected verdicts)."""
    c = iss.suite.curve
    r = c.r
    assert len(positions) == 17
    js = job_seed(ctx_seed, 0)
    d = [item_digits(js, i) for i in positions]
    rows = [[d[t][v] for t in range(17)] for v in range(16) if v != w]
    basis = nullspace_mod(rows, 17, r)
    assert len(basis) >= 2
    rng = random.Random(rng_seed * 16 + w)
    y = [0] * 17
    for vec in basis:
        k = rng.randrange(1, r)
        y = [(a + k * b) % r for a, b in zip(y, vec)]
    assert all(sum(row[t] * y[t] for t in range(17)) % r == 0 for row in rows)
    # the two conditions the construction stands on (a seed for which they fail is changed, the window is not skipped)
    assert all(y), (iss.curve, w, "a zero entry: that item would be valid")
    assert sum(d[t][w] * y[t] for t in range(17)) % r != 0, (iss.curve, w, "window w would pass too")
    batch = base.copy()
    for t, i in enumerate(positions):
        s = batch.sigs[i]
        x = y[t] * pow((iss.sks[batch.owner[i]] + s.e) % r, -1, r) % r
        batch.sigs[i] = Signature(c.g1_add(s.a, c.g1_mul(c.g1, x)), s.e)
    return batch, [0 if v == w else 1 for v in range(16)]


def check_one_window(iss, base, positions, w, on, off, latency=False):
    batch, want = one_window_job(iss, base, positions, w)
    on.set_batch_verification(True, SEED)                  # restarts the context's counter: this job is number 0
    r, o = run(on, batch, "vf"), run(off, batch, "vf")
    tag = (iss.curve, w, latency)
    assert r.verdicts == want, tag + (r.verdicts,)
    assert r.report == (1, 0, batch.n), tag + (r.report,)
    assert r.st == o.st == [0 if k in positions else 1 for k in range(batch.n)], tag + (r.st, o.st)
    oracle_sample(iss, batch, r.st, "vf", [positions[0], positions[-1]])


def make_two_key_batch(curve, owner, L, R, lib_path, seed, window_bits=None):
    """Valid items of two issuers, item i signed by and presented under key owner[i]."""
    iss = kc.Issuers(curve, 2, L, lib_path, seed, window_bits)
    return iss, bv.Batch(iss, owner, owner, R, seed)


def check_one_window_keyed(iss, base, positions, w, group):
    """The keyed form: two keys, two groups, the 17 forged items all under the key of `group`.  Of the 32 verdicts exactly
    entry group * 16 + w is 0; the other key's group passes and is decided by its combination."""
    batch, _ = one_window_job(iss, base, positions, w)
    assert {batch.key_index[i] for i in positions} == {group}
    on, kst = kc.keyed_engine(iss, iss.pks)
    off, _ = kc.keyed_engine(iss, iss.pks)
    assert list(kst) == [1, 1]
    on.set_keyed_batch_verification(True, SEED, 1)         # restarts the context's counter: this job is number 0
    r, o = run(on, batch, "vf", keyed=True), run(off, batch, "vf", keyed=True)
    want = [1] * 32
    want[group * 16 + w] = 0
    assert r.verdicts == want, (iss.curve, w, r.verdicts)
    assert r.report == (2, 1, batch.n), (iss.curve, w, r.report)
    assert r.st == o.st == [0 if k in positions else 1 for k in range(batch.n)], (iss.curve, w, r.st, o.st)
