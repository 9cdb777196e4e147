"""Keyed batch verification on the GPU (tests/keyed_bv_cases.py): the segmented bucket kernel against the oracle, full jobs
with groups at every size where the kernel takes another path -- below, at and above a 64-digit chunk and the 256 buckets,
and one group of two segments -- bad items at the edges of runs and segments, both job forms, core and wire forms, and a key
set replaced while jobs are in flight."""
import functools
import random

import numpy as np
import pytest

import keyed_bv_cases as bv
import keyed_cases as kc
from oracle import bbs, c_port

pytestmark = pytest.mark.gpu

L, R = 8, 3
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4100)
SMALL = (1, 3, 4, 5, 63, 64, 65)
CURVES = ["bls12_381", "bn254"]


@pytest.mark.parametrize("curve", CURVES)
def test_segmented_sums(curve):
    suite = bbs.SUITES[curve]
    c = suite.curve
    rng = random.Random(5)
    sizes = list(SIZES) + [70, 70]                                 # + a group of digits 255 and a group of digits 0
    n = sum(sizes)
    pts, sc = bv.arithmetic_points(c, n, rng)
    groups, first = [], 0
    for s in sizes:
        groups.append((first, s))
        first += s
    digits = np.frombuffer(rng.randbytes(16 * n), dtype=np.uint8).reshape(16, n).copy()
    digits[:, groups[-2][0]:groups[-2][0] + 70] = 255
    digits[:, groups[-1][0]:] = 0
    eng = kc.make_engine(curve, kc.gens_for(suite, 2), suite.api_id)
    got = eng.segmented_sums(pts, digits, groups)
    want = bv.sums_by_scalars(c, sc, digits, groups)
    for g in range(len(groups)):
        assert got[g] == want[g], (curve, sizes[g], [w for w in range(16) if got[g][w] != want[g][w]])
    assert all(p is None for p in got[-1])
    # the small groups once more, every product by itself
    assert got[:4] == bv.sums_term_by_term(c, pts, digits, groups[:4])


@functools.lru_cache(maxsize=None)
def _scene(curve, sizes):
    """Issuer k owns sizes[k] items, scattered over the batch; the bad items; made once, never changed."""
    K = len(sizes)
    iss = kc.Issuers(curve, K, L, None, seed=23)
    owner = [k for k in range(K) for _ in range(sizes[k])]
    random.Random(3).shuffle(owner)
    batch = bv.Batch(iss, owner, owner, R, seed=13)
    bad = []
    for k in range(K):
        run = bv.positions_of(batch, k)
        if sizes[k] in (63, 64, 65, 4100):
            bad += [run[0], run[-1]]
        if sizes[k] == 4100:
            bad += [run[4095], run[4096]]                          # the last item of the first segment, the first of the second
    batch.make_bad(bad)
    return iss, batch, tuple(bad)


def _check_oracle_sample(iss, batch, bad, st, op):
    cp = c_port.port(iss.curve)
    dm = batch.dm()
    sample = sorted(set(range(0, batch.n, max(1, batch.n // 48))) | set(bad))[:64]
    for i in sample:
        pk = iss.pks[batch.key_index[i]]
        if op == "pv":
            p = batch.proofs[i]
            op_ = bbs.Proof(p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, p.commitments, p.challenge)
            want = cp.core_proof_verify(pk, op_, iss.gens, batch.headers[i], batch.phs[i], dm[i], batch.disclosed[i], iss.api_id)
        else:
            want = cp.core_verify(pk, bbs.Signature(batch.sigs[i].a, batch.sigs[i].e), iss.gens, batch.headers[i], batch.msgs[i], iss.api_id)
        assert st[i] == int(want) == (0 if i in bad else 1), (op, i)


@pytest.mark.parametrize("op", ["pv", "vf"])
@pytest.mark.parametrize("curve", CURVES)
def test_full_job(curve, op):
    iss, batch, bad = _scene(curve, SIZES)
    eng, kst = kc.keyed_engine(iss, iss.pks)
    off, rep, names = batch.run(eng, op)
    assert rep == (0, 0, 0) and not any(s in names for s in bv.STAGES)
    eng.set_keyed_batch_verification(True, bv.SEED, 1)
    st, rep, names = batch.run(eng, op)
    assert all(s in names for s in bv.STAGES), names
    assert np.array_equal(st, off), np.nonzero(st != off)[0][:10]
    assert sorted(np.nonzero(st != 1)[0]) == sorted(bad)
    # every group with a bad item failed, every other group passed
    assert rep == (len(SIZES), len(SIZES) - 4, batch.n), rep
    _check_oracle_sample(iss, batch, bad, st, op)


@pytest.mark.job_form(True)
@pytest.mark.parametrize("curve", CURVES)
def test_latency_form_core_and_wire(curve):
    iss, batch, bad = _scene(curve, SMALL)
    eng, kst = kc.keyed_engine(iss, iss.pks)
    for op in ("pv", "vf"):
        off, _, _ = batch.run(eng, op)
        assert sorted(np.nonzero(off != 1)[0]) == sorted(bad)
        eng.set_keyed_batch_verification(True, bv.SEED, 1)
        for form in ("core", "wire"):
            st, rep, names = batch.run(eng, op, form)
            assert np.array_equal(st, off), (op, form, np.nonzero(st != off)[0][:10])
            assert rep == (len(SMALL), len(SMALL) - 3, batch.n), (op, form, rep)
        eng.set_keyed_batch_verification(False)


def test_throughput_form_wire_and_threshold():
    # a threshold inside the sizes leaves the smaller keys to the per-item kernel; a job run twice
    iss, batch, bad = _scene("bls12_381", SMALL)
    eng, kst = kc.keyed_engine(iss, iss.pks)
    off, _, _ = batch.run(eng, "pv", "wire")
    eng.set_keyed_batch_verification(True, bv.SEED, 64)
    job = batch.submit(eng, "pv", "wire")
    job.wait()
    assert np.array_equal(job.result, off)
    groups, passed, items = job.bv_report()
    assert (groups, items) == (2, 64 + 65) and passed == 0          # the keys with at least 64 items
    job.run()
    job.wait()
    assert np.array_equal(job.result, off) and job.bv_report() == (2, 0, 129)
    job.free()


def test_key_set_replaced_in_flight():
    iss, batch, bad = _scene("bls12_381", SMALL)
    eng, kst = kc.keyed_engine(iss, iss.pks)
    eng.set_keyed_batch_verification(True, bv.SEED, 1)
    want, rep, _ = batch.run(eng, "pv")
    jobs = [batch.submit(eng, "pv") for _ in range(3)]
    eng.set_public_keys(iss.pks[::-1])                             # every key moves; the jobs in flight keep the old set
    for j in jobs:
        j.wait()
        assert np.array_equal(j.result, want) and j.bv_report() == rep
        j.free()
