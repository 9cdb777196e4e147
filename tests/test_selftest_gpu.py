"""GPU self-test: the six-lane (wavefront-cooperative) Fp12 arithmetic on the GPU against the one-lane code (run on the host),
operation by operation, and the one-lane multiplication against the oracle's Fp12.

The batched entry (bbs_selftest_f12_batch) lays its items out as the pairing kernels do -- ten six-lane groups per wavefront --
so the tests below it run every operation at every group position, with gated neighbours and ragged wavefronts, on the edge
operands of tests/f12_cases.py, all compared exactly with the oracle's big integers (the line multiplication, whose entries
are in the library's scaling, with the one-lane code)."""
import ctypes
import os
import random
import sys

import numpy as np
import pytest

from bbs_sign_amd import Engine, _lib
from oracle.curves import CURVES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402

pytestmark = pytest.mark.gpu

# (the ops of the single entry, as the first test has always listed them; the batched tests below use fc.OPS, which adds is_one)
OPS = {0: "mul", 1: "frob1", 2: "frob2", 3: "frob3", 4: "inv", 5: "conj", 6: "line", 7: "final_exp", 8: "sqr",
       10: "cyclo_sqr", 11: "pow_x"}


def _run(eng, op, a, b):
    fpb = eng.fpb
    ab = np.frombuffer(b"".join(int(x).to_bytes(fpb, "little") for x in a), dtype=np.uint8).copy()
    bb = np.frombuffer(b"".join(int(x).to_bytes(fpb, "little") for x in b), dtype=np.uint8).copy()
    o1 = np.zeros(12 * fpb, dtype=np.uint8)
    o2 = np.zeros(12 * fpb, dtype=np.uint8)
    rc = eng.lib.bbs_selftest_f12(eng.h, op, ab.ctypes.data_as(_lib.c_u8p), bb.ctypes.data_as(_lib.c_u8p),
                                  o1.ctypes.data_as(_lib.c_u8p), o2.ctypes.data_as(_lib.c_u8p))
    assert rc == 0
    dec = lambda o: [int.from_bytes(o.tobytes()[k * fpb:(k + 1) * fpb], "little") for k in range(12)]
    return dec(o1), dec(o2)


def _tower_to_w(c, t):
    # tower order: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2 (each Fp2 = 2 Fp) ; w-basis g0..g5
    f2 = [(t[2 * k], t[2 * k + 1]) for k in range(6)]
    return [f2[0], f2[3], f2[1], f2[4], f2[2], f2[5]]


@pytest.mark.parametrize("curve", ["bls12_381", "bn254"])
def test_six_lane_fp12_matches_one_lane(curve):
    c = CURVES[curve]
    rng = random.Random(5)
    eng = Engine(curve)
    for op, name in OPS.items():
        for rep in range(2):
            a = [rng.randrange(c.p) for _ in range(12)]
            b = [rng.randrange(c.p) for _ in range(12)]
            if op == 6:
                P = c.g1_mul(c.g1, rng.randrange(1, c.r))
                b[0], b[1] = P
            s, d = _run(eng, op, a, b)
            assert s == d, (curve, name, rep)
            # ... and against the ORACLE's Fp12 (oracle/curves.py, w-basis), operation by operation: the one-lane and
            # the six-lane code share tower.hpp, so their agreement alone would not localise a break in it
            x = _tower_to_w(c, a)
            if op >= 10:                                  # the host makes the input cyclotomic: x^((p^6-1)(p^2+1))
                x = c.f12_mul(c.f12_conj(x), c.f12_inv(x))
                x = c.f12_mul(c.f12_frob(c.f12_frob(x)), x)
            frobk = lambda v, k: v if k == 0 else frobk(c.f12_frob(v), k - 1)
            want = None
            if op == 0:
                want = c.f12_mul(x, _tower_to_w(c, b))
            elif op in (1, 2, 3):
                want = frobk(x, op)
            elif op == 4:
                want = c.f12_inv(x)
            elif op == 5:
                want = c.f12_conj(x)
            elif op == 7:                                 # BLS12-381 raises to 3 (p^12-1)/r, BN254 to (p^12-1)/r
                want = c.final_exp(x)
                if curve == "bls12_381":
                    want = c.f12_pow(want, 3)
            elif op in (8, 10):
                want = c.f12_sqr(x)
            elif op == 11:                                # x^(curve parameter), the sign by conjugation (x unitary)
                want = c.f12_pow(x, abs(c.x_param))
                if c.x_param < 0:
                    want = c.f12_conj(want)
            if want is not None:
                assert _tower_to_w(c, d) == [tuple(v) for v in want], (curve, name, rep, "six-lane vs oracle")
    eng.close()


# =================================================================================================
# the batched entry: group positions, gating, edge operands, is_one; the pairing kernel under divergence
# =================================================================================================
SENTINEL = 0xA5
CURVE_NAMES = ["bls12_381", "bn254"]
ORACLE_OPS = [op for op in fc.OPS if op != 6]
_want_cache = {}


@pytest.fixture(scope="module", params=CURVE_NAMES)
def ctx(request):
    """(curve, engine with a public key: line table 0 is the key's)"""
    c = CURVES[request.param]
    eng = Engine(request.param)
    eng.set_public_key(fc.pairing_pk(request.param))
    yield c, eng
    eng.close()


def _want(c, op, x, y):
    key = (c.name, op, tuple(x), tuple(y))
    if key not in _want_cache:
        _want_cache[key] = fc.expected(c, op, x, y)
    return _want_cache[key]


def _run_batch(eng, c, op, items, active=None, line=(1, 3)):
    """items: [(x, y)].  Returns (out_dist rows, flags, out_single rows) as uint8, prefilled with SENTINEL."""
    n, row = len(items), 12 * c.fp_bytes
    a = np.frombuffer(b"".join(fc.tower_bytes(c, x) for x, _ in items), dtype=np.uint8).copy()
    b = np.frombuffer(b"".join(fc.tower_bytes(c, y) for _, y in items), dtype=np.uint8).copy()
    od = np.full(n * row, SENTINEL, dtype=np.uint8)
    os_ = np.full(n * row, SENTINEL, dtype=np.uint8)
    fl = np.full(n, SENTINEL, dtype=np.uint8)
    act = None if active is None else np.array(active, dtype=np.int8)
    rc = eng.lib.bbs_selftest_f12_batch(eng.h, op, n, a.ctypes.data_as(_lib.c_u8p), b.ctypes.data_as(_lib.c_u8p),
                                        None if act is None else act.ctypes.data_as(_lib.c_i8p), line[0], line[1],
                                        os_.ctypes.data_as(_lib.c_u8p) if op == 6 else None, od.ctypes.data_as(_lib.c_u8p),
                                        fl.ctypes.data_as(_lib.c_i8p))
    assert rc == 0, (c.name, fc.OPS[op], n, rc)
    return od.reshape(n, row), fl, os_.reshape(n, row)


def _check_batch(c, op, cases, active, got, what):
    """Every active item equals the oracle (op 6: the one-lane result) and has its flag; every inactive item's bytes are
    still the sentinel.  cases: [(family, x, y)]."""
    od, fl, os_ = got
    for i, (fam, x, y) in enumerate(cases):
        tag = (c.name, fc.OPS[op], "item %d = wavefront %d group %d" % (i, i // 10, i % 10), fam) + tuple(what)
        if active is not None and not active[i]:
            assert (od[i] == SENTINEL).all() and fl[i] == SENTINEL and (os_[i] == SENTINEL).all(), tag + ("inactive item written",)
            continue
        if op == 6:
            assert not (os_[i] == SENTINEL).all(), tag
            assert od[i].tobytes() == os_[i].tobytes(), tag + ("six-lane vs one-lane",)
        else:
            assert fc.tower_from_bytes(c, od[i].tobytes()) == _want(c, op, x, y), tag + ("six-lane vs oracle",)
        assert fl[i] == (int(list(x) == fc.one()) if op == 12 else 1), tag + ("flag", int(fl[i]))


@pytest.mark.parametrize("op", sorted(fc.OPS))
def test_every_group_position_with_gated_neighbours(ctx, op):
    """n = 1, 10, 11, 23: one group, a full wavefront, one item into the second, a ragged third; a different operand in
    every group; all groups live, only the last group of each wavefront, alternating, none."""
    c, eng = ctx
    pool = fc.position_pool(c, op)
    lines = [(1, 3), (0, fc.n_lines(c) - 1)] if op == 6 else [(1, 3)]
    for n in (1, 10, 11, 23):
        cases = pool[:n]
        for mask, active in fc.active_masks(n).items():
            for line in lines:
                got = _run_batch(eng, c, op, [(x, y) for _, x, y in cases], active, line)
                _check_batch(c, op, cases, active, got, ("n", n, "mask", mask, "line", line))


def _rotations(fams):
    """Shifts s (item j runs at position (j + s) mod n) such that every family visits group 9 and a second wavefront"""
    n = len(fams)
    g9, w1, chosen = set(), set(), []
    for s in range(n):
        at = [(fams[j], (j + s) % n) for j in range(n)]
        new9 = {f for f, q in at if q % 10 == 9} - g9
        new1 = {f for f, q in at if q >= 10} - w1
        if s == 0 or new9 or new1:
            chosen.append(s)
            g9 |= new9
            w1 |= new1
        if g9 == w1 == set(fams):
            break
    assert g9 == w1 == set(fams), (set(fams) - g9, set(fams) - w1)
    return chosen


@pytest.mark.parametrize("op", sorted(op for op in fc.OPS if op != 12))
def test_edge_operands_at_all_positions(ctx, op):
    """Every operand family through every operation it applies to (zero, one, minus one, c w^m, all 36 w^i w^j, internal
    representations of p - 1 and its kin on all coefficients of both operands, subfields, dense), spread over the ten groups
    and rotated until each family has run in group 9 and in a second wavefront."""
    c, eng = ctx
    cases = fc.cases(c, op)
    n = len(cases)
    last = fc.n_lines(c) - 1
    lines = [(t, e) for t in (0, 1) for e in (0, 3, last)] if op == 6 else [(1, 3)]
    for r, s in enumerate(_rotations([f for f, _, _ in cases])):
        rot = [cases[(q - s) % n] for q in range(n)]
        for line in (lines if r == 0 else [lines[r % len(lines)]]):
            got = _run_batch(eng, c, op, [(x, y) for _, x, y in rot], None, line)
            _check_batch(c, op, rot, None, got, ("shift", s, "line", line))


def test_is_one_sees_every_coefficient(ctx):
    """d_is_one is the soundness gate of verify and proof_verify: among items that differ from one in a SINGLE Fp coefficient
    (1 for 0, p - 1, the right internal representation with its lowest or its highest limb changed) only one itself gives 1,
    wherever in the wavefronts it sits."""
    c, eng = ctx
    items = fc.is_one_cases(c)
    (the_one,), others = [it for it in items if it[2]], [it for it in items if not it[2]]
    assert len(others) == 47
    for at in (0, 5, 9, 10, 14, 29, 40, 47):
        batch = others[:at] + [the_one] + others[at:]
        od, fl, _ = _run_batch(eng, c, 12, [(x, fc.zero()) for _, x, _ in batch])
        for i, (what, x, flag) in enumerate(batch):
            tag = (c.name, "is_one", "item %d = wavefront %d group %d" % (i, i // 10, i % 10), what, "one at", at)
            assert fl[i] == flag, tag + ("got", int(fl[i]))
            assert fc.tower_from_bytes(c, od[i].tobytes()) == [tuple(g) for g in x], tag


def test_pairing_kernel_with_gated_skipping_and_full_items_side_by_side(ctx):
    """The production kernel (bbs_pairing_product2_is_one_batch: PairPrep, then the fused six-lane kernel in every job form --
    the primitive has no latency form) at n = 23: valid and invalid pairs, Pa / Pb / both the identity (the group skips one
    or both Miller loops) and points off the curve (status -41: the group is gated out of a live wavefront), the kinds
    rotated so that each sits at every group position and in the ragged wavefront.  Statuses from the oracle's pairing."""
    c, eng = ctx
    by_kind = {}
    for rot in range(6):
        pk, items = fc.pairing_batch(c.name, 23, rot)
        st = eng.pairing_product2_is_one_batch([it[1] for it in items], [it[2] for it in items])
        for i, (kind, _, _, want) in enumerate(items):
            assert st[i] == want, (c.name, "rotation", rot, "item %d = wavefront %d group %d" % (i, i // 10, i % 10), kind, int(st[i]), want)
            by_kind.setdefault(kind, set()).add(want)
    assert by_kind == {"valid": {1}, "invalid": {0}, "Pa identity": {0}, "Pb identity": {0}, "both identity": {1}, "off curve": {-41}}


def test_selftest_entries_check_their_arguments(ctx):
    """The argument checks of the real build (the CPU build refuses every call): ops that do not exist, a line table or entry
    that does not exist, the key's table without a key, n = 0, NULL buffers, a value that is not below p."""
    c, eng = ctx
    lib, h = eng.lib, eng.h
    E_ARG, E_STATE = -100, -102
    row = 12 * c.fp_bytes
    x = np.frombuffer(fc.tower_bytes(c, fc.one()) * 2, dtype=np.uint8).copy()
    od = np.full(2 * row, SENTINEL, dtype=np.uint8)
    fl = np.full(2, SENTINEL, dtype=np.uint8)
    u8, i8 = lambda v: v.ctypes.data_as(_lib.c_u8p), lambda v: v.ctypes.data_as(_lib.c_i8p)
    call = lambda op, n=2, a=x, line=(1, 3), out=od, flag=fl, hh=h: lib.bbs_selftest_f12_batch(
        hh, op, n, None if a is None else u8(a), u8(x), None, line[0], line[1], None, None if out is None else u8(out),
        None if flag is None else i8(flag))
    for op in (-1, 9, 13):
        assert call(op) == E_ARG, op
    for line in ((2, 3), (-1, 3), (1, -1), (1, fc.n_lines(c)), (0, fc.n_lines(c))):
        assert call(6, line=line) == E_ARG, line
    assert call(0, a=None) == E_ARG and call(0, out=None) == E_ARG and call(0, flag=None) == E_ARG and call(0, hh=None) == E_ARG
    bad = x.copy()
    bad[:c.fp_bytes] = np.frombuffer(c.p.to_bytes(c.fp_bytes, "little"), dtype=np.uint8)
    assert call(0, a=bad) == E_ARG
    assert (od == SENTINEL).all() and (fl == SENTINEL).all()                  # a refused call writes nothing
    assert call(0, n=0) == 0 and call(0, n=0, a=None, out=None, flag=None) == 0
    assert (od == SENTINEL).all() and (fl == SENTINEL).all()
    assert call(6, line=(1, fc.n_lines(c) - 1)) == 0 and call(6, line=(0, 0)) == 0 and list(fl) == [1, 1]
    assert lib.bbs_selftest_f12(h, 12, u8(x), u8(x), u8(od), u8(od)) == E_ARG                 # is_one has no place in the single entry
    nokey = Engine(c.name)                                                    # the key's line table needs a key
    try:
        assert call(6, line=(0, 0), hh=nokey.h) == E_STATE
        assert call(6, line=(1, 0), hh=nokey.h) == 0
    finally:
        nokey.close()
