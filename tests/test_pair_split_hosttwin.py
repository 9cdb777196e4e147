"""bbs_selftest_pairing_split through the TEST-ONLY host twin, both curves: the one-lane stages PairPrep -> PairMiller ->
PairFinal against the oracle (tests/pair_split_cases.py).  This is where the expectations of tests/test_pair_split_gpu.py are
proved right before a GPU sees them: the relation of a Miller value to the oracle's miller_loop in both line forms, the
statuses of the item kinds, and the statuses of the final stage on given values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402
import pair_split_cases as ps             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVE_NAMES = ["bls12_381", "bn254"]
SENTINEL = 0xA5
E_ARG, E_STATE = -100, -102


@pytest.fixture(scope="module")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.fixture(scope="module", params=CURVE_NAMES)
def ctx(request, twin):
    from bbs_sign_amd import Engine
    from oracle.curves import CURVES
    eng = Engine(request.param, lib_path=twin)
    eng.set_public_key(fc.pairing_pk(request.param))
    yield CURVES[request.param], eng
    eng.close()


@pytest.mark.parametrize("negate_b", [0, 1])
@pytest.mark.parametrize("unit", [True, False], ids=["unit", "c_nl"])
def test_one_lane_miller_values_and_statuses(ctx, unit, negate_b):
    """n = 23, all six kinds, both line forms, negate_b 0 and 1.  The statement that holds for the one-lane code, and that
    the GPU test then asserts of the six-lane values: value / miller_loop(P, Q) lies in Fp in the (c, nl) form, and in Fp2
    -- outside Fp, for every point of the pool -- in the unit form.  With negate_b the library is handed -Pb and the second
    value is compared with miller_loop(Pb, BP2) = miller_loop(-(-Pb), BP2).  An identity slot gives exactly one; an off-curve
    item is -41 and its rows are untouched; the statuses are the oracle's pairing_product_is_one."""
    c, eng = ctx
    eng.set_unit_lines(unit)
    for rot in (0, 3):
        _, items = ps.miller_batch(c.name, ps.N_TWIN, rot, negate_b)
        rc, st, ms, _ = eng.selftest_pairing_split([it[1] for it in items], [it[2] for it in items], negate_b, dist=False, fill=SENTINEL)
        tag = (c.name, "unit" if unit else "(c, nl)", "negate_b", negate_b, "rotation", rot)
        assert rc == 0, tag
        assert [int(s) for s in st] == [it[4] for it in items], tag
        rows = [None if it[4] == -41 else ms[i] for i, it in enumerate(items)]
        assert all((ms[i] == SENTINEL).all() for i, it in enumerate(items) if it[4] == -41), tag + ("rows of a refused item",)
        ps.check_miller_rows(c, items, rows, unit, ("Fp2",) if unit else ("Fp",), tag)
    eng.set_unit_lines(True)


def test_the_relation_rejects_what_the_boolean_cannot_see(ctx):
    """The relation is sharper than the status: a value with one coefficient off by one, a value times w^2 (an element of
    Fp6, which the final exponentiation kills: the status would not change) and the value of another point all fail it."""
    c, eng = ctx
    _, items = ps.miller_batch(c.name, 7, 0, 0)
    rc, st, ms, _ = eng.selftest_pairing_split([it[1] for it in items], [it[2] for it in items], 0, dist=False)
    assert rc == 0
    (kind, Pa, _, Pb, _), (kind6, Pa6, _, _, _) = items[0], items[6]
    assert kind == kind6 == "valid" and Pa != Pa6
    for pair, P in ((0, Pa), (1, Pb)):
        v = fc.tower_from_bytes(c, ms[0][pair].tobytes())
        assert ps.relation(c, v, P, pair) == "Fp2"
        for k in range(6):
            off = list(v)
            off[k] = ((v[k][0] + 1) % c.p, v[k][1])
            assert ps.relation(c, off, P, pair) == "none", (c.name, pair, k)
        assert ps.relation(c, [tuple(g) for g in c.f12_mul(v, fc.monomial((1, 0), 2))], P, pair) == "none"
    assert ps.relation(c, fc.tower_from_bytes(c, ms[6][0].tobytes()), Pa, 0) == "none"
    assert ps.relation(c, fc.tower_from_bytes(c, ms[0][0].tobytes()), Pa, 1) == "none"          # the key's value against BP2


def test_rotations_cover_every_position():
    K = len(ps.FINAL_KINDS)
    for n in ps.FINAL_SIZES:
        rots = ps.final_rotations(n)
        group0, group9 = range(0, n, 10), range(9, n, 10)
        ragged = range(n - n % 10, n) if n > 10 else []
        for where in (group0, group9, ragged):
            assert not where or {(pos + r) % K for r in rots for pos in where} == set(range(K)), (n, list(where))
    for n in ps.MILLER_SIZES:
        for pos in {0, min(9, n - 1), n - 1}:
            assert {fc.pairing_kinds(n, r)[pos] for r in range(6)} == set(fc.PAIR_KINDS), (n, pos)


def test_inactive_items_are_untouched(ctx):
    c, eng = ctx
    _, items = ps.miller_batch(c.name, ps.N_TWIN, 1, 0)
    for mask, active in fc.active_masks(ps.N_TWIN).items():
        rc, st, ms, _ = eng.selftest_pairing_split([it[1] for it in items], [it[2] for it in items], 0, active=active, dist=False,
                                                   fill=SENTINEL)
        assert rc == 0
        for i, it in enumerate(items):
            if active[i]:
                assert st[i] == it[4], (c.name, mask, i)
                assert (ms[i] == SENTINEL).all() == (it[4] == -41), (c.name, mask, i)
            else:
                assert st[i] == np.int8(SENTINEL - 256) and (ms[i] == SENTINEL).all(), (c.name, mask, i, "inactive item written")


def test_final_stage_on_given_values(ctx):
    """PairFinal on miller_in: the kinds of pair_split_cases.final_pool (no zero operand: see there), rotated and masked."""
    c, eng = ctx
    for n in ps.FINAL_SIZES:
        for rot in ps.final_rotations(n)[:3]:
            items = ps.final_batch(c.name, n, rot)
            for mask, active in fc.active_masks(n).items():
                rc, st, ms, _ = eng.selftest_pairing_split(miller_in=ps.miller_in_bytes(c, items), active=active, dist=False, fill=SENTINEL)
                assert rc == 0 and (ms == SENTINEL).all()
                want = [it[3] if active[i] else SENTINEL - 256 for i, it in enumerate(items)]
                assert [int(s) for s in st] == want, (c.name, n, rot, mask)


def test_round_trip_of_the_one_lane_values(ctx):
    """The values of the first mode, fed back through miller_in, give the first mode's statuses."""
    c, eng = ctx
    _, items = ps.miller_batch(c.name, ps.N_TWIN, 2, 0)
    rc, st, ms, _ = eng.selftest_pairing_split([it[1] for it in items], [it[2] for it in items], 0, dist=False)
    assert rc == 0
    live = [i for i, it in enumerate(items) if it[4] != -41]
    rc, st2, _, _ = eng.selftest_pairing_split(miller_in=b"".join(ms[i].tobytes() for i in live), dist=False)
    assert rc == 0 and [int(s) for s in st2] == [int(st[i]) for i in live]


def test_argument_checks(ctx, twin):
    """NULL handle / status, missing points without miller_in, negate_b outside {0, 1}, a value not below p, miller_dist on
    the host twin: BBS_E_ARG; no public key: BBS_E_STATE; n = 0: BBS_OK.  None of these calls writes anything."""
    from bbs_sign_amd import Engine, _lib
    c, eng = ctx
    lib, h = eng.lib, eng.h
    row = 12 * c.fp_bytes
    n = 2
    _, items = ps.miller_batch(c.name, n, 0, 0)
    pts = lambda k: np.frombuffer(b"".join(eng._g1(it[k]) for it in items), dtype=np.uint8).copy()
    pa, pb = pts(1), pts(2)
    ms = np.full(n * 2 * row, SENTINEL, dtype=np.uint8)
    md = np.full(n * 2 * row, SENTINEL, dtype=np.uint8)
    st = np.full(n, SENTINEL, dtype=np.uint8)
    u8 = lambda v: None if v is None else v.ctypes.data_as(_lib.c_u8p)
    i8 = lambda v: None if v is None else v.ctypes.data_as(_lib.c_i8p)

    def call(hh=h, n=n, a=pa, b=pb, neg=0, mi=None, single=ms, dist=None, status=st):
        return lib.bbs_selftest_pairing_split(hh, n, u8(a), u8(b), neg, None, u8(mi), u8(single), u8(dist), i8(status))

    assert call(hh=None) == E_ARG and call(status=None) == E_ARG
    assert call(a=None) == E_ARG and call(b=None) == E_ARG
    assert call(neg=2) == E_ARG and call(neg=-1) == E_ARG
    assert call(dist=md) == E_ARG                                             # no six-lane values in this build
    good = np.frombuffer(ps.miller_in_bytes(c, ps.final_batch(c.name, n, 0)), dtype=np.uint8).copy()
    bad = good.copy()
    bad[-c.fp_bytes:] = np.frombuffer(c.p.to_bytes(c.fp_bytes, "little"), dtype=np.uint8)
    assert call(mi=bad, a=None, b=None) == E_ARG
    nokey = Engine(c.name, lib_path=twin)
    try:
        assert call(hh=nokey.h) == E_STATE and call(hh=nokey.h, mi=good) == E_STATE
    finally:
        nokey.close()
    assert call(n=0) == 0 and call(n=0, a=None, b=None, single=None) == 0
    assert (ms == SENTINEL).all() and (md == SENTINEL).all() and (st == SENTINEL).all()
    assert call(mi=good, a=None, b=None) == 0 and list(st.view(np.int8)) == [1, 1] and (ms == SENTINEL).all()
    assert call() == 0 and list(st.view(np.int8)) == [it[4] for it in items]
