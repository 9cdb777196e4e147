"""GPU pairing self-test (bbs_selftest_pairing_split): the latency-form kernels PairMillerHalf and PairFinalDist, launched
unchanged with a job's geometry, seen through the VALUES they hand over and not only through their boolean.

The Miller values of every item are compared byte for byte with the one-lane code (run on the host), and with the oracle's
miller_loop through the relation that tests/test_pair_split_hosttwin.py establishes for the one-lane code: value /
miller_loop(P, Q) lies in Fp in the (c, nl) form and in Fp2 (outside Fp) in the unit form.  The statuses are the oracle's
and, item by item, those of the fused kernel PairDist.  The final stage is also run on chosen values (miller_in)."""
import os
import sys

import numpy as np
import pytest

from bbs_sign_amd import Engine, _lib
from oracle.curves import CURVES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402
import pair_split_cases as ps             # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
UNTOUCHED = SENTINEL - 256                # the sentinel as a status
CURVE_NAMES = ["bls12_381", "bn254"]
E_ARG, E_STATE = -100, -102


@pytest.fixture(scope="module", params=CURVE_NAMES)
def ctx(request):
    eng = Engine(request.param)
    eng.set_public_key(fc.pairing_pk(request.param))
    yield CURVES[request.param], eng
    eng.close()


def _where(i):
    return "item %d = wavefront %d group %d" % (i, i // 10, i % 10)


@pytest.mark.parametrize("n", ps.MILLER_SIZES)
def test_miller_values_at_every_group_position(ctx, n):
    """n = 1, 10, 11, 16 (the shape of batch verification's combined checks), 23; the six kinds rotated through every group
    position and the ragged wavefront; all groups live, the last of each wavefront, alternating, none; both line forms;
    negate_b at n = 16 and 23 (the library is handed -Pb, so the product and its status stay the pool's).  Per processed
    item: six-lane == one-lane byte for byte, the oracle relation (Fp in the (c, nl) form, Fp2 outside Fp in the unit form:
    see test_pair_split_hosttwin.py), exactly one for an identity slot, the oracle's status, the fused kernel's status.  An
    off-curve item is -41 with its rows untouched; nothing of an inactive item is written."""
    c, eng = ctx
    try:
        for unit in (True, False):
            eng.set_unit_lines(unit)
            for negate_b in ((0, 1) if n in ps.NEGATE_SIZES else (0,)):
                for rot in range(len(fc.PAIR_KINDS)):
                    _, items = ps.miller_batch(c.name, n, rot, negate_b)
                    pa, pb = [it[1] for it in items], [it[2] for it in items]
                    fused = eng.pairing_product2_is_one_batch(pa, [it[3] for it in items])
                    for mask, active in fc.active_masks(n).items():
                        tag = (c.name, "unit" if unit else "(c, nl)", "negate_b", negate_b, "n", n, "rotation", rot, "mask", mask)
                        rc, st, ms, md = eng.selftest_pairing_split(pa, pb, negate_b, active=active, fill=SENTINEL)
                        assert rc == 0, tag + ("rc", rc)
                        rows = [None] * n
                        for i, (kind, _, _, _, want) in enumerate(items):
                            t = tag + (_where(i), kind)
                            if not active[i]:
                                assert st[i] == UNTOUCHED and (ms[i] == SENTINEL).all() and (md[i] == SENTINEL).all(), t + ("inactive item written",)
                                continue
                            assert st[i] == want, t + ("status", int(st[i]), "oracle", want)
                            assert st[i] == fused[i], t + ("status", int(st[i]), "fused kernel", int(fused[i]))
                            if want == -41:
                                assert (ms[i] == SENTINEL).all() and (md[i] == SENTINEL).all(), t + ("rows of a refused item",)
                                continue
                            assert not (md[i][0] == SENTINEL).all() and not (md[i][1] == SENTINEL).all(), t
                            for pair in (0, 1):
                                assert md[i][pair].tobytes() == ms[i][pair].tobytes(), t + ("pair", pair, "six-lane vs one-lane")
                            rows[i] = md[i]
                        ps.check_miller_rows(c, items, rows, unit, ("Fp2",) if unit else ("Fp",), tag)
    finally:
        eng.set_unit_lines(True)


@pytest.mark.parametrize("n", ps.FINAL_SIZES)
def test_final_stage_on_given_values(ctx, n):
    """PairFinalDist alone on chosen values: (x, 1/x), (x, s/x) with s dense in Fp6 and s in Fp2, (x, -1/x), (x, g/x) with g
    of order r, dense pairs, (one, one), products that differ from one in a single coefficient (one + w: 0; one - i w^3, in
    Fp4: 1), p - 1 in every coefficient of both operands; the statuses from the oracle's final_exp(g0 g1) == 1.  The kinds
    rotated over the group positions, under the four masks.  A zero operand is left out: the final exponentiation inverts,
    no input of the library reaches it with a zero, and the reference does not define its result."""
    c, eng = ctx
    for rot in ps.final_rotations(n):
        items = ps.final_batch(c.name, n, rot)
        mi = ps.miller_in_bytes(c, items)
        for mask, active in fc.active_masks(n).items():
            rc, st, ms, md = eng.selftest_pairing_split(miller_in=mi, active=active, fill=SENTINEL)
            assert rc == 0, (c.name, n, rot, mask, rc)
            assert (ms == SENTINEL).all() and (md == SENTINEL).all()
            for i, (kind, _, _, want) in enumerate(items):
                assert st[i] == (want if active[i] else UNTOUCHED), (c.name, "n", n, "rotation", rot, "mask", mask, _where(i), kind, int(st[i]), want)


@pytest.mark.parametrize("unit", [True, False], ids=["unit", "c_nl"])
def test_round_trip(ctx, unit):
    """The values PairMillerHalf left, fed back through miller_in, give the statuses of the first mode."""
    c, eng = ctx
    try:
        eng.set_unit_lines(unit)
        for n, rot, negate_b in ((16, 1, 1), (23, 4, 0)):
            _, items = ps.miller_batch(c.name, n, rot, negate_b)
            rc, st, _, md = eng.selftest_pairing_split([it[1] for it in items], [it[2] for it in items], negate_b, single=False)
            assert rc == 0
            live = [i for i, it in enumerate(items) if it[4] != -41]
            rc, st2, _, _ = eng.selftest_pairing_split(miller_in=b"".join(md[i].tobytes() for i in live))
            assert rc == 0 and [int(s) for s in st2] == [int(st[i]) for i in live], (c.name, unit, n, rot)
    finally:
        eng.set_unit_lines(True)


def test_argument_checks(ctx):
    """NULL handle / status, missing points without miller_in, negate_b outside {0, 1}, a value not below p: BBS_E_ARG; no
    public key: BBS_E_STATE; n = 0: BBS_OK.  None of these calls writes anything."""
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

    def call(hh=h, n=n, a=pa, b=pb, neg=0, mi=None, single=ms, dist=md, status=st):
        return lib.bbs_selftest_pairing_split(hh, n, u8(a), u8(b), neg, None, u8(mi), u8(single), u8(dist), i8(status))

    assert call(hh=None) == E_ARG and call(status=None) == E_ARG
    assert call(a=None) == E_ARG and call(b=None) == E_ARG
    assert call(neg=2) == E_ARG and call(neg=-1) == E_ARG
    good = np.frombuffer(ps.miller_in_bytes(c, ps.final_batch(c.name, n, 0)), dtype=np.uint8).copy()
    bad = good.copy()
    bad[-c.fp_bytes:] = np.frombuffer(c.p.to_bytes(c.fp_bytes, "little"), dtype=np.uint8)
    assert call(mi=bad, a=None, b=None) == E_ARG
    nokey = Engine(c.name)
    try:
        assert call(hh=nokey.h) == E_STATE and call(hh=nokey.h, mi=good) == E_STATE
    finally:
        nokey.close()
    assert call(n=0) == 0 and call(n=0, a=None, b=None, single=None, dist=None) == 0
    assert (ms == SENTINEL).all() and (md == SENTINEL).all() and (st == SENTINEL).all()       # refused or empty: nothing written
    assert call(mi=good, a=None, b=None) == 0 and list(st.view(np.int8)) == [1, 1]
    assert (ms == SENTINEL).all() and (md == SENTINEL).all()
    assert call(single=None, dist=None) == 0 and list(st.view(np.int8)) == [it[4] for it in items]
    assert call() == 0 and ms.tobytes() == md.tobytes() and not (md == SENTINEL).all()
