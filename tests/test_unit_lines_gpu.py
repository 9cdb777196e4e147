"""Line tables in the unit form (bbs_ctx_set_unit_lines) on the GPU, both curves: the six-lane line multiplication in both
forms (the op 6 self-test: against the one-lane code, and the two forms against each other through the oracle's field
arithmetic), and verify / proof_verify batches of three pairing wavefronts in both forms, single-key and keyed, against the
oracle's statuses (tests/unit_lines_cases.py)."""
import os
import sys

import numpy as np
import pytest

from bbs_sign_amd import _lib
from oracle import bbs
from oracle.curves import CURVES

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f12_cases as fc                    # noqa: E402
import keyed_cases as kc                  # noqa: E402
import keyreg_cases as kr                 # noqa: E402
import unit_lines_cases as ul             # noqa: E402

pytestmark = pytest.mark.gpu

CURVE_NAMES = ["bls12_381", "bn254"]
SENTINEL = 0xA5


def _line_batch(eng, c, items, line):
    """bbs_selftest_f12_batch, op 6: (six-lane rows, one-lane rows, flags)"""
    n, row = len(items), 12 * c.fp_bytes
    a = np.frombuffer(b"".join(fc.tower_bytes(c, x) for x, _ in items), dtype=np.uint8).copy()
    b = np.frombuffer(b"".join(fc.tower_bytes(c, y) for _, y in items), dtype=np.uint8).copy()
    od = np.full(n * row, SENTINEL, dtype=np.uint8)
    os_ = np.full(n * row, SENTINEL, dtype=np.uint8)
    fl = np.full(n, SENTINEL, dtype=np.uint8)
    rc = eng.lib.bbs_selftest_f12_batch(eng.h, 6, n, a.ctypes.data_as(_lib.c_u8p), b.ctypes.data_as(_lib.c_u8p), None, line[0], line[1],
                                        os_.ctypes.data_as(_lib.c_u8p), od.ctypes.data_as(_lib.c_u8p), fl.ctypes.data_as(_lib.c_i8p))
    assert rc == 0, (c.name, line, rc)
    return od.reshape(n, row), os_.reshape(n, row), fl


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_line_multiplication_in_both_forms(curve):
    """n = 11: two wavefronts, the first and the last group position.  Per table and line: six-lane == one-lane in each form,
    and (f * unit line) * c == f * (c, nl) line / R with c read from the table."""
    c = CURVES[curve]
    suite = bbs.SUITES[curve]
    pk = fc.pairing_pk(curve)
    eng = kc.make_engine(curve, kc.gens_for(suite, 2), suite.api_id, pk=pk)
    items = [(x, y) for _, x, y in fc.position_pool(c, 6)[:11]]
    # the (c, nl) tables of the key and of BP2, through the registration hook
    eng.set_unit_lines(False)
    ent, st, _ = kr.key_entries(eng, 0, keys=[pk, c.g2])
    assert st == [1, 1]
    tabs = [ul.parse_table(curve, e)[0] for e in ent]
    last = fc.n_lines(c) - 1
    for table in (0, 1):
        for index in (0, 3, last):
            out = {}
            for unit in (True, False):
                eng.set_unit_lines(unit)
                od, os_, fl = _line_batch(eng, c, items, (table, index))
                for i in range(len(items)):
                    tag = (curve, "unit" if unit else "(c, nl)", "table", table, "line", index, "item", i)
                    assert fl[i] == 1 and not (os_[i] == SENTINEL).all(), tag
                    assert od[i].tobytes() == os_[i].tobytes(), tag + ("six-lane vs one-lane",)
                out[unit] = [fc.tower_from_bytes(c, od[i].tobytes()) for i in range(len(items))]
            cc = tabs[table][index][0]
            rinv = pow(fc.mont_r(c), -1, c.p)          # the unit line is the (c, nl) line times R^-1 / c
            for i in range(len(items)):
                scaled = [c.f2_mul(tuple(g), cc) for g in out[True][i]]
                want = [(g[0] * rinv % c.p, g[1] * rinv % c.p) for g in out[False][i]]
                assert scaled == want, (curve, "table", table, "line", index, "item", i, "unit * c vs (c, nl) / R")
    eng.close()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_tables_on_the_device(curve):
    """the entries of both forms by the KeyBuild stage on the GPU and by the host functions: equal, and nl_unit c == nl"""
    iss = kc.Issuers(curve, 1, ul.L, None, seed=3)
    eng = kc.make_engine(curve, iss.gens, iss.api_id)
    ul.check_tables(eng, curve, paths=(0, 1))
    eng.close()


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_single_key_statuses_in_both_forms(curve):
    ul.check_single_key(curve, None)


@pytest.mark.parametrize("curve", CURVE_NAMES)
def test_keyed_statuses_in_both_forms(curve):
    ul.check_keyed(curve, None)
