"""Line tables in the unit form (bbs_ctx_set_unit_lines) through the TEST-ONLY host twin, both curves: every entry of both
forms against the oracle's field arithmetic -- the generator's table and three random keys, by the host functions and by the
KeyBuild stage -- and the one-lane pairing through both forms (tests/unit_lines_cases.py)."""
import os
import sys

import pytest

import keyed_cases as kc
import unit_lines_cases as ul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.mark.parametrize("curve", CURVES)
def test_unit_entries_are_the_lines_over_c(twin, curve):
    iss = kc.Issuers(curve, 1, ul.L, twin, seed=3)
    eng = kc.make_engine(curve, iss.gens, iss.api_id, twin)
    ul.check_tables(eng, curve, paths=(0, 1))
    eng.close()


def test_switch_arguments(twin):
    from bbs_sign_amd import _lib
    lib = _lib.load_library(twin)
    assert "bbs_ctx_set_unit_lines" in _lib.SIGNATURES and hasattr(lib, "bbs_ctx_set_unit_lines")
    assert lib.bbs_ctx_set_unit_lines(None, 1) == -100        # BBS_E_ARG


@pytest.mark.parametrize("curve", CURVES)
def test_single_key_statuses_in_both_forms(twin, curve):
    ul.check_single_key(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keyed_statuses_in_both_forms(twin, curve):
    ul.check_keyed(curve, twin)
