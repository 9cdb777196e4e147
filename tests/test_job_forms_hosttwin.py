"""The four forms of a job through the TEST-ONLY host twin, both curves, throughput form, 4-bit windows: the cases of
tests/job_form_cases.py -- every (operation, form, input form) reports the recorded stage list, and the four forms of an
operation agree on items they must treat alike."""
import os
import sys

import pytest

import job_form_cases as jf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.mark.parametrize("inp", jf.INPUTS)
@pytest.mark.parametrize("op", jf.OPS)
@pytest.mark.parametrize("curve", CURVES)
def test_forms(twin, curve, op, inp):
    jf.check_forms(curve, twin, op, inp, "twin")
