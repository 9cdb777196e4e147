"""The scenario table of tests/pip_cases.py through the TEST-ONLY host twin, both curves: bbs_selftest_segmented_sums
(PipGroupSumsHost) and bbs_g1_msm_pippenger (PipBuckets / PipSegments / PipWindows).  The twin has neither cooperative kernel;
what this tier proves before a GPU sees the table is the table itself -- its packing into groups and scalar bytes, the
identity points, and every reference sum, which the model, one multiplication of the generator and (small scenarios) the
term-by-term sum must agree on."""
import os
import sys

import pytest

import parity_cases as pc
import pip_cases as pcs
from oracle import bbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.fixture(scope="module", params=CURVES)
def ctx(request, twin):
    suite = bbs.SUITES[request.param]
    eng = pc.make_engine(request.param, pc.gens_for(suite, 2), suite.api_id, twin)
    yield request.param, eng
    eng.close()


def test_segmented_sums(ctx):
    curve, eng = ctx
    pcs.check_segmented_sums(eng, curve)


def test_msm(ctx):
    curve, eng = ctx
    pcs.check_msm(eng, curve)
