"""The scenario table of tests/pip_cases.py on the GPU, both curves: every exceptional branch of the point addition at every
step of the two cooperative bucket kernels -- k_pip_window_seg through bbs_selftest_segmented_sums, k_pip_window through
bbs_g1_msm_pippenger.  tests/test_pip_model.py shows that the table meets every (site, branch) pair; the host-twin tier has
checked the table's packing and references.  The references are computed once per curve and shared by both tests."""
import pytest

import parity_cases as pc
import pip_cases as pcs
from oracle import bbs

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]


@pytest.fixture(scope="module", params=CURVES)
def ctx(request):
    suite = bbs.SUITES[request.param]
    eng = pc.make_engine(request.param, pc.gens_for(suite, 2), suite.api_id)
    yield request.param, eng
    eng.close()


def test_segmented_sums(ctx):
    curve, eng = ctx
    pcs.check_segmented_sums(eng, curve)


def test_msm(ctx):
    curve, eng = ctx
    pcs.check_msm(eng, curve)
