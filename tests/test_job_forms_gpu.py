"""The four forms of a job on the GPU, both curves, throughput form, 8-bit windows: the cases of tests/job_form_cases.py --
every (operation, form, input form) reports the recorded stage list, and the four forms of an operation agree on items they
must treat alike."""
import pytest

import job_form_cases as jf

pytestmark = pytest.mark.gpu
CURVES = ["bls12_381", "bn254"]


@pytest.mark.parametrize("inp", jf.INPUTS)
@pytest.mark.parametrize("op", jf.OPS)
@pytest.mark.parametrize("curve", CURVES)
def test_forms(curve, op, inp):
    jf.check_forms(curve, None, op, inp, "gpu")
