"""Untrusted encodings at every field's boundary (tests/wire_cases.py) on the GPU, both curves, 8-bit windows.  The tables of
the host-twin tier through the device stages, and the lane geometry: the octet forms at 65 items -- PvOctDecode runs lane
3 i + p, so that is 195 decode lanes in four wavefronts, the last one ragged -- with every point-level defect planted at each
point of items 20, 21, 22, 42, 43, 63 and 64 (item 21 has its points in wavefronts 0 and 1, item 42 in 1 and 2), one kind per
run; a run where every item is defective and one where only item 21 is valid.  A rejecting lane is divergent code beside a
square root and two multiplications by the curve parameter."""
import pytest

import wire_cases as wc

pytestmark = pytest.mark.gpu
CURVES = list(wc.CURVES)


@pytest.mark.parametrize("curve", CURVES)
def test_records(curve):
    wc.check_records(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_records_mixed_lengths(curve):
    wc.check_records_mixed(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_records_keyed(curve):
    wc.check_records_keyed(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_octets(curve):
    wc.check_octets(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_flags_and_identities(curve):
    wc.check_flags(curve, None)


def test_subgroup():
    wc.check_subgroup(None)


def test_sign_boundary():
    wc.check_sign_boundary(None)


@pytest.mark.parametrize("curve", CURVES)
def test_precedence(curve):
    wc.check_precedence(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_dst_too_long(curve):
    wc.check_dst_too_long(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_geometry(curve):
    wc.check_geometry(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_geometry_signatures(curve):
    wc.check_geometry_signatures(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_decompress_geometry(curve):
    wc.check_decompress_geometry(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_keys(curve):
    wc.check_keys(curve, None)


@pytest.mark.parametrize("curve", CURVES)
def test_primitives(curve):
    wc.check_primitives(curve, None)
