"""Untrusted encodings at every field's boundary (tests/wire_cases.py) through the TEST-ONLY host twin, both curves, 4-bit
windows, and through the product library's host decoders (no GPU).  The twin runs every lane of every stage on one host
thread: it checks the decisions of the ingest and decode bodies, not their divergence -- that is the GPU tier's."""
import os
import sys

import pytest

import wire_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = list(wc.CURVES)


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.fixture(scope="session")
def lib():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=False, verbose=False)


@pytest.mark.parametrize("curve", CURVES)
def test_host_codec(lib, curve):
    wc.check_host_codec(curve, lib)


@pytest.mark.parametrize("curve", CURVES)
def test_records(twin, curve):
    wc.check_records(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_records_mixed_lengths(twin, curve):
    wc.check_records_mixed(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_records_keyed(twin, curve):
    wc.check_records_keyed(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_octets(twin, curve):
    wc.check_octets(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_flags_and_identities(twin, curve):
    wc.check_flags(curve, twin)


def test_subgroup(twin):
    wc.check_subgroup(twin)


def test_sign_boundary(twin):
    wc.check_sign_boundary(twin)


@pytest.mark.parametrize("curve", CURVES)
def test_precedence(twin, curve):
    wc.check_precedence(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_dst_too_long(twin, curve):
    wc.check_dst_too_long(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_geometry(twin, curve):
    """On one host thread a wavefront means nothing, but the bookkeeping of 65 items does (a zero record for a refused item, a
    neighbour that keeps its 1 or 0): one of the three runs of every point-level kind, the run with every item defective and the
    one with a single valid item; the GPU tier runs them all."""
    w = wc.world(curve)
    pick = ["%s/shift%d" % (kind, k % 3) for k, kind in enumerate(sorted(wc.point_defects(w)))] + ["all defective", "only 21 valid"]
    names = wc.check_geometry(curve, twin, runs=pick)
    assert set(pick) <= set(names) and len(pick) >= 7


@pytest.mark.parametrize("curve", CURVES)
def test_geometry_signatures(twin, curve):
    wc.check_geometry_signatures(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_decompress_geometry(twin, curve):
    wc.check_decompress_geometry(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_keys(twin, curve):
    wc.check_keys(curve, twin)


@pytest.mark.parametrize("curve", CURVES)
def test_primitives(twin, curve):
    wc.check_primitives(curve, twin)
