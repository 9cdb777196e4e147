"""Batched key generation through the TEST-ONLY host twin (both curves): bbs_key_gen_batch and bbs_sk_to_pk_batch against the
library's one-key host functions and the oracle item by item, the reference's key-pair vector, the dst length, the edge scalars
of the comb, the public wrappers, the arguments, and the C++ wrapper (tests/keygen_cases.py, tests/cpp/keygen_batch.cpp)."""
import os
import sys

import pytest

import keygen_cases as kg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def twin():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    return b.build(twin=True, verbose=False)


@pytest.mark.parametrize("n", kg.SIZES)
@pytest.mark.parametrize("curve", kg.CURVES)
def test_key_gen_batch_equals_host_functions(twin, curve, n):
    kg.check_equals_host(curve, n, twin)


def test_reference_key_pair_vector(twin):
    kg.check_reference_vector(twin)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_dst_length(twin, curve):
    kg.check_dst_length(curve, twin)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_sk_to_pk_batch_edge_scalars(twin, curve):
    kg.check_sk_to_pk_edges(curve, twin)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_public_wrappers(twin, curve):
    kg.check_public_wrappers(curve, twin)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_arguments(twin, curve):
    kg.check_arguments(curve, twin)


def test_cpp_wrapper_key_gen_batch_cpu_twin(twin):
    kg.check_cpp_wrapper(twin, "cpp_keygen_batch_twin")
