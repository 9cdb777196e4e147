"""Batched key generation on the GPU: the KgDerive and KgPublic kernels against the library's one-key host functions and the
oracle item by item at the batch sizes where lane indexing, the ragged offsets and the SHA-256 block boundaries can go wrong;
the reference's key-pair vector, the dst length, the edge scalars of the comb, the public wrappers and the C++ wrapper
(tests/keygen_cases.py, tests/cpp/keygen_batch.cpp)."""
import os
import sys

import pytest

import keygen_cases as kg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", kg.SIZES)
@pytest.mark.parametrize("curve", kg.CURVES)
def test_key_gen_batch_kernels_equal_host_functions(curve, n):
    # the refused lanes (17: short key material, 63: over-long key info) stay with their wavefront and must not disturb a
    # neighbour: EVERY item is compared
    kg.check_equals_host(curve, n, None)


def test_reference_key_pair_vector():
    kg.check_reference_vector(None)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_dst_length(curve):
    kg.check_dst_length(curve, None)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_sk_to_pk_batch_edge_scalars(curve):
    kg.check_sk_to_pk_edges(curve, None)


@pytest.mark.parametrize("curve", kg.CURVES)
def test_public_wrappers(curve):
    kg.check_public_wrappers(curve, None)


def test_cpp_wrapper_key_gen_batch_gpu():
    sys.path.insert(0, ROOT)
    from bbs_sign_amd import build as b
    kg.check_cpp_wrapper(b.build(twin=False, verbose=False), "cpp_keygen_batch")
