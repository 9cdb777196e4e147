"""Header, ph, message and api_id bytes at every SHA-256 alignment on the MI355X: the full sweeps of tests/hash_cases.py.

  * S1, the domain: core_sign + core_verify at L = 1 under 72 api_id lengths (every dom_tail_len 0 .. 63 and every padding
    boundary of the DST), under each of them every header length 0 .. 136, 255, 256, 257, 300 at all four pointer
    residues; e of every item from hashlib;
  * the S1 cover set through core_proof_gen / core_proof_verify against the oracle's whole proof;
  * S2, the challenge: core_proof_gen + core_proof_verify at L = 7, R = 0 .. 7, the same ph lengths and residues, the
    whole proof of every item from one proof_init of the Python oracle per R;
  * S3 / S4: raw messages 0 .. 136, 255 .. 257 bytes at four residues through the wire forms and hash_to_scalar_batch,
    and every dst_len 0 .. 255.

Measured wall times: this module 9 s on an MI355X (18 cases, 0.03 .. 1.1 s each; about 100 000 signatures and 11 000 proofs).
The `-m "not gpu"` suite before this module took 671 s on 8 cores; tests/test_hash_hosttwin.py adds 26 s to it (the limit
it was written to: a tenth, 67 s).
"""
import pytest

import hash_cases as hc

pytestmark = pytest.mark.gpu

CURVES = ["bls12_381", "bn254"]
PARTS = 4


@pytest.mark.parametrize("part", range(PARTS))
@pytest.mark.parametrize("curve", CURVES)
def test_sign_domain(curve, part):
    """A quarter of the api_id lengths per case: each holds every dom_tail_len residue mod 4."""
    per = (len(hc.API_LENS) + PARTS - 1) // PARTS
    lens = sorted(hc.API_LENS)[part * per:(part + 1) * per]
    assert {hc.dom_tail_len(curve, 1, a) & 3 for a in lens} == {0, 1, 2, 3}
    assert hc.check_sign_domain(curve, full=True, api_lens=lens) >= len(lens) * 4 * len(hc.SWEEP_LENS)


@pytest.mark.parametrize("curve", CURVES)
def test_proof_domain(curve):
    hc.check_proof_domain(curve)


@pytest.mark.parametrize("curve", CURVES)
def test_challenge(curve):
    assert hc.check_challenge(curve, full=True) >= 8 * 4 * len(hc.SWEEP_LENS)


@pytest.mark.parametrize("curve", CURVES)
def test_wire_messages(curve):
    assert hc.check_wire_messages(curve, full=True) >= 4 * len(hc.MSG_LENS)


@pytest.mark.parametrize("curve", CURVES)
def test_hash_to_scalar(curve):
    assert hc.check_hash_to_scalar(curve) >= 4 * len(hc.MSG_LENS) + 3 * 256


@pytest.mark.parametrize("curve", CURVES)
def test_dst_too_long(curve):
    hc.check_dst_too_long(curve)
