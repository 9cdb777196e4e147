"""The wire model (tests/wire_ref.py) and the builders of the case tables (tests/wire_cases.py), no library needed: the model
inverts the oracle's encoders on random points and on the reference's three octet vectors, the cube roots and point orders the
builders rely on are right, every builder meets its minimum counts, and every rejecting site of the ingests has cases."""
import random

import pytest

from oracle import bbs

import wire_cases as wc
import wire_ref as wr
from test_codec import PK_HEX, PROOF_HEX, SIG_HEX

CURVES = list(wc.CURVES)


@pytest.mark.parametrize("curve", CURVES)
def test_model_inverts_the_oracle_encoders(curve):
    c = bbs.SUITES[curve].curve
    rng = random.Random(11)
    for _ in range(6):
        p = c.g1_mul(c.g1, rng.randrange(1, c.r))
        for q in (p, c.g1_neg(p)):
            assert wr.g1_from_octets(c, bbs.g1_compress(c, q)) == (0, q)
    assert wr.g1_from_octets(c, bbs.g1_compress(c, None)) == (1, None)
    for _ in range(2):
        p = c.g2_mul(c.g2, rng.randrange(1, c.r))
        for q in (p, c.g2_neg(p)):
            assert wr.g2_from_octets(c, bbs.g2_compress(c, q)) == (0, q)
            assert wr.public_key_from_octets(c, bbs.g2_compress(c, q)) == (1, q)
    assert wr.g2_from_octets(c, bbs.g2_compress(c, None)) == (1, None)
    assert wr.public_key_from_octets(c, bbs.g2_compress(c, None)) == (1, None)
    assert wr.public_key_from_octets(c, bbs.g2_compress(c, None)[:-1])[0] == -42


def test_model_reads_the_reference_vectors():
    c = bbs.BLS_SUITE.curve
    st, sig = wr.signature_from_octets(c, bytes.fromhex(SIG_HEX))
    assert st == 1 and (bbs.g1_compress(c, sig.a) + bbs.scalar_be(c, sig.e)).hex() == SIG_HEX
    st, p = wr.proof_from_octets(c, bytes.fromhex(PROOF_HEX))
    assert st == 1 and p.commitments == []
    again = b"".join(bbs.g1_compress(c, q) for q in (p.a_bar, p.b_bar, p.d)) + b"".join(bbs.scalar_be(c, v) for v in (p.e_cap, p.r1_cap, p.r3_cap, p.challenge))
    assert again.hex() == PROOF_HEX
    st, pk = wr.public_key_from_octets(c, bytes.fromhex(PK_HEX))
    assert st == 1 and bbs.g2_compress(c, pk).hex() == PK_HEX
    assert wr.proof_from_octets(c, bytes.fromhex(PROOF_HEX)[:-1])[0] == -42
    assert wr.signature_from_octets(c, bytes.fromhex(SIG_HEX) + b"\0")[0] == -42


def test_field_table():
    for c in (bbs.BLS_SUITE.curve, bbs.BN_SUITE.curve):
        for m, bits in ((c.p, 8 * c.fp_bytes), (c.r, 256)):
            rows = dict(wc.field_values(m, 12345, bits))
            assert rows["m"] == m and rows["alias"] == m + 12345 and rows["ones"] == (1 << bits) - 1
            assert rows["hi+1"] - m == m - rows["hi-1"] == 1 << (32 * ((m.bit_length() - 1) // 32))
            assert all(v >= m for k, v in rows.items() if k in ("m", "m+1", "alias", "ones", "lo+1", "hi+1"))
            assert all(v < m for k, v in rows.items() if k in ("zero", "m-1", "lo-1", "hi-1"))
        assert 2 * c.r < 1 << 256                                    # a scalar's alias always fits


def test_cube_roots_and_sign_boundary():
    c = bbs.BN_SUITE.curve
    assert c.p % 9 == 1 and c.p % 4 == 3
    rng = random.Random(5)
    for _ in range(20):
        a = rng.randrange(1, c.p)
        assert pow(wc.cube_root(c.p, pow(a, 3, c.p)), 3, c.p) == pow(a, 3, c.p)
    below, above = wc.sign_boundary_points()
    assert len(below) >= 8 and len(above) >= 8
    half = (c.p - 1) // 2
    for x, y in below + above:
        assert pow(x, 3, c.p) == (y * y - 3) % c.p and abs(y - half) <= 40
    assert all(y <= half for _, y in below) and all(y > half for _, y in above)
    # y^2 - 3 has three cube roots or none
    w = pow(2, (c.p - 1) // 3, c.p) if pow(2, (c.p - 1) // 3, c.p) != 1 else pow(3, (c.p - 1) // 3, c.p)
    assert w != 1 and pow(w, 3, c.p) == 1
    x, y = below[0]
    assert all(c.g1_is_on_curve((x * pow(w, k, c.p) % c.p, y)) for k in range(3))


def test_points_outside_the_subgroup():
    c = bbs.BLS_SUITE.curve
    pts = wc.off_subgroup_points()
    assert len(pts) >= 10 and {"T_%d" % q for q in wc.H_PRIMES} <= set(pts)
    for q in wc.H_PRIMES:
        t = pts["T_%d" % q]
        assert t is not None and c.g1_mul(t, q) is None and c.g1_is_on_curve(t)
        assert c.g1_mul(pts["G+T_%d" % q], c.r) is not None
    assert c.g1_mul(pts["T_3+T_11"], 33) is None and c.g1_mul(pts["T_3+T_11"], 3) is not None and c.g1_mul(pts["T_3+T_11"], 11) is not None


@pytest.mark.parametrize("curve", CURVES)
def test_builders_meet_their_counts(curve):
    w = wc.world(curve)
    assert sorted(w.alias_at) == [0, 1, 2] and all(w.alias_at[k]["pts"][k][0] + w.c.p < 1 << wr.value_bits(w.c) for k in range(3))
    labels = wc.all_labels(curve)
    alias = [lab for lab in labels if lab.endswith(":alias")]
    assert all(labels[lab] in (-40, -41) for lab in alias) and len(alias) >= 50
    for k in range(3):
        assert labels["pv.oct.x%d:alias" % k] == -40
    assert labels["vf.oct.x:alias"] == -40 and labels["key.oct.half1:alias"] == -40
    assert sum(1 for lab in labels if lab.startswith("pv.oct.pair:")) >= 150 and sum(1 for lab in labels if lab.startswith("vf.oct.pair:")) == 48
    assert len(wc.flag_encodings(w.c, w.vf["a"])) == (24 if curve == "bls12_381" else 12)
    if curve == "bls12_381":
        assert sum(1 for lab in labels if lab.startswith("pv.oct.subgroup")) >= 30
    runs = wc.geometry_runs(w)
    assert all(len(items) == wc.GEOMETRY_N for _, items in runs) and len(runs) == 3 * len(wc.point_defects(w)) + 2
    planted = {(i, p) for name, items in runs if "shift" in name and name.startswith("x>=p") for i, it in enumerate(items) for p in it.get("enc", {})}
    assert planted == {(i, p) for i in wc.GEOMETRY_ITEMS for p in range(3)}


@pytest.mark.parametrize("curve", CURVES)
def test_every_rejecting_site_has_cases(curve):
    """One entry per site; every case an entry names exists, and the model gives it exactly the code that site leads to."""
    labels = wc.all_labels(curve)
    bodies = {site.split(":")[0].split(" ")[0] for site in wc.SITES}
    assert bodies == {"g1_decode_octets", "PvOctIngestBody", "PvIngestBody", "VfIngestBody", "PgIngestBody", "KeyBuild"}
    for site, (code, cases) in wc.SITES.items():
        if curve == "bn254" and "(BLS12-381)" in site:
            continue                              # BN254 has no compression flag and cofactor 1
        assert cases, site
        assert [lab for lab in cases if lab not in labels] == [], site
        assert [(lab, labels[lab]) for lab in cases if labels[lab] != code] == [], (site, code)
    # the codes every body can write are all there
    for body, codes in (("g1_decode_octets", {1, -40, -41}), ("PvOctIngestBody", {-42, -40, -41, -23, -3, -6, -1, -22}),
                        ("PvIngestBody", {-3, -6, -1, -23, -22, -40}), ("VfIngestBody", {-40, -41, -42, -23, -1}),
                        ("PgIngestBody", {-40, -41, -42, -23, -2, -3, -1, -4}), ("KeyBuild", {-40, -41})):
        assert {code for site, (code, _) in wc.SITES.items() if site.startswith(body)} == codes, body
