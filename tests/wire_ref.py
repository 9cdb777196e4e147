"""A validating decoder of the wire forms in plain big integers, and the expected per-item status of the batched entry
points: the MODEL the wire tests compare the library with (tests/wire_cases.py).

Written from the rules of include/bbs_sign_amd.h ("Wire codec", bbs_g1_decompress_batch, bbs_proof_verify_octets_*,
bbs_verify_octets_*, the per-item status codes) and the header comment of bbs_sign_amd/csrc/host_codec.hpp, over
oracle.curves and oracle.bbs.  It shares nothing with the library: no limb arithmetic, no masks taken from the C++ source, the
subgroup test is [r]P == identity by the oracle's double-and-add, the larger root is y > (p - 1) / 2 on integers.

Point codes (bbs_g1_decompress_batch): 0 ok, 1 ok and the identity, -40 malformed / not canonical, -41 not on the curve or
outside the prime-order subgroup.  String and item statuses: 1 ok / Ok(true), 0 Ok(false), < 0 the codes of the header."""
from oracle import bbs

OK, IDENTITY = 0, 1
NONCANONICAL, NOT_ON_CURVE, INVALID_ENCODING = -40, -41, -42


def is_bls(curve):
    return curve.name == "bls12_381"


def value_bits(curve):
    """Bits of a compressed string's first coordinate that carry the value: all but the flag bits."""
    return 8 * curve.fp_bytes - (3 if is_bls(curve) else 2)


def _flags_and_value(curve, b):
    """(compressed, infinity, sign, value) of a compressed string of fp_bytes or 2 fp_bytes octets; the value is the whole
    string as ONE integer in the curve's byte order with the flag bits cleared.  BLS12-381: flags 0x80 / 0x40 / 0x20 in byte 0,
    big-endian.  BN254: 0x80 the larger root, 0x40 the identity, both in the LAST byte, little-endian; no compression flag."""
    if is_bls(curve):
        f = b[0]
        v = int.from_bytes(b, "big") & ((1 << (8 * len(b) - 3)) - 1)
        return bool(f & 0x80), bool(f & 0x40), bool(f & 0x20), v
    f = b[-1]
    v = int.from_bytes(b, "little") & ((1 << (8 * len(b) - 2)) - 1)
    return True, bool(f & 0x40), bool(f & 0x80), v


def fp_sqrt(curve, a):
    """A square root of a in Fp or None (p = 3 mod 4 on both curves)."""
    y = pow(a % curve.p, (curve.p + 1) // 4, curve.p)
    return y if y * y % curve.p == a % curve.p else None


_g1_memo = {}


def g1_from_octets(curve, b):
    """(code, point): the point is None unless the code is 0.  (A pure function of the string: results are kept.)"""
    key = (curve.name, bytes(b))
    if key not in _g1_memo:
        _g1_memo[key] = _g1_from_octets(curve, b)
    return _g1_memo[key]


def _g1_from_octets(curve, b):
    assert len(b) == curve.fp_bytes
    comp, inf, big, x = _flags_and_value(curve, b)
    if not comp:
        return NONCANONICAL, None
    if inf:
        return (NONCANONICAL if (x or big) else IDENTITY), None
    if x >= curve.p:
        return NONCANONICAL, None
    y = fp_sqrt(curve, x * x * x + curve.b)
    if y is None:
        return NOT_ON_CURVE, None
    if (y > (curve.p - 1) // 2) != big:
        y = (curve.p - y) % curve.p
    if curve.g1_mul((x, y), curve.r) is not None:
        return NOT_ON_CURVE, None
    return OK, (x, y)


def g2_from_octets(curve, b):
    """(code, point) for a compressed G2 point: BLS12-381 x.c1 || x.c0, BN254 x.c0 || x.c1."""
    n = curve.fp_bytes
    assert len(b) == 2 * n
    comp, inf, big, v = _flags_and_value(curve, b)
    if not comp:
        return NONCANONICAL, None
    if inf:
        return (NONCANONICAL if (v or big) else IDENTITY), None
    first, second = (v >> (8 * n), v & ((1 << (8 * n)) - 1))          # the coordinate next to the flags, the other one
    c1, c0 = first, second
    if c0 >= curve.p or c1 >= curve.p:
        return NONCANONICAL, None
    x = (c0, c1)
    y = curve.f2_sqrt(curve.f2_add(curve.f2_mul(curve.f2_sqr(x), x), curve.b2))
    if y is None:
        return NOT_ON_CURVE, None
    judged = y[1] if y[1] != 0 else y[0]
    if (judged > (curve.p - 1) // 2) != big:
        y = curve.f2_neg(y)
    if curve.g2_mul((x, y), curve.r) is not None:
        return NOT_ON_CURVE, None
    return OK, (x, y)


def scalar_from_octets(b):
    return int.from_bytes(b, "big")


def signature_from_octets(curve, b):
    """(status, Signature or None): compress(A) || e.  Order: the length, A's code, A = identity (-42), e >= r (-40), e = 0 (-42)."""
    n = curve.fp_bytes
    if len(b) != n + 32:
        return INVALID_ENCODING, None
    code, a = g1_from_octets(curve, b[:n])
    if code < 0:
        return code, None
    if code == IDENTITY:
        return INVALID_ENCODING, None
    e = scalar_from_octets(b[n:])
    if e >= curve.r:
        return NONCANONICAL, None
    if e == 0:
        return INVALID_ENCODING, None
    return 1, bbs.Signature(a, e)


def proof_from_octets(curve, b):
    """(status, Proof or None): compress(Abar) || compress(Bbar) || compress(D) || e^ || r1^ || r3^ || m^_1 .. m^_U || c.
    Order: the shape (-42), the first failing point (its code; the identity is -42), then -40 for any scalar >= r."""
    n = curve.fp_bytes
    fixed = 3 * n + 4 * 32
    if len(b) < fixed or (len(b) - fixed) % 32:
        return INVALID_ENCODING, None
    pts = []
    verdict = None
    for k in range(3):
        code, q = g1_from_octets(curve, b[k * n:(k + 1) * n])
        if verdict is None and code != OK:
            verdict = INVALID_ENCODING if code == IDENTITY else code
        pts.append(q)
    if verdict is not None:
        return verdict, None
    sc = [scalar_from_octets(b[3 * n + 32 * k:3 * n + 32 * k + 32]) for k in range((len(b) - 3 * n) // 32)]
    if any(s >= curve.r for s in sc):
        return NONCANONICAL, None
    return 1, bbs.Proof(pts[0], pts[1], pts[2], sc[0], sc[1], sc[2], sc[3:-1], sc[-1])


def public_key_from_octets(curve, b):
    """(status, key or None): 1 and the key (None = the identity key, which is accepted), -40, -41, or -42 for a wrong length."""
    if len(b) != 2 * curve.fp_bytes:
        return INVALID_ENCODING, None
    code, q = g2_from_octets(curve, b)
    return (1, q) if code >= 0 else (code, None)


# ---- the batched forms ------------------------------------------------------------------------------------------------------
_verdicts = {}


def _memo(key, fn):
    if key not in _verdicts:
        _verdicts[key] = int(fn())
    return _verdicts[key]


class Setting:
    """What a context is set up with: suite, generators [Q1, H_1 .. H_L], the key pair, the api_id (the suite's unless
    given).  dst_too_long: api_id || "H2S_" exceeds 255 bytes, where the reference's expand_message panics (-23, looked at
    after the length check of every core_* function); msg_dst_too_long: api_id || "MAP_MSG_TO_SCALAR_AS_HASH_" does, where
    msg_to_scalars panics in the raw-message forms before anything else of the reference runs, for an item with messages."""

    def __init__(self, suite, gens, sk, api_id=None):
        self.suite, self.gens, self.sk = suite, gens, sk
        self.curve = suite.curve
        self.pk = bbs.sk_to_pk(suite, sk)
        self.api_id = suite.api_id if api_id is None else api_id
        self.L = len(gens) - 1
        self.dst_too_long = len(self.api_id) + len(b"H2S_") > 255
        self.msg_dst_too_long = len(self.api_id) + len(b"MAP_MSG_TO_SCALAR_AS_HASH_") > 255


def _g1_record_code(curve, pt):
    """A G1 record x || y as integers: -40 for a coordinate >= p, -41 off the curve, else 0 (zeros are the identity)."""
    if pt[0] >= curve.p or pt[1] >= curve.p:
        return NONCANONICAL
    if pt == (0, 0):
        return OK
    return OK if curve.g1_is_on_curve(pt) else NOT_ON_CURVE


def _pv_reference_errors(s, u, didx, n_dm):
    """proof_verify_init's own checks in its order, and the duplicate index behind its out-of-bounds panic."""
    l = u + len(didx)
    if any(j >= l for j in didx):
        return -3
    if n_dm != len(didx):
        return -6
    if l != s.L:
        return -1
    if s.dst_too_long:
        return -23
    if len(set(didx)) != len(didx):
        return -22
    return None


def _pv_oracle(s, proof, dm, didx, hdr, ph):
    key = ("pv", s.curve.name, s.sk, proof.a_bar, proof.b_bar, proof.d, proof.e_cap, proof.r1_cap, proof.r3_cap,
           tuple(proof.commitments), proof.challenge, tuple(dm), tuple(didx), hdr, ph)
    return _memo(key, lambda: bbs.core_proof_verify(s.suite, s.pk, proof, s.gens, hdr, ph, list(dm), list(didx), s.api_id))


def core_proof_verify_status(s, pts, sc, cms, dm, didx, hdr=b"", ph=b""):
    """bbs_core_proof_verify_*: pts = three (x, y), sc = [e^, r1^, r3^, c], all as the integers the record carries.  The
    reference's errors first, then -40 (any coordinate >= p, any scalar, commitment or disclosed message >= r), then -41."""
    c = s.curve
    err = _pv_reference_errors(s, len(cms), didx, len(dm))
    if err is not None:
        return err
    codes = [_g1_record_code(c, q) for q in pts]
    if NONCANONICAL in codes or any(v >= c.r for v in list(sc) + list(cms) + list(dm)):
        return NONCANONICAL
    if NOT_ON_CURVE in codes:
        return NOT_ON_CURVE
    proof = bbs.Proof(pts[0], pts[1], pts[2], sc[0], sc[1], sc[2], list(cms), sc[3])
    return _pv_oracle(s, proof, dm, didx, hdr, ph)


def proof_verify_octets_status(s, octets, dm, didx, hdr=b"", ph=b""):
    """bbs_proof_verify_octets_*: -42, the point codes, -40 for the proof's scalars, then -3, -6, -1, -23, -22, then -40 for a
    disclosed message, then the oracle's boolean."""
    st, proof = proof_from_octets(s.curve, octets)
    if st != 1:
        return st
    err = _pv_reference_errors(s, len(proof.commitments), didx, len(dm))
    if err is not None:
        return err
    if any(v >= s.curve.r for v in dm):
        return NONCANONICAL
    return _pv_oracle(s, proof, dm, didx, hdr, ph)


def proof_verify_wire_status(s, octets, dm_raw, didx, hdr=b"", ph=b""):
    """bbs_proof_verify_wire_*: the disclosed messages are raw bytes, hashed to scalars (never out of range)."""
    st, _ = proof_from_octets(s.curve, octets)
    if st != 1:
        return st
    if s.msg_dst_too_long:
        return -23 if dm_raw else proof_verify_octets_status(s, octets, [], didx, hdr, ph)
    return proof_verify_octets_status(s, octets, bbs.msg_to_scalars(s.suite, list(dm_raw), s.api_id), didx, hdr, ph)


def _vf_oracle(s, a, e, msgs, hdr):
    key = ("vf", s.curve.name, s.sk, a, e, tuple(msgs), hdr)
    return _memo(key, lambda: bbs.core_verify(s.suite, s.pk, bbs.Signature(a, e), s.gens, hdr, list(msgs), s.api_id))


def core_verify_status(s, a, e, msgs, hdr=b""):
    """bbs_core_verify_*: a = (x, y) and e as the record carries them.  -1, -23, then -40, then -41, then the oracle."""
    c = s.curve
    if len(msgs) != s.L:
        return -1
    if s.dst_too_long:
        return -23
    code = _g1_record_code(c, a)
    if code == NONCANONICAL or e >= c.r or any(m >= c.r for m in msgs):
        return NONCANONICAL
    if code == NOT_ON_CURVE:
        return NOT_ON_CURVE
    return _vf_oracle(s, a, e, msgs, hdr)


def verify_octets_status(s, octets, msgs, hdr=b""):
    """bbs_verify_octets_*: what signature_from_octets gives when it fails, else core_verify's status."""
    st, sig = signature_from_octets(s.curve, octets)
    if st != 1:
        return st
    return core_verify_status(s, sig.a, sig.e, msgs, hdr)


def verify_wire_status(s, octets, msgs_raw, hdr=b""):
    st, sig = signature_from_octets(s.curve, octets)
    if st != 1:
        return st
    if s.msg_dst_too_long:
        return -23 if msgs_raw else core_verify_status(s, sig.a, sig.e, [], hdr)
    return core_verify_status(s, sig.a, sig.e, bbs.msg_to_scalars(s.suite, list(msgs_raw), s.api_id), hdr)


def core_sign_status(s, msgs):
    """bbs_core_sign_*: -1, -23, then -40 for a message >= r, else 1 (the item is signed)."""
    if len(msgs) != s.L:
        return -1
    if s.dst_too_long:
        return -23
    return NONCANONICAL if any(m >= s.curve.r for m in msgs) else 1


def _pg_reference_errors(s, l, didx):
    if len(didx) > l:
        return -2
    if any(j >= l for j in didx):
        return -3
    if l != s.L:
        return -1
    if len(set(didx)) != len(didx):
        return -4
    if s.dst_too_long:
        return -23
    return None


def core_proof_gen_status(s, a, e, msgs, didx, rnd):
    """bbs_core_proof_gen_*: -2, -3, -1, -4, -23, then -40 (A's coordinates, e, a random scalar, a message), then -41, else 1."""
    c = s.curve
    err = _pg_reference_errors(s, len(msgs), didx)
    if err is not None:
        return err
    code = _g1_record_code(c, a)
    if code == NONCANONICAL or e >= c.r or any(v >= c.r for v in list(rnd) + list(msgs)):
        return NONCANONICAL
    return NOT_ON_CURVE if code == NOT_ON_CURVE else 1


def proof_gen_wire_status(s, octets, n_msgs, didx, rnd):
    """bbs_proof_gen_wire_*: signature_from_octets' failure first, then core_proof_gen's checks (raw messages are hashed)."""
    st, sig = signature_from_octets(s.curve, octets)
    if st != 1:
        return st
    if s.msg_dst_too_long and n_msgs > 0:
        return -23
    err = _pg_reference_errors(s, n_msgs, didx)
    if err is not None:
        return err
    return NONCANONICAL if any(v >= s.curve.r for v in rnd) else 1


def g1_msm_status(curve, fixed_scalars, var_points, var_scalars):
    """bbs_g1_msm_batch: -40 for a scalar >= r or a coordinate >= p, -41 for a point off the curve, else 1."""
    codes = [_g1_record_code(curve, q) for q in var_points]
    if NONCANONICAL in codes or any(v >= curve.r for v in list(fixed_scalars) + list(var_scalars)):
        return NONCANONICAL
    return NOT_ON_CURVE if NOT_ON_CURVE in codes else 1


def pairing_product2_status(s, pa, pb):
    """bbs_pairing_product2_is_one_batch: -40, -41, else e(Pa, pk) e(Pb, BP2) == 1 by the oracle."""
    c = s.curve
    codes = [_g1_record_code(c, pa), _g1_record_code(c, pb)]
    if NONCANONICAL in codes:
        return NONCANONICAL
    if NOT_ON_CURVE in codes:
        return NOT_ON_CURVE
    key = ("pp", c.name, s.sk, pa, pb)
    return _memo(key, lambda: c.pairing_product_is_one([(None if pa == (0, 0) else pa, s.pk), (None if pb == (0, 0) else pb, c.g2)]))


def sk_to_pk_status(curve, sk):
    return NONCANONICAL if sk >= curve.r else 1


def g2_record_status(curve, rec):
    """A key record (x.c0, x.c1, y.c0, y.c1) as integers, as bbs_ctx_add_public_keys takes it: 1, or -41 for a key that
    bbs_ctx_set_public_key would refuse -- a coordinate >= p, a point off the twist or outside the subgroup."""
    if any(v >= curve.p for v in rec):
        return NOT_ON_CURVE
    q = ((rec[0], rec[1]), (rec[2], rec[3]))
    if not curve.g2_is_on_curve(q) or curve.g2_mul(q, curve.r) is not None:
        return NOT_ON_CURVE
    return 1
