"""Key registration (bbs_ctx_add_public_keys, bbs_ctx_add_public_keys_octets, bbs_selftest_key_entries): key material made
with the oracle, and the calls of the test hook.  Shared by tests/test_keyreg_hosttwin.py and tests/test_keyreg_gpu.py."""
import ctypes
import random

import numpy as np

from bbs_sign_amd import _lib
from oracle import bbs

import keyed_cases as kc

NONCANONICAL, NOT_ON_CURVE = -40, -41


def off_subgroup_point(curve):
    """A point ON the twist and OUTSIDE the subgroup of order r: x = (k, 0) for the first small k whose x^3 + b' has a root."""
    c = bbs.SUITES[curve].curve
    for k in range(1, 21):
        x = (k, 0)
        y = c.f2_sqrt(c.f2_add(c.f2_mul(c.f2_sqr(x), x), c.b2))
        if y is None:
            continue
        q = (x, y)
        assert c.g2_is_on_curve(q)
        assert c.g2_mul(q, c.r) is not None, "x = (%d, 0) happens to lie in the subgroup" % k
        return q
    raise AssertionError("no x = (k, 0), k <= 20, is on the twist")


def rootless_x(curve):
    """x = (k, 0) for which x^3 + b' is no square: no point of the twist has it."""
    c = bbs.SUITES[curve].curve
    for k in range(1, 41):
        x = (k, 0)
        if c.f2_sqrt(c.f2_add(c.f2_mul(c.f2_sqr(x), x), c.b2)) is None:
            return x
    raise AssertionError("every x = (k, 0), k <= 40, is on the twist")


def record(n, pk):
    """The affine record of a key (n = fp_bytes): x.c0 || x.c1 || y.c0 || y.c1 little-endian; coordinates are NOT reduced."""
    if pk is None:
        return bytes(4 * n)
    (x0, x1), (y0, y1) = pk
    return b"".join(int(v).to_bytes(n, "little") for v in (x0, x1, y0, y1))


def valid_keys(curve, count, seed):
    suite = bbs.SUITES[curve]
    rng = random.Random(seed)
    return [bbs.sk_to_pk(suite, rng.randrange(1, suite.curve.r)) for _ in range(count)]


def record_cases(curve, seed=7):
    """(keys, expected statuses): valid keys, the identity, OFF_TWIST, a coordinate >= p, a point outside the subgroup -- mixed."""
    c = bbs.SUITES[curve].curve
    v = valid_keys(curve, 3, seed)
    too_big = ((c.p, v[0][0][1]), v[0][1])
    keys = [v[0], kc.OFF_TWIST, None, v[1], off_subgroup_point(curve), too_big, v[2]]
    return keys, [1, NOT_ON_CURVE, 1, 1, NOT_ON_CURVE, NOT_ON_CURVE, 1]


def octet_cases(curve, seed=9):
    """(octet strings, expected statuses, expected keys): both signs of y, the identity encoding, an identity encoding with a
    stray bit, an x >= p, an x without a root, the point outside the subgroup, a wrong compression flag (BLS12-381)."""
    c = bbs.SUITES[curve].curve
    n = c.fp_bytes
    v = valid_keys(curve, 2, seed)
    neg = c.g2_neg(v[0])
    bls = c.name == "bls12_381"
    ident = bbs.g2_compress(c, None)
    stray = bytearray(ident)
    stray[n] |= 1
    big = bytearray(bbs.g2_compress(c, v[1]))
    pb = c.p.to_bytes(n, "big" if bls else "little")
    keep = big[0] & 0xE0 if bls else 0
    big[0:n] = pb                                     # the first coordinate on the wire (x.c1 / x.c0) = p
    if bls:
        big[0] |= keep
    noroot = bbs.g2_compress(c, (rootless_x(curve), (0, 0)))
    off = off_subgroup_point(curve)
    octs = [bbs.g2_compress(c, v[0]), ident, bytes(stray), bbs.g2_compress(c, neg), bytes(big), noroot, bbs.g2_compress(c, off),
            bbs.g2_compress(c, v[1])]
    want = [1, 1, NONCANONICAL, 1, NONCANONICAL, NOT_ON_CURVE, NOT_ON_CURVE, 1]
    keys = [v[0], None, None, neg, None, None, None, v[1]]
    if bls:
        flag = bytearray(bbs.g2_compress(c, v[1]))
        flag[0] &= 0x7F                                # not the compressed form
        octs.insert(3, bytes(flag))
        want.insert(3, NONCANONICAL)
        keys.insert(3, None)
    return octs, want, keys


def _arr(b):
    return np.frombuffer(bytes(b) if len(b) else b"\0", dtype=np.uint8).copy()


def key_entries(eng, path, keys=None, octets=None):
    """bbs_selftest_key_entries: (entries [n] of bytes, statuses, decoded records [n] of bytes (octet form))."""
    eb = int(eng.lib.bbs_selftest_key_entry_bytes(eng.curve))
    rb = 4 * eng.fpb
    n = len(octets) if octets is not None else len(keys)
    ent = np.zeros(max(n, 1) * eb, dtype=np.uint8)
    st = np.full(max(n, 1), -128, dtype=np.int8)
    rec_out = np.full(max(n, 1) * rb, 0xEE, dtype=np.uint8)
    if octets is not None:
        buf = _arr(b"".join(octets))
        rc = eng.lib.bbs_selftest_key_entries(eng.h, n, None, None, buf.ctypes.data_as(_lib.c_u8p), path, ent.ctypes.data_as(_lib.c_u8p),
                                              st.ctypes.data_as(_lib.c_i8p), rec_out.ctypes.data_as(_lib.c_u8p))
    else:
        buf = _arr(b"".join(record(eng.fpb, k) for k in keys))
        ident = np.array([1 if k is None else 0 for k in keys] + [0], dtype=np.int8)
        rc = eng.lib.bbs_selftest_key_entries(eng.h, n, buf.ctypes.data_as(_lib.c_u8p), ident.ctypes.data_as(_lib.c_i8p), None, path,
                                              ent.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p), None)
    assert rc == 0, rc
    e, r = ent.tobytes(), rec_out.tobytes()
    return [e[k * eb:(k + 1) * eb] for k in range(n)], list(st[:n]), [r[k * rb:(k + 1) * rb] for k in range(n)]


def add_raw(eng, keys):
    """bbs_ctx_add_public_keys with records built here (a coordinate >= p stays as it is): (first_index, statuses)."""
    n = len(keys)
    buf = _arr(b"".join(record(eng.fpb, k) for k in keys))
    ident = np.array([1 if k is None else 0 for k in keys] + [0], dtype=np.int8)
    st = np.full(max(n, 1), -128, dtype=np.int8)
    first = ctypes.c_uint32(0xFFFFFFFF)
    rc = eng.lib.bbs_ctx_add_public_keys(eng.h, n, buf.ctypes.data_as(_lib.c_u8p), ident.ctypes.data_as(_lib.c_i8p),
                                         st.ctypes.data_as(_lib.c_i8p), ctypes.byref(first))
    assert rc == 0, rc
    return int(first.value), list(st[:n])


def from_octets_one(eng, octets):
    """bbs_public_key_from_octets for one string: the status an add by octets must give (1 for BBS_OK)."""
    rec = np.zeros(4 * eng.fpb, dtype=np.uint8)
    inf = ctypes.c_int(0)
    rc = eng.lib.bbs_public_key_from_octets(eng.curve, _arr(octets).ctypes.data_as(_lib.c_u8p), rec.ctypes.data_as(_lib.c_u8p), ctypes.byref(inf))
    return (1 if rc == 0 else rc), rec.tobytes(), inf.value
