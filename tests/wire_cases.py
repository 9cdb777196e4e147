"""Untrusted encodings at every field's boundary: the case tables of the wire and record ingests, both curves, and the checks
that run them through the library.  Every expected status comes from the model (tests/wire_ref.py) or the oracle; every builder
asserts what it built.  Shared by tests/test_wire_ref.py (builders only), tests/test_wire_hosttwin.py and tests/test_wire_gpu.py.

A CELL is (label, item, want): the item is a dict of plain integers and bytes in the form the entry point takes, `want` the
model's status.  Labels are what SITES (below) names; a check runs all cells of a table in calls of at most MAX_CALL items."""
import copy
import random

import numpy as np

from bbs_sign_amd import _lib
from bbs_sign_amd.engine import Proof, Signature
from oracle import bbs

import keyreg_cases as kr
import parity_cases as pc
import wire_ref as wr

# One message count serves every table: no ingest body branches on L itself, only on an item's own counts against it, and those
# vary here -- three disclosed messages beside two commitments (shape A), one beside four (shape B), and the length defects give
# items of 4 and 6 messages; five is the smallest count with a first, a middle and a last commitment AND disclosed message.
L = 5
MAX_CALL = 130
CURVES = ("bls12_381", "bn254")
H_BLS = 0x396c8c005555e1568c00aaab0000aaab          # cofactor of BLS12-381's G1: 3 * 11^2 * 10177^2 * 859267^2 * 52437899^2
H_PRIMES = (3, 11, 10177, 859267, 52437899)
GEOMETRY_N = 65
GEOMETRY_ITEMS = (20, 21, 22, 42, 43, 63, 64)


# ---- field values -----------------------------------------------------------------------------------------------------------
def field_values(m, v, bits, zero_ok=True):
    """The table of one field: modulus m, a valid value v, `bits` bits on the wire.  [(name, value)], values distinct."""
    top = 32 * ((m.bit_length() - 1) // 32)
    lo = m & 0xFFFFFFFF
    rows = ([("zero", 0)] if zero_ok else []) + [
        ("m-1", m - 1), ("m", m), ("m+1", m + 1), ("alias", v + m), ("ones", (1 << bits) - 1),
        ("lo-1", m - lo + ((lo - 1) & 0xFFFFFFFF)), ("lo+1", m - lo + ((lo + 1) & 0xFFFFFFFF)),
        ("hi-1", m - (1 << top)), ("hi+1", m + (1 << top))]
    out, seen = [], set()
    for name, val in rows:
        assert 0 <= val < (1 << bits), (name, "does not fit the field's %d bits" % bits)
        if val not in seen:
            seen.add(val)
            out.append((name, val))
    assert v < m and {"m-1", "m", "m+1", "alias", "ones", "hi-1", "hi+1"} <= {n for n, _ in out}
    return out


# ---- encodings --------------------------------------------------------------------------------------------------------------
def enc_x(c, x, big=False, inf=False, comp=True, n_coord=1):
    """A compressed string from its parts, nothing checked: value x in n_coord * fp_bytes octets, the three flags as given."""
    n = c.fp_bytes * n_coord
    if wr.is_bls(c):
        b = bytearray(x.to_bytes(n, "big"))
        b[0] |= (0x80 if comp else 0) | (0x40 if inf else 0) | (0x20 if big else 0)
    else:
        b = bytearray(x.to_bytes(n, "little"))
        b[n - 1] |= (0x40 if inf else 0) | (0x80 if big else 0)
    return bytes(b)


def enc_pt(c, pt):
    """compress(pt) for a point given as integers (x may be an alias x + p): the sign flag is y's."""
    return enc_x(c, pt[0], pt[1] % c.p > (c.p - 1) // 2)


def be32(v):
    return int(v).to_bytes(32, "big")


def pv_octets(c, it):
    return b"".join(it.get("enc", {}).get(k, None) or enc_pt(c, it["pts"][k]) for k in range(3)) + \
        b"".join(be32(v) for v in it["sc"][:3] + it["cms"] + it["sc"][3:]) + it.get("tail", b"")


def vf_octets(c, it):
    return (it.get("enc") or enc_pt(c, it["a"])) + be32(it["e"]) + it.get("tail", b"")


def rootless_x(c):
    x = 7
    while pow((x ** 3 + c.b) % c.p, (c.p - 1) // 2, c.p) == 1:
        x += 1
    assert wr.fp_sqrt(c, x ** 3 + c.b) is None
    return x


# ---- BLS12-381 points outside the subgroup ----------------------------------------------------------------------------------
_off_subgroup = None


def off_subgroup_points():
    """{label: point}: T_q of every prime order q | h, G + T_q, T_3 + T_11, and one point whose order is the product of all
    five primes -- from two points found by a small-x search.  Every one is on the curve and [r]P != identity."""
    global _off_subgroup
    if _off_subgroup is not None:
        return _off_subgroup
    c = bbs.BLS_SUITE.curve
    hh = H_BLS
    for q in H_PRIMES:
        while hh % q == 0:
            hh //= q
    assert hh == 1 and H_BLS == 3 * 11 ** 2 * 10177 ** 2 * 859267 ** 2 * 52437899 ** 2
    starts, x = [], 1
    while len(starts) < 2:
        y = wr.fp_sqrt(c, x ** 3 + c.b)
        if y is not None:
            starts.append((x, y))
        x += 1
    tq = {}
    for s in starts:
        t = c.g1_mul(s, c.r)                              # order divides h
        for q in H_PRIMES:
            if q in tq:
                continue
            e = 1 if q == 3 else 2
            u = c.g1_mul(t, H_BLS // q ** e)              # order divides q^e
            while u is not None and c.g1_mul(u, q) is not None:
                u = c.g1_mul(u, q)
            if u is not None:
                tq[q] = u
    assert sorted(tq) == sorted(H_PRIMES), "a prime of the cofactor has no point among the two starts"
    out = {}
    for q, t in tq.items():
        assert c.g1_is_on_curve(t) and c.g1_mul(t, q) is None
        out["T_%d" % q] = t
        out["G+T_%d" % q] = c.g1_add(c.g1, t)
    out["T_3+T_11"] = c.g1_add(tq[3], tq[11])
    full = None
    for q in H_PRIMES:
        full = c.g1_add(full, tq[q])
    n_full = 1
    for q in H_PRIMES:
        n_full *= q
    assert c.g1_mul(full, n_full) is None and all(c.g1_mul(full, n_full // q) is not None for q in H_PRIMES)
    out["T_all"] = full
    for k, p in out.items():
        assert c.g1_is_on_curve(p) and c.g1_mul(p, c.r) is not None, k
        assert wr.g1_from_octets(c, enc_pt(c, p))[0] == wr.NOT_ON_CURVE, k
    assert len(out) >= 10
    _off_subgroup = out
    return out


# ---- BN254 points at the sign boundary --------------------------------------------------------------------------------------
def cube_root(p, a):
    """A cube root of a mod p, or None: Tonelli-Shanks on the 3-part of p - 1 (p = 1 mod 9 on BN254, so no single
    exponentiation gives it)."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 3, p) != 1:
        return None
    s, t = 0, p - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    g = 2
    while pow(g, (p - 1) // 3, p) == 1:
        g += 1
    gen = pow(g, t, p)                                    # generates the subgroup of order 3^s
    x = pow(a, pow(3, -1, t), p)                          # x^3 = a * w, w in that subgroup and a cube there
    w = pow(x, 3, p) * pow(a, -1, p) % p
    order, lg = 3 ** s, 0
    gamma, ginv = pow(gen, order // 3, p), pow(gen, -1, p)
    for k in range(s):                                    # w = gen^lg, digit by digit in base 3
        hk = pow(w * pow(ginv, lg, p) % p, order // 3 ** (k + 1), p)
        d, gg = 0, 1
        while gg != hk:
            gg, d = gg * gamma % p, d + 1
        lg += d * 3 ** k
    assert lg % 3 == 0
    r = x * pow(ginv, lg // 3, p) % p
    assert pow(r, 3, p) == a
    return r


_boundary = None


def sign_boundary_points(kmax=40):
    """BN254 points (x, y) with y = (p - 1)/2 - k or (p + 1)/2 + k, k < kmax: (below, above), at least 8 each."""
    global _boundary
    if _boundary is None:
        c = bbs.BN_SUITE.curve
        half = (c.p - 1) // 2
        below, above = [], []
        for k in range(kmax):
            for y, side in ((half - k, below), (half + 1 + k, above)):
                x = cube_root(c.p, y * y - c.b)
                if x is not None:
                    assert pow(x, 3, c.p) == (y * y - c.b) % c.p and c.g1_is_on_curve((x, y))
                    side.append((x, y))
        assert len(below) >= 8 and len(above) >= 8, (len(below), len(above))
        _boundary = (below, above)
    return _boundary


# ---- the world: credentials made by the oracle ------------------------------------------------------------------------------
class World:
    def __init__(self, curve):
        self.curve = curve
        self.tables = {}
        suite = bbs.SUITES[curve]
        c = self.c = suite.curve
        rng = self.rng = random.Random(4242 if wr.is_bls(c) else 2424)
        self.s = wr.Setting(suite, pc.gens_for(suite, L + 1), rng.randrange(1, c.r))
        self.hdr, self.ph = b"wire-header", b"ph"
        self.raw = [bytes([65 + j]) * (j + 1) for j in range(L)]
        self.msgs = bbs.msg_to_scalars(suite, self.raw, self.s.api_id)
        self.sig = bbs.core_sign(suite, self.s.sk, self.s.gens, self.hdr, self.msgs, self.s.api_id)
        self.lim = (1 << wr.value_bits(c)) - c.p          # a compressed x below this has an alias x + p that fits
        # shape "A": three disclosed messages; shape "B": four commitments.  Fresh proofs are searched (at most 64) until
        # every point position has an x with an alias, in both shapes' pools together
        self.proofs = {"A": [], "B": []}
        self.alias_at = {}
        for k in range(64):
            shape = "AB"[k & 1]
            self.proofs[shape].append(self._proof(shape))
            for p in range(3):
                if p not in self.alias_at and self.proofs[shape][-1]["pts"][p][0] < self.lim:
                    self.alias_at[p] = self.proofs[shape][-1]
            if len(self.alias_at) == 3 and k >= 3:
                break
        assert sorted(self.alias_at) == [0, 1, 2], "no proof among 64 has an aliasable x at every point position"
        # signatures over other messages until one has an aliasable A.x
        self.sig_alias = None
        for k in range(64):
            raw = self.raw[:-1] + [b"alias-%d" % k]
            m = bbs.msg_to_scalars(suite, raw, self.s.api_id)
            sg = bbs.core_sign(suite, self.s.sk, self.s.gens, self.hdr, m, self.s.api_id)
            if sg.a[0] < self.lim:
                self.sig_alias = {"a": sg.a, "e": sg.e, "msgs": m, "raw": raw, "hdr": self.hdr}
                break
        assert self.sig_alias is not None
        self.vf = {"a": self.sig.a, "e": self.sig.e, "msgs": list(self.msgs), "raw": list(self.raw), "hdr": self.hdr}
        for it in [self.vf, self.sig_alias]:
            assert wr.core_verify_status(self.s, it["a"], it["e"], it["msgs"], it["hdr"]) == 1
        for it in [self.proofs["A"][0], self.proofs["B"][0]] + list(self.alias_at.values()):
            assert self.pv_want(it) == 1 and self.pv_oct_want(it) == 1

    def _proof(self, shape):
        idx = [0, 2, 4] if shape == "A" else [3]
        rnd = [self.rng.randrange(1, self.c.r) for _ in range(5 + L - len(idx))]
        p = bbs.core_proof_gen(self.s.suite, self.s.pk, self.sig, self.hdr, self.s.gens, self.ph, self.msgs, idx, self.s.api_id, rnd)
        return {"pts": [p.a_bar, p.b_bar, p.d], "sc": [p.e_cap, p.r1_cap, p.r3_cap, p.challenge], "cms": list(p.commitments),
                "dm": [self.msgs[j] for j in idx], "dm_raw": [self.raw[j] for j in idx], "idx": list(idx), "hdr": self.hdr, "ph": self.ph}

    def pv_want(self, it):
        return wr.core_proof_verify_status(self.s, it["pts"], it["sc"], it["cms"], it["dm"], it["idx"], it["hdr"], it["ph"])

    def pv_oct_want(self, it):
        return wr.proof_verify_octets_status(self.s, pv_octets(self.c, it), it["dm"], it["idx"], it["hdr"], it["ph"])

    def vf_want(self, it):
        return wr.core_verify_status(self.s, it["a"], it["e"], it["msgs"], it["hdr"])

    def vf_oct_want(self, it):
        return wr.verify_octets_status(self.s, vf_octets(self.c, it), it["msgs"], it["hdr"])


_worlds = {}


def world(curve):
    if curve not in _worlds:
        _worlds[curve] = World(curve)
    return _worlds[curve]


def _per_world(build):
    """A table is built once per world; its items are never modified by the checks."""
    def cached(w):
        if build.__name__ not in w.tables:
            w.tables[build.__name__] = build(w)
        return w.tables[build.__name__]
    cached.__doc__ = build.__doc__
    return cached


def _set_pt(it, k, x=None, y=None):
    q = it["pts"][k]
    it["pts"][k] = (q[0] if x is None else x, q[1] if y is None else y)


def _finish(cells, want_fn):
    """[(label, item)] -> [(label, item, want)]; every alias cell must be refused as not canonical."""
    out = []
    for label, it in cells:
        want = want_fn(it)
        if ":alias" in label:
            assert want == wr.NONCANONICAL, (label, want)
        out.append((label, it, want))
    return out


# ---- tables: record forms ---------------------------------------------------------------------------------------------------
@_per_world
def pv_record_cells(w):
    """core_proof_verify records: each of the six coordinates, the four scalars, the first, a middle and the last commitment
    and disclosed message, each through the whole field table."""
    c, cells = w.c, []
    a, b = w.proofs["A"][0], w.proofs["B"][0]
    for k in range(6):
        for name, val in field_values(c.p, b["pts"][k // 2][k % 2], 8 * c.fp_bytes):
            it = copy.deepcopy(b)
            _set_pt(it, k // 2, **{"xy"[k % 2]: val})
            cells.append(("pv.rec.coord%d:%s" % (k, name), it))
    for k in range(4):
        for name, val in field_values(c.r, b["sc"][k], 256):
            it = copy.deepcopy(b)
            it["sc"][k] = val
            cells.append(("pv.rec.sc%d:%s" % (k, name), it))
    for pos, k in (("first", 0), ("middle", 2), ("last", 3)):
        for name, val in field_values(c.r, b["cms"][k], 256):
            it = copy.deepcopy(b)
            it["cms"][k] = val
            cells.append(("pv.rec.cm_%s:%s" % (pos, name), it))
    for pos, k in (("first", 0), ("middle", 1), ("last", 2)):
        for name, val in field_values(c.r, a["dm"][k], 256):
            it = copy.deepcopy(a)
            it["dm"][k] = val
            cells.append(("pv.rec.dm_%s:%s" % (pos, name), it))
    return _finish(cells, w.pv_want)


@_per_world
def vf_record_cells(w):
    """core_verify records: A.x, A.y, e, and the first, a middle and the last message."""
    c, cells, base = w.c, [], w.vf
    for k in range(2):
        for name, val in field_values(c.p, base["a"][k], 8 * c.fp_bytes):
            it = copy.deepcopy(base)
            it["a"] = (val, base["a"][1]) if k == 0 else (base["a"][0], val)
            cells.append(("vf.rec.A%s:%s" % ("xy"[k], name), it))
    for name, val in field_values(c.r, base["e"], 256):
        it = copy.deepcopy(base)
        it["e"] = val
        cells.append(("vf.rec.e:%s" % name, it))
    for pos, k in (("first", 0), ("middle", 2), ("last", L - 1)):
        for name, val in field_values(c.r, base["msgs"][k], 256):
            it = copy.deepcopy(base)
            it["msgs"][k] = val
            cells.append(("vf.rec.msg_%s:%s" % (pos, name), it))
    return _finish(cells, w.vf_want)


@_per_world
def pg_record_cells(w):
    """core_proof_gen: the signature record's A.x, A.y, e, the first, a middle and the last message and random scalar.  The
    item is (a, e, msgs, idx, rnd); disclosed [1]: 5 + 4 random scalars."""
    c, cells = w.c, []
    rnd = [w.rng.randrange(1, c.r) for _ in range(9)]
    base = {"a": w.sig.a, "e": w.sig.e, "msgs": list(w.msgs), "idx": [1], "rnd": rnd, "hdr": w.hdr, "ph": w.ph}
    for k in range(2):
        for name, val in field_values(c.p, base["a"][k], 8 * c.fp_bytes):
            it = copy.deepcopy(base)
            it["a"] = (val, base["a"][1]) if k == 0 else (base["a"][0], val)
            cells.append(("pg.rec.A%s:%s" % ("xy"[k], name), it))
    for name, val in field_values(c.r, base["e"], 256):
        it = copy.deepcopy(base)
        it["e"] = val
        cells.append(("pg.rec.e:%s" % name, it))
    for what, n_ in (("msgs", L), ("rnd", 9)):
        for pos, k in (("first", 0), ("middle", n_ // 2), ("last", n_ - 1)):
            for name, val in field_values(c.r, base[what][k], 256):
                it = copy.deepcopy(base)
                it[what][k] = val
                cells.append(("pg.rec.%s_%s:%s" % (what, pos, name), it))
    return _finish(cells, lambda it: wr.core_proof_gen_status(w.s, it["a"], it["e"], it["msgs"], it["idx"], it["rnd"]))


@_per_world
def sign_cells(w):
    c, cells = w.c, []
    for pos, k in (("first", 0), ("middle", 2), ("last", L - 1)):
        for name, val in field_values(c.r, w.msgs[k], 256):
            m = list(w.msgs)
            m[k] = val
            cells.append(("sg.msg_%s:%s" % (pos, name), {"msgs": m}))
    return _finish(cells, lambda it: wr.core_sign_status(w.s, it["msgs"]))


# ---- tables: octet forms ----------------------------------------------------------------------------------------------------
@_per_world
def pv_octet_cells(w):
    """Proof octets: x of each point, e^, r1^, r3^, the first, a middle and the last m^, c."""
    c, cells = w.c, []
    b = w.proofs["B"][0]
    bits = wr.value_bits(c)
    for k in range(3):
        src = w.alias_at[k]
        for name, val in field_values(c.p, src["pts"][k][0], bits):
            it = copy.deepcopy(src)
            _set_pt(it, k, x=val)
            cells.append(("pv.oct.x%d:%s" % (k, name), it))
    for k, nm in enumerate(("e^", "r1^", "r3^", "c")):
        for name, val in field_values(c.r, b["sc"][k], 256):
            it = copy.deepcopy(b)
            it["sc"][k] = val
            cells.append(("pv.oct.%s:%s" % (nm, name), it))
    for pos, k in (("first", 0), ("middle", 2), ("last", 3)):
        for name, val in field_values(c.r, b["cms"][k], 256):
            it = copy.deepcopy(b)
            it["cms"][k] = val
            cells.append(("pv.oct.m^_%s:%s" % (pos, name), it))
    a = w.proofs["A"][0]
    for pos, k in (("first", 0), ("middle", 1), ("last", 2)):
        for name, val in field_values(c.r, a["dm"][k], 256):
            it = copy.deepcopy(a)
            it["dm"][k] = val
            cells.append(("pv.oct.dm_%s:%s" % (pos, name), it))
    return _finish(cells, w.pv_oct_want)


@_per_world
def vf_octet_cells(w):
    c, cells = w.c, []
    for name, val in field_values(c.p, w.sig_alias["a"][0], wr.value_bits(c)):
        it = copy.deepcopy(w.sig_alias)
        it["a"] = (val, it["a"][1])
        cells.append(("vf.oct.x:%s" % name, it))
    for name, val in field_values(c.r, w.vf["e"], 256):
        it = copy.deepcopy(w.vf)
        it["e"] = val
        cells.append(("vf.oct.e:%s" % name, it))
    return _finish(cells, w.vf_oct_want)


def flag_encodings(c, pt):
    """[(name, string)]: every flag combination of the curve on the point's x, on x = 0 and on the identity with no stray bit,
    one in the lowest byte and one in the highest value bit (the sign flag is one of the combinations)."""
    bits = wr.value_bits(c)
    out = []
    combos = [(comp, inf, big) for comp in ((True, False) if wr.is_bls(c) else (True,)) for inf in (False, True) for big in (False, True)]
    for what, val in (("x", pt[0]), ("x0", 0), ("stray_lo", 1), ("stray_hi", 1 << (bits - 1))):
        for comp, inf, big in combos:
            if what.startswith("stray") and not inf:
                continue
            out.append(("%s/%s%s%s" % (what, "C" if comp else "-", "I" if inf else "-", "S" if big else "-"), enc_x(c, val, big, inf, comp)))
    assert len(out) == (24 if wr.is_bls(c) else 12)
    return out


@_per_world
def pv_flag_cells(w):
    cells = []
    b = w.proofs["B"][0]
    for k in range(3):
        for name, s in flag_encodings(w.c, b["pts"][k]):
            it = copy.deepcopy(b)
            it["enc"] = {k: s}
            cells.append(("pv.oct.flags%d:%s" % (k, name), it))
    return _finish(cells, w.pv_oct_want)


@_per_world
def vf_flag_cells(w):
    cells = []
    for name, s in flag_encodings(w.c, w.vf["a"]):
        it = copy.deepcopy(w.vf)
        it["enc"] = s
        cells.append(("vf.oct.flags:%s" % name, it))
    return _finish(cells, w.vf_oct_want)


@_per_world
def subgroup_cells(w):
    """BLS12-381: every point outside the subgroup at each of a proof's positions and as a signature's A: all -41."""
    assert wr.is_bls(w.c)
    pv, vf = [], []
    b = w.proofs["B"][0]
    for name, pt in off_subgroup_points().items():
        for k in range(3):
            it = copy.deepcopy(b)
            it["enc"] = {k: enc_pt(w.c, pt)}
            pv.append(("pv.oct.subgroup%d:%s" % (k, name), it))
        it = copy.deepcopy(w.vf)
        it["enc"] = enc_pt(w.c, pt)
        vf.append(("vf.oct.subgroup:%s" % name, it))
    pv, vf = _finish(pv, w.pv_oct_want), _finish(vf, w.vf_oct_want)
    assert all(x[2] == wr.NOT_ON_CURVE for x in pv + vf)
    return pv, vf


# ---- precedence -------------------------------------------------------------------------------------------------------------
def _pv_defects(w):
    """{kind: function that plants it on a proof_verify octets item}.  Two kinds that write the same field do not pair."""
    c = w.c
    nx = rootless_x(c)
    d = {}
    d["shape"] = (("tail",), lambda it: it.__setitem__("tail", b"\0"))
    for k in range(3):
        d["pt%d:-40" % k] = (("pt%d" % k,), lambda it, k=k: it.setdefault("enc", {}).__setitem__(k, enc_x(c, c.p)))
        d["pt%d:-41" % k] = (("pt%d" % k,), lambda it, k=k: it.setdefault("enc", {}).__setitem__(k, enc_x(c, nx)))
        d["pt%d:identity" % k] = (("pt%d" % k,), lambda it, k=k: it.setdefault("enc", {}).__setitem__(k, enc_x(c, 0, inf=True)))
    d["fixed scalar"] = (("sc1",), lambda it: it["sc"].__setitem__(1, c.r))
    d["commitment"] = (("cm",), lambda it: it["cms"].__setitem__(len(it["cms"]) - 1, c.r + 1))
    d["c"] = (("sc3",), lambda it: it["sc"].__setitem__(3, (1 << 256) - 1))
    d["index"] = (("idx",), lambda it: it["idx"].__setitem__(0, L + 3))
    d["count"] = (("dmn",), lambda it: (it["dm"].append(1), it["dm_raw"].append(b"x")))
    d["length"] = (("cmn",), lambda it: it["cms"].insert(0, 7))              # one commitment too many: l = L + 1
    d["duplicate"] = (("idx", "dmn", "cm", "cmn"), lambda it: (it["idx"].append(it["idx"][-1]), it["dm"].append(it["dm"][-1]), it["dm_raw"].append(it["dm_raw"][-1]),
                                                        it["cms"].pop()))
    d["disclosed message"] = (("dm",), lambda it: it["dm"].__setitem__(len(it["idx"]) - 1, c.r + 2))
    return d


@_per_world
def pv_precedence_cells(w):
    """Every ordered pair of defect kinds that can sit on one proof_verify octets item (shape A: three disclosed messages,
    two commitments), and every kind alone."""
    d = _pv_defects(w)
    base = w.proofs["A"][0]
    cells, pairs = [], 0
    for k1, (f1, plant1) in d.items():
        it = copy.deepcopy(base)
        plant1(it)
        cells.append(("pv.oct.defect:%s" % k1, it))
        for k2, (f2, plant2) in d.items():
            if k1 == k2 or set(f1) & set(f2):
                continue
            it = copy.deepcopy(base)
            plant1(it)
            plant2(it)
            cells.append(("pv.oct.pair:%s+%s" % (k1, k2), it))
            pairs += 1
    assert pairs >= 18 * 17 - 9 * 2 - 16, pairs
    out = _finish(cells, w.pv_oct_want)
    alone = {lab.split(":", 1)[1]: want for lab, _, want in out if lab.startswith("pv.oct.defect:")}
    assert alone["shape"] == -42 and alone["pt1:-40"] == -40 and alone["pt2:-41"] == -41 and alone["pt0:identity"] == -42, alone
    assert alone["fixed scalar"] == alone["commitment"] == alone["c"] == alone["disclosed message"] == -40, alone
    assert alone["index"] == -3 and alone["count"] == -6 and alone["length"] == -1 and alone["duplicate"] == -22, alone
    return out


@_per_world
def pv_record_precedence_cells(w):
    """Every ordered pair of defect kinds on one core_proof_verify RECORD item (shape A), and every kind alone."""
    c = w.c
    d = {"index": (("idx",), lambda it: it["idx"].__setitem__(0, L + 3)),
         "count": (("dmn",), lambda it: it["dm"].append(1)),
         "length": (("cmn",), lambda it: it["cms"].append(1)),
         "duplicate": (("idx", "dmn", "cmn", "cm"), lambda it: (it["idx"].append(it["idx"][-1]), it["dm"].append(it["dm"][-1]), it["cms"].pop())),
         "coordinate": (("pt0",), lambda it: _set_pt(it, 0, y=it["pts"][0][1] + c.p)),
         "off curve": (("pt2",), lambda it: _set_pt(it, 2, y=(it["pts"][2][1] + 1) % c.p)),
         "scalar": (("sc",), lambda it: it["sc"].__setitem__(2, c.r)),
         "commitment": (("cm",), lambda it: it["cms"].__setitem__(0, c.r + 1)),
         "disclosed message": (("dm",), lambda it: it["dm"].__setitem__(0, (1 << 256) - 1))}
    base = w.proofs["A"][0]
    cells = []
    for k1, (f1, p1) in d.items():
        it = copy.deepcopy(base)
        p1(it)
        cells.append(("pv.rec.defect:%s" % k1, it))
        for k2, (f2, p2) in d.items():
            if k1 != k2 and not set(f1) & set(f2):
                it = copy.deepcopy(base)
                p1(it)
                p2(it)
                cells.append(("pv.rec.pair:%s+%s" % (k1, k2), it))
    out = _finish(cells, w.pv_want)
    alone = {lab.split(":", 1)[1]: want for lab, _, want in out if lab.startswith("pv.rec.defect:")}
    assert alone == {"index": -3, "count": -6, "length": -1, "duplicate": -22, "coordinate": -40, "off curve": -41, "scalar": -40,
                     "commitment": -40, "disclosed message": -40}, alone
    assert sum(1 for lab, _, _ in out if ".pair:" in lab) >= 9 * 8 - 12
    return out


@_per_world
def vf_precedence_cells(w):
    c = w.c
    nx = rootless_x(c)
    d = {"shape": ("tail", lambda it: it.__setitem__("tail", b"\0")),
         "A:-40": ("a", lambda it: it.__setitem__("enc", enc_x(c, c.p + 1))),
         "A:-41": ("a", lambda it: it.__setitem__("enc", enc_x(c, nx))),
         "A:identity": ("a", lambda it: it.__setitem__("enc", enc_x(c, 0, inf=True))),
         "e>=r": ("e", lambda it: it.__setitem__("e", c.r)),
         "e=0": ("e", lambda it: it.__setitem__("e", 0)),
         "count": ("n", lambda it: (it["msgs"].pop(), it["raw"].pop())),
         "message": ("m", lambda it: it["msgs"].__setitem__(0, c.r))}
    cells, pairs = [], 0
    for k1, (f1, p1) in d.items():
        it = copy.deepcopy(w.vf)
        p1(it)
        cells.append(("vf.oct.defect:%s" % k1, it))
        for k2, (f2, p2) in d.items():
            if k1 != k2 and f1 != f2:
                it = copy.deepcopy(w.vf)
                p1(it)
                p2(it)
                cells.append(("vf.oct.pair:%s+%s" % (k1, k2), it))
                pairs += 1
    assert pairs == 8 * 7 - 3 * 2 - 2
    out = _finish(cells, w.vf_oct_want)
    alone = {lab.split(":", 1)[1]: want for lab, _, want in out if lab.startswith("vf.oct.defect:")}
    assert alone == {"shape": -42, "A:-40": -40, "A:-41": -41, "A:identity": -42, "e>=r": -40, "e=0": -42, "count": -1, "message": -40}, alone
    return out


def _pairs(base, d, prefix, want_fn):
    """Every kind of d alone ("<prefix>.defect:<kind>") and every ordered pair of kinds that write different fields
    ("<prefix>.pair:<k1>+<k2>") planted on copies of base; d = {kind: (fields, plant)}."""
    cells = []
    for k1, (f1, p1) in d.items():
        it = copy.deepcopy(base)
        p1(it)
        cells.append(("%s.defect:%s" % (prefix, k1), it))
        for k2, (f2, p2) in d.items():
            if k1 != k2 and not set(f1) & set(f2):
                it = copy.deepcopy(base)
                p1(it)
                p2(it)
                cells.append(("%s.pair:%s+%s" % (prefix, k1, k2), it))
    out = _finish(cells, want_fn)
    return out, {lab.split(":", 1)[1]: want for lab, _, want in out if ".defect:" in lab}


def pg_base(w):
    """A core_proof_gen item: the world's signature, disclosed [1], 5 + 4 random scalars."""
    rnd = [random.Random(99).randrange(1, w.c.r) for _ in range(9)]
    return {"a": w.sig.a, "e": w.sig.e, "msgs": list(w.msgs), "raw": list(w.raw), "idx": [1], "rnd": rnd, "hdr": w.hdr, "ph": w.ph}


def _pg_want(s):
    return lambda it: wr.core_proof_gen_status(s, it["a"], it["e"], it["msgs"], it["idx"], it["rnd"])


def _pg_defects(w):
    """The defect kinds of a core_proof_gen item.  The number of random scalars is a contract of the call (5 + l - r, r counted
    before deduplication), so every kind that changes l or r resizes them."""
    c = w.c

    def resize(it):
        it["rnd"] = (it["rnd"] * 3)[:5 + len(it["msgs"]) - len(it["idx"])]

    return {"too many indexes": (("idx", "n"), lambda it: (it.__setitem__("idx", list(range(len(it["msgs"]))) + [0]), resize(it))),
            "index": (("idx",), lambda it: it["idx"].__setitem__(0, L + 3)),
            "length": (("n", "msg"), lambda it: (it["msgs"].pop(), it["raw"].pop(), resize(it))),
            "duplicate": (("idx", "n"), lambda it: (it["idx"].append(it["idx"][-1]), resize(it))),
            "coordinate": (("ax",), lambda it: it.__setitem__("a", (it["a"][0] + c.p, it["a"][1]))),
            "off curve": (("ay",), lambda it: it.__setitem__("a", (it["a"][0], (it["a"][1] + 1) % c.p))),
            "e": (("e",), lambda it: it.__setitem__("e", it["e"] + c.r)),
            "random scalar": (("rnd",), lambda it: it["rnd"].__setitem__(0, c.r)),
            "message": (("msg",), lambda it: it["msgs"].__setitem__(0, c.r + 1))}


@_per_world
def pg_record_precedence_cells(w):
    """core_proof_gen records: every kind alone and every ordered pair."""
    out, alone = _pairs(pg_base(w), _pg_defects(w), "pg.rec", _pg_want(w.s))
    assert alone == {"too many indexes": -2, "index": -3, "length": -1, "duplicate": -4, "coordinate": -40, "off curve": -41, "e": -40,
                     "random scalar": -40, "message": -40}, alone
    assert sum(1 for x in out if ".pair:" in x[0]) >= 9 * 8 - 14
    return out


@_per_world
def vf_record_precedence_cells(w):
    """core_verify records: every kind alone and every ordered pair."""
    c = w.c
    d = {"length": (("n",), lambda it: it["msgs"].append(1)),
         "coordinate": (("ax",), lambda it: it.__setitem__("a", (it["a"][0] + c.p, it["a"][1]))),
         "off curve": (("ay",), lambda it: it.__setitem__("a", (it["a"][0], (it["a"][1] + 1) % c.p))),
         "e": (("e",), lambda it: it.__setitem__("e", c.r)),
         "message": (("msg",), lambda it: it["msgs"].__setitem__(1, (1 << 256) - 1))}
    out, alone = _pairs(w.vf, d, "vf.rec", w.vf_want)
    assert alone == {"length": -1, "coordinate": -40, "off curve": -41, "e": -40, "message": -40}, alone
    assert sum(1 for x in out if ".pair:" in x[0]) == 20
    return out


@_per_world
def sign_precedence_cells(w):
    d = {"length": (("n",), lambda it: it["msgs"].pop()), "message": (("msg",), lambda it: it["msgs"].__setitem__(0, w.c.r))}
    out, alone = _pairs({"msgs": list(w.msgs)}, d, "sg", lambda it: wr.core_sign_status(w.s, it["msgs"]))
    assert alone == {"length": -1, "message": -40}
    return out


def pg_wire_cells(s, cells):
    """Signature-octet cells as bbs_proof_gen_wire_batch takes them: [("pg.wire.<label>", item with idx and rnd, want)]; the
    cells whose defect is a message's VALUE do not exist with raw messages and are left out."""
    out = []
    for lab, it, _ in cells:
        if ":message" in lab or "+message" in lab:
            continue
        it = dict(it, idx=[1], rnd=[3 + k for k in range(max(5 + len(it["raw"]) - 1, 0))])
        out.append(("pg.wire." + lab, it, wr.proof_gen_wire_status(s, vf_octets(s.curve, it), len(it["raw"]), it["idx"], it["rnd"])))
    return out


@_per_world
def g1_point_cells(w):
    """[(label, string, code)] for the decode primitive: the flag table, the field table on x, no root, outside the subgroup."""
    c = w.c
    cells = [("g1.flags:" + name, s_) for name, s_ in flag_encodings(c, w.vf["a"])]
    cells += [("g1.x:" + name, enc_x(c, val, w.sig_alias["a"][1] > (c.p - 1) // 2)) for name, val in field_values(c.p, w.sig_alias["a"][0], wr.value_bits(c))]
    cells.append(("g1:no root", enc_x(c, rootless_x(c))))
    if wr.is_bls(c):
        cells += [("g1.subgroup:" + name, enc_pt(c, pt)) for name, pt in off_subgroup_points().items()]
    out = [(lab, s_, wr.g1_from_octets(c, s_)[0]) for lab, s_ in cells]
    assert dict((x[0], x[2]) for x in out)["g1.x:alias"] == wr.NONCANONICAL
    return out


# ---- a DST of more than 255 bytes (-23) -------------------------------------------------------------------------------------
@_per_world
def dst_cells(w):
    """The -23 sites.  Two settings with the world's generators and key: api_id of 252 bytes (api_id || "H2S_" too long: every
    core_* function after its length check) and of 240 bytes (only api_id || "MAP_MSG_TO_SCALAR_AS_HASH_" too long: the
    raw-message forms, before the reference's checks).  {form: cells}; each table has the untouched item (-23), defects that
    are decided earlier and keep their code, and defects that are looked at later and must NOT be reached."""
    c = w.c
    long_ = wr.Setting(w.s.suite, w.s.gens, w.s.sk, api_id=b"L" * 252)
    msg_ = wr.Setting(w.s.suite, w.s.gens, w.s.sk, api_id=b"M" * 240)
    assert long_.dst_too_long and msg_.msg_dst_too_long and not msg_.dst_too_long
    a = w.proofs["A"][0]
    pvd, pvr = _pv_defects(w), pv_record_precedence_cells(w)

    def planted(base, plant):
        it = copy.deepcopy(base)
        plant(it)
        return it

    pv_items = [("valid", copy.deepcopy(a))] + [(k, planted(a, pvd[k][1])) for k in ("shape", "pt1:-41", "c", "index", "count", "length", "duplicate",
                                                                                     "disclosed message")]
    t = {}
    t["pv.oct"] = _finish([("dst.pv.oct:" + k, it) for k, it in pv_items],
                          lambda it: wr.proof_verify_octets_status(long_, pv_octets(c, it), it["dm"], it["idx"], it["hdr"], it["ph"]))
    t["pv.wire"] = _finish([("dst.pv.wire:" + k, it) for k, it in pv_items if k != "disclosed message"],
                           lambda it: wr.proof_verify_wire_status(msg_, pv_octets(c, it), it["dm_raw"], it["idx"], it["hdr"], it["ph"]))
    t["pv.rec"] = _finish([("dst.pv.rec:valid", copy.deepcopy(a))] + [("dst." + lab, it) for lab, it, _ in pvr if ".defect:" in lab],
                          lambda it: wr.core_proof_verify_status(long_, it["pts"], it["sc"], it["cms"], it["dm"], it["idx"], it["hdr"], it["ph"]))
    vfr = vf_record_precedence_cells(w)
    t["vf.rec"] = _finish([("dst.vf.rec:valid", copy.deepcopy(w.vf))] + [("dst." + lab, it) for lab, it, _ in vfr if ".defect:" in lab],
                          lambda it: wr.core_verify_status(long_, it["a"], it["e"], it["msgs"], it["hdr"]))
    vfo = [x for x in vf_precedence_cells(w) if ".defect:" in x[0]]
    t["vf.oct"] = _finish([("dst.vf.oct:valid", copy.deepcopy(w.vf))] + [("dst." + lab, it) for lab, it, _ in vfo],
                          lambda it: wr.verify_octets_status(long_, vf_octets(c, it), it["msgs"], it["hdr"]))
    t["vf.wire"] = _finish([("dst.vf.wire:valid", copy.deepcopy(w.vf))] + [("dst.wire." + lab, it) for lab, it, _ in vfo if ":message" not in lab],
                           lambda it: wr.verify_wire_status(msg_, vf_octets(c, it), it["raw"], it["hdr"]))
    t["pg.wire"] = [("dst." + lab, it, want) for lab, it, want in pg_wire_cells(msg_, [("vf.oct:valid", copy.deepcopy(w.vf), None)] + vfo)]
    pgr = pg_record_precedence_cells(w)
    t["pg.rec"] = _finish([("dst.pg.rec:valid", pg_base(w))] + [("dst." + lab, it) for lab, it, _ in pgr if ".defect:" in lab], _pg_want(long_))
    t["sg"] = _finish([("dst.sg:valid", {"msgs": list(w.msgs)})] + [("dst." + lab, it) for lab, it, _ in sign_precedence_cells(w) if ".defect:" in lab],
                      lambda it: wr.core_sign_status(long_, it["msgs"]))
    want = {lab: x for cells in t.values() for lab, _, x in cells}
    for form in ("pv.oct", "pv.wire", "pv.rec", "vf.rec", "vf.oct", "vf.wire", "pg.rec", "sg"):
        assert want["dst.%s:valid" % form] == -23, form
    assert want["dst.pg.wire.vf.oct:valid"] == -23
    assert want["dst.pv.oct:duplicate"] == want["dst.pv.oct:disclosed message"] == want["dst.pv.rec.defect:coordinate"] == -23     # not reached
    assert want["dst.pv.oct:length"] == -1 and want["dst.pv.oct:c"] == -40 and want["dst.pv.wire:index"] == -23 and want["dst.pg.rec.defect:duplicate"] == -4
    return t, long_, msg_


# ---- lane geometry ----------------------------------------------------------------------------------------------------------
def point_defects(w):
    """{kind: (string, code)}: the point-level defects of the curve."""
    c = w.c
    d = {"x>=p": enc_x(c, c.p), "no root": enc_x(c, rootless_x(c)), "identity": enc_x(c, 0, inf=True), "identity+stray": enc_x(c, 1, inf=True)}
    if wr.is_bls(c):
        d["no flag"] = enc_x(c, w.vf["a"][0], comp=False)
        d["subgroup"] = enc_pt(c, off_subgroup_points()["G+T_11"])
    else:
        d["both flags"] = enc_x(c, 0, True, True)
    return {k: (s, wr.g1_from_octets(c, s)[0]) for k, s in d.items()}


def geometry_runs(w):
    """[(name, [items])] of GEOMETRY_N proof_verify octets items.  Per point-level kind three runs ("kind/shift0..2"): the kind
    sits at ONE point of each of items 20, 21, 22, 42, 43, 63, 64, the position rotating with the item and the shift, so the
    three runs of a kind plant it at every (item, point).  Then one run where every item is defective, the kinds and positions
    rotating, and one where only item 21 is valid.  Item 1 carries a tampered e^ (the oracle's 0) wherever it is not defective."""
    kinds = point_defects(w)
    pool = w.proofs["A"][:2] + w.proofs["B"][:2]

    def background(i):
        it = copy.deepcopy(pool[i % len(pool)])
        if i == 1:
            it["sc"][0] = (it["sc"][0] + 1) % w.c.r
        return it

    runs = []
    for rot, (kind, (s, _)) in enumerate(sorted(kinds.items())):
        for shift in range(3):
            items = [background(i) for i in range(GEOMETRY_N)]
            for j, i in enumerate(GEOMETRY_ITEMS):
                items[i]["enc"] = {(j + shift + rot) % 3: s}
            runs.append(("%s/shift%d" % (kind, shift), items))
    names = sorted(kinds)
    items = [background(i) for i in range(GEOMETRY_N)]
    for i in range(GEOMETRY_N):
        items[i]["enc"] = {i % 3: kinds[names[i % len(names)]][0]}
    runs.append(("all defective", items))
    only = copy.deepcopy(items)
    only[21] = background(21)
    runs.append(("only 21 valid", only))
    return runs


# ---- the rejecting sites and the cases that reach them ----------------------------------------------------------------------
# One entry per rejecting site -- each `return` with a code, each `ok &=`, each `verdict =` / `pre =` / `st =` that writes a code --
# of g1_decode_octets (codec_dev.hpp), PvOctIngestBody (codec_dev.hpp), PvIngestBody (stages_pv.hpp), VfIngestBody (stages_vf.hpp),
# PgIngestBody (stages_pg.hpp) and the decoder of KeyBuild (stages_key.hpp): site -> (the code the site leads to, the cases that
# reach it).  The code is the model's status of EVERY named case (tests/test_wire_ref.py).  A site that decides a point inside a
# string names the point-level cases (g1.*: the code of bbs_g1_decompress_batch).  "(BLS12-381)": the site does not exist on BN254.
SITES = {
    "g1_decode_octets: return -40, no compression flag (BLS12-381)": (-40, ["g1.flags:x/---", "g1.flags:x/--S", "g1.flags:x0/-I-"]),
    "g1_decode_octets: return 1, the identity": (1, ["g1.flags:x0/CI-"]),
    "g1_decode_octets: return -40, identity with a value bit or the sign flag": (-40, ["g1.flags:stray_lo/CI-", "g1.flags:stray_hi/CI-", "g1.flags:x0/CIS"]),
    "g1_decode_octets: return -40, x >= p": (-40, ["g1.x:m", "g1.x:m+1", "g1.x:alias", "g1.x:ones", "g1.x:hi+1"]),
    "g1_decode_octets: return -41, no root": (-41, ["g1:no root"]),
    "g1_decode_octets: return -41, outside the subgroup (BLS12-381)": (-41, ["g1.subgroup:T_3", "g1.subgroup:G+T_11", "g1.subgroup:T_all"]),
    "PvOctIngestBody: status0 = -42, shape": (-42, ["pv.oct.defect:shape", "pv.oct.pair:shape+pt0:-40"]),
    "PvOctIngestBody: verdict = -42, identity point": (-42, ["pv.oct.defect:pt0:identity", "pv.oct.defect:pt2:identity", "pv.oct.pair:pt1:identity+pt2:-41"]),
    "PvOctIngestBody: verdict = c, -40": (-40, ["pv.oct.defect:pt1:-40", "pv.oct.x0:alias", "pv.oct.pair:pt0:-40+pt1:-41"]),
    "PvOctIngestBody: verdict = c, -41": (-41, ["pv.oct.defect:pt2:-41", "pv.oct.pair:pt0:-41+pt1:-40"]),
    "PvOctIngestBody: ok &= e^, r1^, r3^": (-40, ["pv.oct.e^:m", "pv.oct.r1^:alias", "pv.oct.r3^:ones"]),
    "PvOctIngestBody: ok &= c": (-40, ["pv.oct.c:alias", "pv.oct.c:m"]),
    "PvOctIngestBody: ok &= m^": (-40, ["pv.oct.m^_first:alias", "pv.oct.m^_middle:m", "pv.oct.m^_last:alias"]),
    "PvOctIngestBody: verdict = -40, a scalar of the proof": (-40, ["pv.oct.defect:fixed scalar", "pv.oct.pair:commitment+index", "pv.oct.pair:c+length"]),
    "PvOctIngestBody: status0 = -23, msg_dst_too_long": (-23, ["dst.pv.wire:valid", "dst.pv.wire:index"]),
    "PvOctIngestBody: st = -3": (-3, ["pv.oct.defect:index", "pv.oct.pair:index+count", "dst.pv.oct:index"]),
    "PvOctIngestBody: st = -6": (-6, ["pv.oct.defect:count", "pv.oct.pair:count+length"]),
    "PvOctIngestBody: st = -1": (-1, ["pv.oct.defect:length", "pv.oct.pair:length+disclosed message", "dst.pv.oct:length"]),
    "PvOctIngestBody: st = -23, dst_too_long": (-23, ["dst.pv.oct:valid", "dst.pv.oct:duplicate", "dst.pv.oct:disclosed message"]),
    "PvOctIngestBody: st = -22": (-22, ["pv.oct.defect:duplicate", "pv.oct.pair:duplicate+disclosed message"]),
    "PvOctIngestBody: ok &= disclosed message, status0 = -40": (-40, ["pv.oct.dm_first:alias", "pv.oct.dm_middle:m", "pv.oct.dm_last:alias"]),
    "PvIngestBody: st = -3": (-3, ["pv.rec.defect:index", "pv.rec.pair:index+coordinate"]),
    "PvIngestBody: st = -6": (-6, ["pv.rec.defect:count", "pv.rec.pair:count+length"]),
    "PvIngestBody: st = -1": (-1, ["pv.rec.defect:length", "pv.rec.pair:length+scalar"]),
    "PvIngestBody: st = -23": (-23, ["dst.pv.rec:valid", "dst.pv.rec.defect:duplicate", "dst.pv.rec.defect:coordinate"]),
    "PvIngestBody: st = -22": (-22, ["pv.rec.defect:duplicate", "pv.rec.pair:duplicate+off curve"]),
    "PvIngestBody: ok &= coordinate": (-40, ["pv.rec.coord%d:alias" % k for k in range(6)] + ["pv.rec.pair:coordinate+off curve"]),
    "PvIngestBody: ok &= scalar": (-40, ["pv.rec.sc%d:alias" % k for k in range(4)]),
    "PvIngestBody: ok &= disclosed message": (-40, ["pv.rec.dm_first:alias", "pv.rec.dm_middle:alias", "pv.rec.dm_last:alias"]),
    "PvIngestBody: ok &= commitment, status0 = -40": (-40, ["pv.rec.cm_first:alias", "pv.rec.cm_middle:alias", "pv.rec.cm_last:alias"]),
    "VfIngestBody: pre = c, -40": (-40, ["vf.oct.defect:A:-40", "vf.oct.x:alias"]),
    "VfIngestBody: pre = c, -41": (-41, ["vf.oct.defect:A:-41", "vf.oct.pair:A:-41+e=0"]),
    "VfIngestBody: pre = -42, identity": (-42, ["vf.oct.defect:A:identity", "vf.oct.pair:A:identity+e>=r"]),
    "VfIngestBody: pre = -40, e >= r": (-40, ["vf.oct.e:alias", "vf.oct.e:m", "vf.oct.pair:e>=r+count"]),
    "VfIngestBody: pre = -42, e = 0": (-42, ["vf.oct.e:zero", "vf.oct.pair:e=0+message"]),
    "VfIngestBody: status0 = -23, msg_dst_too_long": (-23, ["dst.vf.wire:valid", "dst.wire.vf.oct.defect:count"]),
    "VfIngestBody: status0 = -1": (-1, ["vf.oct.defect:count", "vf.rec.defect:length", "vf.rec.pair:length+coordinate", "dst.vf.rec.defect:length"]),
    "VfIngestBody: status0 = -23, dst_too_long": (-23, ["dst.vf.rec:valid", "dst.vf.oct:valid", "dst.vf.rec.defect:e"]),
    "VfIngestBody: ok &= coordinate": (-40, ["vf.rec.Ax:alias", "vf.rec.Ay:alias", "vf.rec.pair:coordinate+off curve"]),
    "VfIngestBody: ok &= e": (-40, ["vf.rec.e:alias", "vf.rec.pair:e+off curve"]),
    "VfIngestBody: ok &= message, status0 = -40": (-40, ["vf.rec.msg_first:alias", "vf.rec.msg_middle:alias", "vf.rec.msg_last:alias", "sg.msg_last:alias"]),
    "PgIngestBody: pre = c, -40": (-40, ["pg.wire.vf.oct.defect:A:-40", "pg.wire.vf.oct.x:alias"]),
    "PgIngestBody: pre = c, -41": (-41, ["pg.wire.vf.oct.defect:A:-41"]),
    "PgIngestBody: pre = -42, identity": (-42, ["pg.wire.vf.oct.defect:A:identity"]),
    "PgIngestBody: pre = -40, e >= r": (-40, ["pg.wire.vf.oct.e:alias", "pg.wire.vf.oct.pair:e>=r+count"]),
    "PgIngestBody: pre = -42, e = 0": (-42, ["pg.wire.vf.oct.e:zero"]),
    "PgIngestBody: return -23, msg_dst_too_long": (-23, ["dst.pg.wire.vf.oct:valid", "dst.pg.wire.vf.oct.defect:count"]),
    "PgIngestBody: return -2": (-2, ["pg.rec.defect:too many indexes", "pg.rec.pair:too many indexes+e"]),
    "PgIngestBody: return -3": (-3, ["pg.rec.defect:index", "pg.rec.pair:index+length", "pg.rec.pair:index+coordinate"]),
    "PgIngestBody: return -1": (-1, ["pg.rec.defect:length", "pg.rec.pair:length+random scalar", "pg.wire.vf.oct.defect:count"]),
    "PgIngestBody: return -4": (-4, ["pg.rec.defect:duplicate", "pg.rec.pair:duplicate+e", "dst.pg.rec.defect:duplicate"]),
    "PgIngestBody: return -23, dst_too_long": (-23, ["dst.pg.rec:valid", "dst.pg.rec.defect:e", "dst.pg.rec.defect:off curve"]),
    "PgIngestBody: ok &= coordinate": (-40, ["pg.rec.Ax:alias", "pg.rec.Ay:alias", "pg.rec.pair:coordinate+off curve"]),
    "PgIngestBody: ok &= e": (-40, ["pg.rec.e:alias", "pg.rec.pair:e+off curve"]),
    "PgIngestBody: ok &= r1, r2, e~, r1~, r3~": (-40, ["pg.rec.rnd_first:alias", "pg.rec.rnd_middle:alias"]),
    "PgIngestBody: ok &= message": (-40, ["pg.rec.msgs_first:alias", "pg.rec.msgs_middle:alias", "pg.rec.msgs_last:alias"]),
    "PgIngestBody: ok &= m~, status0 = -40": (-40, ["pg.rec.rnd_last:alias", "pg.rec.rnd_last:m"]),
    "KeyBuild decoder: noncanon, no compression flag (BLS12-381)": (-40, ["key.oct:no flag"]),
    "KeyBuild decoder: noncanon, identity with a value bit or the sign flag": (-40, ["key.oct:stray_lo", "key.oct:stray_mid", "key.oct:stray_hi", "key.oct:inf+sign"]),
    "KeyBuild decoder: noncanon, a half of x >= p": (-40, ["key.oct.half0:alias", "key.oct.half0:m", "key.oct.half1:alias", "key.oct.half1:m"]),
    "KeyBuild decoder: refused, no root": (-41, ["key.oct:no root"]),
    "KeyBuild decoder: lt &= record coordinate": (-41, ["key.rec.coord%d:%s" % (k, v) for k in range(4) for v in ("m", "alias")]),
    "KeyBuild: refused, not on the twist": (-41, ["key.rec.coord2:m-1", "key.rec.coord0:zero"]),
    "KeyBuild: refused, [r]Q is not the identity": (-41, ["key.oct:off subgroup"]),
}


def all_labels(curve):
    """{label: the model's status} of every cell of every table of the curve."""
    w = world(curve)
    cells = pv_record_cells(w) + vf_record_cells(w) + pg_record_cells(w) + sign_cells(w) + pv_octet_cells(w) + vf_octet_cells(w) + \
        pv_flag_cells(w) + vf_flag_cells(w) + pv_precedence_cells(w) + vf_precedence_cells(w) + pv_record_precedence_cells(w) + \
        pg_record_precedence_cells(w) + vf_record_precedence_cells(w) + sign_precedence_cells(w)
    cells = cells + pg_wire_cells(w.s, vf_octet_cells(w) + vf_flag_cells(w) + vf_precedence_cells(w))
    if wr.is_bls(w.c):
        pv, vf = subgroup_cells(w)
        cells += pv + vf
    for t in dst_cells(w)[0].values():
        cells = cells + t
    labels = {lab: want for lab, _, want in cells}
    assert len(labels) == len(cells), "two cells share a label"
    labels.update({lab: code for lab, _, code in g1_point_cells(w)})
    labels.update({lab: want for lab, _, want, _ in key_octet_cells(curve)})
    labels.update({lab: want for lab, _, want in key_record_cells(curve)})
    return labels


# ---- keys -------------------------------------------------------------------------------------------------------------------
_g2_memo = {}


def key_want(c, octets):
    k = (c.name, bytes(octets))
    if k not in _g2_memo:
        _g2_memo[k] = wr.public_key_from_octets(c, octets)
    return _g2_memo[k]


def key_octet_cells(curve):
    """[(label, octets, status, key)]: both halves of x through the field table (the half next to the flags has three or two
    bits fewer), the flag combinations on a valid key and on the identity with stray bits."""
    w = world(curve)
    c = w.c
    n = c.fp_bytes
    pk = w.s.pk
    big = wr.g2_from_octets(c, bbs.g2_compress(c, pk))
    assert big == (0, pk)
    sign = (pk[1][1] if pk[1][1] else pk[1][0]) > (c.p - 1) // 2
    (x0, x1) = pk[0]
    cells = []
    # half 0 = the half next to the flags (x.c1 on both curves), half 1 = x.c0.  Half 0 has an alias only when x.c1 is small:
    # the keys of sk = 2, 3, .. are searched (at most 64) for one
    small = None
    for sk in range(2, 66):
        q = bbs.sk_to_pk(w.s.suite, sk)
        if q[0][1] < w.lim:
            small = q
            break
    assert small is not None, "no key among 64 has an aliasable x.c1"
    ssign = (small[1][1] if small[1][1] else small[1][0]) > (c.p - 1) // 2
    for name, val in field_values(c.p, small[0][1], wr.value_bits(c)):
        cells.append(("key.oct.half0:%s" % name, enc_x(c, (val << (8 * n)) | small[0][0], ssign, n_coord=2)))
    for name, val in field_values(c.p, x0, 8 * n):
        cells.append(("key.oct.half1:%s" % name, enc_x(c, (x1 << (8 * n)) | val, sign, n_coord=2)))
    cells.append(("key.oct:valid", bbs.g2_compress(c, pk)))
    cells.append(("key.oct:other root", enc_x(c, (x1 << (8 * n)) | x0, not sign, n_coord=2)))
    cells.append(("key.oct:identity", enc_x(c, 0, inf=True, n_coord=2)))
    cells.append(("key.oct:inf+sign", enc_x(c, 0, True, True, n_coord=2)))
    cells.append(("key.oct:stray_lo", enc_x(c, 1, inf=True, n_coord=2)))
    cells.append(("key.oct:stray_mid", enc_x(c, 1 << (8 * n), inf=True, n_coord=2)))
    cells.append(("key.oct:stray_hi", enc_x(c, 1 << (wr.value_bits(c) + 8 * n - 1), inf=True, n_coord=2)))
    if wr.is_bls(c):
        cells.append(("key.oct:no flag", enc_x(c, (x1 << (8 * n)) | x0, sign, comp=False, n_coord=2)))
    cells.append(("key.oct:off subgroup", bbs.g2_compress(c, kr.off_subgroup_point(curve))))
    rx = kr.rootless_x(curve)
    cells.append(("key.oct:no root", enc_x(c, (rx[1] << (8 * n)) | rx[0], n_coord=2)))
    out = []
    for lab, o in cells:
        st, q = key_want(c, o)
        if ":alias" in lab:
            assert st == wr.NONCANONICAL, lab
        out.append((lab, o, st, q))
    assert {lab: st for lab, _, st, _ in out}["key.oct:other root"] == 1
    return out


def key_record_cells(curve):
    """[(label, record of four integers, status)]: every coordinate of the record through the field table."""
    w = world(curve)
    c = w.c
    pk = w.s.pk
    flat = [pk[0][0], pk[0][1], pk[1][0], pk[1][1]]
    out = [("key.rec:valid", list(flat), 1)]
    for k in range(4):
        for name, val in field_values(c.p, flat[k], 8 * c.fp_bytes):
            rec = list(flat)
            rec[k] = val
            want = wr.g2_record_status(c, rec)
            if name == "alias":
                assert want == wr.NOT_ON_CURVE
            out.append(("key.rec.coord%d:%s" % (k, name), rec, want))
    assert wr.g2_record_status(c, flat) == 1
    return out


# ---- running the tables through the library ---------------------------------------------------------------------------------
def engine(w, lib_path):
    return pc.make_engine(w.curve, w.s.gens, w.s.api_id, lib_path, sk=w.s.sk)


def _chunks(cells):
    for k in range(0, len(cells), MAX_CALL):
        yield cells[k:k + MAX_CALL]


def _compare(cells, got, where):
    bad = [(lab, int(g), want) for (lab, _, want), g in zip(cells, got) if int(g) != want]
    assert not bad, (where, bad[:12], len(bad))


def _eproof(it):
    return Proof(it["pts"][0], it["pts"][1], it["pts"][2], it["sc"][0], it["sc"][1], it["sc"][2], list(it["cms"]), it["sc"][3])


def run_pv_records(w, eng, cells, where="bbs_core_proof_verify_batch"):
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        got = eng.core_proof_verify_batch([_eproof(it) for it in its], [it["dm"] for it in its], [it["idx"] for it in its],
                                          [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, where)


def run_pv_octets(w, eng, cells, submit=False, decode=True):
    """bbs_proof_verify_octets_batch (and _submit), and bbs_proofs_from_octets_batch against the model's decoder: its status,
    the decoded proof, and a zero record for a refused item."""
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        octs = [pv_octets(w.c, it) for it in its]
        args = (octs, [it["dm"] for it in its], [it["idx"] for it in its], [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, eng.proof_verify_octets_batch(*args), "bbs_proof_verify_octets_batch")
        if submit:
            nn, keep, packed = eng._oct_inputs(*args)
            j = eng.proof_verify_octets_submit_packed(nn, packed)
            j.wait()
            _compare(ch, j.result, "bbs_proof_verify_octets_submit")
            j.free()
        if decode:
            check_proofs_from_octets(w, eng, octs)


def check_proofs_from_octets(w, eng, octs):
    n = len(octs)
    flat = np.frombuffer(b"".join(octs) + b"\0", dtype=np.uint8).copy()
    off = np.zeros(n + 1, dtype=np.uint64)
    for i, o in enumerate(octs):
        off[i + 1] = off[i] + len(o)
    rec = 6 * eng.fpb + 128
    pf = np.full(n * rec, 0xEE, dtype=np.uint8)
    cm = np.zeros(max(sum(len(o) for o in octs) // 32, 1) * 32, dtype=np.uint8)
    cmo = np.zeros(n + 1, dtype=np.uint64)
    st = np.full(n, -128, dtype=np.int8)
    rc = eng.lib.bbs_proofs_from_octets_batch(eng.h, n, flat.ctypes.data_as(_lib.c_u8p), off.ctypes.data_as(_lib.c_u64p), pf.ctypes.data_as(_lib.c_u8p),
                                              cm.ctypes.data_as(_lib.c_u8p), cmo.ctypes.data_as(_lib.c_u64p), st.ctypes.data_as(_lib.c_i8p))
    assert rc == 0, rc
    proofs = eng._dec_proofs(pf, cm, cmo, st, n)
    raw = pf.tobytes()
    for i, o in enumerate(octs):
        want, p = wr.proof_from_octets(w.c, o)
        assert int(st[i]) == want, ("bbs_proofs_from_octets_batch", i, int(st[i]), want)
        if want == 1:
            g = proofs[i]
            assert (g.a_bar, g.b_bar, g.d, g.e_cap, g.r1_cap, g.r3_cap, list(g.commitments), g.challenge) == \
                   (p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge), i
        else:
            assert raw[i * rec:(i + 1) * rec] == bytes(rec), ("a refused item's record is not zero", i)


def run_pv_wire(w, eng, cells):
    """bbs_proof_verify_wire_batch: the same proofs with the disclosed messages as raw bytes (cells whose defect is a
    disclosed message's VALUE do not exist in this form and are left out)."""
    keep = [(lab, it, wr.proof_verify_wire_status(w.s, pv_octets(w.c, it), it["dm_raw"], it["idx"], it["hdr"], it["ph"]))
            for lab, it, _ in cells if ".dm_" not in lab and "disclosed message" not in lab]
    for ch in _chunks(keep):
        its = [it for _, it, _ in ch]
        got = eng.proof_verify_wire_batch([pv_octets(w.c, it) for it in its], [it["dm_raw"] for it in its], [it["idx"] for it in its],
                                          [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, "bbs_proof_verify_wire_batch")


def run_vf_records(w, eng, cells):
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        got = eng.core_verify_batch([Signature(it["a"], it["e"]) for it in its], [it["msgs"] for it in its], [it["hdr"] for it in its])
        _compare(ch, got, "bbs_core_verify_batch")


def run_vf_octets(w, eng, cells, wire=True):
    """bbs_verify_octets_batch, bbs_signatures_from_octets_batch (status, record, zeros when refused), bbs_verify_wire_batch and
    bbs_proof_gen_wire_batch (signature octets in) on the cells whose messages exist as raw bytes."""
    c = w.c
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        octs = [vf_octets(c, it) for it in its]
        _compare(ch, eng.verify_octets_batch(octs, [it["msgs"] for it in its], [it["hdr"] for it in its]), "bbs_verify_octets_batch")
        fixed = [(lab, it, o) for (lab, it, _), o in zip(ch, octs) if len(o) == c.fp_bytes + 32]
        n = len(fixed)
        buf = np.frombuffer(b"".join(o for _, _, o in fixed) + b"\0", dtype=np.uint8).copy()
        rec = 2 * eng.fpb + 32
        out = np.full(n * rec, 0xEE, dtype=np.uint8)
        st = np.full(n, -128, dtype=np.int8)
        assert eng.lib.bbs_signatures_from_octets_batch(eng.h, n, buf.ctypes.data_as(_lib.c_u8p), out.ctypes.data_as(_lib.c_u8p), st.ctypes.data_as(_lib.c_i8p)) == 0
        raw = out.tobytes()
        for i, (lab, it, o) in enumerate(fixed):
            want, sig = wr.signature_from_octets(c, o)
            assert int(st[i]) == want, ("bbs_signatures_from_octets_batch", lab, int(st[i]), want)
            r = raw[i * rec:(i + 1) * rec]
            if want == 1:
                assert (eng._g1_dec(r), int.from_bytes(r[2 * eng.fpb:], "little")) == (sig.a, sig.e), lab
            else:
                assert r == bytes(rec), ("a refused signature's record is not zero", lab)
        if wire:
            rawc = [(lab, it, wr.verify_wire_status(w.s, vf_octets(c, it), it["raw"], it["hdr"])) for lab, it, _ in ch if ":message" not in lab
                    and "+message" not in lab]
            ri = [it for _, it, _ in rawc]
            _compare(rawc, eng.verify_wire_batch([vf_octets(c, it) for it in ri], [it["raw"] for it in ri], [it["hdr"] for it in ri]), "bbs_verify_wire_batch")
            run_pg_wire(w, eng, pg_wire_cells(w.s, ch))


def run_pg_wire(w, eng, cells):
    """bbs_proof_gen_wire_batch on cells of pg_wire_cells."""
    its = [it for _, it, _ in cells]
    _, got = eng.proof_gen_wire_batch([vf_octets(w.c, it) for it in its], [it["raw"] for it in its], [it["idx"] for it in its],
                                      [it["rnd"] for it in its], [it["hdr"] for it in its], [w.ph] * len(its))
    _compare(cells, got, "bbs_proof_gen_wire_batch")


def run_pg_records(w, eng, cells):
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        _, got = eng.core_proof_gen_batch([Signature(it["a"], it["e"]) for it in its], [it["msgs"] for it in its], [it["idx"] for it in its],
                                          [it["rnd"] for it in its], [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, "bbs_core_proof_gen_batch")


def run_sign(w, eng, cells):
    _, got = eng.core_sign_batch([it["msgs"] for _, it, _ in cells], [w.hdr] * len(cells))
    _compare(cells, got, "bbs_core_sign_batch")


def check_records(curve, lib_path):
    w = world(curve)
    eng = engine(w, lib_path)
    run_pv_records(w, eng, pv_record_cells(w))
    run_vf_records(w, eng, vf_record_cells(w))
    run_pg_records(w, eng, pg_record_cells(w))
    run_sign(w, eng, sign_cells(w))
    eng.close()


def check_records_mixed(curve, lib_path):
    """The record matrix once through the mixed-length ingests (PvIngestMixed, VfIngestMixed, PgIngestMixed): the same bodies
    through their template parameter; the items have L messages, so the model's statuses hold unchanged."""
    w = world(curve)
    eng = engine(w, lib_path)
    eng.set_mixed_lengths(True)
    eng.set_mixed_lengths_gen(True)
    run_pv_records(w, eng, pv_record_cells(w))
    run_vf_records(w, eng, vf_record_cells(w))
    run_pg_records(w, eng, pg_record_cells(w))
    run_pv_octets(w, eng, pv_octet_cells(w), decode=False)
    run_vf_octets(w, eng, vf_octet_cells(w))          # the signature-octet branch of VfIngestMixed and PgIngestMixed
    eng.close()


def check_records_keyed(curve, lib_path):
    """The scalar and coordinate matrix once through the keyed entries (the same ingest bodies behind a key index): two keys
    registered, every item names the second, which is the world's."""
    w = world(curve)
    eng = engine(w, lib_path)
    other = bbs.sk_to_pk(w.s.suite, 77)
    assert list(eng.set_public_keys([other, w.s.pk])) == [1, 1]
    for ch in _chunks(pv_record_cells(w)):
        its = [it for _, it, _ in ch]
        got = eng.core_proof_verify_keyed_batch([1] * len(its), [_eproof(it) for it in its], [it["dm"] for it in its], [it["idx"] for it in its],
                                                [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, "bbs_core_proof_verify_keyed_batch")
    for ch in _chunks(vf_record_cells(w)):
        its = [it for _, it, _ in ch]
        got = eng.core_verify_keyed_batch([1] * len(its), [Signature(it["a"], it["e"]) for it in its], [it["msgs"] for it in its], [it["hdr"] for it in its])
        _compare(ch, got, "bbs_core_verify_keyed_batch")
    for ch in _chunks(pg_record_cells(w)):
        its = [it for _, it, _ in ch]
        _, got = eng.core_proof_gen_keyed_batch([1] * len(its), [Signature(it["a"], it["e"]) for it in its], [it["msgs"] for it in its],
                                                [it["idx"] for it in its], [it["rnd"] for it in its], [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, "bbs_core_proof_gen_keyed_batch")
    cells = [(lab, it, wr.proof_verify_wire_status(w.s, pv_octets(w.c, it), it["dm_raw"], it["idx"], it["hdr"], it["ph"]))
             for lab, it, _ in pv_octet_cells(w) if ".dm_" not in lab]
    for ch in _chunks(cells):
        its = [it for _, it, _ in ch]
        got = eng.proof_verify_wire_keyed_batch([1] * len(its), [pv_octets(w.c, it) for it in its], [it["dm_raw"] for it in its],
                                                [it["idx"] for it in its], [it["hdr"] for it in its], [it["ph"] for it in its])
        _compare(ch, got, "bbs_proof_verify_wire_keyed_batch")
    cells = [(lab, it, wr.verify_wire_status(w.s, vf_octets(w.c, it), it["raw"], it["hdr"])) for lab, it, _ in vf_octet_cells(w)]
    its = [it for _, it, _ in cells]
    got = eng.verify_wire_keyed_batch([1] * len(its), [vf_octets(w.c, it) for it in its], [it["raw"] for it in its], [it["hdr"] for it in its])
    _compare(cells, got, "bbs_verify_wire_keyed_batch")
    eng.close()


def check_octets(curve, lib_path):
    w = world(curve)
    eng = engine(w, lib_path)
    cells = pv_octet_cells(w)
    run_pv_octets(w, eng, cells, submit=True)
    run_pv_wire(w, eng, cells)
    run_vf_octets(w, eng, vf_octet_cells(w))
    eng.close()


def check_flags(curve, lib_path):
    w = world(curve)
    eng = engine(w, lib_path)
    run_pv_octets(w, eng, pv_flag_cells(w))
    run_vf_octets(w, eng, vf_flag_cells(w))
    # the same strings through the decode primitive: code and point by the model
    check_decompress(w, eng, [s for _, s, _ in g1_point_cells(w)])
    eng.close()


def check_decompress(w, eng, encs):
    n = len(encs)
    buf = np.frombuffer(b"".join(encs) + b"\0", dtype=np.uint8).copy()
    out = np.full(n * 2 * eng.fpb, 0xEE, dtype=np.uint8)
    code = np.full(n, -128, dtype=np.int8)
    assert eng.lib.bbs_g1_decompress_batch(eng.h, n, buf.ctypes.data_as(_lib.c_u8p), out.ctypes.data_as(_lib.c_u8p), code.ctypes.data_as(_lib.c_i8p)) == 0
    raw = out.tobytes()
    for i, s in enumerate(encs):
        want, pt = wr.g1_from_octets(w.c, s)
        assert int(code[i]) == want, ("bbs_g1_decompress_batch", i, s.hex(), int(code[i]), want)
        r = raw[i * 2 * eng.fpb:(i + 1) * 2 * eng.fpb]
        if want == 0:
            assert eng._g1_dec(r) == pt, (i, s.hex())
        else:
            assert r == bytes(2 * eng.fpb), ("a refused point's record is not zero", i)


def check_subgroup(lib_path):
    w = world("bls12_381")
    eng = engine(w, lib_path)
    pv, vf = subgroup_cells(w)
    run_pv_octets(w, eng, pv)
    run_vf_octets(w, eng, vf)
    check_decompress(w, eng, [enc_pt(w.c, p) for p in off_subgroup_points().values()] + [enc_pt(w.c, w.c.g1_neg(p)) for p in off_subgroup_points().values()])
    eng.close()


def check_sign_boundary(lib_path):
    """BN254: every boundary point under both values of the sign flag decodes (code 0) to exactly the root the flag asks for,
    through bbs_g1_decompress_batch and, as A, through bbs_signatures_from_octets_batch."""
    w = world("bn254")
    c = w.c
    eng = engine(w, lib_path)
    below, above = sign_boundary_points()
    encs, pts = [], []
    for (x, y) in below + above:
        for big in (False, True):
            encs.append(enc_x(c, x, big))
            pts.append((x, y if (y > (c.p - 1) // 2) == big else c.p - y))
    for s, pt in zip(encs, pts):
        assert wr.g1_from_octets(c, s) == (0, pt)
    check_decompress(w, eng, encs)
    cells = [("vf.oct.boundary:%d" % i, {"enc": s, "a": pt, "e": 5, "msgs": list(w.msgs), "raw": list(w.raw), "hdr": w.hdr}, None) for i, (s, pt) in enumerate(zip(encs, pts))]
    sigs, st = eng.signatures_from_octets_batch([vf_octets(c, it) for _, it, _ in cells])
    assert list(st) == [1] * len(cells) and [(g.a, g.e) for g in sigs] == [(pt, 5) for pt in pts]
    eng.close()


def check_precedence(curve, lib_path):
    w = world(curve)
    eng = engine(w, lib_path)
    cells = pv_precedence_cells(w)
    run_pv_octets(w, eng, cells)
    run_pv_wire(w, eng, cells)
    run_vf_octets(w, eng, vf_precedence_cells(w))
    run_pv_records(w, eng, pv_record_precedence_cells(w))
    run_vf_records(w, eng, vf_record_precedence_cells(w))
    run_pg_records(w, eng, pg_record_precedence_cells(w))
    run_sign(w, eng, sign_precedence_cells(w))
    eng.close()


def check_dst_too_long(curve, lib_path):
    """The -23 sites of every ingest body (dst_cells): one context whose api_id || "H2S_" exceeds 255 bytes, one where only the
    DST of msg_to_scalars does."""
    w = world(curve)
    t, long_, msg_ = dst_cells(w)
    eng = pc.make_engine(curve, long_.gens, long_.api_id, lib_path, sk=long_.sk)
    run_pv_octets(w, eng, t["pv.oct"], submit=True)
    run_pv_records(w, eng, t["pv.rec"])
    run_vf_records(w, eng, t["vf.rec"])
    run_vf_octets(w, eng, t["vf.oct"], wire=False)
    run_pg_records(w, eng, t["pg.rec"])
    run_sign(w, eng, t["sg"])
    eng.close()
    eng = pc.make_engine(curve, msg_.gens, msg_.api_id, lib_path, sk=msg_.sk)
    its = [it for _, it, _ in t["pv.wire"]]
    got = eng.proof_verify_wire_batch([pv_octets(w.c, it) for it in its], [it["dm_raw"] for it in its], [it["idx"] for it in its],
                                      [it["hdr"] for it in its], [it["ph"] for it in its])
    _compare(t["pv.wire"], got, "bbs_proof_verify_wire_batch")
    its = [it for _, it, _ in t["vf.wire"]]
    _compare(t["vf.wire"], eng.verify_wire_batch([vf_octets(w.c, it) for it in its], [it["raw"] for it in its], [it["hdr"] for it in its]), "bbs_verify_wire_batch")
    run_pg_wire(w, eng, t["pg.wire"])
    eng.close()


def check_geometry(curve, lib_path, runs=None):
    """The octet forms at 65 items: 195 decode lanes in four wavefronts, the last one ragged."""
    w = world(curve)
    eng = engine(w, lib_path)
    all_runs = geometry_runs(w)
    for name, items in all_runs:
        if runs is not None and name not in runs:
            continue
        cells = _finish([("geometry[%s].item%d" % (name, i), it) for i, it in enumerate(items)], w.pv_oct_want)
        want = [x[2] for x in cells]
        if name == "only 21 valid":
            assert want[21] == 1 and all(x < 0 for k, x in enumerate(want) if k != 21)
        elif name == "all defective":
            assert all(x < 0 for x in want)
        else:
            assert sum(1 for x in want if x < 0) == len(GEOMETRY_ITEMS) and want[1] == 0 and want[0] == 1
        run_pv_octets(w, eng, cells, submit=(name == "all defective"))
    eng.close()
    return [name for name, _ in all_runs]


def check_geometry_signatures(curve, lib_path):
    """verify from octets at 65 items (VfOctDecode: one lane per item): each point-level kind at items 0, 20, 63, 64."""
    w = world(curve)
    eng = engine(w, lib_path)
    kinds = point_defects(w)
    for kind, (s, _) in sorted(kinds.items()):
        items = [copy.deepcopy(w.vf if i % 2 else w.sig_alias) for i in range(GEOMETRY_N)]
        for i in (0, 20, 63, 64):
            items[i]["enc"] = s
        cells = _finish([("geometry.vf[%s].item%d" % (kind, i), it) for i, it in enumerate(items)], w.vf_oct_want)
        assert sum(1 for x in cells if x[2] < 0) == 4
        run_vf_octets(w, eng, cells, wire=False)
    eng.close()


def check_decompress_geometry(curve, lib_path):
    """bbs_g1_decompress_batch at n = 1, 63, 64, 65, 129 with a defect at lanes 0, 63, 64 and the last."""
    w = world(curve)
    eng = engine(w, lib_path)
    kinds = sorted(point_defects(w).items())
    good = [enc_pt(w.c, q) for it in w.proofs["A"][:2] + w.proofs["B"][:2] for q in it["pts"]]
    for n in (1, 63, 64, 65, 129):
        encs = [good[i % len(good)] for i in range(n)]
        for j, lane in enumerate(sorted({0, 63, 64, n - 1})):
            if lane < n:
                encs[lane] = kinds[(j + n) % len(kinds)][1][0]
        check_decompress(w, eng, encs)
    eng.close()


def check_keys(curve, lib_path):
    """The G2 key decoder: bbs_ctx_add_public_keys_octets and both paths of bbs_selftest_key_entries on the octet table,
    bbs_ctx_add_public_keys on the record table; then the octet table at n = 1, 63, 64, 65, 129 with defects at lanes 0, 63,
    64 and the last through the device stage (path 1)."""
    w = world(curve)
    eng = engine(w, lib_path)
    cells = key_octet_cells(curve)
    octs = [o for _, o, _, _ in cells]
    first, st, keys = eng.add_public_keys_octets(octs)
    bad = [(lab, int(g), want) for (lab, _, want, _), g in zip(cells, st) if int(g) != want]
    assert not bad, ("bbs_ctx_add_public_keys_octets", bad)
    for (lab, _, want, q), k in zip(cells, keys):
        assert k == (q if want == 1 else None), lab
    for path in (0, 1):
        _, st, recs = kr.key_entries(eng, path, octets=octs)
        bad = [(lab, int(g), want) for (lab, _, want, _), g in zip(cells, st) if int(g) != want]
        assert not bad, ("bbs_selftest_key_entries path %d" % path, bad)
        for (lab, _, want, q), r in zip(cells, recs):
            assert r == (kr.record(eng.fpb, q) if want == 1 else bytes(4 * eng.fpb)), (lab, path)
    rcells = key_record_cells(curve)
    recs = [((r[0], r[1]), (r[2], r[3])) for _, r, _ in rcells]
    _, st = kr.add_raw(eng, recs)
    bad = [(lab, int(g), want) for (lab, _, want), g in zip(rcells, st) if int(g) != want]
    assert not bad, ("bbs_ctx_add_public_keys", bad)
    for path in (0, 1):
        _, st, _ = kr.key_entries(eng, path, keys=recs)
        bad = [(lab, int(g), want) for (lab, _, want), g in zip(rcells, st) if int(g) != want]
        assert not bad, ("bbs_selftest_key_entries (records) path %d" % path, bad)
    good = bbs.g2_compress(w.c, w.s.pk)
    defects = [o for lab, o, want, _ in cells if want < 0]
    for n in (1, 63, 64, 65, 129):
        octs = [good] * n
        for j, lane in enumerate(sorted({0, 63, 64, n - 1})):
            if lane < n:
                octs[lane] = defects[(j + n) % len(defects)]
        _, st, _ = kr.key_entries(eng, 1, octets=octs)
        want = [key_want(w.c, o)[0] for o in octs]
        assert [int(x) for x in st] == want, (n, [int(x) for x in st], want)
    eng.close()


def check_host_codec(curve, lib):
    """The product library's host decoders, no GPU: bbs_signature_from_octets, bbs_proof_from_octets,
    bbs_public_key_from_octets on every octet table, against the model."""
    from bbs_sign_amd import BbsError, api
    w = world(curve)
    c = w.c
    pv = pv_octet_cells(w) + pv_flag_cells(w) + pv_precedence_cells(w)
    vf = vf_octet_cells(w) + vf_flag_cells(w) + vf_precedence_cells(w)
    if wr.is_bls(c):
        a, b = subgroup_cells(w)
        pv, vf = pv + a, vf + b
    for lab, it, _ in pv:
        o = pv_octets(c, it)
        want, p = wr.proof_from_octets(c, o)
        try:
            g = api.octets_to_proof(curve, o, lib)
            got = 1
        except BbsError as e:
            got = e.status
        assert got == want, ("bbs_proof_from_octets", lab, got, want)
        if want == 1:
            assert (g.a_bar, g.b_bar, g.d, g.e_cap, g.r1_cap, g.r3_cap, g.commitments, g.challenge) == \
                   (p.a_bar, p.b_bar, p.d, p.e_cap, p.r1_cap, p.r3_cap, list(p.commitments), p.challenge), lab
    for lab, it, _ in vf:
        o = vf_octets(c, it)
        want, s = wr.signature_from_octets(c, o)
        try:
            g = api.octets_to_signature(curve, o, lib)
            got = 1
        except BbsError as e:
            got = e.status
        assert got == want, ("bbs_signature_from_octets", lab, got, want)
        if want == 1:
            assert (g.a, g.e) == (s.a, s.e), lab
    if not wr.is_bls(c):
        below, above = sign_boundary_points()
        for (x, y) in below + above:
            for big in (False, True):
                g = api.octets_to_signature(curve, enc_x(c, x, big) + be32(7), lib)
                assert g.a == (x, y if (y > (c.p - 1) // 2) == big else c.p - y)
    for lab, o, want, q in key_octet_cells(curve):
        try:
            g = api.octets_to_public_key(curve, o, lib).pk
            got = 1
        except BbsError as e:
            got, g = e.status, None
        assert got == want and g == q, ("bbs_public_key_from_octets", lab, got, want)


def check_primitives(curve, lib_path):
    """bbs_g1_msm_batch, bbs_pairing_product2_is_one_batch and bbs_sk_to_pk_batch: the field table on every scalar and
    coordinate they take."""
    w = world(curve)
    c = w.c
    eng = engine(w, lib_path)
    pt = w.vf["a"]
    rows = []
    for name, val in field_values(c.r, 5, 256):
        rows.append(("msm.fixed:%s" % name, [val, 1], [pt], [3]))
        rows.append(("msm.var_scalar:%s" % name, [2, 1], [pt], [val]))
    for k in range(2):
        for name, val in field_values(c.p, pt[k], 8 * c.fp_bytes):
            rows.append(("msm.coord%d:%s" % (k, name), [2, 1], [(val, pt[1]) if k == 0 else (pt[0], val)], [3]))
    _, st = eng.g1_msm_batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    _compare([(r[0], None, wr.g1_msm_status(c, r[1], r[2], r[3])) for r in rows], st, "bbs_g1_msm_batch")
    # e(A, pk) e(B, BP2) == 1 with B = -(sk A): true for the untouched pair
    pb = c.g1_neg(c.g1_mul(pt, w.s.sk))
    pairs = [("pair:valid", pt, pb)]
    for k in range(4):
        src = (pt, pt, pb, pb)[k]
        for name, val in field_values(c.p, src[k % 2], 8 * c.fp_bytes):
            q = (val, src[1]) if k % 2 == 0 else (src[0], val)
            pairs.append(("pair.coord%d:%s" % (k, name), q if k < 2 else pt, pb if k < 2 else q))
    st = eng.pairing_product2_is_one_batch([r[1] for r in pairs], [r[2] for r in pairs])
    cells = [(r[0], None, wr.pairing_product2_status(w.s, r[1], r[2])) for r in pairs]
    assert cells[0][2] == 1
    _compare(cells, st, "bbs_pairing_product2_is_one_batch")
    sks = field_values(c.r, w.s.sk, 256)
    pks, _, st = eng.sk_to_pk_batch([v for _, v in sks])
    _compare([("sk:%s" % n_, None, wr.sk_to_pk_status(c, v)) for n_, v in sks], st, "bbs_sk_to_pk_batch")
    for (n_, v), pk in zip(sks, pks):
        if 0 < v < c.r and n_ in ("m-1",):
            assert pk == c.g2_neg(c.g2), n_
    eng.close()
