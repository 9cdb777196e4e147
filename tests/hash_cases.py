"""Caller-controlled bytes at every SHA-256 alignment: header, presentation header, raw messages and api_id.

Every result of the library starts from a SHA-256 stream whose path through bbs_sign_amd/csrc/sha256.hpp (byte prologue,
whole blocks straight from memory, whole words, byte tail; aligned or unaligned loads; the three padding classes of
sha256_final) is decided by byte lengths and pointer residues that only the caller chooses.  Sign and verify share that
code, so a round trip cannot see a mistake in it: only bit-identity with an independent hash can.  The expected values
here are plain hashlib (oracle/hashing.py, oracle/bbs.py); group arithmetic is compared for samples only.

Three parts:
  * a pure-Python MODEL of the control flow of sha256_bytes / sha256_word / sha256_final / xmd48_finish (no hashing): it
    names the branches ("labels") a stream visits.  tests/test_hash_hosttwin.py asserts on the CPU that the case lists
    below visit every label the model can produce at each site, and that every (length, pointer residue) pair a builder
    promises is really present in what it built;
  * BUILDERS of the case lists.  The items of a batch lie back to back in a 16-aligned section of the staging image
    (runtime.hpp RaggedIn::place), so an item's pointer residue is its cumulative offset mod 4; the builders put 1-3 byte
    filler items in front of an item to steer it.  Fillers are items like any other and are checked like any other;
  * CHECKERS that take lib_path like parity_cases.py: the same bodies run on the host twin (the cover set: the smallest
    lists with full label cover) and on the GPU (the full sweeps).

Sites: S1 the domain (dom_tail || hdr_len || header, resumed from the midstate), S2 the challenge (.. || ph_len || ph),
S3 raw messages of the wire forms, S4 hash_to_scalar_batch.
"""
import functools
import hashlib

import parity_cases as pc
from bbs_sign_amd import Signature
from oracle import bbs, c_port
from oracle.hashing import hash_to_scalar, i2osp

FPB = {"bls12_381": 48, "bn254": 32}
CURVES = ("bls12_381", "bn254")
SK = 0x1F2E3D4C5B6A79881726354453627180A9B8C7D6E5F40312
MAP_SUFFIX = b"MAP_MSG_TO_SCALAR_AS_HASH_"
DST_TOO_LONG = -23

# api_id lengths of S1: 0..63 give every dom_tail_len; the sparse rest puts dst_len = len + 4 on every padding boundary of
# b1 / b2 (34 + dst_len bytes: 55 | 56 fits / one more block, 63 the 0x80 byte completes the block, 64 fits again) once
# more in the second, third and fourth block of the DST, and ends at the longest DST there is (255)
API_LENS = tuple(range(64)) + (81, 82, 83, 89, 90, 153, 217, 251)
# header / ph / message lengths: every length up to two blocks and a word, and the lengths around 256
SWEEP_LENS = tuple(range(137)) + (255, 256, 257, 300)
MSG_LENS = tuple(range(137)) + (255, 256, 257)


# ================================================================================================
# the path model
# ================================================================================================
def _m_byte(fill):
    fill += 1
    return (0, True) if fill == 64 else (fill, False)


def _m_word(fill, tag, out):
    """sha256_word: the fast branch on a word boundary, four sha256_byte calls otherwise."""
    if fill & 3 == 0:
        out.add(tag + ":word=fast")
        fill += 4
        if fill == 64:
            out.add(tag + ":word-completes-block")
            fill = 0
        return fill
    out.add(tag + ":word=bytes@%d" % (fill & 3))
    for _ in range(4):
        fill, done = _m_byte(fill)
        if done:
            out.add(tag + ":byte-completes-block")
    return fill


def _m_bytes(fill, n, res, tag, out):
    """sha256_bytes over n bytes whose pointer has residue res mod 4."""
    i = 0
    while i < n and fill & 3:
        fill, done = _m_byte(fill)
        i += 1
        if done:
            out.add(tag + ":byte-completes-block")
    out.add(tag + ":prologue=%d" % i)
    if fill & 3:
        out.add(tag + ":ends-in-prologue")              # the input ran out before the stream was word aligned
    while fill == 0 and n - i >= 64:
        out.add(tag + ":direct=" + ("aligned" if (res + i) & 3 == 0 else "unaligned"))
        i += 64
    k = (n - i) // 4
    if k:
        out.add(tag + ":words=" + ("aligned" if (res + i) & 3 == 0 else "unaligned"))
        if fill + 4 * k >= 64:
            out.add(tag + ":word-completes-block")
        fill = (fill + 4 * k) & 63
        i += 4 * k
    out.add(tag + ":tail=%d" % (n - i))
    return fill + (n - i)                               # fill & 3 == 0 here unless the input ended in the prologue: < 64


def _m_final(fill, tag, out):
    """sha256_final: the class of the padding."""
    if fill == 63:
        out.add(tag + ":final=pad-byte-completes-block")
    elif fill >= 56:
        out.add(tag + ":final=one-more-block")
    else:
        out.add(tag + ":final=fits")
    if fill in (55, 56):
        out.add(tag + ":final-edge=%d" % fill)          # the last fill that fits, the first that does not


def _m_dst_prime(fill, dst_len, res, tag, out):
    fill = _m_bytes(fill, dst_len, res, tag + ":dst", out)
    fill, done = _m_byte(fill)
    if done:
        out.add(tag + ":len-byte-completes-block")
    return fill


def _m_xmd(fill, dst_len, res, tag, out):
    """xmd48_finish: l_i_b_str, DST_prime and the final of b0; b1 and b2 hold 32 + 1 + dst_len + 1 bytes."""
    for _ in range(3):
        fill, done = _m_byte(fill)
        if done:
            out.add(tag + ":b0:lib-byte-completes-block")
    _m_final(_m_dst_prime(fill, dst_len, res, tag + ":b0", out), tag + ":b0", out)
    for b in ("b1", "b2"):
        _m_final(_m_dst_prime(33, dst_len, res, tag + ":" + b, out), tag + ":" + b, out)
    return 0


def model(events, fill=0):
    """events: (kind, length, pointer_residue) in stream order, kind = "bytes" | "word" | "byte" | "final" | "xmd", optionally
    "kind:tag" (the tag prefixes the labels).  "word": length / 4 calls of sha256_word (a length field is ("word", 8, 0));
    "xmd": xmd48_finish with a DST of `length` bytes at residue `pointer_residue`.  Returns the set of labels visited."""
    out = set()
    for kind, n, res in events:
        kind, _, tag = kind.partition(":")
        tag = tag or kind
        if kind == "bytes":
            fill = _m_bytes(fill, n, res, tag, out)
        elif kind == "word":
            for _ in range(n // 4):
                fill = _m_word(fill, tag, out)
        elif kind == "byte":
            for _ in range(n):
                fill, done = _m_byte(fill)
                if done:
                    out.add(tag + ":byte-completes-block")
        elif kind == "final":
            _m_final(fill, tag, out)
            fill = 0
        elif kind == "xmd":
            fill = _m_xmd(fill, n, res, tag, out)
        else:
            raise ValueError(kind)
    return out


# ---- the sites ---------------------------------------------------------------------------------
# A site's stream is: [constant part, known fill] || length field || caller bytes || xmd48_finish.  The labels of the first
# three depend on (fill, length, residue) only and those of the finish on (fill before it, dst_len) only, so both are cached.
@functools.lru_cache(maxsize=None)
def _front(fill, n, res, name):
    out = set()
    f = fill
    if name != "msg":
        # the length field; what its bytes are decides whether a branch that orders or drops them wrongly can show
        value = "zero" if n == 0 else ("one-byte" if n < 256 else "two-bytes")
        out.add(name + ":len:value=%s@%d" % (value, f & 3))
        f = _m_word(_m_word(f, name + ":len", out), name + ":len", out)
    f = _m_bytes(f, n, res, name, out)
    return frozenset(out), f


@functools.lru_cache(maxsize=None)
def _finish(fill, dst_len, name):
    out = set()
    _m_xmd(fill, dst_len, 0, name, out)
    return frozenset(out)


def dom_tail_len(curve, L, api_len):
    F = FPB[curve]
    return (2 * F + 8 + F * (L + 1) + api_len) % 64


def s1_labels(curve, api_len, hdr_len, res, L=1):
    """domain_from_header, then e = hash_to_scalar(sk || msgs || domain) of sign."""
    t = dom_tail_len(curve, L, api_len)
    out = set()
    f = _m_bytes(0, t, 0, "tail", out)
    front, f = _front(f, hdr_len, res, "hdr")
    return (frozenset(out) | front | _finish(f, api_len + 4, "dom") | frozenset(["hdr:fill&3=%d" % (t & 3)])
            | _finish(32 * (L + 2) % 64, api_len + 4, "e"))


def ph_fill(curve, R):
    return (8 + 40 * R + 5 * FPB[curve] + 32) % 64


def s2_labels(curve, R, ph_len, res, api_len):
    front, f = _front(ph_fill(curve, R), ph_len, res, "ph")
    return front | _finish(f, api_len + 4, "chal") | frozenset(["ph:fill=%d" % ph_fill(curve, R)])


def msg_labels(msg_len, res, dst_len):
    front, f = _front(0, msg_len, res, "msg")
    return front | _finish(f, dst_len, "h2s")


def _front_universe(fills, name, max_len=300):
    out = set()
    for fill in fills:
        for n in range(max_len + 1):
            for res in range(4):
                out |= _front(fill, n, res, name)[0]
    return out


@functools.lru_cache(maxsize=None)
def universe(site, curve):
    """Every label the model can produce at a site, over every length, residue and DST the site's callers can choose."""
    if site == "S1":
        out = _front_universe(range(64), "hdr")
        for t in range(64):
            _m_bytes(0, t, 0, "tail", out)
        out |= {"hdr:fill&3=%d" % k for k in range(4)}
        for d in range(4, 256):
            for f in range(64):
                out |= _finish(f, d, "dom")
            out |= _finish(32, d, "e")
        return frozenset(out)
    if site == "S2":
        fills = sorted({ph_fill(curve, R) for R in range(8)})
        out = _front_universe(fills, "ph")
        out |= {"ph:fill=%d" % f for f in fills}
        d = len(bbs.SUITES[curve].api_id) + 4
        for f in range(64):                              # ph of any length leaves any fill
            out |= _finish(f, d, "chal")
        return frozenset(out)
    if site == "S3":
        d = len(bbs.SUITES[curve].api_id + MAP_SUFFIX)
        out = _front_universe([0], "msg")
        for f in range(64):
            out |= _finish(f, d, "h2s")
        return frozenset(out)
    if site == "S4":
        out = _front_universe([0], "msg")
        for d in range(256):
            for f in range(64):
                out |= _finish(f, d, "h2s")
        return frozenset(out)
    raise ValueError(site)


def greedy_cover(cands, label_fn, want=None):
    """The candidates (in order of choice) of a greedy set cover of the labels all candidates produce (or of `want`)."""
    sets = {}
    for c in cands:
        sets.setdefault(label_fn(*c), c)                 # the first candidate of every distinct label set
    todo = set(want) if want is not None else set().union(*sets)
    chosen = []
    while todo:
        best = max(sets, key=lambda s: len(s & todo))
        if not best & todo:
            break
        chosen.append(sets[best])
        todo -= best
    return chosen


# ================================================================================================
# builders
# ================================================================================================
def blob(tag, n):
    """n deterministic bytes."""
    return hashlib.shake_128(tag.encode() if isinstance(tag, str) else tag).digest(n) if n else b""


def scalar(curve, tag):
    return int.from_bytes(hashlib.shake_128(("scalar-" + tag).encode()).digest(40), "big") % bbs.SUITES[curve].curve.r


def order_promises(lengths):
    """(length, residue) for every length at all four residues, ordered so that most items need no filler in front."""
    out, cur = [], 0
    for n in lengths:
        left = [0, 1, 2, 3]
        while left:
            r = cur % 4 if cur % 4 in left else left[0]
            left.remove(r)
            out.append((n, r))
            cur = r + n
    return out


def steer(promises, tag):
    """Byte strings that, laid back to back from a 4-aligned base, put promise k = (length, residue) at item where[k].
    Returns (items, where); the other items are the 1-3 byte fillers."""
    items, where, cur = [], [], 0
    for k, (n, r) in enumerate(promises):
        pad = (r - cur) % 4
        if pad:
            items.append(blob("%s-filler-%d" % (tag, k), pad))
            cur += pad
        where.append(len(items))
        items.append(blob("%s-item-%d" % (tag, k), n))
        cur += n
    return items, where


def residues(items):
    out, cur = [], 0
    for it in items:
        out.append(cur % 4)
        cur += len(it)
    return out


def assert_promises(items, where, promises):
    res = residues(items)
    assert len(where) == len(promises)
    for k, (n, r) in enumerate(promises):
        assert len(items[where[k]]) == n and res[where[k]] == r, (k, n, r, len(items[where[k]]), res[where[k]])
    for i in set(range(len(items))) - set(where):
        assert 1 <= len(items[i]) <= 3, (i, len(items[i]))        # a filler


def api_id_of(n):
    return blob("api-id-%d" % n, n)


# ---- the plans: what a checker runs, as plain data ----------------------------------------------
@functools.lru_cache(maxsize=None)
def s1_cover(curve):
    """The smallest list of (api_len, hdr_len, residue) the model needs for every S1 label."""
    cands = [(a, h, r) for a in API_LENS for h in SWEEP_LENS for r in range(4)]
    return tuple(greedy_cover(cands, lambda a, h, r: s1_labels(curve, a, h, r)))


@functools.lru_cache(maxsize=None)
def s1_plan(curve, full, every_api_len=True):
    """{api_len: promises}.  full: every header length at every residue under every api_id length.  Otherwise the cover set,
    and (every_api_len) one more header under each api_id length the cover set does not use: every dom_tail_len is run."""
    if full:
        p = tuple(order_promises(SWEEP_LENS))
        return {a: p for a in API_LENS}
    plan = {}
    for a, h, r in s1_cover(curve):
        plan.setdefault(a, []).append((h, r))
    if every_api_len:
        for a in API_LENS:
            plan.setdefault(a, [(1 + a % 7, a % 4)])
    return {a: tuple(sorted(set(v))) for a, v in sorted(plan.items())}


@functools.lru_cache(maxsize=None)
def s2_plan(curve, full):
    """{R: promises of ph}"""
    if full:
        p = tuple(order_promises(SWEEP_LENS))
        return {R: p for R in range(8)}
    a = len(bbs.SUITES[curve].api_id)
    cands = [(R, n, r) for R in range(8) for n in SWEEP_LENS for r in range(4)]
    plan = {R: [(R + 1, R % 4)] for R in range(8)}
    for R, n, r in greedy_cover(cands, lambda R, n, r: s2_labels(curve, R, n, r, a)):
        plan[R].append((n, r))
    return {R: tuple(sorted(set(v))) for R, v in plan.items()}


@functools.lru_cache(maxsize=None)
def s3_plan(curve, full):
    """promises of raw messages under the suite's api_id"""
    if full:
        return tuple(order_promises(MSG_LENS))
    d = len(bbs.SUITES[curve].api_id + MAP_SUFFIX)
    cands = [(n, r) for n in MSG_LENS for r in range(4)]
    return tuple(sorted(greedy_cover(cands, lambda n, r: msg_labels(n, r, d))))


def s4_dst_messages(d):
    """three message lengths for the DST of d bytes: together with d they move b0 through every fill"""
    return (d % 5, (61 * d + 17) % 64 + 1, 64 + (29 * d + 7) % 73)


def plan_labels(site, curve, full):
    """The labels a plan visits, by the model, INCLUDING its fillers (computed from the items the builders make)."""
    out = set()
    if site == "S1":
        for a, promises in s1_plan(curve, full).items():
            items, where = steer(promises, "s1-%s-%d" % (curve, a))
            for it, r in zip(items, residues(items)):
                out |= s1_labels(curve, a, len(it), r)
    elif site == "S2":
        a = len(bbs.SUITES[curve].api_id)
        for R, promises in s2_plan(curve, full).items():
            items, where = steer(promises, "s2-%s-%d" % (curve, R))
            for it, r in zip(items, residues(items)):
                out |= s2_labels(curve, R, len(it), r, a)
    elif site == "S3":
        d = len(bbs.SUITES[curve].api_id + MAP_SUFFIX)
        items, where = steer(s3_plan(curve, full), "s3-" + curve)
        for it, r in zip(items, residues(items)):
            out |= msg_labels(len(it), r, d)
    elif site == "S4":
        d = len(bbs.SUITES[curve].api_id + MAP_SUFFIX)
        items, where = steer(order_promises(MSG_LENS), "s4-" + curve)
        for it, r in zip(items, residues(items)):
            out |= msg_labels(len(it), r, d)
        for d in range(256):
            items = [blob("s4-dst-%d-%d" % (d, k), n) for k, n in enumerate(s4_dst_messages(d))]
            for it, r in zip(items, residues(items)):
                out |= msg_labels(len(it), r, d)
    return out


def check_model_cover(curve):
    """Every plan visits every label of its site, and holds every (length, residue) pair it promises."""
    for site in ("S1", "S2", "S3", "S4"):
        want = universe(site, curve)
        for full in (False, True):
            got = plan_labels(site, curve, full)
            assert want - got == set(), (site, curve, full, sorted(want - got))
            assert got - want == set(), (site, curve, full, sorted(got - want))
    for full in (False, True):
        for a, promises in s1_plan(curve, full).items():
            items, where = steer(promises, "s1-%s-%d" % (curve, a))
            assert_promises(items, where, promises)
        assert set(s1_plan(curve, full)) == set(API_LENS)
        for R, promises in s2_plan(curve, full).items():
            items, where = steer(promises, "s2-%s-%d" % (curve, R))
            assert_promises(items, where, promises)
        items, where = steer(s3_plan(curve, full), "s3-" + curve)
        assert_promises(items, where, s3_plan(curve, full))
    full = {(n, r) for n in SWEEP_LENS for r in range(4)}
    assert all(set(p) == full for p in s1_plan(curve, True).values()) and all(set(p) == full for p in s2_plan(curve, True).values())
    assert set(s3_plan(curve, True)) == {(n, r) for n in MSG_LENS for r in range(4)}
    assert {dom_tail_len(curve, 1, a) for a in range(64)} == set(range(64))
    assert len(s1_cover(curve)) <= 64
    # the cached per-site label functions say what model() says of the same stream of events
    for a, h, r in s1_cover(curve):
        ev = [("bytes:tail", dom_tail_len(curve, 1, a), 0), ("word:hdr:len", 8, 0), ("bytes:hdr", h, r), ("xmd:dom", a + 4, 0)]
        extra = s1_labels(curve, a, h, r) - model(ev)
        assert model(ev) <= s1_labels(curve, a, h, r) and all(x.startswith(("e:", "hdr:fill&3=", "hdr:len:value=")) for x in extra), (a, h, r, extra)
        assert {x for x in extra if x.startswith("e:")} == model([("word:e", 96, 0), ("xmd:e", a + 4, 0)], fill=0) - {"e:word=fast", "e:word-completes-block"}
    for n, r in s3_plan(curve, False):
        d = len(bbs.SUITES[curve].api_id + MAP_SUFFIX)
        assert model([("bytes:msg", n, r), ("xmd:h2s", d, 0)]) == msg_labels(n, r, d)
    # the model itself against the block arithmetic of SHA-256 for the padding classes
    for n in range(200):
        got = model([("bytes", n, 0), ("final", 0, 0)])
        blocks = (n + 9 + 63) // 64 - n // 64
        cls = "pad-byte-completes-block" if n % 64 == 63 else ("one-more-block" if blocks == 2 else "fits")
        assert "final:final=" + cls in got, (n, got)


# ================================================================================================
# expected values: hashlib only
# ================================================================================================
_pk_cache, _gen_cache = {}, {}


def public_key(curve, sk=SK):
    if (curve, sk) not in _pk_cache:
        _pk_cache[(curve, sk)] = c_port.port(curve).sk_to_pk(sk)
    return _pk_cache[(curve, sk)]


def generators(curve, count):
    if (curve, count) not in _gen_cache:
        _gen_cache[(curve, count)] = pc.gens_for(bbs.SUITES[curve], count)
    return _gen_cache[(curve, count)]


class Expect:
    """The hashing of one context (curve, L generators, api_id, key) restated with hashlib: calculate_domain
    (core_utilities.rs:24-63) from its constant prefix, and e of sign (sign.rs:90-118)."""

    def __init__(self, curve, L, api_id, sk=SK, gens=None):
        self.curve, self.L, self.api_id, self.sk = curve, L, api_id, sk
        self.suite = bbs.SUITES[curve]
        self.c = self.suite.curve
        self.gens = list(gens) if gens is not None else generators(curve, L + 1)
        assert len(self.gens) == L + 1
        self.pk = public_key(curve, sk)
        self.dst = api_id + b"H2S_"
        self.prefix = (bbs.g2_compress(self.c, self.pk) + i2osp(L, 8) + b"".join(bbs.g1_compress(self.c, g) for g in self.gens) + api_id)
        assert (64 + len(self.prefix)) % 64 == dom_tail_len(curve, L, len(api_id))
        h = blob("expect-self-check", 5)
        assert self.domain(h) == bbs.calculate_domain(self.suite, self.pk, self.gens[0], self.gens[1:], h, api_id)

    def domain(self, header):
        return hash_to_scalar(self.c, self.prefix + i2osp(len(header), 8) + header, self.dst)

    def e(self, msgs, header):
        ser = bbs.scalar_be(self.c, self.sk) + b"".join(bbs.scalar_be(self.c, m) for m in msgs) + bbs.scalar_be(self.c, self.domain(header))
        return hash_to_scalar(self.c, ser, self.dst)

    def msg_scalar(self, raw):
        return hash_to_scalar(self.c, raw, self.api_id + MAP_SUFFIX)


def sig_octets(curve, sig):
    c = bbs.SUITES[curve].curve
    return bbs.g1_compress(c, sig.a) + bbs.scalar_be(c, sig.e)


def proof_octets(curve, p):
    c = bbs.SUITES[curve].curve
    return (bbs.g1_compress(c, p.a_bar) + bbs.g1_compress(c, p.b_bar) + bbs.g1_compress(c, p.d)
            + b"".join(bbs.scalar_be(c, x) for x in [p.e_cap, p.r1_cap, p.r3_cap] + list(p.commitments) + [p.challenge]))


def header_negatives(h):
    """the header with its last byte flipped, cut by one byte, extended by a zero byte"""
    assert len(h) >= 1
    return [h[:-1] + bytes([h[-1] ^ 0x01]), h[:-1], h + b"\x00"]


def _ones(st, n, what):
    got = [int(x) for x in st]
    assert got == [1] * n, (what, [(i, s) for i, s in enumerate(got) if s != 1][:8])


def _same_proof(got, want, what):
    assert got is not None and pc.proof_eq(got, want), what


def _oracle_proof_gen(E, sig, header, ph, msgs, disclosed, rnd, python):
    s = bbs.Signature(sig.a, sig.e)
    if python:
        return bbs.core_proof_gen(E.suite, E.pk, s, header, E.gens, ph, msgs, disclosed, E.api_id, rnd)
    return c_port.port(E.curve).core_proof_gen(E.pk, s, header, E.gens, ph, msgs, disclosed, E.api_id, rnd)


# ================================================================================================
# S1: the domain
# ================================================================================================
def check_sign_domain(curve, lib_path=None, full=False, api_lens=None, every_api_len=True):
    """core_sign at L = 1 under every api_id length: e of EVERY item from hashlib, A against the oracle's core_sign for one
    item of every (fill & 3 at the header, final class of b0 and of b1 / b2) the plan meets -- the first of each residue by
    the Python oracle, the rest by its C port --, every signature through core_verify_batch in the same layout, and for
    the Python-oracle samples the three altered headers (status 0).  Returns the number of items it compared."""
    plan = s1_plan(curve, full, every_api_len)
    eng = None
    seen, python_done, count = set(), set(), 0
    for a in (api_lens if api_lens is not None else sorted(plan)):
        api_id = api_id_of(a)
        E = Expect(curve, 1, api_id)
        if eng is None:
            eng = pc.make_engine(curve, E.gens, api_id, lib_path, sk=SK)
            assert eng.public_key() == E.pk
        else:
            eng.set_generators(E.gens, api_id)
        headers, where = steer(plan[a], "s1-%s-%d" % (curve, a))
        res = residues(headers)
        n = len(headers)
        msgs = [[scalar(curve, "s1-%d-%d" % (a, i))] for i in range(n)]
        sigs, st = eng.core_sign_batch(msgs, headers)
        _ones(st, n, (curve, a, "core_sign"))
        for i in range(n):
            assert sigs[i].e == E.e(msgs[i], headers[i]), (curve, "api_id length", a, "item", i, "header length", len(headers[i]), "residue", res[i])
        vs, vm, vh, expect = list(sigs), list(msgs), list(headers), [1] * n
        t = dom_tail_len(curve, 1, a)
        for i in range(n):
            labels = s1_labels(curve, a, len(headers[i]), res[i])
            key = (t & 3,) + tuple(sorted(x for x in labels if x.startswith("dom:") and ":final=" in x))
            python = t & 3 not in python_done and len(headers[i]) >= 1
            if key in seen and not python:
                continue
            seen.add(key)
            if python:
                python_done.add(t & 3)
                want = bbs.core_sign(E.suite, SK, E.gens, headers[i], msgs[i], api_id)
                for h in header_negatives(headers[i]):
                    vs.append(Signature(want.a, want.e)); vm.append(msgs[i]); vh.append(h); expect.append(0)
            else:
                want = c_port.port(curve).core_sign(SK, E.gens, headers[i], msgs[i], api_id)
            assert (sigs[i].a, sigs[i].e) == (want.a, want.e), (curve, a, i, "A")
        st = eng.core_verify_batch(vs, vm, vh)
        assert [int(x) for x in st] == expect, (curve, a, "core_verify", [(i, int(s)) for i, s in enumerate(st) if s != expect[i]][:8])
        count += n
    if api_lens is None:
        assert python_done == {0, 1, 2, 3}, python_done
    if eng is not None:
        eng.close()
    return count


def check_proof_domain(curve, lib_path=None):
    """The S1 cover set (at most 64 items) through core_proof_gen / core_proof_verify at L = 1 against the oracle's whole
    proof: the C port, and the Python oracle for the first item of four api_id lengths."""
    plan = s1_plan(curve, False, False)
    assert sum(len(v) for v in plan.values()) <= 64
    eng, python_left = None, 4
    for a in sorted(plan):
        api_id = api_id_of(a)
        E = Expect(curve, 1, api_id)
        if eng is None:
            eng = pc.make_engine(curve, E.gens, api_id, lib_path, sk=SK)
        else:
            eng.set_generators(E.gens, api_id)
        headers, where = steer(plan[a], "s1-%s-%d" % (curve, a))
        n = len(headers)
        msgs = [[scalar(curve, "s1p-%d-%d" % (a, i))] for i in range(n)]
        phs = [blob("s1p-ph-%d-%d" % (a, i), (3 * i + a) % 9) for i in range(n)]
        disclosed = [[0] if (i + a) % 2 else [] for i in range(n)]
        rnds = [[scalar(curve, "s1p-rnd-%d-%d-%d" % (a, i, k)) or 1 for k in range(5 + 1 - len(disclosed[i]))] for i in range(n)]
        sigs, st = eng.core_sign_batch(msgs, headers)
        _ones(st, n, (curve, a, "core_sign"))
        proofs, st = eng.core_proof_gen_batch(sigs, msgs, disclosed, rnds, headers, phs)
        _ones(st, n, (curve, a, "core_proof_gen"))
        for i in range(n):
            python = python_left > 0 and i == 0
            python_left -= python
            _same_proof(proofs[i], _oracle_proof_gen(E, sigs[i], headers[i], phs[i], msgs[i], disclosed[i], rnds[i], python), (curve, a, i))
        dm = [[msgs[i][j] for j in disclosed[i]] for i in range(n)]
        _ones(eng.core_proof_verify_batch(proofs, dm, disclosed, headers, phs), n, (curve, a, "core_proof_verify"))
    assert python_left == 0
    eng.close()


# ================================================================================================
# S2: the challenge
# ================================================================================================
def check_challenge(curve, lib_path=None, full=False):
    """core_proof_gen / core_proof_verify at L = 7 with R = 0 .. 7 disclosed; within an R group only ph varies.  One
    proof_init of the Python oracle per R, then proof_challenge_calculate and proof_finalize per item: the WHOLE proof of
    every item is compared, proof_verify accepts every item, and the three altered phs of one item per R give 0."""
    L = 7
    suite = bbs.SUITES[curve]
    E = Expect(curve, L, suite.api_id)
    eng = pc.make_engine(curve, E.gens, E.api_id, lib_path, sk=SK)
    msgs = [scalar(curve, "s2-msg-%d" % j) for j in range(L)]
    header = blob("s2-header", 11)
    sig = eng.core_sign(header, msgs)
    assert sig.e == E.e(msgs, header)
    osig = bbs.Signature(sig.a, sig.e)
    count = 0
    for R, promises in sorted(s2_plan(curve, full).items()):
        disclosed = sorted((3 * k + R) % L for k in range(R))
        assert len(set(disclosed)) == R
        undisclosed = [j for j in range(L) if j not in disclosed]
        rnd = [scalar(curve, "s2-rnd-%d-%d" % (R, k)) or 1 for k in range(5 + L - R)]
        dm = [msgs[j] for j in disclosed]
        init = bbs.proof_init(suite, E.pk, osig, E.gens, rnd, header, msgs, undisclosed, E.api_id)
        assert init.scalar == E.domain(header)
        phs, where = steer(promises, "s2-%s-%d" % (curve, R))
        n = len(phs)
        proofs, st = eng.core_proof_gen_batch([sig] * n, [msgs] * n, [disclosed] * n, [rnd] * n, [header] * n, phs)
        _ones(st, n, (curve, R, "core_proof_gen"))
        um = [msgs[j] for j in undisclosed]
        res = residues(phs)
        for i in range(n):
            ch = bbs.proof_challenge_calculate(suite, init, dm, disclosed, phs[i], E.api_id)
            _same_proof(proofs[i], bbs.proof_finalize(suite, init, ch, sig.e, rnd, um), (curve, "R", R, "item", i, "ph length", len(phs[i]), "residue", res[i]))
        k = max(range(n), key=lambda i: (min(len(phs[i]), 5), -i))         # the first item with a ph of >= 5 bytes, if any
        vp = list(proofs) + [proofs[k]] * 3
        vph = list(phs) + header_negatives(phs[k])
        st = eng.core_proof_verify_batch(vp, [dm] * (n + 3), [disclosed] * (n + 3), [header] * (n + 3), vph)
        assert [int(x) for x in st] == [1] * n + [0] * 3, (curve, R, [(i, int(s)) for i, s in enumerate(st) if s != (i < n)][:8])
        count += n
    eng.close()
    return count


# ================================================================================================
# S3: raw messages of the wire forms; S4: hash_to_scalar_batch
# ================================================================================================
def check_wire_messages(curve, lib_path=None, full=False):
    """sign_wire_batch / verify_wire_batch at L = 1: one raw message per item, every length at every residue of the message
    section.  e of every signature from hashlib over the hashlib message scalar, A of four items against the oracle's C port,
    every signature accepted by verify_wire_batch in the same layout; one byte of a message flipped gives 0."""
    suite = bbs.SUITES[curve]
    c = suite.curve
    E = Expect(curve, 1, suite.api_id)
    eng = pc.make_engine(curve, E.gens, E.api_id, lib_path, sk=SK)
    raw, where = steer(s3_plan(curve, full), "s3-" + curve)
    n = len(raw)
    headers = [blob("s3-h-%d" % i, i % 3) for i in range(n)]
    octs, st = eng.sign_wire_batch([[m] for m in raw], headers)
    _ones(st, n, (curve, "sign_wire"))
    res = residues(raw)
    for i in range(n):
        assert octs[i][-32:] == bbs.scalar_be(c, E.e([E.msg_scalar(raw[i])], headers[i])), (curve, "item", i, "message length", len(raw[i]), "residue", res[i])
    for i in sorted({0, n // 3, (2 * n) // 3, n - 1}):
        assert octs[i] == sig_octets(curve, c_port.port(curve).core_sign(SK, E.gens, headers[i], [E.msg_scalar(raw[i])], E.api_id)), (curve, i)
    k = next(i for i in range(n) if len(raw[i]) >= 4)
    forged = raw[k][:-1] + bytes([raw[k][-1] ^ 0x80])
    st = eng.verify_wire_batch(octs + [octs[k]], [[m] for m in raw] + [[forged]], headers + [headers[k]])
    assert [int(x) for x in st] == [1] * n + [0], (curve, [(i, int(s)) for i, s in enumerate(st) if s != (i < n)][:8])
    eng.close()
    return n


def check_hash_to_scalar(curve, lib_path=None):
    """hash_to_scalar_batch: every message length at every residue under the suite's message DST, and every dst_len
    0 .. 255 with three messages each; all against hashlib."""
    suite = bbs.SUITES[curve]
    c = suite.curve
    eng = pc.make_engine(curve, generators(curve, 2), suite.api_id, lib_path)
    dst = suite.api_id + MAP_SUFFIX
    promises = order_promises(MSG_LENS)
    raw, where = steer(promises, "s4-" + curve)
    assert_promises(raw, where, promises)
    got = eng.hash_to_scalar_batch(raw, dst)
    res = residues(raw)
    for i, m in enumerate(raw):
        assert got[i] == hash_to_scalar(c, m, dst), (curve, "item", i, "message length", len(m), "residue", res[i])
    count = len(raw)
    for d in range(256):
        dst = blob("s4-dst-%d" % d, d)
        raw = [blob("s4-dst-%d-%d" % (d, k), n) for k, n in enumerate(s4_dst_messages(d))]
        got = eng.hash_to_scalar_batch(raw, dst)
        for k, m in enumerate(raw):
            assert got[k] == hash_to_scalar(c, m, dst), (curve, "dst_len", d, "message length", len(m))
        count += len(raw)
    eng.close()
    return count


# ================================================================================================
# a DST beyond 255 bytes
# ================================================================================================
def check_dst_too_long(curve, lib_path=None):
    """api_id of 252 bytes: api_id || "H2S_" has 256, the reference's expand_message panics -> -23 from all four operations.
    api_id of 230 bytes: only api_id || "MAP_MSG_TO_SCALAR_AS_HASH_" is too long -> -23 from the wire forms, and only for
    items that hash a message; the core forms and an item without a message to hash work, against hashlib / the oracle."""
    E = Expect(curve, 1, api_id_of(251))
    eng = pc.make_engine(curve, E.gens, E.api_id, lib_path, sk=SK)
    msgs, header, ph = [scalar(curve, "long-m")], blob("long-h", 6), blob("long-p", 3)
    rnd1, rnd0 = [scalar(curve, "long-r-%d" % k) or 1 for k in range(5)], [scalar(curve, "long-q-%d" % k) or 1 for k in range(6)]
    sig = eng.core_sign(header, msgs)
    assert sig.e == E.e(msgs, header)                                      # dst_len 255: the longest there is
    proof = eng.core_proof_gen(sig, header, ph, msgs, [0], rnd1)
    _same_proof(proof, _oracle_proof_gen(E, sig, header, ph, msgs, [0], rnd1, False), (curve, 251))
    assert eng.core_proof_verify(proof, header, ph, msgs, [0]) is True
    eng.set_generators(E.gens, api_id_of(252))
    sigs, st = eng.core_sign_batch([msgs], [header])
    assert [int(x) for x in st] == [DST_TOO_LONG] and sigs == [None]
    assert [int(x) for x in eng.core_verify_batch([sig], [msgs], [header])] == [DST_TOO_LONG]
    proofs, st = eng.core_proof_gen_batch([sig], [msgs], [[0]], [rnd1], [header], [ph])
    assert [int(x) for x in st] == [DST_TOO_LONG] and proofs == [None]
    assert [int(x) for x in eng.core_proof_verify_batch([proof], [msgs], [[0]], [header], [ph])] == [DST_TOO_LONG]
    # 230 bytes
    E = Expect(curve, 1, api_id_of(230))
    eng.set_generators(E.gens, E.api_id)
    raw = blob("long-raw", 9)
    sig = eng.core_sign(header, msgs)
    assert sig.e == E.e(msgs, header)
    assert eng.core_verify(sig, header, msgs) is True
    p1 = eng.core_proof_gen(sig, header, ph, msgs, [0], rnd1)
    p0 = eng.core_proof_gen(sig, header, ph, msgs, [], rnd0)
    _same_proof(p1, _oracle_proof_gen(E, sig, header, ph, msgs, [0], rnd1, False), (curve, 230, 1))
    _same_proof(p0, _oracle_proof_gen(E, sig, header, ph, msgs, [], rnd0, False), (curve, 230, 0))
    assert [int(x) for x in eng.core_proof_verify_batch([p1, p0], [msgs, []], [[0], []], [header] * 2, [ph] * 2)] == [1, 1]
    octs, st = eng.sign_wire_batch([[raw]], [header])
    assert [int(x) for x in st] == [DST_TOO_LONG] and octs == [b""]
    so = sig_octets(curve, sig)
    assert [int(x) for x in eng.verify_wire_batch([so], [[raw]], [header])] == [DST_TOO_LONG]
    octs, st = eng.proof_gen_wire_batch([so], [[raw]], [[0]], [rnd1], [header], [ph])
    assert [int(x) for x in st] == [DST_TOO_LONG]
    st = eng.proof_verify_wire_batch([proof_octets(curve, p1), proof_octets(curve, p0)], [[raw], []], [[0], []], [header] * 2, [ph] * 2)
    assert [int(x) for x in st] == [DST_TOO_LONG, 1]                       # nothing to hash in the second item
    eng.close()


# ================================================================================================
# other layouts
# ================================================================================================
MIXED_HEADERS = ((0, 0), (1, 0), (2, 1), (3, 3), (5, 2), (61, 3), (64, 0), (67, 3), (130, 2))


def check_mixed_lengths(curve, lib_path=None):
    """set_mixed_lengths with set_mixed_lengths_gen on an L = 4 context, api_id lengths 1, 2, 3: an item with l = 0 .. 4
    messages uses the prefix pref[l], whose tail differs from every other.  Expected as a context made for that count: e from
    hashlib, the whole proof from the oracle's C port over the first l + 1 generators."""
    L = 4
    gens = generators(curve, L + 1)
    eng = None
    for a in (1, 2, 3):
        api_id = api_id_of(a)
        if eng is None:
            eng = pc.make_engine(curve, gens, api_id, lib_path, sk=SK)
            eng.set_mixed_lengths(True)
            eng.set_mixed_lengths_gen(True)
        else:
            eng.set_generators(gens, api_id)
        Es = [Expect(curve, l, api_id, gens=gens[:l + 1]) for l in range(L + 1)]
        assert len({dom_tail_len(curve, l, a) for l in range(L + 1)}) >= 2
        headers, where = steer(MIXED_HEADERS, "mixed-%d" % a)
        assert_promises(headers, where, MIXED_HEADERS)
        n = len(headers)
        counts = [(i + a) % (L + 1) for i in range(n)]
        assert set(counts) == set(range(L + 1))
        msgs = [[scalar(curve, "mixed-%d-%d-%d" % (a, i, j)) for j in range(counts[i])] for i in range(n)]
        sigs, st = eng.core_sign_batch(msgs, headers)
        _ones(st, n, (curve, a, "core_sign"))
        for i in range(n):
            assert sigs[i].e == Es[counts[i]].e(msgs[i], headers[i]), (curve, a, i, counts[i])
        _ones(eng.core_verify_batch(sigs, msgs, headers), n, (curve, a, "core_verify"))
        disclosed = [list(range(0, counts[i], 2)) for i in range(n)]
        phs = [blob("mixed-ph-%d-%d" % (a, i), (i * 5 + a) % 7) for i in range(n)]
        rnds = [[scalar(curve, "mixed-r-%d-%d-%d" % (a, i, k)) or 1 for k in range(5 + counts[i] - len(disclosed[i]))] for i in range(n)]
        proofs, st = eng.core_proof_gen_batch(sigs, msgs, disclosed, rnds, headers, phs)
        _ones(st, n, (curve, a, "core_proof_gen"))
        for i in range(n):
            _same_proof(proofs[i], _oracle_proof_gen(Es[counts[i]], sigs[i], headers[i], phs[i], msgs[i], disclosed[i], rnds[i], False), (curve, a, i))
        dm = [[msgs[i][j] for j in disclosed[i]] for i in range(n)]
        _ones(eng.core_proof_verify_batch(proofs, dm, disclosed, headers, phs), n, (curve, a, "core_proof_verify"))
    eng.close()


def check_keyed(curve, lib_path=None):
    """Keyed verification with two keys: the S1 cover set signed by two issuers (e of every item from hashlib), verified on
    one context whose key set holds both; the altered headers of one item per api_id length give 0."""
    plan = s1_plan(curve, False, False)
    sks = (SK, SK + 12345)
    signers, veng = None, None
    for a in sorted(plan):
        api_id = api_id_of(a)
        Es = [Expect(curve, 1, api_id, sk=sk) for sk in sks]
        if veng is None:
            signers = [pc.make_engine(curve, Es[0].gens, api_id, lib_path, sk=sk) for sk in sks]
            veng = pc.make_engine(curve, Es[0].gens, api_id, lib_path)
        else:
            for e in signers + [veng]:
                e.set_generators(Es[0].gens, api_id)
        assert [int(x) for x in veng.set_public_keys([E.pk for E in Es])] == [1, 1]
        headers, where = steer(plan[a], "s1-%s-%d" % (curve, a))
        n = len(headers)
        owner = [(i + a) % 2 for i in range(n)] + [0, 1][:max(0, 2 - n)]
        headers = headers + [blob("keyed-extra-%d" % a, 2 + a % 3)] * max(0, 2 - n)       # both keys sign under every api_id
        n = len(headers)
        msgs = [[scalar(curve, "keyed-%d-%d" % (a, i))] for i in range(n)]
        sigs = [None] * n
        for k in (0, 1):
            idx = [i for i in range(n) if owner[i] == k]
            s, st = signers[k].core_sign_batch([msgs[i] for i in idx], [headers[i] for i in idx])
            _ones(st, len(idx), (curve, a, k, "core_sign"))
            for t, i in enumerate(idx):
                assert s[t].e == Es[k].e(msgs[i], headers[i]), (curve, a, i, k)
                sigs[i] = s[t]
        j = max(range(n), key=lambda i: (min(len(headers[i]), 1), -i))
        expect = [1] * n
        vs, vm, vh, vk = list(sigs), list(msgs), list(headers), list(owner)
        if headers[j]:
            for h in header_negatives(headers[j]):
                vs.append(sigs[j]); vm.append(msgs[j]); vh.append(h); vk.append(owner[j]); expect.append(0)
        vs.append(sigs[0]); vm.append(msgs[0]); vh.append(headers[0]); vk.append(1 - owner[0]); expect.append(0)     # the other key
        st = veng.core_verify_keyed_batch(vk, vs, vm, vh)
        assert [int(x) for x in st] == expect, (curve, a, [int(x) for x in st], expect)
    for e in signers + [veng]:
        e.close()
