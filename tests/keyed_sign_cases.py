"""Keyed sign (bbs_ctx_set_secret_keys, bbs_ctx_add_secret_keys, bbs_core_sign_keyed_*, bbs_sign_wire_keyed_*).  Shared by the
host-twin tier (tests/test_keyed_sign_hosttwin.py) and the GPU tier (tests/test_keyed_sign_gpu.py).

The rule that defines correctness: item i, presented with key index k_i and its own message count l_i, gets the status AND the
signature bytes a single-key context with secret key k_i (made with generators[0 .. l_i] in the mixed form) gives that item
alone; an index at or beyond the set's size, or one naming a refused key, gives BBS_ST_UNKNOWN_KEY (-44), an index naming an
accepted key that was registered public-only gives BBS_ST_NO_SECRET_KEY (-45), and both leave no output whatever else is wrong
with the item.

Expected values: the plain-C restatement of the oracle for EVERY item (core_sign with (sk_{k_i}, generators[: l_i + 1])), a
handful of items through the pure-Python oracle, and as second witness single-key contexts of the same library, one per key
(set_secret_key).  Everything is compared as octet strings, b"" for an item that failed; the raw output buffers of failed
items are checked to be all zero where a test says so.

The key set of every test (SignRing): K ordinary keys, the identity key (sk = 0), two refused scalars (r and 2^256 - 1), and one
key appended public-only.  Sign takes neither signatures nor proofs as inputs, so the lists here (SItems) are made without the
per-(key, length) signing contexts keyed_mixed_cases.KItems builds.

BBS_ST_PANIC_SK_PLUS_E_ZERO (-20) cannot be planted: e is a hash over sk, the messages and the domain, so an item with
sk + e = 0 mod r is a preimage nobody has.  No test fakes it.

Clearing the signing set's memory before release is required of the code and is not tested here: seeing it would mean reading
memory after it was released."""
import ctypes
import functools
import random

import numpy as np
import pytest

from keyed_cases import UNKNOWN_KEY
from keyed_mixed_cases import Ring
from mixed_gen_cases import same_bytes
from mixed_len_cases import World, lengths_mod, prefix_bytes, same, sig_octets
from oracle import bbs
from parity_cases import make_engine

NO_SECRET_KEY = -45
FOUR = tuple((form, submit) for form in ("core", "wire") for submit in (False, True))
EXPORTS = ("bbs_core_sign_keyed_submit", "bbs_core_sign_keyed_batch", "bbs_sign_wire_keyed_submit", "bbs_sign_wire_keyed_batch")
REGISTRATION = ("bbs_ctx_set_secret_keys", "bbs_ctx_add_secret_keys", "bbs_ctx_secret_key_count")
H2S = b"MAP_MSG_TO_SCALAR_AS_HASH_"


class SignRing:
    """Ring's K worlds as the ordinary keys, then sk = 0, sk = r, sk = 2^256 - 1, then one key appended public-only."""

    def __init__(self, curve, lib_path, L, K=3, api_id=None):
        self.ring = Ring(curve, lib_path, L, K, api_id=api_id)
        self.curve, self.lib_path, self.L, self.K = curve, lib_path, L, K
        self.worlds, self.gens, self.api_id = self.ring.worlds, self.ring.gens, self.ring.api_id
        self.w = self.worlds[0]
        r = self.w.c.r
        self.sks = [w.sk for w in self.worlds] + [0, r, (1 << 256) - 1]
        self.IDENTITY, self.REFUSED, self.REFUSED2, self.PUBLIC_ONLY = K, K + 1, K + 2, K + 3
        self.key_status = [1] * (K + 1) + [-40, -40]
        self.public_only = World(curve, lib_path, L, seed=77, api_id=self.api_id, gens=self.gens).pk
        self.size = K + 4
        self.pks = [w.pk for w in self.worlds] + [None, None, None, self.public_only]

    def bare(self):
        return make_engine(self.curve, self.gens, self.api_id, self.lib_path)

    def register(self, eng):
        st, pks, first = eng.set_secret_keys(self.sks)
        assert list(st) == self.key_status and first == 0 and pks == self.pks[:self.K + 3], (list(st), first)
        first, st = eng.add_public_keys([self.public_only])
        assert first == self.PUBLIC_ONLY and list(st) == [1]
        assert eng.secret_key_count() == self.K + 1 and eng.public_key_count() == self.size
        return eng

    def engine(self, on=True, api_id=None):
        eng = self.bare() if api_id is None else make_engine(self.curve, self.gens, api_id, self.lib_path)
        if on:
            eng.set_keyed_mixed_lengths(True)
        return self.register(eng)

    def kind(self, k):
        """1: signs; -44; -45."""
        k = int(k)
        if k >= self.size or k in (self.REFUSED, self.REFUSED2):
            return UNKNOWN_KEY
        return NO_SECRET_KEY if k == self.PUBLIC_ONLY else 1


@functools.lru_cache(maxsize=8)
def scalars_of(curve, lib_path, api_id, raw):
    eng = make_engine(curve, list(bbs.synthetic_generators(bbs.SUITES[curve], 1)), api_id, lib_path)
    out = eng.hash_to_scalar_batch(list(raw), api_id + H2S) if raw else []
    eng.close()
    return tuple(out)


class SItems:
    """n items to sign: raw messages, their scalars (msg_to_scalars under the ring's api_id), headers."""

    def __init__(self, sr, lengths, seed=3, headers=None):
        n = len(lengths)
        self.sr, self.w, self.n, self.lengths = sr, sr.w, n, list(lengths)
        self.raw = [[b"sign-%d-msg-%d-%d" % (i, j, seed) for j in range(l)] for i, l in enumerate(lengths)]
        flat = scalars_of(sr.curve, sr.lib_path, sr.api_id, tuple(m for r in self.raw for m in r))
        self.msgs, at = [], 0
        for l in lengths:
            self.msgs.append(list(flat[at:at + l]))
            at += l
        self.headers = list(headers) if headers is not None else [bytes([i % 251]) * (i % 5) for i in range(n)]

    def copy(self):
        o = SItems.__new__(SItems)
        o.__dict__.update(self.__dict__)
        o.raw, o.msgs, o.headers = [list(x) for x in self.raw], [list(x) for x in self.msgs], list(self.headers)
        return o


def want_keyed(sr, it, key_index, L, mixed=True, idx=None, python=False, sks=None):
    """(octet strings, statuses) of the rule through the C port (python = True: the pure-Python oracle).  sks: another list of
    secret keys to sign with (the neighbour's)."""
    idx = list(range(it.n)) if idx is None else idx
    r = sr.w.c.r
    out, st = [], []
    for i in idx:
        k, l = int(key_index[i]), len(it.msgs[i])
        code = sr.kind(k)
        if code == 1 and (l > L if mixed else l != L):
            code = -1
        if code == 1 and any(m >= r for m in it.msgs[i]):
            code = -40
        st.append(code)
        if code != 1:
            out.append(b"")
            continue
        sk = (sr.sks if sks is None else sks)[k]
        if python:
            s = bbs.core_sign(sr.w.suite, sk, sr.gens[:l + 1], it.headers[i], it.msgs[i], sr.api_id)
        else:
            s = sr.w.cp.core_sign(sk, sr.gens[:l + 1], it.headers[i], it.msgs[i], sr.api_id)
        out.append(sig_octets(sr.w, s))
    return out, st


def as_octets(sr, sigs, st):
    return [sig_octets(sr.w, s) if s is not None else b"" for s in sigs], [int(x) for x in st]


def run_keyed(eng, it, key_index, form="core", submit=False, idx=None):
    """Every export ends as (octet strings, statuses)."""
    idx = list(range(it.n)) if idx is None else idx
    ki = np.asarray([key_index[i] for i in idx], dtype=np.uint32)
    H = [it.headers[i] for i in idx]
    if form == "wire":
        R = [it.raw[i] for i in idx]
        if not submit:
            o, st = eng.sign_wire_keyed_batch(ki, R, H)
        else:
            job = eng.sign_wire_keyed_submit(ki, R, H)
            job.wait()
            o, st = job.output()
            job.free()
        return list(o), [int(x) for x in st]
    M = [it.msgs[i] for i in idx]
    if submit:
        job = eng.core_sign_keyed_submit(ki, M, H)
        job.wait()
        sigs, st = job.output()
        job.free()
    else:
        sigs, st = eng.core_sign_keyed_batch(ki, M, H)
    return as_octets(it.sr, sigs, st)


def run_raw(eng, it, key_index, form):
    """The batch export called directly with output buffers full of 0xAA: (the raw record / octet string of every item, statuses)."""
    from bbs_sign_amd import _lib
    from bbs_sign_amd.engine import _ragged_bytes, _u8, _u64
    n = it.n
    ki, kip = eng._key_index(key_index, n)
    hb, ho = _ragged_bytes(it.headers)
    st = np.full(n, -128, dtype=np.int8)
    rec = eng.fpb + 32 if form == "wire" else 2 * eng.fpb + 32
    out = np.full(n * rec, 0xAA, dtype=np.uint8)
    if form == "wire":
        mb, mbo, mio = eng._raw_msgs(it.raw)
        rc = eng.lib.bbs_sign_wire_keyed_batch(eng.h, n, kip, _u8(mb), _u64(mbo), _u64(mio), _u8(hb), _u64(ho), _u8(out), st.ctypes.data_as(_lib.c_i8p))
    else:
        ms, mo = eng._scalars(it.msgs)
        rc = eng.lib.bbs_core_sign_keyed_batch(eng.h, n, kip, _u8(ms), _u64(mo), _u8(hb), _u64(ho), _u8(out), st.ctypes.data_as(_lib.c_i8p))
    assert rc == 0, rc
    b = out.tobytes()
    return [b[i * rec:(i + 1) * rec] for i in range(n)], [int(x) for x in st]


def single_key_witness(sr, it, key_index, mixed=True, idx=None, api_id=None, form="core"):
    """Second witness: the items of every key that signs through a single-key context of that key (bbs_ctx_set_secret_key; mixed
    lengths of the producing side on or off as the keyed job's).  Other keys: (their code, b"")."""
    idx = list(range(it.n)) if idx is None else idx
    out, st = {i: b"" for i in idx}, {i: sr.kind(key_index[i]) for i in idx}
    for k in sorted({int(key_index[i]) for i in idx if sr.kind(key_index[i]) == 1}):
        mine = [i for i in idx if int(key_index[i]) == k]
        eng = make_engine(sr.curve, sr.gens, sr.api_id if api_id is None else api_id, sr.lib_path, sk=sr.sks[k])
        eng.set_mixed_lengths_gen(mixed)
        H = [it.headers[i] for i in mine]
        if form == "wire":
            o, s = eng.sign_wire_batch([it.raw[i] for i in mine], H)
        else:
            o, s = as_octets(sr, *eng.core_sign_batch([it.msgs[i] for i in mine], H))
        eng.close()
        for t, i in enumerate(mine):
            out[i], st[i] = o[t], int(s[t])
    return [out[i] for i in idx], [st[i] for i in idx]


def boundary(n):
    """The positions that straddle the wavefront boundaries of a list of n items."""
    return [p for p in (0, 63, 64, 65, 127, 128, 129) if p < n] if n > 65 else [0, n // 3, n // 2, n - 1]


def not_signing(sr):
    return [sr.REFUSED, sr.size, sr.PUBLIC_ONLY, sr.REFUSED2, 0xFFFFFFFF, sr.PUBLIC_ONLY, sr.REFUSED]


# ---- case 1: the exports ----------------------------------------------------------------------------------------------------
def check_export(lib_path=None):
    from bbs_sign_amd import Engine, _lib, api
    lib = _lib.load_library(lib_path)
    for name in EXPORTS + REGISTRATION:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    for name in ("set_secret_keys", "add_secret_keys", "secret_key_count", "core_sign_keyed_batch", "core_sign_keyed_submit",
                 "sign_wire_keyed_batch", "sign_wire_keyed_submit"):
        assert callable(getattr(Engine, name))
    assert api.sign_many_issuers([]) == []
    assert lib.bbs_ctx_secret_key_count(None) == 0


# ---- case 2: every key and every length in every wavefront ------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def every_base(curve, lib_path, n, L, K, mixed):
    sr = SignRing(curve, lib_path, L, K)
    pos = boundary(n)
    lengths = lengths_mod(n) if mixed else [L] * n
    if not mixed:                                # an item of another count gets -1
        lengths[5], lengths[n - 3] = L - 1, L + 1
    key_index = [i % K for i in range(n)]
    for p, k in zip(pos, not_signing(sr)):
        key_index[p] = k
    for i in range(n):
        if i % 11 == 5 and i not in pos:
            key_index[i] = sr.IDENTITY
    return sr, key_index, SItems(sr, lengths)


def check_every_key_and_length(curve, lib_path=None, n=130, L=33, K=3, mixed=True, exports=FOUR, python_sample=()):
    sr, key_index, it = every_base(curve, lib_path, n, L, K, mixed)
    pos = boundary(n)
    want = want_keyed(sr, it, key_index, L, mixed)
    assert [want[1][p] for p in pos] == [sr.kind(k) for k in not_signing(sr)][:len(pos)]
    assert {UNKNOWN_KEY, NO_SECRET_KEY, 1} <= set(want[1]) and (-1 in want[1] or (mixed and n < 36))
    for w0 in range(0, n - 63, 64):              # every full wavefront holds every key that signs
        assert {key_index[i] for i in range(w0, min(w0 + 64, n))} >= set(range(K)) | {sr.IDENTITY}
    if mixed:
        assert 0 in it.lengths and (n < 36 or L + 1 in it.lengths) and (n < 70 or all(l in it.lengths for l in range(L + 2)))
    # each key has an item the neighbouring key's secret signs differently
    neighbour = [sr.sks[(k + 1) % K] for k in range(K)] + [sr.sks[0]]
    for k in list(range(K)) + [sr.IDENTITY]:
        i = next(i for i in range(n) if key_index[i] == k and want[1][i] == 1)
        other = want_keyed(sr, it, key_index, L, mixed, [i], sks=neighbour + sr.sks[K + 1:])
        assert other[1] == [1] and other[0][0] != want[0][i], (curve, "key", k)
    eng = sr.engine(on=mixed)
    fpb = sr.w.c.fp_bytes
    for form, submit in exports:
        got = run_keyed(eng, it, key_index, form, submit)
        same_bytes(got, want, (curve, form, "submit" if submit else "batch", "mixed" if mixed else "fixed"))
        assert all(len(o) == (fpb + 32 if s == 1 else 0) for o, s in zip(*got))
    eng.close()
    same_bytes(single_key_witness(sr, it, key_index, mixed), want, (curve, "single-key contexts, one per key"))
    if python_sample:
        assert all(want[1][i] == 1 for i in python_sample)
        py = want_keyed(sr, it, key_index, L, mixed, list(python_sample), python=True)
        same_bytes(py, ([want[0][i] for i in python_sample], [want[1][i] for i in python_sample]), (curve, "python oracle"))


# ---- case 3: round trip on one context --------------------------------------------------------------------------------------
def check_round_trip(curve, lib_path=None, n=130, L=33, K=3):
    """What sign_wire_keyed_batch made verifies on the SAME context under the SAME key_index (the public half of a secret key
    has the secret's index), and under no neighbouring key."""
    sr = SignRing(curve, lib_path, L, K)
    it = SItems(sr, [i % (L + 1) for i in range(n)], seed=8)
    owner = [i % K for i in range(n)]
    eng = sr.engine()
    octs, st = eng.sign_wire_keyed_batch(owner, it.raw, it.headers)
    assert list(st) == [1] * n
    same(eng.verify_wire_keyed_batch(owner, octs, it.raw, it.headers), [1] * n, (curve, "own keys"))
    same(eng.verify_wire_keyed_batch([(k + 1) % K for k in owner], octs, it.raw, it.headers), [0] * n, (curve, "rotated keys"))
    eng.close()


# ---- case 4: registration ---------------------------------------------------------------------------------------------------
def raw_register(eng, fn, sks, with_first):
    from bbs_sign_amd import _lib
    from bbs_sign_amd.engine import _bytes_arr, _u8
    n = len(sks)
    buf = _bytes_arr(b"".join(eng._fr(s) for s in sks)) if n else np.zeros(1, dtype=np.uint8)
    pk, ident, st = np.full(max(n, 1) * 4 * eng.fpb, 0xAA, dtype=np.uint8), np.full(max(n, 1), 0x55, dtype=np.int8), np.zeros(max(n, 1), dtype=np.int8)
    first = ctypes.c_uint32(0xDEAD)
    tail = (ctypes.byref(first),) if with_first else ()
    rc = getattr(eng.lib, fn)(eng.h, n, _u8(buf), st.ctypes.data_as(_lib.c_i8p), _u8(pk), ident.ctypes.data_as(_lib.c_i8p), *tail)
    return rc, [int(x) for x in st[:n]], pk.tobytes()[:n * 4 * eng.fpb], ident.tobytes()[:n], first.value


def check_registration(curve, lib_path=None, L=4, K=3):
    from bbs_sign_amd import Engine, _lib
    from bbs_sign_amd.engine import _bytes_arr, _u8
    sr = SignRing(curve, lib_path, L, K)
    eng = sr.bare()
    fpb, n = eng.fpb, len(sr.sks)
    # bbs_sk_to_pk_batch's output, byte for byte, and the oracle's sk_to_pk
    buf = _bytes_arr(b"".join(eng._fr(s) for s in sr.sks))
    pk0, id0, st0 = np.zeros(n * 4 * fpb, dtype=np.uint8), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int8)
    assert eng.lib.bbs_sk_to_pk_batch(eng.h, n, _u8(buf), _u8(pk0), id0.ctypes.data_as(_lib.c_i8p), None, st0.ctypes.data_as(_lib.c_i8p)) == 0
    rc, st, pk, ident, _ = raw_register(eng, "bbs_ctx_set_secret_keys", sr.sks, False)
    assert rc == 0 and st == sr.key_status == [int(x) for x in st0]
    assert pk == pk0.tobytes() and ident == id0.tobytes()
    rec = 4 * fpb
    for k in range(n):
        got = pk[k * rec:(k + 1) * rec]
        if st[k] != 1 or sr.sks[k] == 0:
            assert got == bytes(rec) and ident[k] == (1 if sr.sks[k] == 0 else 0), k
        else:
            (x0, x1), (y0, y1) = sr.w.cp.sk_to_pk(sr.sks[k])
            assert got == b"".join(int(v).to_bytes(fpb, "little") for v in (x0, x1, y0, y1)) and ident[k] == 0, k
            assert sr.pks[k] == ((x0, x1), (y0, y1)), k            # (World: the pure-Python oracle's sk_to_pk)
    assert eng.secret_key_count() == K + 1 and eng.public_key_count() == n
    it = SItems(sr, [L] * (n + 2), seed=4)
    ki = list(range(n + 2))
    sr.size = n                                 # (no public-only key yet)
    base = want_keyed(sr, it, [k if k < n else 0 for k in ki], L, False)
    want = ([base[0][k] if k < n else b"" for k in ki], [base[1][k] if k < n else UNKNOWN_KEY for k in ki])
    same_bytes(run_keyed(eng, it, ki), want, (curve, "after set"))
    # a public-only append keeps the signing set; a secret append keeps old indexes and bytes
    first, stp = eng.add_public_keys([sr.public_only])
    assert first == n and list(stp) == [1] and eng.secret_key_count() == K + 1 and eng.public_key_count() == n + 1
    extra = World(curve, lib_path, L, seed=91, api_id=sr.api_id, gens=sr.gens)
    rc, st2, pk2, id2, first = raw_register(eng, "bbs_ctx_add_secret_keys", [extra.sk, sr.w.c.r + 5, sr.sks[0]], True)
    assert rc == 0 and st2 == [1, -40, 1] and first == n + 1 and id2 == bytes(3)
    assert pk2[:rec] == b"".join(int(v).to_bytes(fpb, "little") for v in extra.pk[0] + extra.pk[1])
    assert pk2[rec:2 * rec] == bytes(rec) and pk2[2 * rec:] == pk[:rec]                 # (a duplicate key is legal)
    assert eng.secret_key_count() == K + 3 and eng.public_key_count() == n + 4
    sr.size = n + 4
    it2 = SItems(sr, [L] * (n + 5), seed=4)
    got = run_keyed(eng, it2, list(range(n + 5)), "wire")
    same_bytes((got[0][:n], got[1][:n]), (want[0][:n], want[1][:n]), (curve, "old indexes after the appends"))
    assert got[1][n:] == [NO_SECRET_KEY, 1, UNKNOWN_KEY, 1, UNKNOWN_KEY], got[1][n:]
    assert got[0][n + 1] == sig_octets(sr.w, sr.w.cp.core_sign(extra.sk, sr.gens, it2.headers[n + 1], it2.msgs[n + 1], sr.api_id))
    assert got[0][n + 3] == sig_octets(sr.w, sr.w.cp.core_sign(sr.sks[0], sr.gens, it2.headers[n + 3], it2.msgs[n + 3], sr.api_id))
    # what was signed under a secret-registered key verifies under the same index; add with n = 0 reports the size
    assert list(eng.verify_wire_keyed_batch([n + 1], [got[0][n + 1]], [it2.raw[n + 1]], [it2.headers[n + 1]])) == [1]
    rc, _, _, _, first = raw_register(eng, "bbs_ctx_add_secret_keys", [], True)
    assert rc == 0 and first == n + 4
    # NULL arguments
    f32 = ctypes.c_uint32(0)
    one = _bytes_arr(eng._fr(1))
    st1 = np.zeros(1, dtype=np.int8)
    sp = st1.ctypes.data_as(_lib.c_i8p)
    assert eng.lib.bbs_ctx_add_secret_keys(eng.h, 1, _u8(one), sp, None, None, None) == -100
    assert eng.lib.bbs_ctx_add_secret_keys(eng.h, 1, None, sp, None, None, ctypes.byref(f32)) == -100
    assert eng.lib.bbs_ctx_add_secret_keys(eng.h, 1, _u8(one), None, None, None, ctypes.byref(f32)) == -100
    assert eng.lib.bbs_ctx_add_secret_keys(None, 1, _u8(one), sp, None, None, ctypes.byref(f32)) == -100
    assert eng.lib.bbs_ctx_set_secret_keys(eng.h, 1, None, sp, None, None) == -100
    assert eng.lib.bbs_ctx_set_secret_keys(eng.h, 1, _u8(one), None, None, None) == -100
    assert eng.lib.bbs_ctx_set_secret_keys(None, 1, _u8(one), sp, None, None) == -100
    assert eng.secret_key_count() == K + 3 and eng.public_key_count() == n + 4         # (nothing changed)
    # the outputs may be NULL
    assert eng.lib.bbs_ctx_add_secret_keys(eng.h, 1, _u8(one), sp, None, None, ctypes.byref(f32)) == 0 and f32.value == n + 4 and st1[0] == 1
    # a replace; set(0) clears both sets; set_public_keys drops the signing set
    st3, pks3, first = eng.set_secret_keys([sr.sks[1]])
    assert list(st3) == [1] and pks3 == [sr.worlds[1].pk] and (eng.secret_key_count(), eng.public_key_count()) == (1, 1)
    st3, _, _ = eng.set_secret_keys([])
    assert (eng.secret_key_count(), eng.public_key_count()) == (0, 0)
    eng.set_secret_keys(sr.sks[:2])
    eng.set_public_keys([sr.worlds[0].pk])
    assert (eng.secret_key_count(), eng.public_key_count()) == (0, 1)
    eng.set_secret_keys(sr.sks[:2])
    eng.set_public_keys([])
    assert (eng.secret_key_count(), eng.public_key_count()) == (0, 0)
    eng.set_secret_keys(sr.sks[:2])
    eng.set_generators(sr.gens, sr.api_id)
    assert (eng.secret_key_count(), eng.public_key_count()) == (0, 0)
    eng.close()
    # without generators
    e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
    for fn, wf in (("bbs_ctx_set_secret_keys", False), ("bbs_ctx_add_secret_keys", True)):
        assert raw_register(e, fn, [1, 2], wf)[0] == -102
    e.close()


# ---- case 5: codes that override --------------------------------------------------------------------------------------------
DEFECTS = (("length", -1), ("message_not_canonical", -40))


def override_base(curve, lib_path, n, L, K):
    sr = SignRing(curve, lib_path, L, K)
    pos = boundary(n)
    base = SItems(sr, [3 + (i * 7) % (L - 3) for i in range(n)], seed=9)
    good = [i % K for i in range(n)]
    key_index = list(good)
    for p, k in zip(pos[1:], not_signing(sr)):         # pos[0] keeps a key that signs: the defect's own code
        key_index[p] = k
    assert {sr.kind(key_index[p]) for p in pos} == {1, UNKNOWN_KEY, NO_SECRET_KEY}
    return sr, pos, base, good, key_index


def check_overriding_codes(curve, lib_path=None, n=130, L=33, K=3):
    """-44 and -45 override a planted structural defect (a length mismatch, a non-canonical message) and leave zero outputs;
    the same defects under a key that signs give the single-key codes."""
    sr, pos, base, good, key_index = override_base(curve, lib_path, n, L, K)
    eng = sr.engine()
    for kind, code in DEFECTS:
        it = base.copy()
        for p in pos:
            if kind == "length":
                it.msgs[p] = it.msgs[p] + [5] * (L + 1 - len(it.msgs[p]))
                it.raw[p] = it.raw[p] + [b"extra"] * (L + 1 - len(it.raw[p]))
            else:
                it.msgs[p] = it.msgs[p][:-1] + [sr.w.c.r]
        for form in ("core",) if kind == "message_not_canonical" else ("core", "wire"):      # the wire form hashes its messages
            wit = single_key_witness(sr, it, good, True, form=form)
            assert [wit[1][p] for p in pos] == [code] * len(pos) and all(s == 1 for i, s in enumerate(wit[1]) if i not in pos), (curve, kind, form)
            want = (list(wit[0]), [sr.kind(key_index[i]) if sr.kind(key_index[i]) != 1 else s for i, s in enumerate(wit[1])])
            same_bytes(want, want_keyed(sr, it, key_index, L), (curve, kind, form, "C port"))
            same_bytes(run_keyed(eng, it, key_index, form), want, (curve, kind, form))
            raw, st = run_raw(eng, it, key_index, form)
            assert st == want[1] and all(raw[p] == bytes(len(raw[p])) for p in pos), (curve, kind, form, "zero outputs")
    eng.close()


def check_overriding_dst_too_long(curve, lib_path=None, n=130, L=33, K=3):
    """-44 and -45 override -23 as well: the DST of msg_to_scalars (240 bytes of api_id; wire form, items with messages) and of
    the domain hash (252; every item).  -23 is a property of the context's api_id, not of an item."""
    sr, pos, base, good, key_index = override_base(curve, lib_path, n, L, K)
    for m, form in ((240, "wire"), (252, "core")):
        aid = b"x" * m
        e = sr.engine(api_id=aid)
        wit = single_key_witness(sr, base, good, True, api_id=aid, form=form)
        assert set(wit[1]) == {-23}, (curve, m, sorted(set(wit[1])))
        want = ([b""] * n, [sr.kind(key_index[i]) if sr.kind(key_index[i]) != 1 else -23 for i in range(n)])
        same_bytes(run_keyed(e, base, key_index, form), want, (curve, "-23", m, form))
        raw, st = run_raw(e, base, key_index, form)
        assert st == want[1] and all(x == bytes(len(x)) for x in raw)
        e.close()


# ---- case 6: stale pooled buffers -------------------------------------------------------------------------------------------
def check_stale_buffers(curve, lib_path=None, n=130, L=33, K=3):
    """A keyed job of good items, then same-shape jobs whose items all fail at ingest (too long) or at the gate, on the same
    context: the pools hand the later jobs the first one's buffers, and nothing of it may come out."""
    sr = SignRing(curve, lib_path, L, K)
    it = SItems(sr, [L] * n, seed=5)
    good = [i % K for i in range(n)]
    gate = [(sr.REFUSED, sr.PUBLIC_ONLY, sr.size)[i % 3] for i in range(n)]
    long_ = it.copy()
    for i in range(n):
        long_.msgs[i], long_.raw[i] = it.msgs[i] + [5], it.raw[i] + [b"extra"]
    eng = sr.engine()
    want = want_keyed(sr, it, good, L)
    assert want[1] == [1] * n
    for form in ("core", "wire"):
        raw, st = run_raw(eng, it, good, form)
        assert st == [1] * n and all(x != bytes(len(x)) for x in raw)
        if form == "wire":
            assert raw == want[0]
        raw, st = run_raw(eng, it, gate, form)
        assert st == [sr.kind(k) for k in gate] and all(x == bytes(len(x)) for x in raw), (curve, form, "gate")
        same_bytes(run_keyed(eng, it, good, form), want, (curve, form, "good again"))
        raw, st = run_raw(eng, long_, good, form)
        assert st == [-1] * n and all(x == bytes(len(x)) for x in raw), (curve, form, "ingest")
    eng.close()


# ---- case 7: set-up and lifetime --------------------------------------------------------------------------------------------
def check_setup(curve, lib_path=None, L=6, K=3):
    from bbs_sign_amd import Engine, _lib
    from bbs_sign_amd.engine import _ragged_bytes, _u8, _u64
    sr = SignRing(curve, lib_path, L, K)
    n = 4 * K
    it = SItems(sr, [(i * 5 + i // K) % (L + 1) for i in range(n)])
    owner = [i % K for i in range(n)]
    assert len(set(it.lengths)) >= 4 and L in it.lengths
    want = want_keyed(sr, it, owner, L)
    assert want[1] == [1] * n
    full = [i for i in range(n) if it.lengths[i] == L]
    only_L = ([want[0][i] if i in full else b"" for i in range(n)], [1 if i in full else -1 for i in range(n)])

    def refused(eng, code):
        for form, submit in FOUR:
            with pytest.raises(Exception, match=code):
                run_keyed(eng, it, owner, form, submit)

    # without generators
    e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
    refused(e, "BBS_E_STATE")
    e.close()
    # without a signing set while the keyed switch is off; a missing set is the empty set with the switch on -- also where the
    # key set knows the keys (registered public-only)
    e = sr.bare()
    refused(e, "BBS_E_STATE")
    e.set_public_keys([w.pk for w in sr.worlds])
    refused(e, "BBS_E_STATE")
    e.set_keyed_mixed_lengths(True)
    for form, submit in FOUR:
        same_bytes(run_keyed(e, it, owner, form, submit), ([b""] * n, [UNKNOWN_KEY] * n), (curve, "no signing set, switch on", form, submit))
    e.set_public_keys([])
    same_bytes(run_keyed(e, it, owner), ([b""] * n, [UNKNOWN_KEY] * n), (curve, "no set at all, switch on"))
    e.close()
    # the producing side's single-key switch on and the keyed switch off: BBS_E_STATE; both on: mixed counts; both off: l = L only
    e = sr.engine(on=False)
    same_bytes(run_keyed(e, it, owner), only_L, (curve, "both switches off"))
    e.set_mixed_lengths_gen(True)
    refused(e, "BBS_E_STATE")
    e.set_keyed_mixed_lengths(True)
    same_bytes(run_keyed(e, it, owner), want, (curve, "both switches on"))
    e.set_mixed_lengths_gen(False)
    # NULL key_index, NULL status, NULL ctx; n = 0
    ms, mo = e._scalars(it.msgs)
    hb, ho = _ragged_bytes(it.headers)
    st = np.zeros(n, dtype=np.int8)
    out = np.zeros(n * (2 * e.fpb + 32), dtype=np.uint8)
    ki = np.asarray(owner, dtype=np.uint32)
    kp, sp = ki.ctypes.data_as(_lib.c_u32p), st.ctypes.data_as(_lib.c_i8p)
    args = (_u8(ms), _u64(mo), _u8(hb), _u64(ho), _u8(out))
    assert e.lib.bbs_core_sign_keyed_batch(e.h, n, None, *args, sp) == -100
    assert e.lib.bbs_core_sign_keyed_batch(e.h, n, kp, *args, None) == -100
    assert e.lib.bbs_core_sign_keyed_batch(None, n, kp, *args, sp) == -100
    assert e.lib.bbs_core_sign_keyed_batch(e.h, 0, None, *args, sp) == 0                 # n = 0: nothing is read
    for form, submit in FOUR:
        assert run_keyed(e, it, owner, form, submit, idx=[])[0] == []
    # an unrelated single secret key set on the context: the same bytes
    e.set_secret_key(World(curve, lib_path, L, seed=78, api_id=sr.api_id, gens=sr.gens).sk)
    same_bytes(run_keyed(e, it, owner), want, (curve, "an unrelated single key"))
    # a job keeps what it was created with: the signing set, the key set, the rows per (key, length), the generators' tables
    for change in ("append", "replace", "switch", "generators"):
        ki = np.asarray(owner, dtype=np.uint32)
        held = e.sign_wire_keyed_submit(ki, it.raw, it.headers) if change != "switch" else e.core_sign_keyed_submit(ki, it.msgs, it.headers)
        if change == "append":
            assert e.add_secret_keys([sr.sks[1]])[2] == sr.size
        elif change == "replace":
            e.set_secret_keys(sr.sks[1:K] + sr.sks[:1])
        elif change == "switch":
            e.set_keyed_mixed_lengths(False)
        else:
            e.set_generators(bbs.synthetic_generators(sr.w.suite, L + 1, b"keyed-sign-other-generators"), sr.api_id)
        held.wait()
        out = held.output()
        held.free()
        if change == "switch":
            out = as_octets(sr, *out)
        same_bytes((list(out[0]), [int(x) for x in out[1]]), want, (curve, "held job", change))
        if change == "replace":
            got = run_keyed(e, it, owner, "wire")
            assert got[1] == [1] * n and all(a != b for a, b in zip(got[0], want[0])), (curve, "the replaced set signs with its own keys")
            sr.register(e)
        elif change == "switch":
            e.set_keyed_mixed_lengths(True)
    assert (e.secret_key_count(), e.public_key_count()) == (0, 0)                        # (the generators took both sets)
    e.close()                                                                            # (every job waited and freed)
    # any order of generators, registration and the switch ends in the same bytes
    for route in (1, 2, 3):
        e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
        if route == 3:
            e.set_keyed_mixed_lengths(True)                # the switch before the generators
        e.set_generators(sr.gens, sr.api_id)
        if route == 1:
            e.set_keyed_mixed_lengths(True)
            e.set_secret_keys(sr.sks[:K])
        elif route == 2:
            e.set_secret_keys(sr.sks[:1])
            e.set_keyed_mixed_lengths(True)
            assert e.add_secret_keys(sr.sks[1:K])[2] == 1
        else:
            e.add_public_keys([sr.worlds[0].pk])            # a public-only key first: the secret keys come behind it
            assert e.add_secret_keys(sr.sks[:K])[2] == 1
        shift = 1 if route == 3 else 0
        same_bytes(run_keyed(e, it, [k + shift for k in owner]), want, (curve, "route", route))
        if route == 3:
            assert run_keyed(e, it, [0] * n)[1] == [NO_SECRET_KEY] * n
        e.close()


# ---- case 8: prefix boundaries per key --------------------------------------------------------------------------------------
def check_prefix_boundaries(curve, lib_path=None, which=0, L=8):
    """Header and api_id lengths that put the end of `key octets || count || generators || api_id` on, one before and one after
    a SHA-256 block edge (the api_ids of keyed_gen_cases.check_prefix_boundaries, one per test case), under two keys, with
    headers of 0, 55, 56 and 64 bytes, every length 0 .. L under both keys."""
    lens = (39, 40, 41) if curve == "bls12_381" else (23, 24, 25)
    K = 2
    hl = (0, 55, 56, 64)
    ends = {m: {l: prefix_bytes(curve, l, m) % 64 for l in range(L + 1)} for m in lens}
    m = lens[which]
    assert sum(1 for l in ends[m] if ends[m][l] == (63, 0, 1)[which]) >= 2, (m, ends[m])
    sr = SignRing(curve, lib_path, L, K, api_id=bytes(65 + k % 26 for k in range(m)))
    lengths = [l for l in range(L + 1) for _ in hl for _ in range(K)]
    owner = [k for l in range(L + 1) for _ in hl for k in range(K)]
    it = SItems(sr, lengths, headers=[bytes([7 + l]) * h for l in range(L + 1) for h in hl for _ in range(K)])
    eng = sr.engine()
    want = want_keyed(sr, it, owner, L)
    assert want[1] == [1] * it.n
    same_bytes(run_keyed(eng, it, owner), want, (curve, m, "core"))
    same_bytes(run_keyed(eng, it, owner, "wire", True), want, (curve, m, "wire"))
    eng.close()


# ---- case 9: the reference's vector -----------------------------------------------------------------------------------------
def check_reference_vector(lib_path=None, L=5):
    """The BLS12-381 signature vector of src/tests/test_vector.rs:139-192 signed as a keyed item of one message on a context made
    for L messages, the vector's key registered behind two others."""
    from bbs_sign_amd import api
    curve = "bls12_381"
    S = bbs.BLS_SUITE
    H = bytes.fromhex
    sk = int("60e55110f76883a13d030b2f6bd11883422d5abde717569fc0731f51237169fc", 16)
    m1 = H("9872ad089e452c7b6e283dfac2a80d58e8d0ff71cc4d5e310a1debdda4a45f02")
    header = H("11223344556677889900aabbccddeeff")
    sig = ("84773160b824e194073a57493dac1a20b667af70cd2352d8af241c77658da5253aa8458317cca0eae615690d55b1f271"
           "64657dcafee1d5c1973947aa70e2cfbb4c892340be5969920d0916067b4565a0")
    eng = make_engine(curve, api.create_generators(curve, L + 1, lib_path), S.api_id, lib_path)
    eng.set_keyed_mixed_lengths(True)
    st, pks, first = eng.set_secret_keys([12345, 54321, sk])
    assert list(st) == [1, 1, 1]
    octs, st = eng.sign_wire_keyed_batch([2, 0, 7], [[m1]] * 3, [header] * 3)
    assert list(st) == [1, 1, UNKNOWN_KEY] and octs[0].hex() == sig and octs[1] and octs[1].hex() != sig and octs[2] == b""
    msg = eng.hash_to_scalar_batch([m1], S.api_id + H2S)
    sigs, st = eng.core_sign_keyed_batch([2], [[msg[0]]], [header])
    assert list(st) == [1] and (bbs.g1_compress(S.curve, sigs[0].a) + bbs.scalar_be(S.curve, sigs[0].e)).hex() == sig
    eng.close()
    got = api.sign_many_issuers([(api.SecretKey(curve, 777, lib_path), b"h", [b"x"]), (api.SecretKey(curve, sk, lib_path), header, [m1])])
    assert api.signature_to_octets(curve, got[1], lib_path).hex() == sig
    api.clear_caches()


# ---- case 10: the public layer ----------------------------------------------------------------------------------------------
def check_public_layer(lib_path=None):
    """api.sign_many_issuers over 12 items of 3 issuers on one curve and 6 on the other, counts 0 .. 6, in one list."""
    from bbs_sign_amd import BbsError, api
    rng = random.Random(98)
    lengths = [0, 1, 2, 3, 4, 5, 6, 2, 3, 4, 1, 5]
    items = []
    for curve in ("bls12_381", "bn254"):
        r = bbs.SUITES[curve].curve.r
        sks = [api.SecretKey(curve, rng.randrange(1, r), lib_path) for _ in range(3)]
        for i, l in enumerate(lengths[:6] if curve == "bn254" else lengths[6:] + lengths[:6]):
            items.append((sks[i % 3], b"h%d" % i, [b"sign-issuers-%d-%d" % (i, j) for j in range(l)]))
    n = len(items)
    assert n == 18 and {it[0].curve for it in items} == {"bls12_381", "bn254"}
    refused = 9
    items[refused] = (api.SecretKey(items[refused][0].curve, bbs.SUITES[items[refused][0].curve].curve.r, lib_path),) + items[refused][1:]
    got = api.sign_many_issuers(items)
    assert len(api._issuer_cache) == 2                     # one engine, one device call, per curve
    assert isinstance(got[refused], BbsError) and got[refused].status == UNKNOWN_KEY, got[refused]      # returned, not raised
    ok = [i for i in range(n) if i != refused]
    by_key = {}
    for i in ok:
        by_key.setdefault(id(items[i][0]), []).append(i)
    for idx in by_key.values():
        sk = items[idx[0]][0]
        want = api.sign_many(sk, [(items[i][2], items[i][1]) for i in idx])
        for i, w in zip(idx, want):
            assert not isinstance(got[i], BbsError) and (got[i].a, got[i].e) == (w.a, w.e), i
    pks = {id(it[0]): it[0].sk_to_pk() for it in items if it[0] is not items[refused][0]}
    verdicts = api.verify_many_issuers([(pks[id(items[i][0])], got[i], items[i][1], items[i][2]) for i in ok])
    assert verdicts == [True] * len(ok), verdicts
    assert all(ie.eng.secret_key_count() == 3 and ie.eng.public_key_count() <= 4 for ie in api._issuer_cache.values())     # keys registered once
    again = api.sign_many_issuers([items[i] for i in ok[:4]])
    assert [(s.a, s.e) for s in again] == [(got[i].a, got[i].e) for i in ok[:4]]
    assert all(ie.eng.secret_key_count() == 3 for ie in api._issuer_cache.values())
    api.clear_caches()
