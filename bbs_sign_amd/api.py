"""Mirror of the reference's PUBLIC interface (README.md:43-128) over the MI355X engine:

    SecretKey.key_gen / .sk_to_pk / .sign        src/key_gen.rs:46-90, src/sign.rs:32-60
    PublicKey.verify                              src/verify.rs:18-50
    proof_gen / proof_verify                      src/proof_gen.rs:78-113, src/proof_verify.rs:19-61

Messages are byte strings, exactly as in the reference.  What the reference recomputes on every
call -- create_generators (33 hash-to-curve operations at L = 32) and the api_id strings -- is
computed once per (ciphersuite, L) by the host side of the library (bbs_create_generators) and kept
in an engine context; msg_to_scalars runs on the device (bbs_hash_to_scalar_batch).

Both ciphersuites of the reference (src/constants.rs): BLS12-381 (simplified SWU hash-to-curve) and BN254
(Shallue-van de Woestijne, restated from RFC 9380 and pinned by the reference's P1 constant).
"""
from __future__ import annotations

import ctypes
import secrets
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .engine import BbsError, BbsRuntimeError, Engine, Proof, Signature, _bytes_arr, _u8

CIPHERSUITE_ID = {"bls12_381": b"BBS_BLS12381G1_XMD:SHA-256_SSWU_RO_",
                  "bn254": b"BBS_QUUX-V01-CS02-with-BN254G1_XMD:SHA-256_SVDW_RO_"}
SCALAR_ORDER = {
    "bls12_381": 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001,
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
}
KEYGEN_ERRORS = {-7: "InvalidKeyMaterialLength", -8: "InvalidKeyInfoLength", -9: "InvalidSecretKey"}


def api_id(curve: str) -> bytes:
    return CIPHERSUITE_ID[curve] + b"H2G_HM2S_"


_gen_cache: Dict[Tuple[str, int, Optional[str]], list] = {}
_eng_cache: Dict[tuple, Engine] = {}


def create_generators(curve: str, count: int, lib_path: Optional[str] = None) -> list:
    """create_generators::<E, H>(count, api_id) (src/utils/interface_utilities.rs:47-73)."""
    key = (curve, count, lib_path)
    if key not in _gen_cache:
        lib = _lib.load_library(lib_path)
        fpb = int(lib.bbs_fp_bytes(0 if curve == "bls12_381" else 1))
        aid = _bytes_arr(api_id(curve))
        out = np.zeros(max(count, 1) * 2 * fpb, dtype=np.uint8)
        rc = lib.bbs_create_generators(0 if curve == "bls12_381" else 1, count, _u8(aid), len(api_id(curve)), _u8(out))
        if rc:
            raise BbsRuntimeError(rc, "bbs_create_generators")
        b = out.tobytes()
        gens = []
        for k in range(count):
            x = int.from_bytes(b[k * 2 * fpb:k * 2 * fpb + fpb], "little")
            y = int.from_bytes(b[k * 2 * fpb + fpb:(k + 1) * 2 * fpb], "little")
            gens.append(None if x == 0 and y == 0 else (x, y))
        _gen_cache[key] = gens
    return list(_gen_cache[key])


def _engine(curve: str, L: int, *, sk: Optional[int] = None, pk="unset", device: int = 0,
            lib_path: Optional[str] = None, window_bits: Optional[int] = None) -> Engine:
    key = (curve, L, sk, None if pk is None else (pk if pk == "unset" else tuple(map(tuple, pk))), device, lib_path)
    eng = _eng_cache.get(key)
    if eng is None:
        if window_bits is None and lib_path is not None:
            window_bits = 4              # host-twin test library: small tables
        eng = Engine(curve, device=device, lib_path=lib_path, window_bits=window_bits)
        eng.set_generators(create_generators(curve, L + 1, lib_path), api_id(curve))
        if sk is not None:
            eng.set_secret_key(sk)
        elif pk != "unset":
            eng.set_public_key(pk)
        _eng_cache[key] = eng
    return eng


def clear_caches():
    for e in _eng_cache.values():
        e.close()
    _eng_cache.clear()
    for e in _issuer_cache.values():
        e.eng.close()
    _issuer_cache.clear()
    _gen_cache.clear()


def msg_to_scalars(eng: Engine, curve: str, messages: Sequence[bytes]) -> List[int]:
    """msg_to_scalars (src/utils/interface_utilities.rs:76-88), on the device."""
    if not messages:
        return []
    return eng.hash_to_scalar_batch(list(messages), api_id(curve) + b"MAP_MSG_TO_SCALAR_AS_HASH_")


class PublicKey:
    """key_gen.rs:12-15; pk is None (identity, `PublicKey::default()`) or ((x0, x1), (y0, y1))."""

    def __init__(self, curve: str, pk, lib_path: Optional[str] = None, device: int = 0):
        self.curve, self.pk, self.lib_path, self.device = curve, pk, lib_path, device

    def verify(self, signature: Signature, header: bytes, messages: Sequence[bytes]) -> bool:
        """PublicKey::verify (src/verify.rs:18-50)."""
        eng = _engine(self.curve, len(messages), pk=self.pk, device=self.device, lib_path=self.lib_path)
        return eng.core_verify(signature, header, msg_to_scalars(eng, self.curve, messages))


class SecretKey:
    def __init__(self, curve: str, sk: int, lib_path: Optional[str] = None, device: int = 0):
        self.curve, self.sk, self.lib_path, self.device = curve, sk, lib_path, device

    @classmethod
    def key_gen(cls, curve: str, key_material: bytes, key_info: bytes, key_dst: bytes,
                lib_path: Optional[str] = None, device: int = 0) -> "SecretKey":
        """SecretKey::key_gen (src/key_gen.rs:46-81); errors as BbsError(KeyGenError variant)."""
        lib = _lib.load_library(lib_path)
        km, ki, kd = _bytes_arr(key_material), _bytes_arr(key_info), _bytes_arr(key_dst)
        out = np.zeros(32, dtype=np.uint8)
        rc = lib.bbs_key_gen(0 if curve == "bls12_381" else 1, _u8(km), len(key_material), _u8(ki), len(key_info),
                             _u8(kd), len(key_dst), _u8(out))
        if rc in KEYGEN_ERRORS:
            e = BbsError(rc)
            e.variant = KEYGEN_ERRORS[rc]
            raise e
        if rc:
            raise BbsRuntimeError(rc, "bbs_key_gen")
        return cls(curve, int.from_bytes(out.tobytes(), "little"), lib_path, device)

    def sk_to_pk(self) -> PublicKey:
        """SecretKey::sk_to_pk (src/key_gen.rs:83-90)."""
        eng = _engine(self.curve, 0, sk=self.sk, device=self.device, lib_path=self.lib_path)
        return PublicKey(self.curve, eng.public_key(), self.lib_path, self.device)

    def sign(self, messages: Sequence[bytes], header: bytes) -> Signature:
        """SecretKey::sign (src/sign.rs:32-60)."""
        eng = _engine(self.curve, len(messages), sk=self.sk, device=self.device, lib_path=self.lib_path)
        return eng.core_sign(header, msg_to_scalars(eng, self.curve, messages))


def key_gen_batch(curve: str, key_materials: Sequence[bytes], key_infos: Sequence[bytes], key_dst: bytes,
                  lib_path: Optional[str] = None, device: int = 0) -> list:
    """SecretKey::key_gen followed by sk_to_pk (src/key_gen.rs:46-90) for many keys in ONE device call (bbs_key_gen_batch).
    Entry k of the result is ``(SecretKey, PublicKey)``, or the exception SecretKey.key_gen would raise for item k (returned,
    not raised: the other items stand): a BbsError with the same ``.variant``."""
    eng = _engine(curve, 0, device=device, lib_path=lib_path)
    sks, pks, _, st = eng.key_gen_batch(list(key_materials), list(key_infos), key_dst)
    out = []
    for k in range(len(sks)):
        rc = int(st[k])
        if rc == 1:
            out.append((SecretKey(curve, sks[k], lib_path, device), PublicKey(curve, pks[k], lib_path, device)))
        elif rc in KEYGEN_ERRORS:
            e = BbsError(rc)
            e.variant = KEYGEN_ERRORS[rc]
            out.append(e)
        else:
            out.append(BbsRuntimeError(rc, "bbs_key_gen"))
    return out


def sk_to_pk_batch(secret_keys: Sequence[SecretKey]) -> List[PublicKey]:
    """SecretKey::sk_to_pk (src/key_gen.rs:83-90) for many keys in one device call per (curve, library, device)."""
    out: List[Optional[PublicKey]] = [None] * len(secret_keys)
    groups: Dict[tuple, List[int]] = {}
    for k, s in enumerate(secret_keys):
        groups.setdefault((s.curve, s.lib_path, s.device), []).append(k)
    for (curve, lib_path, device), idx in groups.items():
        eng = _engine(curve, 0, device=device, lib_path=lib_path)
        pks, _, st = eng.sk_to_pk_batch([secret_keys[k].sk for k in idx])
        for k, pk, rc in zip(idx, pks, st):
            if rc != 1:
                raise BbsRuntimeError(-100, "bbs_sk_to_pk_batch (secret key %d is not below the group order)" % k)
            out[k] = PublicKey(curve, pk, lib_path, device)
    return out


def hash_to_g1(curve: str, msg: bytes, dst: bytes, lib_path: Optional[str] = None):
    """The suite's hash-to-G1 (src/utils/interface_utilities.rs:24-44), host side of the library."""
    lib = _lib.load_library(lib_path)
    cid = 0 if curve == "bls12_381" else 1
    fpb = int(lib.bbs_fp_bytes(cid))
    out = np.zeros(2 * fpb, dtype=np.uint8)
    m, d = _bytes_arr(msg), _bytes_arr(dst)
    rc = lib.bbs_hash_to_g1(cid, _u8(m), len(msg), _u8(d), len(dst), _u8(out))
    if rc:
        raise BbsRuntimeError(rc, "bbs_hash_to_g1")
    b = out.tobytes()
    x, y = int.from_bytes(b[:fpb], "little"), int.from_bytes(b[fpb:], "little")
    return None if x == 0 and y == 0 else (x, y)


def calculate_random_scalars(curve: str, count: int) -> List[int]:
    """calculate_random_scalars (src/utils/core_utilities.rs:70-81): 48 random bytes mod r each."""
    r = SCALAR_ORDER[curve]
    return [int.from_bytes(secrets.token_bytes(48), "big") % r for _ in range(count)]


def proof_gen(pk: PublicKey, signature: Signature, header: bytes, ph: bytes, messages: Sequence[bytes],
              disclosed_indexes: Sequence[int], random_scalars: Optional[Sequence[int]] = None) -> Proof:
    """proof_gen (src/proof_gen.rs:78-113).  ``random_scalars`` (5 + L - R of them) replaces the draw at
    :145-149; by default they are drawn here exactly as the reference draws them."""
    L, R = len(messages), len(disclosed_indexes)
    eng = _engine(pk.curve, L, pk=pk.pk, device=pk.device, lib_path=pk.lib_path)
    if random_scalars is None:
        random_scalars = calculate_random_scalars(pk.curve, max(5 + L - R, 0))
    return eng.core_proof_gen(signature, header, ph, msg_to_scalars(eng, pk.curve, messages), disclosed_indexes,
                              random_scalars)


def proof_verify(pk: PublicKey, proof: Proof, header: bytes, ph: bytes, disclosed_messages: Sequence[bytes],
                 disclosed_indexes: Sequence[int]) -> bool:
    """proof_verify (src/proof_verify.rs:19-61): L is inferred as commitments + disclosed indexes."""
    L = len(proof.commitments) + len(disclosed_indexes)
    eng = _engine(pk.curve, L, pk=pk.pk, device=pk.device, lib_path=pk.lib_path)
    return eng.core_proof_verify(proof, header, ph, msg_to_scalars(eng, pk.curve, disclosed_messages), disclosed_indexes)


# ------------------------------------------------------------------ many items, any lengths
def _mixed_engine(pk: PublicKey, L: int) -> Engine:
    """A cached engine of this key with bbs_ctx_set_mixed_lengths on, made for L messages or more: its own cache entries, so
    that the one-item functions above keep their fixed-length engines."""
    who = (pk.curve, None if pk.pk is None else tuple(map(tuple, pk.pk)), pk.device, pk.lib_path)
    # any cached mixed engine of this key made for at least L messages serves (the smallest such): one copy of the tables
    fits = [k for k in _eng_cache if k[0] == "mixed" and k[2:] == who and k[1] >= L]
    if fits:
        return _eng_cache[min(fits, key=lambda k: k[1])]
    eng = Engine(pk.curve, device=pk.device, lib_path=pk.lib_path, window_bits=4 if pk.lib_path is not None else None)
    eng.set_generators(create_generators(pk.curve, L + 1, pk.lib_path), api_id(pk.curve))
    eng.set_public_key(pk.pk)
    eng.set_mixed_lengths(True)
    for k in [k for k in _eng_cache if k[0] == "mixed" and k[2:] == who]:      # the shorter ones it replaces
        _eng_cache.pop(k).close()
    _eng_cache[("mixed", L) + who] = eng
    return eng


def _many(items, to_octets, run, at=0):
    """Shared tail of verify_many / proof_verify_many (and the *_many_issuers forms, whose object is entry 1 of an item): items
    whose object cannot be written as octets keep the codec's BbsError, the others run in ONE device call; statuses become
    booleans or BbsError objects."""
    out: list = [None] * len(items)
    octs, idx = [], []
    for i, it in enumerate(items):
        try:
            octs.append(to_octets(it[at]))
            idx.append(i)
        except BbsError as e:
            out[i] = e
    if idx:
        for i, s in zip(idx, run(octs, [items[i] for i in idx])):
            out[i] = BbsError(int(s)) if s < 0 else bool(s)
    return out


def verify_many(pk: PublicKey, items: Sequence[tuple]) -> list:
    """PublicKey.verify for many items ``(signature, header, messages)`` whose message counts may differ, in ONE device call:
    one cached engine whose L is the largest count present, with mixed lengths on, through the wire form.  Entry i is the
    boolean ``pk.verify(*items[i])`` returns, or the BbsError it raises (returned, not raised: the other items stand)."""
    if not items:
        return []
    eng = _mixed_engine(pk, max(len(it[2]) for it in items))
    return _many(items, lambda sig: signature_to_octets(pk.curve, sig, pk.lib_path),
                 lambda octs, its: eng.verify_wire_batch(octs, [list(it[2]) for it in its], [it[1] for it in its]))


def proof_verify_many(pk: PublicKey, items: Sequence[tuple]) -> list:
    """proof_verify for many items ``(proof, header, ph, disclosed_messages, disclosed_indexes)`` of any message counts
    (commitments + disclosed indexes each), in ONE device call, as verify_many."""
    if not items:
        return []
    eng = _mixed_engine(pk, max(len(it[0].commitments) + len(it[4]) for it in items))
    return _many(items, lambda proof: proof_to_octets(pk.curve, proof, pk.lib_path),
                 lambda octs, its: eng.proof_verify_wire_batch(octs, [list(it[3]) for it in its], [list(it[4]) for it in its],
                                                               [it[1] for it in its], [it[2] for it in its]))


# ------------------------------------------------------------------ many items, any lengths: the producing side
def _mixed_gen_engine(key, L: int) -> Engine:
    """A cached engine of this SecretKey (sign) or PublicKey (proof_gen) with bbs_ctx_set_mixed_lengths_gen on, made for L
    messages or more: its own cache entries, as _mixed_engine's -- the smallest cached one that fits serves, a longer list
    replaces the shorter ones."""
    secret = isinstance(key, SecretKey)
    name = ("sk", key.sk) if secret else (None if key.pk is None else tuple(map(tuple, key.pk)))
    who = (key.curve, name, key.device, key.lib_path)
    fits = [k for k in _eng_cache if k[0] == "mixed_gen" and k[2:] == who and k[1] >= L]
    if fits:
        return _eng_cache[min(fits, key=lambda k: k[1])]
    eng = Engine(key.curve, device=key.device, lib_path=key.lib_path, window_bits=4 if key.lib_path is not None else None)
    eng.set_generators(create_generators(key.curve, L + 1, key.lib_path), api_id(key.curve))
    if secret:
        eng.set_secret_key(key.sk)
    else:
        eng.set_public_key(key.pk)
    eng.set_mixed_lengths_gen(True)
    for k in [k for k in _eng_cache if k[0] == "mixed_gen" and k[2:] == who]:      # the shorter ones it replaces
        _eng_cache.pop(k).close()
    _eng_cache[("mixed_gen", L) + who] = eng
    return eng


def sign_many(sk: SecretKey, items: Sequence[tuple]) -> list:
    """SecretKey.sign for many items ``(messages, header)`` whose message counts may differ, in ONE device call: one cached
    engine whose L is the largest count present, with bbs_ctx_set_mixed_lengths_gen on, through the wire form.  Entry i is the
    Signature ``sk.sign(*items[i])`` returns, or the BbsError it raises (returned, not raised: the other items stand)."""
    if not items:
        return []
    eng = _mixed_gen_engine(sk, max(len(it[0]) for it in items))
    octs, st = eng.sign_wire_batch([list(it[0]) for it in items], [it[1] for it in items])
    return [BbsError(int(s)) if s < 0 else octets_to_signature(sk.curve, o, sk.lib_path) for o, s in zip(octs, st)]


def _device_draw(eng: Engine, curve: str, call):
    """``call(job_seed)`` with bbs_ctx_set_seeded_random_scalars on for its duration: ONE fresh 32-byte job seed from the
    operating system per device call (a seed never serves two jobs), DST = api_id || "SEEDED_RANDOM_SCALARS_"."""
    eng.set_seeded_random_scalars(True, api_id(curve) + b"SEEDED_RANDOM_SCALARS_")
    try:
        return call(secrets.token_bytes(32))
    finally:
        eng.set_seeded_random_scalars(False)


def proof_gen_many(pk: PublicKey, items: Sequence[tuple], device_random: bool = False) -> list:
    """proof_gen for many items ``(signature, header, ph, messages, disclosed_indexes[, random_scalars])`` of any message
    counts, in ONE device call, as sign_many.  Entry i is the Proof ``proof_gen(pk, *items[i])`` returns with the same random
    scalars (drawn here, as there, where an item has none), or the BbsError it raises (returned, not raised).  A wrong number of
    random scalars in one item fails the whole call (BbsRuntimeError, BBS_E_ARG), as it fails the one-item call.
    ``device_random=True``: when NO item gives scalars of its own, the scalars are drawn on the device from one fresh job seed
    (bbs_ctx_set_seeded_random_scalars) instead of one by one here; a list in which an item brings its own is served as before."""
    if not items:
        return []
    eng = _mixed_gen_engine(pk, max(len(it[3]) for it in items))
    on_device = device_random and not any(len(it) > 5 and it[5] is not None for it in items)
    rnds = [] if on_device else [list(it[5]) if len(it) > 5 and it[5] is not None else
                                 calculate_random_scalars(pk.curve, max(5 + len(it[3]) - len(it[4]), 0)) for it in items]
    out: list = [None] * len(items)
    octs, idx = [], []
    for i, it in enumerate(items):
        try:
            octs.append(signature_to_octets(pk.curve, it[0], pk.lib_path))
            idx.append(i)
        except BbsError as e:           # a signature that cannot be written as octets keeps the codec's error
            out[i] = e
    if idx:
        its = [items[i] for i in idx]
        def call(r):
            return eng.proof_gen_wire_batch(octs, [list(it[3]) for it in its], [list(it[4]) for it in its], r, [it[1] for it in its], [it[2] for it in its])
        po, st = _device_draw(eng, pk.curve, call) if on_device else call([rnds[i] for i in idx])
        for i, o, s in zip(idx, po, st):
            out[i] = BbsError(int(s)) if s < 0 else octets_to_proof(pk.curve, o, pk.lib_path)
    return out


# ------------------------------------------------------------------ many items, any issuers, any lengths
class _IssuerEngine:
    """One engine per (curve, device, lib_path) with bbs_ctx_set_keyed_mixed_lengths on: made for the largest count seen, its
    key set grows by appending and a key is registered once (``index``: key -> its index in the set)."""

    def __init__(self, curve, device, lib_path, L, keys=()):
        self.L = L
        self.index: Dict[object, int] = {}
        self.sk_index: Dict[int, int] = {}          # sign_many_issuers: secret key -> its index in the signing set
        self.octets: Dict[object, bytes] = {}       # register_keys=False: key -> its compressed string (key_octets)
        self.eng = Engine(curve, device=device, lib_path=lib_path, window_bits=4 if lib_path is not None else None)
        self.eng.set_generators(create_generators(curve, L + 1, lib_path), api_id(curve))
        self.eng.set_keyed_mixed_lengths(True)
        self.register(keys)

    @staticmethod
    def name(pk):
        return None if pk is None else tuple(map(tuple, pk))

    def register(self, pks):
        """Appends the keys that are not in the set yet (in one call); returns nothing: ``index`` has them afterwards.  A key
        the library refuses keeps its index -- its items get BBS_ST_UNKNOWN_KEY, as the keyed entry points decide them."""
        new, seen = [], set()
        for pk in pks:
            if self.name(pk) not in self.index and self.name(pk) not in seen:
                new.append(pk)
                seen.add(self.name(pk))
        if new:
            first, _ = self.eng.add_public_keys(new)
            for k, pk in enumerate(new):
                self.index[self.name(pk)] = first + k

    def key_octets(self, pk_obj) -> bytes:
        """The compressed string of a key for the job-local key sets (``register_keys=False``), remembered per key: what
        public_key_to_octets writes, if it decodes to the same key again; otherwise (coordinates that cannot be written, a point
        that is not on the twist: its string would name ANOTHER key) a string every decoder refuses, so that the items of such
        a key get BBS_ST_UNKNOWN_KEY as they do when the key is registered.  The engine's key set is not touched."""
        name = self.name(pk_obj.pk)
        o = self.octets.get(name)
        if o is None:
            try:
                o = public_key_to_octets(pk_obj)
                if self.name(octets_to_public_key(pk_obj.curve, o, pk_obj.lib_path, pk_obj.device).pk) != name:
                    raise BbsError(-41)
            except BbsError:
                o = b"\xff" * (2 * self.eng.fpb)
            self.octets[name] = o
        return o

    def keys_in_order(self):
        by_index = sorted(self.index.items(), key=lambda kv: kv[1])
        return [None if name is None else tuple(name) for name, _ in by_index]

    def register_secret(self, sks):
        """Appends the secret keys that are not in the signing set yet (in one call, bbs_ctx_add_secret_keys); ``sk_index`` has
        them afterwards.  The public half of a key gets the same index, so what was signed here verifies here without another
        registration.  A scalar the library refuses (>= r) keeps its index: its items get BBS_ST_UNKNOWN_KEY."""
        new = []
        for sk in sks:
            if sk not in self.sk_index and sk not in new:
                new.append(sk)
        if new:
            st, pks, first = self.eng.add_secret_keys(new)
            for k, sk in enumerate(new):
                self.sk_index[sk] = first + k
                if st[k] == 1:
                    self.index.setdefault(self.name(pks[k]), first + k)


_issuer_cache: Dict[tuple, _IssuerEngine] = {}
_bv_lock = threading.Lock()          # _many_issuers: one call at a time switches keyed batch verification on a cached engine


def _issuer_engine(curve, device, lib_path, L, pks) -> _IssuerEngine:
    """The cached keyed engine of (curve, device, lib_path), made for L messages or more, with ``pks`` registered.  A list that
    needs a larger L replaces the engine -- its keys are registered again, in their order -- as _mixed_engine replaces shorter
    engines."""
    who = (curve, device, lib_path)
    ie = _issuer_cache.get(who)
    if ie is None or ie.L < L:
        old = ie.keys_in_order() if ie is not None else []
        old_sks = sorted(ie.sk_index, key=ie.sk_index.get) if ie is not None else []
        if ie is not None:
            _issuer_cache.pop(who).eng.close()
        ie = _issuer_cache[who] = _IssuerEngine(curve, device, lib_path, L, old)
        ie.register_secret(old_sks)
    ie.register(pks)
    return ie


def sign_many_issuers(items: Sequence[tuple]) -> list:
    """SecretKey.sign for many items ``(sk, header, messages)`` of ANY issuers and ANY message counts, in ONE device call per
    (curve, device, lib_path): the cached engine of verify_many_issuers / proof_gen_many_issuers, whose signing key set grows by
    appending (a key is registered once per engine), through bbs_sign_wire_keyed_batch.  Entry i is the Signature
    ``items[i][0].sign(items[i][2], items[i][1])`` returns, or the BbsError it raises (returned, not raised: the other items
    stand).  One divergence: a secret key that is not below the group order is registered as a refused key, and its items get
    ``BbsError(-44)`` (BBS_ST_UNKNOWN_KEY), where the one-item form fails with a BbsRuntimeError from bbs_ctx_set_secret_key."""
    out: list = [None] * len(items)
    groups: Dict[tuple, List[int]] = {}
    for i, it in enumerate(items):
        groups.setdefault((it[0].curve, it[0].device, it[0].lib_path), []).append(i)
    for (curve, device, lib_path), idx in groups.items():
        its = [items[i] for i in idx]
        ie = _issuer_engine(curve, device, lib_path, max(len(it[2]) for it in its), [])
        ie.register_secret([it[0].sk for it in its])
        octs, st = ie.eng.sign_wire_keyed_batch([ie.sk_index[it[0].sk] for it in its], [list(it[2]) for it in its], [it[1] for it in its])
        for i, o, s in zip(idx, octs, st):
            out[i] = BbsError(int(s)) if s < 0 else octets_to_signature(curve, o, lib_path)
    return out


def _own_keys(ie: _IssuerEngine, its, key_cache=0):
    """register_keys=False: the distinct keys of ``its`` (entry 0 of an item) as compressed strings, in the order they are met,
    and the index of every item's key among them -- what the ``*_with_keys_*`` forms take.  Sets the capacity of the cached
    engine's job-local key cache where it differs from ``key_cache``."""
    if ie.eng.job_key_cache_report()["capacity"] != int(key_cache):
        ie.eng.set_job_key_cache(int(key_cache))
    local: Dict[object, int] = {}
    key_octets = []
    for it in its:
        if ie.name(it[0].pk) not in local:
            local[ie.name(it[0].pk)] = len(key_octets)
            key_octets.append(ie.key_octets(it[0]))
    return key_octets, [local[ie.name(it[0].pk)] for it in its]


def _many_issuers(items, count, to_octets, run, batch_verification=False, register_keys=True, run_own=None, key_cache=0):
    """Items of any issuers and counts: ONE device call per (curve, device, lib_path) through the wire keyed forms.
    register_keys=False: the keys are NOT registered on the cached engine -- the call deduplicates the keys of its items, writes
    them as octets and goes through the ``*_with_keys_*`` wire form (``run_own``): the job prepares them on the device and
    releases them, ``index`` and the engine's key set stay as they were.  key_cache (with register_keys=False only): the capacity
    of the cached engine's job-local key cache (Engine.set_job_key_cache), set when it differs from what the engine has.
    batch_verification: bbs_ctx_set_keyed_batch_verification on the cached engine for this call -- True: the library's default
    threshold; an integer >= 1: that many items per key -- with a fresh seed from the operating system, and off again
    afterwards.  Off is the state the cache keeps its engines in (nothing else holds them), so that is the prior state.  Calls
    that ask for it take ``_bv_lock`` in turn; a call WITHOUT it that runs on the same engine meanwhile may find the switch on,
    which changes how its items are decided, not what is decided."""
    min_items = 0 if batch_verification is True else int(batch_verification)
    if min_items < 0:
        raise ValueError("batch_verification: True, False or a number of items per key")
    out: list = [None] * len(items)
    groups: Dict[tuple, List[int]] = {}
    for i, it in enumerate(items):
        groups.setdefault((it[0].curve, it[0].device, it[0].lib_path), []).append(i)
    for (curve, device, lib_path), idx in groups.items():
        its = [items[i] for i in idx]
        ie = _issuer_engine(curve, device, lib_path, max(count(it) for it in its), [it[0].pk for it in its] if register_keys else [])
        if register_keys:
            call = lambda: _many(its, lambda obj: to_octets(curve, obj, lib_path),
                                 lambda octs, kept: run(ie.eng, [ie.index[ie.name(it[0].pk)] for it in kept], octs, kept), at=1)
        else:
            def own(octs, kept):
                key_octets, kidx = _own_keys(ie, kept, key_cache)
                return run_own(ie.eng, key_octets, kidx, octs, kept)
            call = lambda: _many(its, lambda obj: to_octets(curve, obj, lib_path), own, at=1)
        if batch_verification:
            with _bv_lock:
                ie.eng.set_keyed_batch_verification(True, None, min_items)
                try:
                    got = call()
                finally:
                    ie.eng.set_keyed_batch_verification(False)
        else:
            got = call()
        for i, g in zip(idx, got):
            out[i] = g
    return out


def verify_many_issuers(items: Sequence[tuple], batch_verification: bool = False, register_keys: bool = True, key_cache: int = 0) -> list:
    """PublicKey.verify for many items ``(pk, signature, header, messages)`` of ANY issuers and ANY message counts, in ONE
    device call per (curve, device, lib_path): one cached engine with bbs_ctx_set_keyed_mixed_lengths on, whose L is the
    largest count seen and whose key set grows by appending (a key is registered once).  Entry i is the boolean
    ``items[i][0].verify(*items[i][1:])`` returns, or the BbsError it raises (returned, not raised: the other items stand).
    One divergence: a ``pk`` the library refuses (not on the twist or outside the subgroup -- octets_to_public_key never returns
    one) is registered as a refused key, and its items get ``BbsError(-44)`` (BBS_ST_UNKNOWN_KEY), where the one-item form
    fails with a BbsRuntimeError from bbs_ctx_set_public_key.
    ``batch_verification=True`` switches bbs_ctx_set_keyed_batch_verification on for this call: the items of an issuer that
    has enough of them in the list (the library's default threshold; an integer >= 1 instead of True: that many) are checked by
    16 combined pairing products; the entries are the same.
    ``register_keys=False`` is for a verifier that does not know its issuers in advance: the keys of THIS list travel with the
    job (bbs_verify_wire_with_keys_batch), are prepared on the device by the job and released with it; the cached engine's key
    set does not grow.  The entries are the same.  Worth it for lists that bring many keys that will not be seen again; a
    handful of recurring issuers is served better by the default, which prepares a key once -- or by ``key_cache=N`` (with
    ``register_keys=False`` only): the cached engine keeps the prepared keys of these calls in N slots on the device
    (Engine.set_job_key_cache) and a later call prepares only the keys no slot holds.  The entries are the same."""
    return _many_issuers(items, lambda it: len(it[3]), signature_to_octets,
                         lambda eng, kidx, octs, its: eng.verify_wire_keyed_batch(kidx, octs, [list(it[3]) for it in its], [it[2] for it in its]),
                         batch_verification, register_keys,
                         lambda eng, keys, kidx, octs, its: eng.verify_wire_with_keys_batch(keys, kidx, octs, [list(it[3]) for it in its], [it[2] for it in its]),
                         key_cache)


def proof_verify_many_issuers(items: Sequence[tuple], batch_verification: bool = False, register_keys: bool = True, key_cache: int = 0) -> list:
    """proof_verify for many items ``(pk, proof, header, ph, disclosed_messages, disclosed_indexes)`` of any issuers and any
    message counts (commitments + disclosed indexes each), as verify_many_issuers (``batch_verification``, ``register_keys`` and
    ``key_cache`` included)."""
    return _many_issuers(items, lambda it: len(it[1].commitments) + len(it[5]), proof_to_octets,
                         lambda eng, kidx, octs, its: eng.proof_verify_wire_keyed_batch(
                             kidx, octs, [list(it[4]) for it in its], [list(it[5]) for it in its], [it[2] for it in its], [it[3] for it in its]),
                         batch_verification, register_keys,
                         lambda eng, keys, kidx, octs, its: eng.proof_verify_wire_with_keys_batch(
                             keys, kidx, octs, [list(it[4]) for it in its], [list(it[5]) for it in its], [it[2] for it in its], [it[3] for it in its]),
                         key_cache)


def proof_gen_many_issuers(items: Sequence[tuple], device_random: bool = False, register_keys: bool = True, key_cache: int = 0) -> list:
    """proof_gen for many items ``(pk, signature, header, ph, messages, disclosed_indexes[, random_scalars])`` of ANY issuers
    and ANY message counts, in ONE device call per (curve, device, lib_path): the cached engine of verify_many_issuers (its
    keys are registered once, whichever side meets them first), through bbs_proof_gen_wire_keyed_batch.  Entry i is the Proof
    ``proof_gen(*items[i])`` returns with the same random scalars (drawn here, as there, where an item has none), or the
    BbsError it raises (returned, not raised: the other items stand).  A signature that cannot be written as octets keeps the
    codec's error; a wrong number of random scalars in one item fails the whole call (BbsRuntimeError, BBS_E_ARG), as in
    proof_gen_many; a ``pk`` the library refuses gives ``BbsError(-44)``, the divergence verify_many_issuers describes.
    ``device_random=True``: as proof_gen_many -- when no item gives scalars of its own they are drawn on the device, from one
    fresh job seed per device call.
    ``register_keys=False`` is for a holder-side service that meets its issuer keys next to the credentials: the keys of THIS
    list travel with the job (bbs_proof_gen_wire_with_keys_batch), which prepares their domain midstates on the device and
    releases them; the cached engine's key set and ``index`` stay as they were.  ``key_cache=N`` (with ``register_keys=False``
    only): as verify_many_issuers -- the prepared keys stay in N slots of the cached engine, shared with the verify functions.
    The entries are the same."""
    out: list = [None] * len(items)
    on_device = device_random and not any(len(it) > 6 and it[6] is not None for it in items)
    groups: Dict[tuple, List[int]] = {}
    for i, it in enumerate(items):
        groups.setdefault((it[0].curve, it[0].device, it[0].lib_path), []).append(i)
    for (curve, device, lib_path), group in groups.items():
        ie = _issuer_engine(curve, device, lib_path, max(len(items[i][4]) for i in group), [items[i][0].pk for i in group] if register_keys else [])
        octs, idx = [], []
        for i in group:
            try:
                octs.append(signature_to_octets(curve, items[i][1], lib_path))
                idx.append(i)
            except BbsError as e:
                out[i] = e
        if not idx:
            continue
        its = [items[i] for i in idx]
        def call(r, ie=ie, its=its, octs=octs):
            rest = (octs, [list(it[4]) for it in its], [list(it[5]) for it in its], r, [it[2] for it in its], [it[3] for it in its])
            if register_keys:
                return ie.eng.proof_gen_wire_keyed_batch([ie.index[ie.name(it[0].pk)] for it in its], *rest)
            return ie.eng.proof_gen_wire_with_keys_batch(*_own_keys(ie, its, key_cache), *rest)
        if on_device:
            po, st = _device_draw(ie.eng, curve, call)
        else:
            po, st = call([list(it[6]) if len(it) > 6 and it[6] is not None else
                           calculate_random_scalars(curve, max(5 + len(it[4]) - len(it[5]), 0)) for it in its])
        for i, o, s in zip(idx, po, st):
            out[i] = BbsError(int(s)) if s < 0 else octets_to_proof(curve, o, lib_path)
    return out


# ---------------------------------------------------------------------------------- wire codec
def _curve_id(curve: str) -> int:
    return 0 if curve == "bls12_381" else 1


def _codec_check(rc: int, where: str):
    if rc == 0:
        return
    if rc in (-40, -41, -42):
        raise BbsError(rc)
    raise BbsRuntimeError(rc, where)


def _g1_rec(fpb, p) -> bytes:
    return bytes(2 * fpb) if p is None else int(p[0]).to_bytes(fpb, "little") + int(p[1]).to_bytes(fpb, "little")


def _g1_unrec(fpb, b):
    x, y = int.from_bytes(b[:fpb], "little"), int.from_bytes(b[fpb:2 * fpb], "little")
    return None if x == 0 and y == 0 else (x, y)


def signature_to_octets(curve: str, sig: Signature, lib_path: Optional[str] = None) -> bytes:
    """signature = compress(A) || I2OSP(e, 32)  (the byte string of src/tests/test_vector.rs:188-191)."""
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    rec = _bytes_arr(_g1_rec(fpb, sig.a) + int(sig.e).to_bytes(32, "little"))
    out = np.zeros(fpb + 32, dtype=np.uint8)
    _codec_check(lib.bbs_signature_to_octets(_curve_id(curve), _u8(rec), _u8(out)), "bbs_signature_to_octets")
    return out.tobytes()


def octets_to_signature(curve: str, octets: bytes, lib_path: Optional[str] = None) -> Signature:
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    if len(octets) != fpb + 32:
        raise BbsError(-42)
    rec = np.zeros(2 * fpb + 32, dtype=np.uint8)
    _codec_check(lib.bbs_signature_from_octets(_curve_id(curve), _u8(_bytes_arr(octets)), _u8(rec)), "bbs_signature_from_octets")
    b = rec.tobytes()
    return Signature(_g1_unrec(fpb, b), int.from_bytes(b[2 * fpb:], "little"))


def proof_to_octets(curve: str, proof: Proof, lib_path: Optional[str] = None) -> bytes:
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    pf = _bytes_arr(_g1_rec(fpb, proof.a_bar) + _g1_rec(fpb, proof.b_bar) + _g1_rec(fpb, proof.d)
                    + b"".join(int(x).to_bytes(32, "little") for x in (proof.e_cap, proof.r1_cap, proof.r3_cap, proof.challenge)))
    cm = _bytes_arr(b"".join(int(x).to_bytes(32, "little") for x in proof.commitments))
    out = np.zeros(3 * fpb + 32 * (4 + len(proof.commitments)), dtype=np.uint8)
    _codec_check(lib.bbs_proof_to_octets(_curve_id(curve), _u8(pf), _u8(cm), len(proof.commitments), _u8(out)), "bbs_proof_to_octets")
    return out.tobytes()


def octets_to_proof(curve: str, octets: bytes, lib_path: Optional[str] = None) -> Proof:
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    cap = max(len(octets) // 32, 1)
    pf = np.zeros(6 * fpb + 128, dtype=np.uint8)
    cm = np.zeros(cap * 32, dtype=np.uint8)
    n = ctypes.c_size_t(0)
    _codec_check(lib.bbs_proof_from_octets(_curve_id(curve), _u8(_bytes_arr(octets)), len(octets), _u8(pf), _u8(cm), cap,
                                           ctypes.byref(n)), "bbs_proof_from_octets")
    b, c = pf.tobytes(), cm.tobytes()
    pts = [_g1_unrec(fpb, b[k * 2 * fpb:(k + 1) * 2 * fpb]) for k in range(3)]
    sc = [int.from_bytes(b[6 * fpb + 32 * k:6 * fpb + 32 * (k + 1)], "little") for k in range(4)]
    return Proof(pts[0], pts[1], pts[2], sc[0], sc[1], sc[2],
                 [int.from_bytes(c[32 * k:32 * k + 32], "little") for k in range(n.value)], sc[3])


def public_key_to_octets(pk: PublicKey) -> bytes:
    lib = _lib.load_library(pk.lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(pk.curve)))
    out = np.zeros(2 * fpb, dtype=np.uint8)
    if pk.pk is None:
        rec, inf = _bytes_arr(bytes(4 * fpb)), 1
    else:
        (x0, x1), (y0, y1) = pk.pk
        rec, inf = _bytes_arr(b"".join(int(v).to_bytes(fpb, "little") for v in (x0, x1, y0, y1))), 0
    _codec_check(lib.bbs_public_key_to_octets(_curve_id(pk.curve), _u8(rec), inf, _u8(out)), "bbs_public_key_to_octets")
    return out.tobytes()


def octets_to_public_key(curve: str, octets: bytes, lib_path: Optional[str] = None, device: int = 0) -> PublicKey:
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    if len(octets) != 2 * fpb:
        raise BbsError(-42)
    rec = np.zeros(4 * fpb, dtype=np.uint8)
    inf = ctypes.c_int(0)
    _codec_check(lib.bbs_public_key_from_octets(_curve_id(curve), _u8(_bytes_arr(octets)), _u8(rec), ctypes.byref(inf)),
                 "bbs_public_key_from_octets")
    if inf.value:
        return PublicKey(curve, None, lib_path, device)
    b = rec.tobytes()
    f = [int.from_bytes(b[i * fpb:(i + 1) * fpb], "little") for i in range(4)]
    return PublicKey(curve, ((f[0], f[1]), (f[2], f[3])), lib_path, device)


def register_public_keys(curve: str, octets: Sequence[bytes], L: int = 0, lib_path: Optional[str] = None,
                         device: int = 0) -> Tuple[int, List[PublicKey]]:
    """Decode, check and register many issuer keys as they travel (compressed octets) in ONE call: they are appended to the key
    set of the (curve, L) engine (bbs_ctx_add_public_keys_octets), ready for the keyed verification entry points.  Returns
    ``(first_index, keys)``: keys[k] is what octets_to_public_key returns for octets[k] and has index first_index + k in the set.
    A refused key raises BbsError with the code octets_to_public_key raises for it (the first refused key's).  The call is one
    pass over the keys, so the set HAS GROWN by len(octets) entries when it raises -- the accepted keys are registered, a
    refused key occupies an index that no item can use -- and the exception carries ``first_index`` and ``statuses`` (one per
    key: 1, -40, -41).  Only a string of the wrong length (-42) is refused before anything is registered."""
    lib = _lib.load_library(lib_path)
    fpb = int(lib.bbs_fp_bytes(_curve_id(curve)))
    if any(len(o) != 2 * fpb for o in octets):
        raise BbsError(-42)
    eng = _engine(curve, L, device=device, lib_path=lib_path)
    first, st, keys = eng.add_public_keys_octets(list(octets))
    for code in st:
        if code != 1:
            e = BbsError(int(code))
            e.first_index, e.statuses = first, [int(x) for x in st]
            raise e
    return first, [PublicKey(curve, k, lib_path, device) for k in keys]
