"""Batched key generation (bbs_key_gen_batch, bbs_sk_to_pk_batch): the inputs, the references -- the library's own one-key
host functions and the oracle, each computed once per curve -- and the checks.  Shared by tests/test_keygen_hosttwin.py and
tests/test_keygen_gpu.py; ``lib_path`` is the host twin or None (the product library, on the GPU)."""
import ctypes
import os
import random
import subprocess

import numpy as np

from bbs_sign_amd import _lib, api
from bbs_sign_amd.engine import Engine, _bytes_arr, _u8, _u64
from oracle import bbs

import public_api_cases as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["bls12_381", "bn254"]
SIZES = [1, 64, 65, 129]          # one partial wavefront, one exact, a spill into the next, an odd third
N_MAX = 129
SHORT_AT, LONG_INFO_AT = 17, 63   # key_material of 31 bytes (-7); key_info of 65536 bytes (-8)
BOUNDARY_AT = {5: 0, 6: -1, 7: 1}     # the hashed string ends exactly on / one below / one above a multiple of 64
BIG_KM_AT, MAX_INFO_AT = 20, 30   # key_material of 1024 bytes; key_info of exactly 65535 bytes
KM_SHORT, KI_LONG, DST_LONG, NONCANONICAL = -7, -8, -23, -40
FILL = 0xEE                        # what the output arrays hold before a call: a word the call does not write shows


def key_dst(curve):
    return bbs.SUITES[curve].api_id + b"KEYGEN_DST_"


def _rand(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


_items = {}


def items(curve):
    """The 129 (key_material, key_info) pairs of a curve; a batch of n items is their first n."""
    if curve not in _items:
        rng = random.Random(1009)
        dst = key_dst(curve)
        kms = [_rand(rng, 32 + (k * 7) % 97) for k in range(N_MAX)]
        kis = [_rand(rng, (k * 13) % 131) for k in range(N_MAX)]
        # what is hashed: Z_pad(64) || km || I2OSP(len(ki), 2) || ki || I2OSP(48, 2) || 0 || dst || I2OSP(len(dst), 1)
        fixed = 64 + 32 + 2 + 3 + len(dst) + 1
        for k, delta in BOUNDARY_AT.items():
            kms[k] = _rand(rng, 32)
            kis[k] = _rand(rng, (delta - fixed) % 64 + 64)
            assert (fixed + len(kis[k]) - delta) % 64 == 0
        kms[BIG_KM_AT] = _rand(rng, 1024)
        kis[MAX_INFO_AT] = _rand(rng, 65535)
        kms[SHORT_AT] = _rand(rng, 31)
        kis[LONG_INFO_AT] = _rand(rng, 65536)
        _items[curve] = (kms, kis)
    return _items[curve]


def engine(curve, lib_path):
    """A bare context: no generators, no key."""
    return Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else None)


def _ragged(chunks, junk):
    """Ragged bytes whose offsets do not start at zero: `junk` bytes lie in front of the first item."""
    off = np.zeros(len(chunks) + 1, dtype=np.uint64)
    off[0] = junk
    for i, c in enumerate(chunks):
        off[i + 1] = off[i] + len(c)
    return _bytes_arr(b"\xa5" * junk + b"".join(chunks)), off


def raw_key_gen(eng, kms, kis, dst, pk=True):
    """bbs_key_gen_batch itself: (rc, sk bytes, records, octets, statuses), the outputs as the call left them."""
    n = len(kms)
    kb, ko = _ragged(kms, 5)
    ib, io = _ragged(kis, 3)
    d = _bytes_arr(dst)
    rec, ob = 4 * eng.fpb, 2 * eng.fpb
    sk = np.full(max(n, 1) * 32, FILL, dtype=np.uint8)
    pkb = np.full(max(n, 1) * rec, FILL, dtype=np.uint8)
    oc = np.full(max(n, 1) * ob, FILL, dtype=np.uint8)
    st = np.full(max(n, 1), 99, dtype=np.int8)
    rc = eng.lib.bbs_key_gen_batch(eng.h, n, _u8(kb), _u64(ko), _u8(ib), _u64(io), _u8(d), len(dst), _u8(sk),
                                   _u8(pkb) if pk else None, _u8(oc) if pk else None, st.ctypes.data_as(_lib.c_i8p))
    s, p, o = sk.tobytes(), pkb.tobytes(), oc.tobytes()
    return (rc, [s[32 * i:32 * (i + 1)] for i in range(n)], [p[rec * i:rec * (i + 1)] for i in range(n)],
            [o[ob * i:ob * (i + 1)] for i in range(n)], [int(x) for x in st[:n]])


def raw_sk_to_pk(eng, sks):
    n = len(sks)
    buf = _bytes_arr(b"".join(int(s).to_bytes(32, "little") for s in sks))
    rec, ob = 4 * eng.fpb, 2 * eng.fpb
    pkb = np.full(max(n, 1) * rec, FILL, dtype=np.uint8)
    oc = np.full(max(n, 1) * ob, FILL, dtype=np.uint8)
    ident = np.full(max(n, 1), 99, dtype=np.int8)
    st = np.full(max(n, 1), 99, dtype=np.int8)
    rc = eng.lib.bbs_sk_to_pk_batch(eng.h, n, _u8(buf), _u8(pkb), ident.ctypes.data_as(_lib.c_i8p), _u8(oc), st.ctypes.data_as(_lib.c_i8p))
    p, o = pkb.tobytes(), oc.tobytes()
    return (rc, [p[rec * i:rec * (i + 1)] for i in range(n)], [int(x) for x in ident[:n]], [o[ob * i:ob * (i + 1)] for i in range(n)],
            [int(x) for x in st[:n]])


def record(fpb, pk):
    if pk is None:
        return bytes(4 * fpb)
    (x0, x1), (y0, y1) = pk
    return b"".join(int(v).to_bytes(fpb, "little") for v in (x0, x1, y0, y1))


def host_one(curve, lib_path, scratch, km, ki, dst):
    """What a caller had before the batch call: bbs_key_gen, then bbs_ctx_set_secret_key + bbs_ctx_get_public_key on a scratch
    context, then bbs_public_key_to_octets.  (status, sk bytes, record, octets); zeros for a refused item."""
    lib = scratch.lib
    out = np.zeros(32, dtype=np.uint8)
    rc = lib.bbs_key_gen(scratch.curve, _u8(_bytes_arr(km)), len(km), _u8(_bytes_arr(ki)), len(ki), _u8(_bytes_arr(dst)), len(dst), _u8(out))
    if rc:
        return rc, bytes(32), bytes(4 * scratch.fpb), bytes(2 * scratch.fpb)
    sk = out.tobytes()
    scratch.set_secret_key(int.from_bytes(sk, "little"))
    pk = scratch.public_key()
    return 1, sk, record(scratch.fpb, pk), api.public_key_to_octets(api.PublicKey(curve, pk, lib_path))


_host, _oracle = {}, {}


def host_reference(curve, lib_path):
    """host_one of the 129 items, once per (curve, library)."""
    key = (curve, lib_path)
    if key not in _host:
        kms, kis = items(curve)
        scratch = engine(curve, lib_path)
        _host[key] = [host_one(curve, lib_path, scratch, kms[k], kis[k], key_dst(curve)) for k in range(N_MAX)]
        scratch.close()
        st = [h[0] for h in _host[key]]
        assert st == [KM_SHORT if k == SHORT_AT else KI_LONG if k == LONG_INFO_AT else 1 for k in range(N_MAX)]
    return _host[key]


def oracle_reference(curve):
    """(sk, pk) of every accepted item by oracle.bbs.key_gen / sk_to_pk, once per curve; None for the two refused items."""
    if curve not in _oracle:
        suite = bbs.SUITES[curve]
        kms, kis = items(curve)
        ref = []
        for k in range(N_MAX):
            if k in (SHORT_AT, LONG_INFO_AT):
                ref.append(None)
                continue
            sk = bbs.key_gen(suite, kms[k], kis[k], key_dst(curve))
            ref.append((sk, bbs.sk_to_pk(suite, sk)))
        _oracle[curve] = ref
    return _oracle[curve]


# ---------------------------------------------------------------------------------------------- a
def check_equals_host(curve, n, lib_path):
    kms, kis = items(curve)
    host, orc = host_reference(curve, lib_path), oracle_reference(curve)
    eng = engine(curve, lib_path)
    rc, sk, rec, octs, st = raw_key_gen(eng, kms[:n], kis[:n], key_dst(curve))
    assert rc == 0
    assert st == [h[0] for h in host[:n]]
    wrong = [k for k in range(n) if (sk[k], rec[k], octs[k]) != host[k][1:]]
    assert not wrong, (curve, n, wrong[:10])
    for k in range(n):
        if st[k] != 1:
            assert sk[k] == bytes(32) and rec[k] == bytes(4 * eng.fpb) and octs[k] == bytes(2 * eng.fpb), (curve, n, k)
        else:
            assert (int.from_bytes(sk[k], "little"), rec[k]) == (orc[k][0], record(eng.fpb, orc[k][1])), (curve, n, k, "oracle")
    # the secret keys alone (both pk outputs NULL: only the derive stage runs)
    rc, sk1, _, _, st1 = raw_key_gen(eng, kms[:n], kis[:n], key_dst(curve), pk=False)
    assert rc == 0 and st1 == st and sk1 == sk
    eng.close()


# ---------------------------------------------------------------------------------------------- b
def check_reference_vector(lib_path):
    """src/tests/test_vector.rs:139-160 as item 40 of 65 (BLS12-381); key_gen.rs:127-150 in two lanes (BN254)."""
    kms, kis = items("bls12_381")
    kms, kis = list(kms[:65]), [k[:40] for k in kis[:65]]
    kms[40], kis[40] = pa.IKM, pa.KEY_INFO
    eng = engine("bls12_381", lib_path)
    sks, pks, octs, st = eng.key_gen_batch(kms, kis, pa.KEY_DST)
    assert st[40] == 1 and list(st).count(1) == 64 and st[SHORT_AT] == KM_SHORT
    assert int(sks[40]).to_bytes(32, "big").hex() == "60e55110f76883a13d030b2f6bd11883422d5abde717569fc0731f51237169fc"
    assert octs[40].hex() == ("a820f230f6ae38503b86c70dc50b61c58a77e45c39ab25c0652bbaa8fa136f2851bd4781c9dcde39fc9d1d52c9e60268"
                              "061e7d7632171d91aa8d460acee0e96f1e7c4cfb12d3ff9ab5d5dc91c277db75c845d649ef3c4f63aebc364cd55ded0c")
    assert octs[40] == bbs.g2_compress(bbs.BLS_SUITE.curve, pks[40])
    eng.close()
    suite = bbs.BN_SUITE
    kms, kis = items("bn254")
    kms, kis = list(kms[:65]), [b""] * 65
    dst = b"BBS-SIG-KEYGEN-SALT-"
    kms[3] = kms[64] = bytes([1] * 32)
    eng = engine("bn254", lib_path)
    sks, pks, octs, st = eng.key_gen_batch(kms, kis, dst)
    want = bbs.key_gen(suite, bytes([1] * 32), b"", dst)
    assert st[3] == st[64] == 1 and sks[3] == sks[64] == want
    assert pks[3] == pks[64] == bbs.sk_to_pk(suite, want)
    assert octs[3] == octs[64] == bbs.g2_compress(suite.curve, pks[3])
    assert sks[2] != want and sks[4] != want
    eng.close()


# ---------------------------------------------------------------------------------------------- c
def check_dst_length(curve, lib_path):
    kms, kis = items(curve)
    kms, kis = kms[:65], kis[:65]
    eng, scratch = engine(curve, lib_path), engine(curve, lib_path)
    dst = bytes((7 * i + 1) & 0xff for i in range(255))
    rc, sk, rec, octs, st = raw_key_gen(eng, kms, kis, dst)
    assert rc == 0
    for k in range(65):
        assert (st[k], sk[k], rec[k], octs[k]) == host_one(curve, lib_path, scratch, kms[k], kis[k], dst), (curve, k)
    dst += b"\x01"
    rc, sk, rec, octs, st = raw_key_gen(eng, kms, kis, dst)
    assert rc == 0
    assert st == [KM_SHORT if k == SHORT_AT else KI_LONG if k == LONG_INFO_AT else DST_LONG for k in range(65)]
    assert st == [host_one(curve, lib_path, scratch, kms[k], kis[k], dst)[0] for k in range(65)]
    assert all(s == bytes(32) for s in sk) and all(r == bytes(4 * eng.fpb) for r in rec) and all(o == bytes(2 * eng.fpb) for o in octs)
    eng.close()
    scratch.close()


# ---------------------------------------------------------------------------------------------- d
WB = 8                             # the comb's window (stages_kg.hpp KG_WB): the edge scalars below are stated for it


def edge_scalars(curve):
    """65 scalars: the edges of the comb (8-bit windows, 32 of them) at fixed places among random ones.  {position: scalar}, list."""
    r = bbs.SUITES[curve].curve.r
    top_shift = 256 - WB
    top = r >> top_shift
    low_f = (top << top_shift) | ((1 << top_shift) - 1)      # the largest value below r whose low 31 digits are all 0xFF
    if low_f >= r:
        low_f -= 1 << top_shift
    edges = {0: 0, 1: 1, 2: 2, 9: r - 1, 17: r, 31: (1 << 256) - 1, 40: low_f, 41: top << top_shift, 63: r - 2, 64: 3}
    for i, w in enumerate((1, 256 // WB // 2 - 1, 256 // WB - 1)):      # the second window, the last of the scalar's low half, the top one
        edges[50 + i] = 1 << (WB * w)
        edges[54 + i] = ((1 << WB) - 1) << (WB * w)
    rng = random.Random(77)
    sc = [rng.randrange(1, r) for _ in range(65)]
    for k, v in edges.items():
        sc[k] = v
    assert low_f < r and (low_f & ((1 << top_shift) - 1)) == (1 << top_shift) - 1 and low_f + (1 << top_shift) >= r
    assert edges[52] < r <= edges[56] < 1 << 256
    return edges, sc


def check_sk_to_pk_edges(curve, lib_path):
    c = bbs.SUITES[curve].curve
    edges, sc = edge_scalars(curve)
    eng = engine(curve, lib_path)
    rc, rec, ident, octs, st = raw_sk_to_pk(eng, sc)
    assert rc == 0
    for k, s in enumerate(sc):
        if s >= c.r:
            assert (st[k], ident[k], rec[k], octs[k]) == (NONCANONICAL, 0, bytes(4 * eng.fpb), bytes(2 * eng.fpb)), (curve, k)
            continue
        q = c.g2_mul(c.g2, s)
        assert (q is None) == (s == 0)
        assert (st[k], ident[k], rec[k], octs[k]) == (1, int(s == 0), record(eng.fpb, q), bbs.g2_compress(c, q)), (curve, k, hex(s))
    # 255 * 2^248 is above r on both curves: refused like every other scalar >= r
    assert st[56] == NONCANONICAL and st[17] == st[31] == NONCANONICAL and st[0] == 1 and ident[0] == 1
    pks, octs2, st2 = eng.sk_to_pk_batch(sc)
    assert list(st2) == st and octs2 == [o if s == 1 else None for o, s in zip(octs, st)]
    assert pks[0] is None and pks[17] is None and pks[1] == c.g2
    eng.close()


# ---------------------------------------------------------------------------------------------- e
def check_public_wrappers(curve, lib_path):
    kms = [bytes([40 + k] * (32 + k)) for k in range(4)]
    kis = [b"", b"tenant-1", b"", b"x" * 9]
    kms[1] = bytes(31)                      # InvalidKeyMaterialLength
    kis[2] = bytes(65536)                   # InvalidKeyInfoLength
    dst = key_dst(curve)
    got = api.key_gen_batch(curve, kms, kis, dst, lib_path=lib_path)
    assert len(got) == 4
    pairs = []
    for k in range(4):
        try:
            sk = api.SecretKey.key_gen(curve, kms[k], kis[k], dst, lib_path)
        except api.BbsError as e:
            assert isinstance(got[k], api.BbsError) and (got[k].status, got[k].variant) == (e.status, e.variant), (curve, k)
            continue
        assert isinstance(got[k], tuple) and got[k][0].sk == sk.sk and got[k][1].pk == sk.sk_to_pk().pk, (curve, k)
        pairs.append(got[k])
    assert [type(g) for g in got] == [tuple, api.BbsError, api.BbsError, tuple]
    assert (got[1].variant, got[2].variant) == ("InvalidKeyMaterialLength", "InvalidKeyInfoLength")
    assert [p.pk for p in api.sk_to_pk_batch([s for s, _ in pairs])] == [p.pk for _, p in pairs]
    for sk, pk in pairs:
        sig = sk.sign([b"one message"], b"header")
        assert pk.verify(sig, b"header", [b"one message"]) is True
        assert pk.verify(sig, b"header", [b"another"]) is False
    octs = [api.public_key_to_octets(pk) for _, pk in pairs]
    _, keys = api.register_public_keys(curve, octs, L=1, lib_path=lib_path)
    assert [k.pk for k in keys] == [pk.pk for _, pk in pairs]


# ---------------------------------------------------------------------------------------------- f
def check_arguments(curve, lib_path):
    import keyed_cases as kc
    E_ARG = -100
    bare = engine(curve, lib_path)          # no generators: both calls work on it (every check above used one as well)
    lib, h = bare.lib, bare.h
    km, off = _bytes_arr(bytes(range(32))), np.array([0, 32], dtype=np.uint64)
    zoff = np.array([0, 0], dtype=np.uint64)
    dst = _bytes_arr(b"dst")
    sk, pk, oc = np.zeros(32, dtype=np.uint8), np.zeros(4 * bare.fpb, dtype=np.uint8), np.zeros(2 * bare.fpb, dtype=np.uint8)
    st, ident = np.zeros(1, dtype=np.int8), np.zeros(1, dtype=np.int8)
    i8 = lambda a: a.ctypes.data_as(_lib.c_i8p)
    kg = lib.bbs_key_gen_batch
    assert kg(h, 1, _u8(km), _u64(off), None, None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == 0 and st[0] == 1
    assert kg(h, 1, _u8(km), _u64(off), None, _u64(zoff), _u8(dst), 3, _u8(sk), None, None, i8(st)) == 0 and st[0] == 1
    assert kg(None, 1, _u8(km), _u64(off), None, None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG
    assert kg(h, 1, None, _u64(off), None, None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG
    assert kg(h, 1, _u8(km), None, None, None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG
    assert kg(h, 1, _u8(km), _u64(off), _u8(km), None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG      # key_info without offsets
    assert kg(h, 1, _u8(km), _u64(off), None, _u64(off), _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG    # lengths without key_info
    assert kg(h, 1, _u8(km), _u64(off), None, None, None, 3, _u8(sk), _u8(pk), _u8(oc), i8(st)) == E_ARG
    assert kg(h, 1, _u8(km), _u64(off), None, None, _u8(dst), 3, None, _u8(pk), _u8(oc), i8(st)) == E_ARG
    assert kg(h, 1, _u8(km), _u64(off), None, None, _u8(dst), 3, _u8(sk), _u8(pk), _u8(oc), None) == E_ARG
    assert kg(h, 0, None, None, None, None, None, 0, None, None, None, None) == 0
    sp = lib.bbs_sk_to_pk_batch
    one = _bytes_arr((5).to_bytes(32, "little"))
    assert sp(h, 1, _u8(one), _u8(pk), i8(ident), _u8(oc), i8(st)) == 0 and st[0] == 1 and ident[0] == 0
    assert sp(h, 1, _u8(one), None, None, _u8(oc), i8(st)) == 0 and sp(h, 1, _u8(one), _u8(pk), None, None, i8(st)) == 0
    assert sp(None, 1, _u8(one), _u8(pk), i8(ident), _u8(oc), i8(st)) == E_ARG
    assert sp(h, 1, None, _u8(pk), i8(ident), _u8(oc), i8(st)) == E_ARG
    assert sp(h, 1, _u8(one), None, i8(ident), None, i8(st)) == E_ARG
    assert sp(h, 1, _u8(one), _u8(pk), i8(ident), _u8(oc), None) == E_ARG
    assert sp(h, 0, None, None, None, None, None) == 0
    assert bare.key_gen_batch([], [], b"dst")[0] == [] and bare.sk_to_pk_batch([])[0] == []
    bare.close()
    # a context with generators, a secret key and a key set keeps all three
    iss = kc.Issuers(curve, 2, 2, lib_path, seed=13)
    eng = kc.make_engine(curve, iss.gens, iss.api_id, lib_path, sk=iss.sks[0])
    eng.set_public_keys([iss.pks[0], None, iss.pks[1]])
    before = (eng.public_key(), eng.public_key_count())
    sks, pks, _, st = eng.key_gen_batch([bytes(range(40)), bytes(31)], [b"", b""], b"dst")
    assert list(st) == [1, KM_SHORT] and pks[0] == bbs.sk_to_pk(iss.suite, sks[0])
    assert eng.sk_to_pk_batch([iss.sks[1]])[0] == [iss.pks[1]]
    assert (eng.public_key(), eng.public_key_count()) == before == (iss.pks[0], 3)
    eng.close()


# ---------------------------------------------------------------------------------------------- g
def check_cpp_wrapper(lib, exe_name):
    src = os.path.join(ROOT, "tests", "cpp", "keygen_batch.cpp")
    exe = os.path.join(ROOT, "bbs_sign_amd", "build", exe_name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    libdir, libname = os.path.dirname(lib), os.path.basename(lib)
    cmd = ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-o", exe, "-L", libdir, "-l:" + libname,
           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L", "/opt/rocm/lib", "-lpthread"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-3000:]
