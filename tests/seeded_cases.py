"""Seeded random scalars drawn on the device (bbs_ctx_set_seeded_random_scalars, bbs_seeded_random_scalars_batch).  Shared by
the host-twin tier (tests/test_seeded_hosttwin.py) and the GPU tier (tests/test_seeded_gpu.py).

The rule that defines correctness: with the switch on, item i's random scalars are the reference's
seeded_random_scalars(seed_i, dst, 5 + l_i - r_i) (src/utils/core_utilities.rs:84-100), seed_i being the item's own bytes or
job_seed || I2OSP(i, 8), and its status and output bytes are those of the switch-off call that is given those scalars -- but
for -24 and -23, which the reference's draw raises after -2 / -3 and before every other code of core_proof_gen.

Expected values: the pure-Python oracle's seeded_random_scalars for every draw, the plain-C restatement of the oracle's
core_proof_gen for every proof (a sample through the pure-Python oracle), the reference's own vectors, and as second witness
the same library with the switch off and the oracle's scalars uploaded.  Everything is compared as octet strings, b"" for an
item that failed."""
import random

import numpy as np
import pytest

from keyed_cases import UNKNOWN_KEY
from keyed_gen_cases import run_keyed, want_keyed
from keyed_mixed_cases import KItems, Ring
from mixed_gen_cases import producer, proof_octets, run_proof, same_bytes, want_proof
from mixed_len_cases import Items, World, sig_octets
from oracle import bbs
from parity_cases import make_engine

EXPORTS = ("bbs_ctx_set_seeded_random_scalars", "bbs_seeded_random_scalars_batch")
E_ARG, DST_TOO_LONG, ELL_TOO_BIG = -100, -23, -24
H = bytes.fromhex
# src/utils/core_utilities.rs:103-113 (the draft's fixture: seed and DST of mocked_calculate_random_scalars)
MOCK_SEED = H("332e313431353932363533353839373933323338343632363433333833323739")
MOCK_DST = b"BBS_BLS12381G1_XMD:SHA-256_SSWU_RO_H2G_HM2S_MOCK_RANDOM_SCALARS_DST_"
# src/tests/test_vector.rs:199-260
KAT_PK = H("a820f230f6ae38503b86c70dc50b61c58a77e45c39ab25c0652bbaa8fa136f2851bd4781c9dcde39fc9d1d52c9e60268"
           "061e7d7632171d91aa8d460acee0e96f1e7c4cfb12d3ff9ab5d5dc91c277db75c845d649ef3c4f63aebc364cd55ded0c")
KAT_M1 = H("9872ad089e452c7b6e283dfac2a80d58e8d0ff71cc4d5e310a1debdda4a45f02")
KAT_HEADER = H("11223344556677889900aabbccddeeff")
KAT_PH = H("bed231d880675ed101ead304512e043ade9958dd0241ea70b4b3957fba941501")
KAT_SIG = H("84773160b824e194073a57493dac1a20b667af70cd2352d8af241c77658da5253aa8458317cca0eae615690d55b1f271"
            "64657dcafee1d5c1973947aa70e2cfbb4c892340be5969920d0916067b4565a0")
KAT_PROOF = ("94916292a7a6bade28456c601d3af33fcf39278d6594b467e128a3f83686a104ef2b2fcf72df0215eeaf69262ffe8194a19fab31a82ddbe06908985abc4c"
             "9825788b8a1610942d12b7f5debbea8985296361206dbace7af0cc834c80f33e0aadaeea5597befbb651827b5eed5a66f1a959bb46cfd5ca1a817a1447"
             "5960f69b32c54db7587b5ee3ab665fbd37b506830a49f21d592f5e634f47cee05a025a2f8f94e73a6c15f02301d1178a92873b6e8634bafe4983c3e15a"
             "663d64080678dbf29417519b78af042be2b3e1c4d08b8d520ffab008cbaaca5671a15b22c239b38e940cfeaa5e72104576a9ec4a6fad78c532381aeaa6"
             "fb56409cef56ee5c140d455feeb04426193c57086c9b6d397d9418")


def dst_of(w):
    return w.api_id + b"SEEDED_RANDOM_SCALARS_"


def seeds_for(n, salt=0):
    """Per-item seeds of varied length, the empty seed among them."""
    return [bytes((salt + 7 * i + k) % 256 for k in range((5 * i + salt) % 41)) for i in range(n)]


def job_seeds(job_seed, n):
    return [job_seed + i.to_bytes(8, "big") for i in range(n)]


def draws(suite, lengths, disclosed, seeds, dst):
    """What the device is to draw for every item (r counted before deduplication); [] where nothing is drawn."""
    out = []
    for l, d, s in zip(lengths, disclosed, seeds):
        c = 5 + l - len(d)
        out.append(bbs.seeded_random_scalars(suite, s, dst, c) if len(d) <= l and all(j < l for j in d) and c <= 170 else [])
    return out


def run_any(eng, it, X, form="core", how="batch", key_index=None):
    """A list through one export: X is the list of per-item seeds (or, with the switch off, of rows of scalars) or the job
    seed.  Every export ends as (octet strings, statuses)."""
    S, M, D, Hd, P = it.sigs, it.msgs, it.disclosed, it.headers, it.phs

    def done(job, octets=False):
        if how == "upload":
            job.run()
            out = job.proofs()
        else:
            job.wait()
            out = job.output()
        job.free()
        return out if octets else (proof_octets(eng, out[0]), out[1])
    if key_index is not None:
        ki = np.asarray(key_index, dtype=np.uint32)
        if form == "wire":
            octs = [sig_octets(it.w, s) for s in S]
            if how == "submit":
                return done(eng.proof_gen_wire_keyed_submit(ki, octs, it.raw, D, X, Hd, P), True)
            return eng.proof_gen_wire_keyed_batch(ki, octs, it.raw, D, X, Hd, P)
        if how == "submit":
            return done(eng.core_proof_gen_keyed_submit(ki, S, M, D, X, Hd, P))
        proofs, st = eng.core_proof_gen_keyed_batch(ki, S, M, D, X, Hd, P)
        return proof_octets(eng, proofs), st
    if form == "wire":
        return eng.proof_gen_wire_batch([sig_octets(it.w, s) for s in S], it.raw, D, X, Hd, P)
    if form == "octets":
        if how == "submit":
            return done(eng.proof_gen_octets_submit(S, M, D, X, Hd, P), True)
        return eng.proof_gen_octets_batch(S, M, D, X, Hd, P)
    if how == "upload":
        return done(eng.core_proof_gen_upload(S, M, D, X, Hd, P))
    if how == "submit":
        return done(eng.core_proof_gen_submit(S, M, D, X, Hd, P))
    proofs, st = eng.core_proof_gen_batch(S, M, D, X, Hd, P)
    return proof_octets(eng, proofs), st


ROUTES = (("core", "batch"), ("core", "upload"), ("core", "submit"), ("octets", "batch"), ("octets", "submit"), ("wire", "batch"))


# ---- case 0: the exports ----------------------------------------------------------------------------------------------------
def check_export(lib_path=None):
    from bbs_sign_amd import Engine, _lib, api
    import inspect
    lib = _lib.load_library(lib_path)
    for name in EXPORTS:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.bbs_ctx_set_seeded_random_scalars(None, 1, None, 0) == E_ARG
    assert callable(Engine.set_seeded_random_scalars) and callable(Engine.seeded_random_scalars_batch)
    for f in (api.proof_gen_many, api.proof_gen_many_issuers):
        assert inspect.signature(f).parameters["device_random"].default is False


# ---- case 1: the reference's vectors ----------------------------------------------------------------------------------------
def check_reference_vectors(lib_path=None, L=5):
    """test_vector.rs:86-97 through the primitive, and the proof of :199-260 from the mock seed as a per-item seed: the wire form,
    the core form and one keyed export, on a context made for L messages with mixed lengths on (the vector has one)."""
    from bbs_sign_amd import api
    curve = "bls12_381"
    S = bbs.BLS_SUITE
    gens = api.create_generators(curve, L + 1, lib_path)
    pk = api.octets_to_public_key(curve, KAT_PK, lib_path)
    eng = make_engine(curve, gens, S.api_id, lib_path, pk=pk.pk)
    rows, st = eng.seeded_random_scalars_batch([MOCK_SEED], [10], MOCK_DST)
    assert list(st) == [1]
    assert bbs.scalar_be(S.curve, rows[0][0]).hex() == "04f8e2518993c4383957ad14eb13a023c4ad0c67d01ec86eeb902e732ed6df3f"
    assert bbs.scalar_be(S.curve, rows[0][9]).hex() == "485e2adab17b76f5334c95bf36c03ccf91cef77dcfcdc6b8a69e2090b3156663"
    assert rows[0] == bbs.mocked_calculate_random_scalars(S, 10)
    eng.set_mixed_lengths_gen(True)
    eng.set_seeded_random_scalars(True, MOCK_DST)
    po, st = eng.proof_gen_wire_batch([KAT_SIG, KAT_SIG], [[KAT_M1]] * 2, [[0]] * 2, [MOCK_SEED, MOCK_SEED + b"x"], [KAT_HEADER] * 2, [KAT_PH] * 2)
    assert list(st) == [1, 1] and po[0].hex() == KAT_PROOF and po[1] and po[1].hex() != KAT_PROOF
    msg = eng.hash_to_scalar_batch([KAT_M1], S.api_id + b"MAP_MSG_TO_SCALAR_AS_HASH_")
    s = eng.signatures_from_octets_batch([KAT_SIG])[0][0]
    proofs, st = eng.core_proof_gen_batch([s], [[msg[0]]], [[0]], [MOCK_SEED], [KAT_HEADER], [KAT_PH])
    assert list(st) == [1] and eng.proofs_to_octets_batch(proofs)[0].hex() == KAT_PROOF
    eng.close()
    eng = make_engine(curve, gens, S.api_id, lib_path)
    eng.set_keyed_mixed_lengths(True)
    assert list(eng.set_public_keys([bbs.sk_to_pk(S, 12345), pk.pk])) == [1, 1]
    eng.set_seeded_random_scalars(True, MOCK_DST)
    po, st = eng.proof_gen_wire_keyed_batch([1, 0, 9], [KAT_SIG] * 3, [[KAT_M1]] * 3, [[0]] * 3, [MOCK_SEED] * 3, [KAT_HEADER] * 3, [KAT_PH] * 3)
    assert list(st) == [1, 1, UNKNOWN_KEY] and po[0].hex() == KAT_PROOF and po[1] and po[1].hex() != KAT_PROOF and po[2] == b""
    eng.close()


# ---- case 2: the chain's edges, through the primitive -------------------------------------------------------------------------
def check_chain_edges(curve, lib_path=None):
    """Independent sweeps, every item against the oracle: counts (odd ones leave the last block half used; 170 is ell = 255, 171
    is refused), seed lengths 0 .. 130 (every padding residue of b_0 twice), DST lengths on both sides of the padding boundaries
    of b_i's 34 + D bytes (D = 21 / 22, 85 / 86), 255 and 256 (refused)."""
    suite = bbs.SUITES[curve]
    eng = make_engine(curve, bbs.synthetic_generators(suite, 2, b"seeded-chain-edges"), suite.api_id, lib_path)
    dst = dst_of(suite)
    seeds = [b"count-%d" % c for c in (1, 2, 5, 6, 9, 10, 170, 171)] + [bytes((3 * k + n) % 256 for k in range(n)) for n in range(131)]
    counts = [1, 2, 5, 6, 9, 10, 170, 171] + [3 + n % 2 for n in range(131)]
    rows, st = eng.seeded_random_scalars_batch(seeds, counts, dst)
    assert [int(x) for x in st] == [ELL_TOO_BIG if c > 170 else 1 for c in counts]
    for i, (s, c) in enumerate(zip(seeds, counts)):
        assert rows[i] == (bbs.seeded_random_scalars(suite, s, dst, c) if c <= 170 else []), (curve, "item", i, c, len(s))
    total = 0
    for D in (0, 1, 21, 22, 23, 29, 30, 85, 86, 255, 256):
        d = bytes((11 * D + k) % 256 for k in range(D))
        sd, cn = [b"", b"dst-%d" % D, bytes(range(64))], [1, 2, 5]
        rows, st = eng.seeded_random_scalars_batch(sd, cn, d)
        if D > 255:
            assert [int(x) for x in st] == [DST_TOO_LONG] * 3 and rows == [[], [], []]
            rows, st = eng.seeded_random_scalars_batch(sd, [1, 171, 5], d)        # ell is looked at first (utilities_helper.rs:46-52)
            assert [int(x) for x in st] == [DST_TOO_LONG, ELL_TOO_BIG, DST_TOO_LONG]
            continue
        assert [int(x) for x in st] == [1] * 3
        assert rows == [bbs.seeded_random_scalars(suite, s, d, c) for s, c in zip(sd, cn)], (curve, "dst length", D)
        total += 3
    assert len(seeds) + total < 600
    eng.close()


# ---- case 3 and 4: every proof_gen form, per-item seeds and the job seed ----------------------------------------------------------
def check_every_form(curve, lib_path=None, n=130, L=5, mixed=False, routes=ROUTES, python_sample=()):
    """U_i = 0 .. 5 (fixed lengths) or l_i = 0 .. 5 (mixed), headers, ph and seeds of varied length, through every export and
    form of the single-key context: per-item seeds, then the same list under a job seed."""
    w = World(curve, lib_path, L)
    rng = random.Random(11)
    if mixed:
        it = Items(w, [i % (L + 1) for i in range(n)])
        assert set(it.lengths) == set(range(L + 1))
    else:
        it = Items(w, [L] * n, disclosed=[sorted(rng.sample(range(L), L - i % (L + 1))) for i in range(n)])
        assert {L - len(d) for d in it.disclosed} == set(range(L + 1))
    dst = dst_of(w)
    eng = producer(w, on=mixed)
    seeds = seeds_for(n)
    assert b"" in seeds and len({len(s) for s in seeds}) > 20
    js = bytes(range(100, 132))
    for what, X, per_item in (("per-item seeds", seeds, seeds), ("job seed", js, job_seeds(js, n))):
        rnds = draws(w.suite, it.lengths, it.disclosed, per_item, dst)
        want = [want_proof(it, i, rnds, eng) for i in range(n)]
        want = ([o for _, o in want], [s for s, _ in want])
        assert want[1] == [1] * n
        for i in python_sample:
            assert want_proof(it, i, rnds, eng, python=True) == (1, want[0][i]), (curve, "python oracle", i)
        # the same engine with the switch off and those scalars uploaded
        same_bytes(run_proof(eng, it, rnds, "core"), want, (curve, what, "switch off, scalars uploaded"))
        eng.set_seeded_random_scalars(True, dst)
        for form, how in routes:
            same_bytes(run_any(eng, it, X, form, how), want, (curve, what, form, how, "mixed" if mixed else "fixed"))
        eng.set_seeded_random_scalars(False)
    # two job seeds: every item differs; the same seed: the same bytes
    eng.set_seeded_random_scalars(True, dst)
    a, b, c = (run_any(eng, it, s, "wire") for s in (js, bytes(range(101, 133)), js))
    assert list(a[1]) == list(b[1]) == [1] * n and all(x != y for x, y in zip(a[0], b[0])) and a[0] == c[0]
    same_bytes(a, want, (curve, "job seed again"))
    eng.close()


def check_every_form_keyed(curve, lib_path=None, n=130, L=5, K=3, mixed=True, exports=(("core", False), ("core", True), ("wire", False), ("wire", True))):
    ring = Ring(curve, lib_path, L, K)
    owner = [i % K for i in range(n)]
    it = KItems(ring, owner, [i % (L + 1) for i in range(n)] if mixed else [L] * n)
    key_index = list(owner)
    unknown = (0, n - 1) if n < 66 else (0, 63, 64, n - 1)
    for p in unknown:
        key_index[p] = len(ring.keys) + 3
    dst = dst_of(ring.worlds[0])
    eng = ring.engine(on=mixed)
    seeds = seeds_for(n, 9)
    js = bytes(range(7, 39))
    for what, X, per_item in (("per-item seeds", seeds, seeds), ("job seed", js, job_seeds(js, n))):
        rnds = draws(ring.worlds[0].suite, it.lengths, it.disclosed, per_item, dst)
        want = want_keyed(ring, it, key_index, rnds, eng, L)
        assert all(s == (UNKNOWN_KEY if i in unknown else 1) for i, s in enumerate(want[1]))
        same_bytes(run_keyed(eng, it, rnds, key_index), want, (curve, "keyed", what, "switch off, scalars uploaded"))
        eng.set_seeded_random_scalars(True, dst)
        for form, submit in exports:
            got = run_any(eng, it, X, form, "submit" if submit else "batch", key_index)
            same_bytes(got, want, (curve, "keyed", what, form, submit, mixed))
        eng.set_seeded_random_scalars(False)
    eng.close()


# ---- case 5: the order of the codes -----------------------------------------------------------------------------------------
def check_order_of_codes(curve, lib_path=None, L=5):
    """-2 and -3 come before the draw (their seed, the empty one, is not read); -24 and -23 come from the draw, before
    proof_init's -1; an unknown key overrides all of them."""
    w = World(curve, lib_path, L)
    it = Items(w, [L] * 6, disclosed=[[0, 1], [], [], [], [], [2]])
    it.disclosed[1], it.disclosed[2] = [0, 1, 2, 3, 4, 4], [5]
    r = w.c.r
    it.msgs[3] = [(7 * j + 1) % r for j in range(166)]          # l = 166, r = 0: 171 scalars, ell = 257
    it.msgs[4] = it.msgs[4][:3]                                  # l = 3 on a context of 5
    seeds = [b"s0", b"", b"", b"s3", b"s4", b"s5"]
    dst = dst_of(w)
    rnds = draws(w.suite, [len(m) for m in it.msgs], it.disclosed, seeds, dst)
    eng = producer(w, on=False)
    p0, p5 = want_proof(it, 0, rnds, eng)[1], want_proof(it, 5, rnds, eng)[1]
    eng.set_seeded_random_scalars(True, dst)
    for form in ("core", "octets"):
        same_bytes(run_proof(eng, it, seeds, form), ([p0, b"", b"", b"", b"", p5], [1, -2, -3, ELL_TOO_BIG, -1, 1]), (curve, form, "codes"))
    eng.set_seeded_random_scalars(True, bytes(256))
    for form in ("core", "octets"):
        same_bytes(run_proof(eng, it, seeds, form), ([b""] * 6, [DST_TOO_LONG, -2, -3, ELL_TOO_BIG, DST_TOO_LONG, DST_TOO_LONG]), (curve, form, "long dst"))
    eng.close()
    # the wire form: a signature that does not decode keeps its code, whatever its seed would have drawn
    it2 = Items(w, [L] * 3, disclosed=[[0], [1], []])
    it2.disclosed[2] = [0, 1, 2, 3, 4, 4]
    octs = [sig_octets(w, s) for s in it2.sigs]
    octs[1] = octs[1][:-32] + bytes(32)                          # e = 0
    s2 = [b"a", b"", b""]
    rn2 = draws(w.suite, it2.lengths, it2.disclosed, s2, dst)
    eng = producer(w, on=False)
    eng.set_seeded_random_scalars(True, bytes(256))
    po, st = eng.proof_gen_wire_batch(octs, it2.raw, it2.disclosed, s2, it2.headers, it2.phs)
    assert list(st) == [DST_TOO_LONG, -42, -2]
    eng.set_seeded_random_scalars(True, dst)
    po, st = eng.proof_gen_wire_batch(octs, it2.raw, it2.disclosed, s2, it2.headers, it2.phs)
    assert list(st) == [1, -42, -2] and po[0] == want_proof(it2, 0, rn2, eng)[1] and po[1] == po[2] == b""
    eng.close()
    # keyed: the same lists under a key that is not there
    ring = Ring(curve, lib_path, L, 2)
    kit = KItems(ring, [0] * 6, [L] * 6, disclosed=[[0, 1], [], [], [], [], [2]])
    kit.disclosed = [list(d) for d in it.disclosed]
    kit.msgs[3], kit.msgs[4] = it.msgs[3], kit.msgs[4][:3]
    for on in (False, True):
        e = ring.engine(on=on)
        for d, codes in ((dst, [1, -2, -3, ELL_TOO_BIG, 1 if on else -1, 1]), (bytes(256), [DST_TOO_LONG, -2, -3, ELL_TOO_BIG, DST_TOO_LONG, DST_TOO_LONG])):
            e.set_seeded_random_scalars(True, d)
            _, st = run_keyed(e, kit, seeds, [0] * 6)
            assert [int(x) for x in st] == codes, (curve, on, len(d), list(st))
            _, st = run_keyed(e, kit, seeds, [7] * 6)
            assert [int(x) for x in st] == [UNKNOWN_KEY] * 6, (curve, on, len(d), list(st))
        e.close()


# ---- case 6: stale buffers --------------------------------------------------------------------------------------------------
def check_stale_buffers(curve, lib_path=None, n=130, L=5):
    """A job of U = 5 (10 scalars per item) and then, on the same context, a smaller job of U = 0 with other seeds: the pooled
    scratch of the first is reused, the bytes of the second are the oracle's."""
    w = World(curve, lib_path, L)
    big = Items(w, [L] * n, disclosed=[[]] * n)
    m = n // 2 + 1
    small = Items(w, [L] * m, seed=5, disclosed=[list(range(L))] * m)
    dst = dst_of(w)
    eng = producer(w, on=False)
    eng.set_seeded_random_scalars(True, dst)
    for it, seeds in ((big, seeds_for(n, 1)), (small, seeds_for(m, 2)), (big, seeds_for(n, 3))):
        rnds = draws(w.suite, it.lengths, it.disclosed, seeds, dst)
        want = [want_proof(it, i, rnds, eng) for i in range(it.n)]
        for form in ("core", "wire"):
            same_bytes(run_proof(eng, it, seeds, form), ([o for _, o in want], [s for s, _ in want]), (curve, form, it.n, "stale"))
    eng.close()


# ---- case 7: set-up and the switch's lifetime -------------------------------------------------------------------------------
def check_setup(curve, lib_path=None, n=9, L=5):
    from bbs_sign_amd import BbsRuntimeError
    w = World(curve, lib_path, L)
    it = Items(w, [L] * n)
    dst = dst_of(w)
    seeds = [bytes([i + 1]) * 32 for i in range(n)]             # 32-byte "scalars" that are in range, read as scalars while off
    assert all(int.from_bytes(s, "little") < w.c.r for s in seeds)
    rnds = draws(w.suite, it.lengths, it.disclosed, seeds, dst)
    eng = producer(w, on=False)
    want = [want_proof(it, i, rnds, eng) for i in range(n)]
    want = ([o for _, o in want], [s for s, _ in want])
    base = int(eng.lib.bbs_ctx_table_bytes(eng.h))
    # off (the default): random_scalars are scalars, and the contract on their number holds
    one = [[int.from_bytes(s, "little")] * (5 + L - len(d)) for s, d in zip(seeds, it.disclosed)]
    as_scalars = [want_proof(it, i, one, eng) for i in range(n)]
    same_bytes(run_proof(eng, it, one, "core"), ([o for _, o in as_scalars], [s for s, _ in as_scalars]), (curve, "off"))
    with pytest.raises(BbsRuntimeError) as e:
        run_proof(eng, it, [x[:1] for x in one], "core")
    assert e.value.rc == E_ARG
    # a job keeps what it was created with
    eng.set_seeded_random_scalars(True, dst)
    assert int(eng.lib.bbs_ctx_table_bytes(eng.h)) == base + len(dst)
    held = eng.core_proof_gen_upload(it.sigs, it.msgs, it.disclosed, seeds, it.headers, it.phs)
    eng.set_seeded_random_scalars(False)
    assert int(eng.lib.bbs_ctx_table_bytes(eng.h)) == base
    plain = eng.core_proof_gen_upload(it.sigs, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    eng.set_seeded_random_scalars(True, b"another dst")
    for job in (held, plain):
        job.run()
        proofs, st = job.proofs()
        job.free()
        same_bytes((proof_octets(eng, proofs), st), want, (curve, "held job"))
    # the new DST is the one in force
    other = draws(w.suite, it.lengths, it.disclosed, seeds, b"another dst")
    got = run_proof(eng, it, seeds, "core")
    assert [int(x) for x in got[1]] == [1] * n and got[0] == [want_proof(it, i, other, eng)[1] for i in range(n)]
    # misuse
    assert eng.lib.bbs_ctx_set_seeded_random_scalars(None, 1, None, 0) == E_ARG
    with pytest.raises(BbsRuntimeError) as e:
        eng.seeded_random_scalars_batch([b"a", b"b"], [1, 0], dst)
    assert e.value.rc == E_ARG
    assert eng.seeded_random_scalars_batch([], [], dst)[0] == []
    with pytest.raises(ValueError):
        eng.core_proof_gen_batch(it.sigs, it.msgs, it.disclosed, b"short job seed", it.headers, it.phs)
    eng.close()


# ---- case 8: the public layer -----------------------------------------------------------------------------------------------
def check_public_layer(lib_path=None):
    from bbs_sign_amd import BbsError, api
    rng = random.Random(5)
    items, many = [], []
    for curve in ("bls12_381", "bn254"):
        r = bbs.SUITES[curve].curve.r
        sks = [api.SecretKey(curve, rng.randrange(1, r), lib_path) for _ in range(2)]
        pks = [sk.sk_to_pk() for sk in sks]
        for i, l in enumerate((0, 1, 3, 5, 2)):
            msgs = [b"seeded-public-%d-%d" % (i, j) for j in range(l)]
            sig = sks[i % 2].sign(msgs, b"h%d" % i)
            items.append((pks[i % 2], sig, b"h%d" % i, b"ph%d" % i, msgs, sorted(rng.sample(range(l), l // 2))))
        if curve == "bls12_381":
            many = [it[1:] for it in items if it[0] is pks[0]]
            many_pk = pks[0]

    def verdicts(its, proofs):
        assert not any(isinstance(p, BbsError) for p in proofs), proofs
        return [api.proof_verify(it[0], p, it[2], it[3], [it[4][j] for j in it[5]], it[5]) for it, p in zip(its, proofs)]
    a, b = api.proof_gen_many_issuers(items, device_random=True), api.proof_gen_many_issuers(items, device_random=True)
    assert verdicts(items, a) == [True] * len(items) and verdicts(items, b) == [True] * len(items)
    assert all(api.proof_to_octets(it[0].curve, x, lib_path) != api.proof_to_octets(it[0].curve, y, lib_path) for it, x, y in zip(items, a, b))
    mine = [(many_pk,) + it for it in many]
    a, b = api.proof_gen_many(many_pk, many, device_random=True), api.proof_gen_many(many_pk, many, device_random=True)
    assert verdicts(mine, a) == [True] * len(many) and verdicts(mine, b) == [True] * len(many)
    assert all(api.proof_to_octets("bls12_381", x, lib_path) != api.proof_to_octets("bls12_381", y, lib_path) for x, y in zip(a, b))
    # the switch is off again behind the call: the default path still takes scalars
    assert verdicts(mine, api.proof_gen_many(many_pk, many)) == [True] * len(many)
    api.clear_caches()
