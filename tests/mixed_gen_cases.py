"""Mixed message counts on one context for the PRODUCING side (bbs_ctx_set_mixed_lengths_gen).  Shared by the host-twin tier
(tests/test_mixed_gen_hosttwin.py) and the GPU tier (tests/test_mixed_gen_gpu.py).

The rule that defines correctness: the status AND the output bytes of item i, whose own message count is l_i, are what a
context made with generators[0 .. l_i] (same key, api_id, modes and random scalars) gives that item alone.

Expected values: the plain-C restatement of the oracle (oracle/c: core_sign / core_proof_gen with generators[: l_i + 1]; no
pairings here, so EVERY item goes through it), a sample through the pure-Python oracle, and as second witness fixed-length
contexts of the same library, one per length (mixed_len_cases.Items makes every signature and proof with World.signer(l)).
Everything is compared as octet strings: compress(A) || e for a signature, the proof's wire form for a proof, b"" for an item
that failed."""
import random

import numpy as np
import pytest

from bbs_sign_amd import Signature
from oracle import bbs
from mixed_len_cases import Items, World, disclosed_for, lengths_mod, sig_octets
from parity_cases import make_engine

FORMS = ("core", "octets", "wire")
HASHCTX_BYTES = 32 + 8 + 64 + 4 + 256 + 4            # HashCtx of stages_common.hpp: 368, no padding


def producer(w, L=None, on=True):
    eng = make_engine(w.curve, w.gens[:(w.L if L is None else L) + 1], w.api_id, w.lib_path, sk=w.sk)
    eng.set_mixed_lengths_gen(on)
    return eng


def random_scalars_of(it, seed=3, disclosed_given=False):
    """The random scalars Items drew for its proofs: the same generator, consumed in the same order (the proofs it made with
    them are compared byte for byte below, so a drift here cannot pass)."""
    rng = random.Random(seed)
    if not disclosed_given:
        for i, l in enumerate(it.lengths):
            disclosed_for(i, l, rng)
    return [[rng.randrange(1, it.w.c.r) for _ in range(5 + l - len(d))] for l, d in zip(it.lengths, it.disclosed)]


def proof_octets(eng, proofs):
    """Octet strings of a list of proofs (None -> b"")."""
    ok = [p for p in proofs if p is not None]
    octs = iter(eng.proofs_to_octets_batch(ok) if ok else [])
    return [next(octs) if p is not None else b"" for p in proofs]


# ---- expected values -------------------------------------------------------------------------------------------------------
def want_sign(it, i, python=False):
    w = it.w
    l = len(it.msgs[i])
    if l > w.L:
        return -1, b""
    if python:
        s = bbs.core_sign(w.suite, w.sk, w.gens[:l + 1], it.headers[i], it.msgs[i], w.api_id)
    else:
        s = w.cp.core_sign(w.sk, w.gens[:l + 1], it.headers[i], it.msgs[i], w.api_id)
    return 1, sig_octets(w, s)


def want_proof(it, i, rnds, eng, python=False):
    w = it.w
    l = len(it.msgs[i])
    if l > w.L:
        return -1, b""
    sig = bbs.Signature(it.sigs[i].a, it.sigs[i].e)
    if python:
        p = bbs.core_proof_gen(w.suite, w.pk, sig, it.headers[i], w.gens[:l + 1], it.phs[i], it.msgs[i], it.disclosed[i], w.api_id, rnds[i])
    else:
        p = w.cp.core_proof_gen(w.pk, sig, it.headers[i], w.gens[:l + 1], it.phs[i], it.msgs[i], sorted(it.disclosed[i]), w.api_id, rnds[i])
    assert len(p.commitments) == l - len(it.disclosed[i])
    return 1, proof_octets(eng, [p])[0]


# ---- running a list through a context: every form ends as (octet strings, statuses) ----------------------------------------
def run_sign(eng, it, form="core", idx=None, how="batch"):
    idx = list(range(it.n)) if idx is None else idx
    M, R, H = [it.msgs[i] for i in idx], [it.raw[i] for i in idx], [it.headers[i] for i in idx]
    if form == "wire":
        return eng.sign_wire_batch(R, H)
    if form == "octets":
        if how == "submit":
            job = eng.sign_octets_submit(M, H)
            job.wait()
            out = job.output()
            job.free()
            return out
        return eng.sign_octets_batch(M, H)
    if how == "upload":
        job = eng.core_sign_upload(M, H)
        job.run()
        sigs, st = job.signatures()
        job.free()
    elif how == "submit":
        job = eng.core_sign_submit(M, H)
        job.wait()
        sigs, st = job.output()
        job.free()
    else:
        sigs, st = eng.core_sign_batch(M, H)
    return [sig_octets(it.w, s) if s is not None else b"" for s in sigs], st


def run_proof(eng, it, rnds, form="core", idx=None, how="batch"):
    idx = list(range(it.n)) if idx is None else idx
    S, M, D = [it.sigs[i] for i in idx], [it.msgs[i] for i in idx], [it.disclosed[i] for i in idx]
    X, H, P = [rnds[i] for i in idx], [it.headers[i] for i in idx], [it.phs[i] for i in idx]
    if form == "wire":
        return eng.proof_gen_wire_batch([sig_octets(it.w, s) for s in S], [it.raw[i] for i in idx], D, X, H, P)
    if form == "octets":
        return eng.proof_gen_octets_batch(S, M, D, X, H, P)
    if how == "upload":
        job = eng.core_proof_gen_upload(S, M, D, X, H, P)
        job.run()
        proofs, st = job.proofs()
        job.free()
    elif how == "submit":
        job = eng.core_proof_gen_submit(S, M, D, X, H, P)
        job.wait()
        proofs, st = job.output()
        job.free()
    else:
        proofs, st = eng.core_proof_gen_batch(S, M, D, X, H, P)
    for t, i in enumerate(idx):
        if proofs[t] is not None:              # exactly l - r commitments are delivered
            assert len(proofs[t].commitments) == len(it.msgs[i]) - len(it.disclosed[i]), (i, len(proofs[t].commitments))
    return proof_octets(eng, proofs), st


def same_bytes(got, want, what):
    """got, want: (octet strings, statuses)."""
    gs, ws = [int(x) for x in got[1]], [int(x) for x in want[1]]
    bad = [i for i in range(len(ws)) if gs[i] != ws[i]]
    assert not bad, (what, "statuses", bad[:10], [gs[i] for i in bad[:10]], [ws[i] for i in bad[:10]])
    bad = [i for i in range(len(ws)) if bytes(got[0][i]) != bytes(want[0][i])]
    assert not bad, (what, "bytes", bad[:10])


def fixed_witness(it, eng):
    """What the fixed-length contexts of every item's own length gave (Items), as octet strings."""
    L = it.w.L
    st = [1 if l <= L else -1 for l in it.lengths]
    sg = [sig_octets(it.w, it.sigs[i]) if st[i] == 1 else b"" for i in range(it.n)]
    pf = proof_octets(eng, [it.proofs[i] if st[i] == 1 else None for i in range(it.n)])
    return (sg, st), (pf, st)


# ---- case 1: the export ---------------------------------------------------------------------------------------------------
def check_export(lib_path=None):
    from bbs_sign_amd import _lib
    lib = _lib.load_library(lib_path)
    assert "bbs_ctx_set_mixed_lengths_gen" in _lib.SIGNATURES and hasattr(lib, "bbs_ctx_set_mixed_lengths_gen")
    assert lib.bbs_ctx_set_mixed_lengths_gen(None, 1) == -100        # BBS_E_ARG


# ---- cases 2 and 3: every length in every wavefront -------------------------------------------------------------------------
def check_every_length(curve, lib_path=None, n=130, L=33, forms=FORMS, python_sample=(), hows=("batch", "upload", "submit")):
    w = World(curve, lib_path, L)
    lengths = lengths_mod(n)
    if L + 1 not in lengths:                    # a short list: its last item is the one above the context's count
        lengths[-1] = L + 1
    it = Items(w, lengths)
    assert 0 in it.lengths and L + 1 in it.lengths and (n < 70 or all(l in it.lengths for l in range(L + 2)))
    if n >= 70:
        assert any(any(j >= 32 for j in d) for d in it.disclosed) and any(d == [] for d in it.disclosed)
    rnds = random_scalars_of(it)
    eng = producer(w)
    fix_s, fix_p = fixed_witness(it, eng)
    # sign
    want = [want_sign(it, i) for i in range(n)]
    want = ([o for _, o in want], [s for s, _ in want])
    assert want[1] == [-1 if l > L else 1 for l in it.lengths]
    same_bytes(fix_s, want, (curve, "sign", "fixed-length contexts against the C port"))
    for form in forms:
        for how in (hows if form == "core" else ("batch",)):
            got = run_sign(eng, it, form, how=how)
            same_bytes(got, want, (curve, "sign", form, how))
            assert all(o == b"" for o, l in zip(got[0], it.lengths) if l > L)
    for i in python_sample:
        assert want_sign(it, i, python=True) == (want[1][i], want[0][i]), (curve, "sign", "python oracle", i)
    # proof_gen
    want = [want_proof(it, i, rnds, eng) for i in range(n)]
    want = ([o for _, o in want], [s for s, _ in want])
    same_bytes(fix_p, want, (curve, "proof_gen", "fixed-length contexts against the C port"))
    fpb = w.c.fp_bytes
    for form in forms:
        for how in (hows if form == "core" else ("batch",)):
            got = run_proof(eng, it, rnds, form, how=how)
            same_bytes(got, want, (curve, "proof_gen", form, how))
            for i in range(n):
                l, r = it.lengths[i], len(it.disclosed[i])
                assert len(got[0][i]) == (3 * fpb + 32 * (4 + l - r) if l <= L else 0), (curve, form, i)
    for i in python_sample:
        assert want_proof(it, i, rnds, eng, python=True) == (want[1][i], want[0][i]), (curve, "proof_gen", "python oracle", i)
    eng.close()


# ---- case 4: stale buffers ------------------------------------------------------------------------------------------------
def check_stale_buffers(curve, lib_path=None, n=130, L=33):
    """A job of all-length-L items, then a job of short items of the same n on the same context: the pools hand the second
    job the first one's fscal, fscal2, msgs, mtilde and out_mhat."""
    w = World(curve, lib_path, L)
    full = Items(w, [L] * n, seed=5)
    short = Items(w, [(0, 1, L - 1)[i % 3] for i in range(n)], seed=6)
    assert all(m != 0 for ms in full.msgs for m in ms)
    rf, rs = random_scalars_of(full, 5), random_scalars_of(short, 6)
    eng = producer(w)
    fs, fp = fixed_witness(full, eng)
    ss, sp = fixed_witness(short, eng)
    same_bytes(run_sign(eng, full), fs, (curve, "sign", "full"))
    same_bytes(run_sign(eng, short), ss, (curve, "sign", "short after full"))
    for form in ("core", "octets"):
        same_bytes(run_proof(eng, full, rf, form), fp, (curve, "proof_gen", form, "full"))
        same_bytes(run_proof(eng, short, rs, form), sp, (curve, "proof_gen", form, "short after full"))
    # an uploaded job, run twice: the second run reads what the first one wrote, and the same prefixes
    job = eng.core_proof_gen_upload(short.sigs, short.msgs, short.disclosed, rs, short.headers, short.phs)
    for _ in range(2):
        job.run()
        proofs, st = job.proofs()
        same_bytes((proof_octets(eng, proofs), st), sp, (curve, "proof_gen", "re-run"))
    job.free()
    eng.close()


# ---- case 5: the length is the item's, not the context's ------------------------------------------------------------------
def check_item_length_defects(curve, lib_path=None, n=130, L=33, positions=(0, 63, 64, 129)):
    w = World(curve, lib_path, L)
    lengths = [3 + (i * 7) % (L - 3) for i in range(n)]                  # 3 .. L - 1: every defect fits every position
    rng = random.Random(9)
    disclosed = [[0] if i in positions else disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
    base = Items(w, lengths, disclosed=disclosed)
    rnds0 = random_scalars_of(base, disclosed_given=True)
    eng = producer(w)
    good_s, good_p = fixed_witness(base, eng)
    same_bytes(run_sign(eng, base), good_s, (curve, "sign", "no defect"))
    same_bytes(run_proof(eng, base, rnds0), good_p, (curve, "proof_gen", "no defect"))
    r = w.c.r

    def planted(kind):
        it, rnds = base.copy(), [list(x) for x in rnds0]
        for p in positions:
            l = lengths[p]
            if kind == "too_long":                 # l = L + 1
                it.msgs[p] = it.msgs[p] + [5] * (L + 1 - l)
                it.raw[p] = it.raw[p] + [b"extra"] * (L + 1 - l)
                rnds[p] = rnds[p] + [7] * (L + 1 - l)
            elif kind == "more_indexes_than_messages":     # r > l
                it.disclosed[p] = list(range(l)) + [0]
                rnds[p] = rnds[p][:5]
            elif kind == "index_in_l_L":           # a disclosed index in [l, L): in range for the context, not for the item
                it.disclosed[p] = [0, l]
                rnds[p] = rnds[p][:5 + l - 2]
            elif kind == "duplicate":
                it.disclosed[p] = [0, 0]
                rnds[p] = rnds[p][:5 + l - 2]
            elif kind == "message_not_canonical":
                it.msgs[p] = it.msgs[p][:-1] + [r]
        return it, rnds

    for kind, code, ops in (("too_long", -1, ("sg", "pg")), ("more_indexes_than_messages", -2, ("pg",)), ("index_in_l_L", -3, ("pg",)),
                            ("duplicate", -4, ("pg",)), ("message_not_canonical", -40, ("sg", "pg"))):
        it, rnds = planted(kind)
        forms = ("core",) if kind == "message_not_canonical" else ("core", "wire")      # the wire form hashes its messages
        for op in ops:
            good = good_s if op == "sg" else good_p
            want = ([b"" if i in positions else good[0][i] for i in range(n)], [code if i in positions else 1 for i in range(n)])
            for form in forms:
                got = run_sign(eng, it, form) if op == "sg" else run_proof(eng, it, rnds, form)
                same_bytes(got, want, (curve, op, kind, form))         # the neighbours keep their bytes
            # second witness: a fixed-length context of the PRESENTED length decides the same
            if kind != "too_long":
                for p in positions[:2]:
                    f = w.signer(len(it.msgs[p]))
                    got = run_sign(f, it, "core", [p]) if op == "sg" else run_proof(f, it, rnds, "core", [p])
                    same_bytes(got, ([b""], [code]), (curve, op, kind, "fixed", p))
                    f.close()
    # a wrong count of random scalars for ONE item: the whole call is refused
    for p in positions:
        rnds = [list(x) for x in rnds0]
        rnds[p] = rnds[p] + [1]
        with pytest.raises(Exception, match="BBS_E_ARG"):
            run_proof(eng, base, rnds)
        rnds[p] = rnds[p][:-2]
        with pytest.raises(Exception, match="BBS_E_ARG"):
            run_proof(eng, base, rnds, "octets")
    same_bytes(run_proof(eng, base, rnds0), good_p, (curve, "proof_gen", "after the refused calls"))
    eng.close()


# ---- case 6: prefix boundaries --------------------------------------------------------------------------------------------
def check_prefix_boundaries(curve, lib_path=None, L=8):
    from mixed_len_cases import prefix_bytes
    suite = bbs.SUITES[curve]
    lens = (39, 40, 41) if curve == "bls12_381" else (23, 24, 25)
    on, before, after = set(), set(), set()
    for m in lens:
        on |= {l for l in range(L + 1) if prefix_bytes(curve, l, m) % 64 == 0}
        before |= {l for l in range(L + 1) if prefix_bytes(curve, l, m) % 64 == 63}
        after |= {l for l in range(L + 1) if prefix_bytes(curve, l, m) % 64 == 1}
    assert on and before and after, (on, before, after)
    hl = (0, 55, 56, 64)
    for aid in [suite.api_id] + [bytes(65 + k % 26 for k in range(m)) for m in lens]:
        w = World(curve, lib_path, L, api_id=aid)
        lengths = [l for l in range(L + 1) for _ in hl]
        it = Items(w, lengths, headers=[bytes([7 + l]) * h for l in range(L + 1) for h in hl])
        rnds = random_scalars_of(it)
        eng = producer(w)
        want = [want_sign(it, i) for i in range(it.n)]
        same_bytes(run_sign(eng, it), ([o for _, o in want], [s for s, _ in want]), (curve, "sign", len(aid)))
        want = [want_proof(it, i, rnds, eng) for i in range(it.n)]
        same_bytes(run_proof(eng, it, rnds), ([o for _, o in want], [s for s, _ in want]), (curve, "proof_gen", len(aid)))
        eng.close()


# ---- case 7: switch semantics ---------------------------------------------------------------------------------------------
def check_switch(curve, lib_path=None, n=23, L=8):
    from mixed_len_cases import run as run_verify, same
    w = World(curve, lib_path, L)
    lengths = [i % (L + 1) for i in range(n)]
    it = Items(w, lengths)
    rnds = random_scalars_of(it)
    eng = make_engine(curve, w.gens, w.api_id, lib_path, sk=w.sk)
    good_s, good_p = fixed_witness(it, eng)
    only_L = lambda good: ([good[0][i] if lengths[i] == L else b"" for i in range(n)], [1 if l == L else -1 for l in lengths])
    # off by default
    same_bytes(run_sign(eng, it), only_L(good_s), (curve, "sign", "default"))
    same_bytes(run_proof(eng, it, rnds), only_L(good_p), (curve, "proof_gen", "default"))
    # bbs_ctx_set_mixed_lengths alone leaves sign and proof_gen fixed-length
    eng.set_mixed_lengths(True)
    same_bytes(run_sign(eng, it), only_L(good_s), (curve, "sign", "the verifying switch alone"))
    same_bytes(run_proof(eng, it, rnds), only_L(good_p), (curve, "proof_gen", "the verifying switch alone"))
    eng.set_mixed_lengths(False)
    # the new switch alone leaves verify and proof_verify fixed-length
    eng.set_mixed_lengths_gen(True)
    same_bytes(run_sign(eng, it), good_s, (curve, "sign", "on"))
    same_bytes(run_proof(eng, it, rnds), good_p, (curve, "proof_gen", "on"))
    for op in ("vf", "pv"):
        same(run_verify(eng, it, op), [1 if l == L else -1 for l in lengths], (curve, op, "the producing switch alone"))
    # a job uploaded before a flip runs with the stages it had
    j_on = eng.core_proof_gen_upload(it.sigs, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    s_on = eng.core_sign_upload(it.msgs, it.headers)
    eng.set_mixed_lengths_gen(False)
    j_off = eng.core_proof_gen_upload(it.sigs, it.msgs, it.disclosed, rnds, it.headers, it.phs)
    s_off = eng.core_sign_upload(it.msgs, it.headers)
    # off again: -1 for l != L
    same_bytes(run_sign(eng, it), only_L(good_s), (curve, "sign", "switched off"))
    same_bytes(run_proof(eng, it, rnds, "octets"), only_L(good_p), (curve, "proof_gen", "switched off"))
    eng.set_mixed_lengths_gen(True)
    for job, want in ((j_on, good_p), (j_off, only_L(good_p))):
        job.run()
        proofs, st = job.proofs()
        same_bytes((proof_octets(eng, proofs), st), want, (curve, "proof_gen", "job from before the flip"))
        job.free()
    for job, want in ((s_on, good_s), (s_off, only_L(good_s))):
        job.run()
        sigs, st = job.signatures()
        same_bytes(([sig_octets(w, s) if s is not None else b"" for s in sigs], st), want, (curve, "sign", "job from before the flip"))
        job.free()
    eng.close()
    # every order of {generators, key, switch} gives the same bytes
    from bbs_sign_amd import Engine
    import parity_cases as pc
    steps = {"g": lambda e: e.set_generators(w.gens, w.api_id), "k": lambda e: e.set_secret_key(w.sk), "s": lambda e: e.set_mixed_lengths_gen(True)}
    for order in ("gks", "gsk", "kgs", "ksg", "sgk", "skg"):
        e = Engine(curve, lib_path=lib_path, window_bits=4 if lib_path else 8)
        if pc.LATENCY_MODE is not None:
            e.set_latency_mode(pc.LATENCY_MODE)
        for c in order:
            steps[c](e)
        same_bytes(run_sign(e, it), good_s, (curve, "sign", "order", order))
        same_bytes(run_proof(e, it, rnds), good_p, (curve, "proof_gen", "order", order))
        e.close()
    # a holder's context (public key only), and a key replaced after the switch: the prefixes follow
    h = make_engine(curve, w.gens, w.api_id, lib_path, pk=w.pk)
    h.set_mixed_lengths_gen(True)
    same_bytes(run_proof(h, it, rnds), good_p, (curve, "proof_gen", "public key only"))
    w2 = World(curve, lib_path, L, seed=8)
    it2 = Items(w2, lengths, seed=4)
    h.set_public_key(w2.pk)
    same_bytes(run_proof(h, it2, random_scalars_of(it2, 4)), fixed_witness(it2, h)[1], (curve, "proof_gen", "new public key"))
    h.set_secret_key(w.sk)
    same_bytes(run_sign(h, it), good_s, (curve, "sign", "secret key after the switch"))
    h.close()
    # L = 0: the context has no message generator; an item with l = 0 on a longer context is covered above (lengths has 0)
    assert lengths[0] == 0 and good_s[1][0] == 1 and good_p[1][0] == 1
    w0 = World(curve, lib_path, 0)
    it0 = Items(w0, [0, 0, 1], seed=2)
    e0 = producer(w0)
    same_bytes(run_sign(e0, it0), fixed_witness(it0, e0)[0], (curve, "sign", "L = 0"))
    same_bytes(run_proof(e0, it0, random_scalars_of(it0, 2)), fixed_witness(it0, e0)[1], (curve, "proof_gen", "L = 0"))
    assert [int(x) for x in run_sign(e0, it0)[1]] == [1, 1, -1]
    e0.close()


def check_table_bytes(curve, lib_path=None, L=7):
    """bbs_ctx_table_bytes grows by (L + 1) * sizeof(HashCtx) when the FIRST of the two length switches goes on, and by nothing
    for the second."""
    w = World(curve, lib_path, L)
    tb = lambda e: int(e.lib.bbs_ctx_table_bytes(e.h))
    for first, second in (("set_mixed_lengths_gen", "set_mixed_lengths"), ("set_mixed_lengths", "set_mixed_lengths_gen")):
        eng = make_engine(curve, w.gens, w.api_id, lib_path, sk=w.sk)
        off = tb(eng)
        getattr(eng, first)(True)
        assert tb(eng) == off + (L + 1) * HASHCTX_BYTES, (first, tb(eng), off)
        getattr(eng, second)(True)
        assert tb(eng) == off + (L + 1) * HASHCTX_BYTES, (second, tb(eng), off)
        getattr(eng, first)(False)
        assert tb(eng) == off + (L + 1) * HASHCTX_BYTES
        getattr(eng, second)(False)
        assert tb(eng) == off
        eng.close()
    nokey = make_engine(curve, w.gens, w.api_id, lib_path)        # no key: no prefixes to count, and no job
    before = tb(nokey)
    nokey.set_mixed_lengths_gen(True)
    assert tb(nokey) == before
    with pytest.raises(Exception, match="BBS_E_STATE"):
        nokey.core_sign_batch([[1]], [b""])
    nokey.close()


# ---- cases 8 and 11: the round trip on the device, and the issuer --------------------------------------------------------------
def _public_world(curve, lib_path, n, max_l, seed):
    from bbs_sign_amd import Engine, api
    import parity_cases as pc
    suite = bbs.SUITES[curve]
    rng = random.Random(seed)
    sk = rng.randrange(1, suite.curve.r)
    lengths = [i % (max_l + 2) for i in range(n)]                     # one length above the context's per period
    raw = [[b"gen-item-%d-%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    headers = [bytes([i % 7]) * (i % 4) for i in range(n)]
    phs = [bytes([i % 5]) * (i % 3) for i in range(n)]
    disclosed = [disclosed_for(i, l, rng) for i, l in enumerate(lengths)]
    rnds = [[rng.randrange(1, suite.curve.r) for _ in range(5 + l - len(d))] for l, d in zip(lengths, disclosed)]
    wb = 4 if lib_path else 8
    eng = Engine(curve, lib_path=lib_path, window_bits=wb)
    if pc.LATENCY_MODE is not None:
        eng.set_latency_mode(pc.LATENCY_MODE)
    eng.set_generators(api.create_generators(curve, max_l + 1, lib_path), suite.api_id)
    eng.set_secret_key(sk)
    eng.set_mixed_lengths_gen(True)
    return suite, sk, lengths, raw, headers, phs, disclosed, rnds, wb, eng


def check_round_trip(curve, lib_path=None, n=40, max_l=12):
    from bbs_sign_amd import api
    suite, sk, lengths, raw, headers, phs, disclosed, rnds, wb, eng = _public_world(curve, lib_path, n, max_l, 55)
    pk = api.SecretKey(curve, sk, lib_path).sk_to_pk()
    so, st = eng.sign_wire_batch(raw, headers)
    assert [int(x) for x in st] == [1 if l <= max_l else -1 for l in lengths]
    ok = [i for i in range(n) if lengths[i] <= max_l]
    filler = next(so[i] for i in ok)
    po, st = eng.proof_gen_wire_batch([o or filler for o in so], raw, disclosed, rnds, headers, phs)
    assert [int(x) for x in st] == [1 if l <= max_l else -1 for l in lengths]
    eng.close()
    sigs = {i: api.octets_to_signature(curve, so[i], lib_path) for i in ok}
    proofs = {i: api.octets_to_proof(curve, po[i], lib_path) for i in ok}
    assert api.verify_many(pk, [(sigs[i], headers[i], raw[i]) for i in ok]) == [True] * len(ok)
    assert api.proof_verify_many(pk, [(proofs[i], headers[i], phs[i], [raw[i][j] for j in disclosed[i]], disclosed[i]) for i in ok]) == [True] * len(ok)
    # one corrupted byte: False for that item only
    k = ok[len(ok) // 2]
    bs = bytearray(so[k]); bs[-1] ^= 1
    bp = bytearray(po[k]); bp[-1] ^= 1
    vs = [(api.octets_to_signature(curve, bytes(bs), lib_path) if i == k else sigs[i], headers[i], raw[i]) for i in ok]
    assert api.verify_many(pk, vs) == [i != k for i in ok]
    vp = [(api.octets_to_proof(curve, bytes(bp), lib_path) if i == k else proofs[i], headers[i], phs[i], [raw[i][j] for j in disclosed[i]], disclosed[i]) for i in ok]
    assert api.proof_verify_many(pk, vp) == [i != k for i in ok]


def check_against_issuer(curve, lib_path=None, n=56, max_l=12):
    from bbs_sign_amd import Issuer
    suite, sk, lengths, raw, headers, phs, disclosed, rnds, wb, eng = _public_world(curve, lib_path, n, max_l, 77)
    iss = Issuer(curve, suite.api_id, lib_path=lib_path, max_messages=max_l, window_bits=wb)
    iss.set_secret_key(sk)
    so_i, st_i = iss.sign(raw, headers)
    so, st = eng.sign_wire_batch(raw, headers)
    same_bytes((so, st), (so_i, st_i), (curve, "sign", "issuer"))
    assert [int(x) for x in st] == [1 if l <= max_l else -1 for l in lengths]
    filler = next(o for o in so if o)
    sin = [o or filler for o in so]
    # the defects that have a wire form, planted in good items
    cand = iter(i for i in range(n) if 4 <= lengths[i] <= max_l)
    i = next(cand); disclosed[i] = list(range(lengths[i])) + [0]; rnds[i] = rnds[i][:5]; a = i
    i = next(cand); disclosed[i] = [0, lengths[i]]; rnds[i] = rnds[i][:5]; b = i
    i = next(cand); disclosed[i] = [1, 1]; rnds[i] = (rnds[i] + [3] * lengths[i])[:5 + lengths[i] - 2]; c = i
    po_i, st_i = iss.proof_gen(sin, raw, disclosed, rnds, headers, phs)
    po, st = eng.proof_gen_wire_batch(sin, raw, disclosed, rnds, headers, phs)
    iss.close()
    eng.close()
    same_bytes((po, st), (po_i, st_i), (curve, "proof_gen", "issuer"))
    assert (int(st[a]), int(st[b]), int(st[c])) == (-2, -3, -4), (int(st[a]), int(st[b]), int(st[c]))
    assert all(int(st[i]) == (1 if lengths[i] <= max_l else -1) for i in range(n) if i not in (a, b, c))


# ---- case 9: the reference's vectors on a longer context ------------------------------------------------------------------
def check_reference_vectors_on_longer_context(lib_path=None, L=5):
    """The reference's one-message signature and proof vectors (src/tests/test_vector.rs:163-193, :199-260, the constants of
    tests/parity_cases.py check_kat_vectors) come out of a context made for five messages, byte for byte."""
    S = bbs.BLS_SUITE
    H = bytes.fromhex
    ikm = H("746869732d49532d6a7573742d616e2d546573742d494b4d2d746f2d67656e65726174652d246528724074232d6b6579")
    key_info = H("746869732d49532d736f6d652d6b65792d6d657461646174612d746f2d62652d757365642d696e2d746573742d6b65792d67656e")
    key_dst = H("4242535f424c53313233383147315f584d443a5348412d3235365f535357555f524f5f4832475f484d32535f4b455947454e5f4453545f")
    m1 = H("9872ad089e452c7b6e283dfac2a80d58e8d0ff71cc4d5e310a1debdda4a45f02")
    header = H("11223344556677889900aabbccddeeff")
    ph = H("bed231d880675ed101ead304512e043ade9958dd0241ea70b4b3957fba941501")
    sig = ("84773160b824e194073a57493dac1a20b667af70cd2352d8af241c77658da5253aa8458317cca0eae615690d55b1f271"
           "64657dcafee1d5c1973947aa70e2cfbb4c892340be5969920d0916067b4565a0")
    proof = "94916292a7a6bade28456c601d3af33fcf39278d6594b467e128a3f83686a104ef2b2fcf72df0215eeaf69262ffe8194a19fab31a82ddbe06908985abc4c9825788b8a1610942d12b7f5debbea8985296361206dbace7af0cc834c80f33e0aadaeea5597befbb651827b5eed5a66f1a959bb46cfd5ca1a817a14475960f69b32c54db7587b5ee3ab665fbd37b506830a49f21d592f5e634f47cee05a025a2f8f94e73a6c15f02301d1178a92873b6e8634bafe4983c3e15a663d64080678dbf29417519b78af042be2b3e1c4d08b8d520ffab008cbaaca5671a15b22c239b38e940cfeaa5e72104576a9ec4a6fad78c532381aeaa6fb56409cef56ee5c140d455feeb04426193c57086c9b6d397d9418"
    sk = bbs.key_gen(S, ikm, key_info, key_dst)
    eng = make_engine("bls12_381", bbs.create_generators(S, L + 1, S.api_id), S.api_id, lib_path, sk=sk)
    eng.set_mixed_lengths_gen(True)
    so, st = eng.sign_wire_batch([[m1], [m1] * L], [header, header])
    assert list(st) == [1, 1] and so[0].hex() == sig and so[1].hex() != sig
    msg = eng.hash_to_scalar_batch([m1], S.api_id + b"MAP_MSG_TO_SCALAR_AS_HASH_")
    s = eng.signatures_from_octets_batch([so[0]])[0][0]
    rnd = bbs.mocked_calculate_random_scalars(S, 5)
    po, st = eng.proof_gen_octets_batch([s], [[msg[0]]], [[0]], [rnd], [header], [ph])
    assert list(st) == [1] and po[0].hex() == proof
    eng.close()


# ---- case 10: the public layer --------------------------------------------------------------------------------------------
def check_public_layer(curve, lib_path=None):
    from bbs_sign_amd import BbsError, api
    from parity_cases import proof_eq
    suite = bbs.SUITES[curve]
    rng = random.Random(99)
    sk = api.SecretKey(curve, rng.randrange(1, suite.curve.r), lib_path)
    pk = sk.sk_to_pk()
    lengths = [0, 1, 2, 3, 4, 5, 2, 3]
    msgs = [[b"public-gen-%d-%d" % (i, j) for j in range(l)] for i, l in enumerate(lengths)]
    headers = [b"h%d" % i for i in range(len(lengths))]
    items = list(zip(msgs, headers))
    assert api.sign_many(sk, []) == [] and api.proof_gen_many(pk, []) == []
    got = api.sign_many(sk, items)
    sigs = [sk.sign(m, h) for m, h in items]
    assert [(g.a, g.e) for g in got] == [(s.a, s.e) for s in sigs]
    disclosed = [sorted(rng.sample(range(l), l // 2)) for l in lengths]
    disclosed[6] = [0, 2]                                    # index 2 of an item of 2 messages: InvalidDisclosedIndex, in place
    disclosed[7] = [1, 1]                                    # a duplicate
    rnds = [[rng.randrange(1, suite.curve.r) for _ in range(max(5 + l - len(d), 0))] for l, d in zip(lengths, disclosed)]
    pitems = [(s, h, b"ph", m, d, x) for s, h, m, d, x in zip(sigs, headers, msgs, disclosed, rnds)]
    got = api.proof_gen_many(pk, pitems)
    for i, item in enumerate(pitems):
        try:
            want = api.proof_gen(pk, *item)
        except BbsError as e:
            assert isinstance(got[i], BbsError) and got[i].status == e.status, (curve, i, got[i], e)
            continue
        assert proof_eq(got[i], want), (curve, i)
    assert isinstance(got[6], BbsError) and got[6].status == -3 and isinstance(got[7], BbsError) and got[7].status == -4
    assert all(not isinstance(g, BbsError) for g in got[:6])
    # random scalars drawn by the call where an item brings none: the proof verifies
    drawn = api.proof_gen_many(pk, [it[:5] for it in pitems[:6]])
    assert api.proof_verify_many(pk, [(p, h, b"ph", [m[j] for j in d], d) for p, h, m, d in zip(drawn, headers, msgs, disclosed)]) == [True] * 6
    # one engine per key serves growing L: a shorter list reuses the engine made for the longest list seen, a longer one replaces it
    for key in (sk, pk):
        e5 = api._mixed_gen_engine(key, 5)
        assert api._mixed_gen_engine(key, 3) is e5 and api._mixed_gen_engine(key, 0) is e5
        e7 = api._mixed_gen_engine(key, 7)
        assert e7 is not e5 and api._mixed_gen_engine(key, 5) is e7
    assert [(g.a, g.e) for g in api.sign_many(sk, items[:3])] == [(s.a, s.e) for s in sigs[:3]]
    assert api._mixed_gen_engine(sk, 2) is api._mixed_gen_engine(sk, 7)
    assert sum(1 for k in api._eng_cache if k[0] == "mixed_gen" and k[2] == curve) == 2          # the signer's and the holder's
