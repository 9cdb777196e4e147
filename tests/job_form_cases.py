"""The four forms of a job (single, mixed, keyed, keyed mixed) of the four operations, in the core and the wire input form.
Shared by the host-twin tier (tests/test_job_forms_hosttwin.py) and the GPU tier (tests/test_job_forms_gpu.py).

Two properties of the layer that decides and binds a job's form (csrc/job_form.hpp), neither of which needs an oracle:

* Stage lists.  A job of every (operation, form, input form) reports exactly the stage names of STAGES below, which were
  recorded from the commit before the form layer was unified; the two tiers differ in the pairing stages only.
* The four forms agree.  With every item at the full count L, ONE registered key equal to the context's single key and
  key_index all zero, the four forms of an operation compute the same thing: identical statuses, and for sign and proof_gen
  (deterministic given the random scalars) identical signatures, proofs and octet strings.

Shape: n = 11, L = 3 -- ten items fill one six-lane pairing wavefront and the eleventh starts a second, so a keyed job has one
key-uniform wavefront and one mixed slot.  Item BAD is spoiled per operation so that the statuses are not all equal: verify
a forged e (0), proof_verify r1^ + 1 (0), proof_gen a disclosed index L (-3), sign L + 1 messages (-1)."""
import ctypes
import functools
import random

import numpy as np

from bbs_sign_amd import Proof, Signature, _lib
from bbs_sign_amd.engine import Job, _ragged_bytes, _u8, _u64
from mixed_len_cases import Items, World, sig_octets
from parity_cases import make_engine

N, L, BAD = 11, 3, 5
OPS = ("pv", "vf", "pg", "sg")
FORMS = ("single", "mixed", "keyed", "keyed_mixed")
INPUTS = ("core", "wire")
WANT_BAD = {"vf": 0, "pv": 0, "pg": -3, "sg": -1}


# STAGES[tier][op][form]: the stage names of a throughput-form job, as recorded on each tier.  The core and the wire input form
# of an operation recorded the same list in every form (their ingest and decode kernels run at upload and are no stages), so
# one list stands for both.
STAGES = {
    "twin": {
        "pv": {
            "single": ["pair_miller", "pair_final_exp", "pv_t1_chain", "pv_var_mul", "pv_scalars", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "mixed": ["pair_miller", "pair_final_exp", "pv_t1_chain", "pv_var_mul", "pv_scalars_mixed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "keyed": ["pair_miller_keyed", "pair_final_exp", "pv_t1_chain", "pv_var_mul", "pv_scalars_keyed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "keyed_mixed": ["pair_miller_keyed", "pair_final_exp", "pv_t1_chain", "pv_var_mul", "pv_scalars_keyed_mixed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
        },
        "vf": {
            "single": ["vf_var_mul", "vf_scalars", "vf_fixed_chunks", "vf_combine", "pair_miller", "pair_final_exp"],
            "mixed": ["vf_var_mul", "vf_scalars_mixed", "vf_fixed_chunks", "vf_combine", "pair_miller", "pair_final_exp"],
            "keyed": ["vf_var_mul", "vf_scalars_keyed", "vf_fixed_chunks", "vf_combine", "pair_miller_keyed", "pair_final_exp"],
            "keyed_mixed": ["vf_var_mul", "vf_scalars_keyed_mixed", "vf_fixed_chunks", "vf_combine", "pair_miller_keyed", "pair_final_exp"],
        },
        "pg": {
            "single": ["pg_scalars", "pg_b_parts", "pg_b_combine", "pg_tables", "pg_var_parts", "pg_finalize", "pg_emit"],
            "mixed": ["pg_scalars_mixed", "pg_b_parts", "pg_b_combine", "pg_tables", "pg_var_parts", "pg_finalize_mixed", "pg_emit_mixed"],
            "keyed": ["pg_scalars_keyed", "pg_b_parts", "pg_b_combine", "pg_tables", "pg_var_parts", "pg_finalize", "pg_emit"],
            "keyed_mixed": ["pg_scalars_keyed_mixed", "pg_b_parts", "pg_b_combine", "pg_tables", "pg_var_parts", "pg_finalize_mixed", "pg_emit_mixed"],
        },
        "sg": {
            "single": ["sg_scalars", "sg_msm_parts", "sg_combine", "sg_emit"],
            "mixed": ["sg_scalars_mixed", "sg_msm_parts", "sg_combine", "sg_emit"],
            "keyed": ["sg_scalars_keyed", "sg_msm_parts", "sg_combine", "sg_emit"],
            "keyed_mixed": ["sg_scalars_keyed_mixed", "sg_msm_parts", "sg_combine", "sg_emit"],
        },
    },
    "gpu": {
        "pv": {
            "single": ["pairing_6lane", "pv_t1_chain", "pv_var_mul", "pv_scalars", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "mixed": ["pairing_6lane", "pv_t1_chain", "pv_var_mul", "pv_scalars_mixed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "keyed": ["pairing_6lane_keyed", "pv_t1_chain", "pv_var_mul", "pv_scalars_keyed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
            "keyed_mixed": ["pairing_6lane_keyed", "pv_t1_chain", "pv_var_mul", "pv_scalars_keyed_mixed", "pv_fixed_chunks", "pv_challenge", "pv_finish"],
        },
        "vf": {
            "single": ["vf_var_mul", "vf_scalars", "vf_fixed_chunks", "vf_combine", "pairing_6lane"],
            "mixed": ["vf_var_mul", "vf_scalars_mixed", "vf_fixed_chunks", "vf_combine", "pairing_6lane"],
            "keyed": ["vf_var_mul", "vf_scalars_keyed", "vf_fixed_chunks", "vf_combine", "pairing_6lane_keyed"],
            "keyed_mixed": ["vf_var_mul", "vf_scalars_keyed_mixed", "vf_fixed_chunks", "vf_combine", "pairing_6lane_keyed"],
        },
    },
}
for _op in ("pg", "sg"):        # (no pairing stage: recorded alike on both tiers)
    STAGES["gpu"][_op] = STAGES["twin"][_op]


@functools.lru_cache(maxsize=4)
def world(curve, lib_path):
    """The key, N good items of L messages, and the inputs of every operation with item BAD spoiled."""
    w = World(curve, lib_path, L)
    it = Items(w, [L] * N)
    rng = random.Random(11)
    c = w.c
    sigs = list(it.sigs)
    sigs[BAD] = Signature(sigs[BAD].a, (sigs[BAD].e + 1) % c.r)
    proofs = list(it.proofs)
    p = proofs[BAD]
    proofs[BAD] = Proof(p.a_bar, p.b_bar, p.d, p.e_cap, (p.r1_cap + 1) % c.r, p.r3_cap, list(p.commitments), p.challenge)
    disclosed = [list(d) for d in it.disclosed]
    disclosed[BAD] = [L]
    rnds = [[rng.randrange(1, c.r) for _ in range(5 + L - len(d))] for d in disclosed]
    msgs, raw = [list(m) for m in it.msgs], [list(r) for r in it.raw]
    msgs[BAD].append(msgs[BAD][0])
    raw[BAD].append(raw[BAD][0])
    return w, it, {"vf_sigs": sigs, "pv_proofs": proofs, "pg_disclosed": disclosed, "pg_rnds": rnds, "sg_msgs": msgs, "sg_raw": raw}


def engine(w, form):
    eng = make_engine(w.curve, w.gens, w.api_id, w.lib_path, sk=w.sk)          # (the secret key brings its public key)
    if form == "mixed":
        eng.set_mixed_lengths(True)
        eng.set_mixed_lengths_gen(True)
    if form == "keyed_mixed":
        eng.set_keyed_mixed_lengths(True)
    if form.startswith("keyed"):
        st, pks, first = eng.set_secret_keys([w.sk])
        assert list(st) == [1] and pks == [w.pk] and first == 0
    return eng


def _producing_submit(eng, fn, n, args, out_args, decode):
    """A single-key wire submit of sign / proof_gen (the engine wraps only their keyed and batch forms)."""
    st = np.full(max(n, 1), -128, dtype=np.int8)
    j = ctypes.c_void_p()
    eng._chk(getattr(eng.lib, fn)(eng.h, n, *args, *out_args, st.ctypes.data_as(_lib.c_i8p), ctypes.byref(j)), fn)
    job = Job(eng, j, n)
    job.result = st[:n]
    job._decode = lambda: (decode(st), st[:n])
    return job


def submit(eng, w, it, x, op, form, inp):
    """The submit export of (operation, form, input form) -> job."""
    keyed = form.startswith("keyed")
    ki = (np.zeros(N, dtype=np.uint32),) if keyed else ()
    H, Ph = it.headers, it.phs
    if op == "vf":
        if inp == "core":
            return (eng.core_verify_keyed_submit if keyed else eng.core_verify_submit)(*ki, x["vf_sigs"], it.msgs, H)
        octs = [sig_octets(w, s) for s in x["vf_sigs"]]
        if keyed:
            return eng.verify_wire_keyed_submit(*ki, octs, it.raw, H)
        n, keep, args, fix = eng._vf_wire_args(octs, it.raw, H)
        return eng._status_submit("bbs_verify_wire_submit", n, args, fixup=fix)
    if op == "pv":
        if inp == "core":
            return (eng.core_proof_verify_keyed_submit if keyed else eng.core_proof_verify_submit)(*ki, x["pv_proofs"], it.dm, it.disclosed, H, Ph)
        octs = eng.proofs_to_octets_batch(x["pv_proofs"])
        return (eng.proof_verify_wire_keyed_submit if keyed else eng.proof_verify_wire_submit)(*ki, octs, it.draw, it.disclosed, H, Ph)
    if op == "sg":
        if inp == "core":
            return (eng.core_sign_keyed_submit if keyed else eng.core_sign_submit)(*ki, x["sg_msgs"], H)
        if keyed:
            return eng.sign_wire_keyed_submit(*ki, x["sg_raw"], H)
        mb, mbo, mio = eng._raw_msgs(x["sg_raw"])
        hb, ho = _ragged_bytes(H)
        rec = eng.fpb + 32
        out = np.zeros(N * rec, dtype=np.uint8)
        job = _producing_submit(eng, "bbs_sign_wire_submit", N, (_u8(mb), _u64(mbo), _u64(mio), _u8(hb), _u64(ho)), (_u8(out),),
                                lambda st: [out[i * rec:(i + 1) * rec].tobytes() if st[i] == 1 else b"" for i in range(N)])
        job._keep = (mb, mbo, mio, hb, ho)
        return job
    D, X = x["pg_disclosed"], x["pg_rnds"]
    if inp == "core":
        return (eng.core_proof_gen_keyed_submit if keyed else eng.core_proof_gen_submit)(*ki, it.sigs, it.msgs, D, X, H, Ph)
    octs = [sig_octets(w, s) for s in it.sigs]
    if keyed:
        return eng.proof_gen_wire_keyed_submit(*ki, octs, it.raw, D, X, H, Ph)
    ob, bad = eng._sig_octets(octs)
    mb, mbo, mio = eng._raw_msgs(it.raw)
    di, dio = eng._indexes(D)
    rs, ro = eng._scalars(X)
    hb, ho = _ragged_bytes(H)
    pb, po = _ragged_bytes(Ph)
    oc = np.zeros(sum(3 * eng.fpb + 32 * (4 + len(m)) for m in it.raw), dtype=np.uint8)
    oo = np.zeros(N + 1, dtype=np.uint64)
    job = _producing_submit(eng, "bbs_proof_gen_wire_submit", N,
                            (_u8(ob), _u8(mb), _u64(mbo), _u64(mio), _u64(di), _u64(dio), _u8(rs), _u64(ro), _u8(hb), _u64(ho), _u8(pb), _u64(po)),
                            (_u8(oc), _u64(oo)), lambda st: [oc[int(oo[i]):int(oo[i + 1])].tobytes() for i in range(N)])
    job._keep = (ob, mb, mbo, mio, di, dio, rs, ro, hb, ho, pb, po)
    return job


def stage_names(job):
    out = []
    while True:
        nm = job.eng.lib.bbs_job_stage_name(job.h, len(out))
        if not nm:
            return out
        out.append(nm.decode())


def plain(w, v):
    """A signature, a proof or an octet string as something that compares by value."""
    if isinstance(v, Signature):
        return sig_octets(w, v)
    if isinstance(v, Proof):
        return (v.a_bar, v.b_bar, v.d, v.e_cap, v.r1_cap, v.r3_cap, tuple(v.commitments), v.challenge)
    return v


def run(curve, lib_path, op, form, inp):
    """-> (stage names, statuses, outputs or None)"""
    w, it, x = world(curve, lib_path)
    eng = engine(w, form)
    job = submit(eng, w, it, x, op, form, inp)
    names = stage_names(job)
    job.wait()
    st = [int(s) for s in job.result]
    out = None
    if op in ("sg", "pg"):
        o, st2 = job.output()
        assert [int(s) for s in st2] == st
        out = [plain(w, v) for v in o]
    job.free()
    eng.close()
    return names, st, out


def check_forms(curve, lib_path, op, inp, tier):
    """One (operation, input form): the stage list of every form, and the four forms against each other."""
    want_st = [WANT_BAD[op] if i == BAD else 1 for i in range(N)]
    first = None
    for form in FORMS:
        names, st, out = run(curve, lib_path, op, form, inp)
        assert names == STAGES[tier][op][form], (curve, op, inp, form, names)
        assert st == want_st, (curve, op, inp, form, st)
        if out is not None:
            assert all((v not in (None, b"")) == (i != BAD) for i, v in enumerate(out)), (curve, op, inp, form)
            if first is None:
                first = out
            assert out == first, (curve, op, inp, form, [i for i in range(N) if out[i] != first[i]])
