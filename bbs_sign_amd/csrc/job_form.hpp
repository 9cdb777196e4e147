// The form of a job (stages_common.hpp Form: Single, Mixed, Keyed, KeyedMixed), decided ONCE per upload and bound in one
// place for the four operations: the state a job keeps of its form, the checks of an upload, the key indexes and the pairing
// order built on the host, the prefixes the scalar stage reads, and the two launches that differ by form (ingest body, scalar
// stage).  An upload keeps what is its own: its buffers, its stage list, and for verify / proof_verify the pairing stage.
#pragma once
#include "runtime.hpp"

// what a job keeps of its form
template <class C>
struct JobForm {
    Form form = Form::Single;
    DomainSrc<C> src{};                      // what the scalar stage reads (kidx: KEY_NONE = unknown / refused, decided by KeyGate)
    uint32_t* len = nullptr;                 // src.len as the MIXED ingest bodies write it
    bool mixed() const { return form_mixed(form); }
};
// verify / proof_verify: plus the keyed pairing order
template <class C>
struct PairedJobForm : JobForm<C> {
    PairKeyedArgs<C> pair{};                 // the pairing step (points, gate, output: copied from the job's PairArgs at launch)
    bool unit = false;                       // line form of the key set the job holds (KeySet::unit)
};

// The form of an upload and its state checks.  The context's switches are read HERE, once: the checks, the stages and the
// data of the job all go by this one look, whatever a setter does meanwhile.  What differs per operation: the key set a keyed
// job needs (Ctx::keys, sign: Ctx::sign_keys), the single-key switch (mixed_lengths, producing side: mixed_lengths_gen) and
// the single key (pk_set, sign: sk_set).
enum class FormOp { Verify, ProofGen, Sign };          // Verify: verify and proof_verify
template <bool KEYED, class C>
int decide_form(const Ctx<C>* ctx, FormOp op, size_t n, const uint32_t* key_index, Form& form) {
    const bool have_key_set = op == FormOp::Sign ? ctx->sign_keys != nullptr : ctx->keys != nullptr;
    const bool single_mixed = op == FormOp::Verify ? ctx->mixed_lengths : ctx->mixed_lengths_gen;
    const bool have_single_key = op == FormOp::Sign ? ctx->sk_set : ctx->pk_set;
    if constexpr (KEYED) {
        const bool keyed_mixed = ctx->keyed_mixed_lengths;
        // (keyed jobs of mixed counts treat a missing key set as the empty set: every item is BBS_ST_UNKNOWN_KEY)
        if (!ctx->gens_set || (!have_key_set && !keyed_mixed)) return BBS_E_STATE;
        // (the single-key switch alone builds no prefix per (key, length): that is bbs_ctx_set_keyed_mixed_lengths)
        if (single_mixed && !keyed_mixed) return BBS_E_STATE;
        if (n && !key_index) return BBS_E_ARG;
        form = keyed_mixed ? Form::KeyedMixed : Form::Keyed;
    } else {
        if (!ctx->gens_set || !have_single_key) return BBS_E_STATE;
        form = single_mixed ? Form::Mixed : Form::Single;
    }
    return BBS_OK;
}

// ---- keyed forms: per-item key indexes and the pairing order, built on the host before the staging image ----------------
// Item i -> its key (KEY_NONE: unknown / refused) and the pairing order.  Items are sorted by key, stably (a counting sort);
// key k with c items fills floor(c / 10) key-uniform wavefronts, its c mod 10 remaining items go to the mixed wavefronts
// behind them.  `words` = [kidx n][uniform slots][mixed slots][wave keys]; it travels in the job's staging image (the one
// asynchronous copy), keyed_bind points the job at it.
template <class C, class J>
void keyed_order(J* j, Ctx<C>* ctx, size_t n, const uint32_t* key_index, PairedJobForm<C>& jf, std::vector<uint32_t>& words) {
    constexpr uint32_t W = (uint32_t)KEY_SLOTS_PER_WAVE;
    const auto ks = ctx->keys;
    j->key_set = ks;
    const size_t nk = ks ? ks->n : 0;         // (no set: only where bbs_ctx_set_keyed_mixed_lengths is on -- every index is unknown)
    std::vector<uint32_t> cnt(nk, 0);
    words.assign(3 * n + n / W + 1, 0);
    uint32_t* kid = words.data();
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = key_index[i];
        const bool ok = k < nk && ks->status[k] == 1;
        kid[i] = ok ? k : KEY_NONE;
        if (ok) cnt[k]++;
    }
    std::vector<uint32_t> ufirst(nk), mfirst(nk), seen(nk, 0);
    size_t nu = 0, nm = 0;
    for (size_t k = 0; k < nk; k++) {
        ufirst[k] = (uint32_t)nu; nu += cnt[k] / W * W;
        mfirst[k] = (uint32_t)nm; nm += cnt[k] % W;
    }
    uint32_t* uslot = words.data() + n;
    uint32_t* mslot = uslot + nu;
    uint32_t* wkey = mslot + nm;
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = kid[i];
        if (k == KEY_NONE) continue;
        const uint32_t full = cnt[k] / W * W, s = seen[k]++;
        if (s < full) uslot[ufirst[k] + s] = (uint32_t)i;
        else mslot[mfirst[k] + s - full] = (uint32_t)i;
    }
    for (size_t k = 0, w = 0; k < nk; k++)
        for (uint32_t q = 0; q < cnt[k] / W; q++) wkey[w++] = (uint32_t)k;
    words.resize(n + nu + nm + nu / W);
    jf.src.keys = ks ? ks->d.template as<KeyEntry<C>>() : nullptr;
    jf.pair.keys = jf.src.keys; jf.pair.n_uni = nu; jf.pair.n_slots = nu + nm;
    jf.unit = ks ? ks->unit : ctx->lines_unit();
}
// the same look at the key set for a job without a pairing step (keyed proof_gen): `words` = [kidx n] and nothing else
template <class C, class J>
void keyed_indexes(J* j, Ctx<C>* ctx, size_t n, const uint32_t* key_index, JobForm<C>& jf, std::vector<uint32_t>& words) {
    const auto ks = ctx->keys;
    j->key_set = ks;
    const size_t nk = ks ? ks->n : 0;         // (no set: only where bbs_ctx_set_keyed_mixed_lengths is on -- every index is unknown)
    words.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = key_index[i];
        words[i] = (k < nk && ks->status[k] == 1) ? k : KEY_NONE;
    }
    jf.src.keys = ks ? ks->d.template as<KeyEntry<C>>() : nullptr;
}
// keyed sign: the same look at the key set AND at the signing set (Ctx::SignSet) -- KEY_NONE as above, KEY_NO_SECRET for an
// accepted key without a secret half; only an index that names a secret row is passed on.  BBS_E_STATE (fail closed) where the
// two sets do not belong together: a set that was replaced between the two looks.  src.sks = the rows on the device (null: none).
template <class C, class J>
int keyed_sign_indexes(J* j, Ctx<C>* ctx, size_t n, const uint32_t* key_index, JobForm<C>& jf, std::vector<uint32_t>& words) {
    const auto ss = ctx->sign_keys;
    keyed_indexes<C>(j, ctx, n, key_index, jf, words);
    const auto ks = std::static_pointer_cast<const typename Ctx<C>::KeySet>(j->key_set);
    if (ss && (!ks || ss->lineage != ks->lineage || ss->n > ks->n)) return BBS_E_STATE;
    j->sign_key_set = ss;
    // (no signing set: only where bbs_ctx_set_keyed_mixed_lengths is on -- the empty set, every index is unknown)
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = words[i];
        if (!ss) words[i] = KEY_NONE;
        else if (k != KEY_NONE && !(k < ss->n && ss->has[k])) words[i] = KEY_NO_SECRET;
    }
    jf.src.sks = ss ? ss->d.template as<uint32_t>() : nullptr;
    return BBS_OK;
}
// the device half: d = the words' place in the device copy of the staging image
template <class C>
void keyed_bind(JobForm<C>& jf, const uint32_t* d) { jf.src.kidx = d; }
template <class C>
void keyed_bind(PairedJobForm<C>& jf, size_t n, const uint32_t* d) {
    jf.src.kidx = d;
    jf.pair.kidx = d; jf.pair.slot_item = d + n; jf.pair.wave_key = d + n + jf.pair.n_slots;
}
// behind the ingest stage: items with an unknown key are decided (BBS_ST_UNKNOWN_KEY)
template <class J>
int keyed_gate(J* j, size_t n, const uint32_t* kidx, int8_t* status0) {
    return rt::launch<KeyGate>(j->stream(), KeyGateArgs{n, kidx, status0}, n) ? BBS_E_HIP : BBS_OK;
}
// the pairing step of a keyed job on the main (aux = 0) or second stream, as add_pairing_stages: the fused kernel in both job
// forms.  jf->pair.p is copied from *pa when the stage is launched.
template <class C, class J>
void add_keyed_pairing_stages(J* j, PairedJobForm<C>* jf, const PairArgs<C>* pa, int aux) {
#ifdef BBS_HOST_TWIN
    j->stages.push_back({"pair_miller_keyed", [j, jf, pa, aux]() {
        jf->pair.p = *pa;
        return rt::launch<PairMillerKeyed<C>>(aux ? j->stream_aux() : j->stream(), jf->pair, jf->pair.n_slots * 2);
    }, aux, 0});
    j->stages.push_back({"pair_final_exp", [j, pa, aux]() { return rt::launch<PairFinal<C>>(aux ? j->stream_aux() : j->stream(), *pa, pa->n); }, aux, 0});
#else
    j->stages.push_back({"pairing_6lane_keyed", [j, jf, pa, aux]() {
        jf->pair.p = *pa;
        // the key set the job holds and BP2's table on the device must agree (they do unless the form was switched under the job)
        if (jf->unit != j->ctx->dev_lines_unit) return -1;
        rt::Stream& st = aux ? j->stream_aux() : j->stream();
        const size_t nt = ((jf->pair.n_slots + GRP_PER_WAVE - 1) / GRP_PER_WAVE) * 64;
        return jf->unit ? rt::launch<PairDistKeyed<C, true>>(st, jf->pair, nt) : rt::launch<PairDistKeyed<C, false>>(st, jf->pair, nt);
    }, aux, 0});
#endif
}

// ---- mixed forms: the per-item length array and the prefixes the scalar stage starts from ---------------------------------
// Mixed: the context's prefixes per length (its LenSet, held by the job).  KeyedMixed: the prefixes per (key, length); they must
// be the rows of the key set keyed_order / keyed_indexes bound the job to (fail closed otherwise: a set that was replaced
// between the two looks).  The other two forms bind nothing.  nn = max(n, 1).
template <class C, class J>
int form_bind(J* j, Ctx<C>* ctx, size_t nn, JobForm<C>& jf) {
    if (jf.form == Form::Mixed) {
        std::shared_ptr<const typename Ctx<C>::LenSet> ls;
        if (const int rc = ctx->sync_lengths(ls)) return rc;
        j->len_set = ls;
        jf.src.pref = ls->d.template as<HashCtx>();
    } else if (jf.form == Form::KeyedMixed) {
        const auto kl = ctx->key_lens;
        jf.src.stride = (uint32_t)ctx->L + 1;
        if (j->key_set) {         // (an empty set has no rows and no item that reads one: KeyGate decides every item)
            if (!kl || kl->of.get() != j->key_set.get() || kl->stride != (size_t)jf.src.stride) return BBS_E_STATE;
            j->key_len_set = kl;
            jf.src.pref = kl->d.template as<HashCtx>();
        }
    } else return BBS_OK;
    int rc = BBS_OK;
    jf.src.len = jf.len = j->template scratch<uint32_t>(nn, rc);
    return rc;
}

// ---- the two launches that differ by form ------------------------------------------------------------------------------------
// an operation's ingest kernel in its plain or its MIXED body (which serves Mixed and KeyedMixed: it records the item's count)
template <class Plain, class Mixed, class C, class J, class A>
int launch_ingest(J* j, const JobForm<C>& jf, const A& ia, size_t n) {
    const int rc = jf.mixed() ? rt::launch<Mixed>(j->stream(), MixedIngestArgs<A>{ia, jf.len}, n) : rt::launch<Plain>(j->stream(), ia, n);
    return rc ? BBS_E_HIP : BBS_OK;
}
// The scalar stage of job j (members a, jf) in the job's form.  names: "<op>_scalars" and its _mixed, _keyed, _keyed_mixed, in
// the order of Form.  Single: the fixed-length single-key stage over the operation's own arguments; Derived<C, F>: the stage
// in a derived form.  The keyed forms are instantiated only where KEYED (the keyed translation units).
template <class C, bool KEYED, class Single, template <class, Form> class Derived, class J>
void add_scalar_stage(J* j, const char* const (&names)[4]) {
    using FA = FormArgs<C, decltype(j->a)>;
    const Form f = j->jf.form;
    const char* nm = names[(int)f];
    if constexpr (KEYED) {
        if (f == Form::KeyedMixed) j->stages.push_back({nm, [j]() { return rt::launch<Derived<C, Form::KeyedMixed>>(j->stream(), FA{j->a, j->jf.src}, j->n); }});
        else j->stages.push_back({nm, [j]() { return rt::launch<Derived<C, Form::Keyed>>(j->stream(), FA{j->a, j->jf.src}, j->n); }});
    } else if (f == Form::Mixed) j->stages.push_back({nm, [j]() { return rt::launch<Derived<C, Form::Mixed>>(j->stream(), FA{j->a, j->jf.src}, j->n); }});
    else j->stages.push_back({nm, [j]() { return rt::launch<Single>(j->stream(), j->a, j->n); }});
}
