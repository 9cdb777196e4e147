// The form of a job (stages_common.hpp Form: Single, Mixed, Keyed, KeyedMixed), decided ONCE per upload and bound in one
// place for the four operations: the state a job keeps of its form, the checks of an upload, the key indexes and the pairing
// order built on the host, the prefixes the scalar stage reads, and the two launches that differ by form (ingest body, scalar
// stage).  An upload keeps what is its own: its buffers, its stage list, and for verify / proof_verify the pairing stage.
#pragma once
#include "runtime.hpp"

// keyed batch verification (bbs_ctx_set_keyed_batch_verification; pippenger.hpp): the plan keyed_bv_plan makes of a job whose
// context has the switch on, and the arguments of the five stages add_keyed_bv_stages builds on it.  G == 0: no group formed.
template <class C>
struct KeyedBv {
    uint32_t G = 0, n_segs = 0, items = 0;   // groups, segments, items that belong to a group
    size_t n_pos = 0;                        // positions of the bv order (a multiple of 4)
    // the plan's words in the job's staging image (offsets in words from `at`): pos_of_item[n], item_group[n], segs[3 n_segs],
    // grp_seg[2 G], grp_run[2 G], the virtual items' kidx[16 G], their pairing order [slots][wave keys], their gates [16 G bytes]
    size_t at = 0, o_grp = 0, o_segs = 0, o_gseg = 0, o_grun = 0, o_vkidx = 0, o_vslots = 0, o_gates = 0;
    size_t v_uni = 0, v_slots = 0;           // the virtual items' pairing order: uniform slots, all slots
    KeyedRlcPrepArgs<C> prep{};
    PipSegArgs<C> seg{};
    PairArgs<C> vpa{};                       // the 16 G virtual items: points = the groups' window sums, out = the verdicts
    PairKeyedArgs<C> vpair{};
    KeyedBvDecideArgs dec{};
    int8_t* verdicts = nullptr;              // [16 G], cleared before every run: a check that never ran reads as failed
};
// A job-local key set (bbs_*_with_keys_*): the distinct keys of ONE job arrive as compressed octets with the call, travel in the
// job's staging image and are prepared on the device by the job itself -- KeyBuild (stages_key.hpp), and KeyLenBuild where the job
// is of mixed counts -- on its main stream in front of its ingest kernel, into arrays the job owns and releases.  The context's
// key set is neither read nor changed.  The keys are prepared with the upload, once, as the ingest kernel runs once: a job
// that is run again (bbs_job_run) finds its entries, its key statuses and its ingest statuses as the first run did.
// What the host cannot know when it plans such a job is which keys are accepted: keyed_order gives every index < n_keys its slot,
// JobKeyGate decides on the device.  op_key.hpp has the launches (the kernels live in the key units only).
template <class C>
struct JobKeys {
    bool on = false;
    // proof_gen (bbs_*proof_gen*_with_keys_*): the job reads the `hash` of an entry and nothing else.  Uncached, its keys are
    // prepared by KeyDomainBuild (no line table, no workspace); its gate refuses no key for the form of its table.  The MISSES
    // of a cached job are prepared by the full KeyBuild all the same: a slot of the cache is whole, whoever published it.
    bool domain_only = false;
    size_t n_keys = 0;
    const uint8_t* pk_octets = nullptr;      // the caller's array (read while the staging words are planned)
    size_t oct_at = 0;                       // place of the strings in the staging words, in words
    const uint32_t* d_oct = nullptr;         // the strings on the device
    KeyEntry<C>* entries = nullptr;          // [n_keys]
    int8_t* status = nullptr;                // [n_keys] KeyBuild's codes: 1, BBS_ST_NONCANONICAL, BBS_ST_NOT_ON_CURVE
    HashCtx* rows = nullptr;                 // [n_keys][L + 1], jobs of mixed counts only
    std::vector<uint32_t> grp_key;           // keyed batch verification: key of group g (bbs_job_bv_report leaves refused keys out)
    std::vector<uint32_t> grp_items;
    // The job-local key cache (bbs_ctx_set_job_key_cache; runtime.hpp Ctx::KeyCacheGen, key_cache.hpp).  cache == null: the job is
    // not cached (switch off, or bypassed) and everything above is what it says.  Otherwise THE CACHE IS THE JOB'S KEY SET: the job
    // reads keys, key statuses and rows from the cache's arrays by SLOT.  The host plans in the job's own key numbering (counts,
    // pairing order, groups: those of the keyed twin) and then translates key -> slot in the places of the staging words that
    // hold a key id: kidx, the wave keys, the virtual items' kidx and wave keys (keyed_order).  entries / status / rows above
    // then hold the job's MISSES only, [n_build()], prepared as ever and copied into their slots by KeyCachePublish.
    // Both pointers are owned by JobBase::key_cache_pin, which outlives the job's streams.
    typename Ctx<C>::KeyCacheGen* cache = nullptr;
    KeyCachePlan* plan = nullptr;
    size_t slot_at = 0;                      // place of the misses' slots in the staging words
    const uint32_t* d_slot_of = nullptr;     // [n_build()] on the device
    std::vector<std::shared_ptr<typename Ctx<C>::KeyCacheEvent>> wait_events;     // of hit slots still being published (another job's stream)
    size_t n_build() const { return cache ? plan->miss_key.size() : n_keys; }
    const KeyEntry<C>* use_entries() const { return cache ? cache->entries.template as<KeyEntry<C>>() : entries; }
    const int8_t* use_status() const { return cache ? cache->status.template as<int8_t>() : status; }
    const HashCtx* use_rows() const { return cache ? cache->rows.template as<HashCtx>() : rows; }
};
// what a cached job holds of the cache from its upload until it is freed (a job may be run again): the generation and its pins
template <class C>
struct KeyCachePin {
    Ctx<C>* ctx = nullptr;
    std::shared_ptr<typename Ctx<C>::KeyCacheGen> gen;
    KeyCachePlan plan;
    ~KeyCachePin() {                         // (an upload that failed before its entries were on their way gives its slots back)
        if (!gen || !plan.planned) return;
        std::lock_guard<std::mutex> g(ctx->mu);
        gen->book.release(plan);
    }
};
// what a job keeps of its form
template <class C>
struct JobForm {
    Form form = Form::Single;
    DomainSrc<C> src{};                      // what the scalar stage reads (kidx: KEY_NONE = unknown / refused, decided by KeyGate)
    uint32_t* len = nullptr;                 // src.len as the MIXED ingest bodies write it
    JobKeys<C> jk{};                         // the job's own keys (bbs_*_with_keys_*); off: the context's key set
    bool mixed() const { return form_mixed(form); }
};
// verify / proof_verify: plus the keyed pairing order
template <class C>
struct PairedJobForm : JobForm<C> {
    PairKeyedArgs<C> pair{};                 // the pairing step (points, gate, output: copied from the job's PairArgs at launch)
    bool unit = false;                       // line form of the key set the job holds (KeySet::unit)
    KeyedBv<C> bv{};                         // keyed batch verification, where the context's switch was on at upload
};
// op_key.hpp (instantiated in tu_key_*.hip).  prepare: allocates status (and rows, stride = L + 1; 0: none) through `alloc`
// (device bytes owned by the job, null = no memory), clears the entries and launches KeyBuild (and KeyLenBuild) on st.
// gate: JobKeyGate behind the ingest kernel.
template <class C> int job_keys_prepare(Ctx<C>* ctx, rt::Stream& st, JobKeys<C>& jk, bool unit, uint32_t stride, const std::function<void*(size_t)>& alloc,
                                        std::shared_ptr<const void>& blob_held);
template <class C> int job_keys_gate(rt::Stream& st, const JobKeys<C>& jk, bool unit, size_t n, const uint32_t* kidx, int8_t* status0);
extern template int job_keys_prepare<BlsCurve>(Ctx<BlsCurve>*, rt::Stream&, JobKeys<BlsCurve>&, bool, uint32_t, const std::function<void*(size_t)>&, std::shared_ptr<const void>&);
extern template int job_keys_prepare<BnCurve>(Ctx<BnCurve>*, rt::Stream&, JobKeys<BnCurve>&, bool, uint32_t, const std::function<void*(size_t)>&, std::shared_ptr<const void>&);
extern template int job_keys_gate<BlsCurve>(rt::Stream&, const JobKeys<BlsCurve>&, bool, size_t, const uint32_t*, int8_t*);
extern template int job_keys_gate<BnCurve>(rt::Stream&, const JobKeys<BnCurve>&, bool, size_t, const uint32_t*, int8_t*);

// The form of an upload and its state checks.  The context's switches are read HERE, once: the checks, the stages and the
// data of the job all go by this one look, whatever a setter does meanwhile.  What differs per operation: the key set a keyed
// job needs (Ctx::keys, sign: Ctx::sign_keys), the single-key switch (mixed_lengths, producing side: mixed_lengths_gen) and
// the single key (pk_set, sign: sk_set).
enum class FormOp { Verify, ProofGen, Sign };          // Verify: verify and proof_verify
template <bool KEYED, class C>
int decide_form(const Ctx<C>* ctx, FormOp op, size_t n, const uint32_t* key_index, Form& form, bool job_keys = false) {
    // (job_keys: the job brings its own key set -- the context's is not looked at and need not exist)
    const bool have_key_set = job_keys || (op == FormOp::Sign ? ctx->sign_keys != nullptr : ctx->keys != nullptr);
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
// The ordering itself, for n items with keys kid[i] (KEY_NONE: in no slot) and cnt[k] items per key: `order` = [uniform
// slots][mixed slots][wave keys].  It orders the real items of a job and the virtual items of keyed batch verification alike.
inline void keyed_slots(const uint32_t* kid, size_t n, const std::vector<uint32_t>& cnt, std::vector<uint32_t>& order, size_t& n_uni, size_t& n_slots) {
    constexpr uint32_t W = (uint32_t)KEY_SLOTS_PER_WAVE;
    const size_t nk = cnt.size();
    std::vector<uint32_t> ufirst(nk), mfirst(nk), seen(nk, 0);
    size_t nu = 0, nm = 0;
    for (size_t k = 0; k < nk; k++) {
        ufirst[k] = (uint32_t)nu; nu += cnt[k] / W * W;
        mfirst[k] = (uint32_t)nm; nm += cnt[k] % W;
    }
    order.assign(nu + nm + nu / W, 0);
    uint32_t* uslot = order.data();
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
    n_uni = nu; n_slots = nu + nm;
}
// Keyed batch verification, beside the slot map: the BV ORDER of a job (pippenger.hpp).  Key k forms a group iff cnt[k] >=
// min_items; the grouped items are sorted by key, stably, every group's run starting at a multiple of 4; a run is cut into
// segments of at most PIP_TILE items; group g has the 16 virtual items g * 16 + w under its key, ordered for the pairing
// kernel by keyed_slots as real items are.  Appends the plan to `words` (layout: KeyedBv) -- nothing where no group forms.
template <class C>
void keyed_bv_plan(size_t n, const std::vector<uint32_t>& cnt, size_t min_items, KeyedBv<C>& bv, std::vector<uint32_t>& words) {
    const size_t nk = cnt.size();
    std::vector<uint32_t> group_of(nk, BV_NONE), first, seen;
    std::vector<uint32_t> vcnt(nk, 0);
    size_t cur = 0, items = 0;
    uint32_t G = 0;
    for (size_t k = 0; k < nk; k++) {
        if (!cnt[k] || cnt[k] < min_items) continue;
        group_of[k] = G++;
        vcnt[k] = 16;
        first.push_back((uint32_t)cur);
        cur += ((size_t)cnt[k] + 3) & ~(size_t)3;
        items += cnt[k];
    }
    bv = KeyedBv<C>{};
    if (!G || cur > 0xFFFFFFF0ull) return;
    bv.G = G; bv.items = (uint32_t)items; bv.n_pos = cur;
    seen.assign(G, 0);
    std::vector<uint32_t> pw(2 * n, BV_NONE);           // pos_of_item, item_group
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = words[i];                     // (kidx of the real items)
        const uint32_t g = k == KEY_NONE ? BV_NONE : group_of[k];
        if (g == BV_NONE) continue;
        pw[i] = first[g] + seen[g]++;
        pw[n + i] = g;
    }
    bv.o_grp = n;
    bv.o_segs = pw.size();
    std::vector<uint32_t> gseg(2 * (size_t)G), grun(2 * (size_t)G), vkid(16 * (size_t)G);
    uint32_t n_segs = 0;
    for (size_t k = 0; k < nk; k++) {
        const uint32_t g = group_of[k];
        if (g == BV_NONE) continue;
        gseg[2 * g] = n_segs;
        for (uint32_t off = 0; off < cnt[k]; off += PIP_TILE) {
            pw.push_back(first[g] + off); pw.push_back(std::min<uint32_t>(PIP_TILE, cnt[k] - off)); pw.push_back(g);
            n_segs++;
        }
        gseg[2 * g + 1] = n_segs - gseg[2 * g];
        grun[2 * g] = first[g]; grun[2 * g + 1] = cnt[k];
        for (int w = 0; w < 16; w++) vkid[16 * (size_t)g + w] = (uint32_t)k;
    }
    bv.n_segs = n_segs;
    bv.o_gseg = pw.size(); pw.insert(pw.end(), gseg.begin(), gseg.end());
    bv.o_grun = pw.size(); pw.insert(pw.end(), grun.begin(), grun.end());
    bv.o_vkidx = pw.size(); pw.insert(pw.end(), vkid.begin(), vkid.end());
    std::vector<uint32_t> vorder;
    keyed_slots(vkid.data(), vkid.size(), vcnt, vorder, bv.v_uni, bv.v_slots);
    bv.o_vslots = pw.size(); pw.insert(pw.end(), vorder.begin(), vorder.end());
    bv.o_gates = pw.size(); pw.insert(pw.end(), 4 * (size_t)G, 0x01010101u);       // 16 G gate bytes, all 1
    bv.at = words.size();
    words.insert(words.end(), pw.begin(), pw.end());
}
// A job-local key set in the staging words, shared by the paired jobs (keyed_order) and proof_gen (keyed_indexes).
// to_slots: a cached job planned in its own key numbering; `count` words that hold a key id become slots of the cache.
// strings: behind the plan, the strings of the keys the job prepares -- all of them, or a cached job's misses and then their slots.
template <class C>
void job_keys_to_slots(const JobKeys<C>& jk, uint32_t* w, size_t count) {
    const KeyCachePlan& p = *jk.plan;
    for (size_t i = 0; i < count; i++) if (w[i] != KEY_NONE) w[i] = p.slot_of[w[i]];
}
template <class C>
void job_keys_strings(JobKeys<C>& jk, std::vector<uint32_t>& words) {
    constexpr size_t KW = 2 * C::FpP::NC, KB = 2 * Ctx<C>::FPB;
    jk.oct_at = words.size();
    if (!jk.cache) {
        words.resize(jk.oct_at + jk.n_keys * KW);
        if (jk.n_keys) std::memcpy(words.data() + jk.oct_at, jk.pk_octets, jk.n_keys * KB);
        return;
    }
    const KeyCachePlan& p = *jk.plan;
    const size_t m = p.miss_key.size();
    jk.slot_at = jk.oct_at + m * KW;
    words.resize(jk.slot_at + m);
    for (size_t t = 0; t < m; t++) {
        std::memcpy(words.data() + jk.oct_at + t * KW, jk.pk_octets + (size_t)p.miss_key[t] * KB, KB);
        words[jk.slot_at + t] = p.miss_slot[t];
    }
}
// A job-local key set (jf.jk.on): the set is the job's own, every index < n_keys counts as accepted here (JobKeyGate decides on
// the device), and the key strings follow the plan in `words`.
template <class C, class J>
void keyed_order(J* j, Ctx<C>* ctx, size_t n, const uint32_t* key_index, PairedJobForm<C>& jf, std::vector<uint32_t>& words) {
    JobKeys<C>& jk = jf.jk;
    const auto ks = jk.on ? nullptr : ctx->keys;
    j->key_set = ks;
    const size_t nk = jk.on ? jk.n_keys : (ks ? ks->n : 0);     // (no set: only where bbs_ctx_set_keyed_mixed_lengths is on -- every index is unknown)
    std::vector<uint32_t> cnt(nk, 0);
    words.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        const uint32_t k = key_index[i];
        const bool ok = k < nk && (jk.on || ks->status[k] == 1);
        words[i] = ok ? k : KEY_NONE;
        if (ok) cnt[k]++;
    }
    std::vector<uint32_t> order;
    size_t nu = 0, ns = 0;
    keyed_slots(words.data(), n, cnt, order, nu, ns);
    words.insert(words.end(), order.begin(), order.end());
    jf.src.keys = jk.on ? jk.use_entries() : (ks ? ks->d.template as<KeyEntry<C>>() : nullptr);
    jf.pair.keys = jf.src.keys; jf.pair.n_uni = nu; jf.pair.n_slots = ns;
    jf.unit = ks ? ks->unit : ctx->lines_unit();
    if (ctx->keyed_bv) keyed_bv_plan<C>(n, cnt, ctx->keyed_bv_min, jf.bv, words);
    if (!jk.on) return;
    if (jf.bv.G)                               // (the groups in key order, as keyed_bv_plan numbers them)
        for (size_t k = 0; k < nk; k++)
            if (cnt[k] && cnt[k] >= ctx->keyed_bv_min) { jk.grp_key.push_back((uint32_t)k); jk.grp_items.push_back(cnt[k]); }
    if (jk.cache) {
        // a cached job: everything above was planned in the job's numbering; now key -> slot wherever the words hold a key id
        job_keys_to_slots<C>(jk, words.data(), n);                                                      // kidx
        job_keys_to_slots<C>(jk, words.data() + n + ns, nu / KEY_SLOTS_PER_WAVE);                       // the wave keys
        if (jf.bv.G) {
            uint32_t* b = words.data() + jf.bv.at;
            job_keys_to_slots<C>(jk, b + jf.bv.o_vkidx, (size_t)16 * jf.bv.G);                          // the virtual items' kidx
            job_keys_to_slots<C>(jk, b + jf.bv.o_vslots + jf.bv.v_slots, jf.bv.v_uni / KEY_SLOTS_PER_WAVE);     // and their wave keys
        }
    }
    job_keys_strings<C>(jk, words);
}
// the device half of a job-local key set, behind the staging image: d = the words' place on the device
template <class C>
void job_keys_bind(JobKeys<C>& jk, const uint32_t* d) { jk.d_oct = d + jk.oct_at; jk.d_slot_of = d + jk.slot_at; }
// the same look at the key set for a job without a pairing step (keyed proof_gen): `words` = [kidx n] and nothing else
// A job-local key set (jf.jk.on) as in keyed_order: every index < n_keys is passed on (the gate decides on the device), a cached
// job's indexes become slots, and the key strings follow.
template <class C, class J>
void keyed_indexes(J* j, Ctx<C>* ctx, size_t n, const uint32_t* key_index, JobForm<C>& jf, std::vector<uint32_t>& words) {
    if (JobKeys<C>& jk = jf.jk; jk.on) {
        j->key_set = nullptr;
        words.resize(n);
        for (size_t i = 0; i < n; i++) words[i] = key_index[i] < jk.n_keys ? key_index[i] : KEY_NONE;
        if (jk.cache) job_keys_to_slots<C>(jk, words.data(), n);
        job_keys_strings<C>(jk, words);
        jf.src.keys = jk.use_entries();
        return;
    }
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
// A job-local key set, first half (in front of keyed_order): the checks of the call and the entries' array, which the plan points at.
// on = the upload came through a bbs_*_with_keys_* export.
// With the job-local key cache on, the look at the cache happens here as well (jf.form has been decided): the generation of the
// job's form, the plan of its keys -- hits pinned, slots claimed for the misses, or the job bypassed -- and the events of hit
// slots another job is still publishing.  The job's own arrays then hold its misses only.
template <class C, class J>
int job_keys_cache_plan(J* j, Ctx<C>* ctx, JobForm<C>& jf) {
    JobKeys<C>& jk = jf.jk;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        if (!ctx->job_key_cache_cap) return BBS_OK;
    }
    std::shared_ptr<const typename Ctx<C>::KeyBlob> kb;
    if (const int rc = ctx->sync_key_blob(kb)) return rc;
    const uint32_t stride = jf.form == Form::KeyedMixed ? (uint32_t)ctx->L + 1 : 0;
    auto pin = std::make_shared<KeyCachePin<C>>();      // (declared in front of the lock: its destructor takes it)
    pin->ctx = ctx;
    std::lock_guard<std::mutex> g(ctx->mu);
    if (!ctx->job_key_cache_cap) return BBS_OK;
    if (const int rc = ctx->job_key_cache_gen(kb, ctx->lines_unit(), stride, pin->gen)) return rc;
    if (!pin->gen->book.plan(jk.pk_octets, jk.n_keys, pin->plan, ctx->job_key_cache_counters)) {
        ctx->job_key_cache_counters.bypassed_jobs++;
        j->key_cache_bypassed = true;
        return BBS_OK;
    }
    for (const uint32_t s : pin->plan.hit_slots) {
        auto& e = pin->gen->slot_event[s];
        if (!e) continue;
        if (rt::event_done(e->ev)) { e.reset(); continue; }
        if (std::find(jk.wait_events.begin(), jk.wait_events.end(), e) == jk.wait_events.end()) jk.wait_events.push_back(e);
    }
    jk.cache = pin->gen.get(); jk.plan = &pin->plan;
    j->key_cache_hits = pin->plan.hits; j->key_cache_misses = pin->plan.misses;
    j->key_cache_pin = pin;
    return BBS_OK;
}
template <class C, class J>
int job_keys_begin(J* j, Ctx<C>* ctx, bool on, size_t n_keys, const uint8_t* pk_octets, JobForm<C>& jf, bool domain_only = false) {
    JobKeys<C>& jk = jf.jk;
    jk.on = on;
    if (!on) return BBS_OK;
    jk.domain_only = domain_only;
    if ((n_keys && !pk_octets) || n_keys > 0xFFFFFFF0ull) return BBS_E_ARG;
    jk.n_keys = n_keys; jk.pk_octets = pk_octets;
    j->has_job_keys = true;
    if (const int rc = job_keys_cache_plan<C>(j, ctx, jf)) return rc;
    int rc = BBS_OK;
    jk.entries = j->template scratch<KeyEntry<C>>(std::max<size_t>(jk.n_build(), 1), rc);
    return rc;
}
// second half, behind form_bind and in front of the ingest kernel: the key stage (and KeyLenBuild) on the job's main stream, the
// job's own prefixes per (key, length) bound, bbs_job_key_statuses answered from the device array on request.  unit: the line
// form of the tables the job reads (a paired job's jf.unit) or, where it reads none (proof_gen), the context's -- the form a
// cached job's misses are published in.
template <class C, class J>
int job_keys_launch(J* j, Ctx<C>* ctx, JobForm<C>& jf, bool unit) {
    JobKeys<C>* jk = &jf.jk;
    if (!jk->on) return BBS_OK;
    const uint32_t stride = jf.form == Form::KeyedMixed ? (uint32_t)ctx->L + 1 : 0;
    if (jk->cache && (jk->cache->unit != unit || jk->cache->stride != stride)) return BBS_E_STATE;      // (a form switched between the two looks: fail closed)
    auto alloc = [j](size_t b) -> void* { int rc = BBS_OK; return j->template scratch<uint8_t>(std::max<size_t>(b, 1), rc); };
    if (const int rc = job_keys_prepare<C>(ctx, j->stream(), *jk, unit, stride, alloc, j->key_blob)) return rc;
    if (stride) jf.src.pref = jk->use_rows();
    j->key_statuses = [j, jk](std::vector<int8_t>& v) {
        v.assign(jk->n_keys, 0);
        if (j->use() || rt::sync(j->stream())) return (int)BBS_E_HIP;
        if (!jk->n_keys) return (int)BBS_OK;
        if (!jk->cache) return rt::d2h(v.data(), jk->status, v.size(), j->stream()) ? (int)BBS_E_HIP : (int)BBS_OK;
        // a cached job: the codes of its slots, in the job's key order (one copy of the span of slots it names)
        const std::vector<uint32_t>& slot_of = jk->plan->slot_of;
        const auto mm = std::minmax_element(slot_of.begin(), slot_of.end());
        std::vector<int8_t> span((size_t)*mm.second - *mm.first + 1);
        if (rt::d2h(span.data(), jk->use_status() + *mm.first, span.size(), j->stream())) return (int)BBS_E_HIP;
        for (size_t k = 0; k < v.size(); k++) v[k] = span[slot_of[k] - *mm.first];
        return (int)BBS_OK;
    };
    return BBS_OK;
}
// the device half: d = the words' place in the device copy of the staging image
template <class C>
void keyed_bind(JobForm<C>& jf, const uint32_t* d) {
    jf.src.kidx = d;
    if (jf.jk.on) job_keys_bind<C>(jf.jk, d);
}
template <class C>
void keyed_bind(PairedJobForm<C>& jf, size_t n, const uint32_t* d) {
    jf.src.kidx = d;
    jf.pair.kidx = d; jf.pair.slot_item = d + n; jf.pair.wave_key = d + n + jf.pair.n_slots;
    if (jf.jk.on) job_keys_bind<C>(jf.jk, d);
    KeyedBv<C>& bv = jf.bv;
    if (!bv.G) return;
    const uint32_t* b = d + bv.at;
    bv.prep.pos_of_item = b;
    bv.dec.item_group = b + bv.o_grp;
    bv.seg.segs = b + bv.o_segs; bv.seg.grp_seg = b + bv.o_gseg; bv.seg.grp_run = b + bv.o_grun;
    bv.vpair.keys = jf.pair.keys; bv.vpair.kidx = b + bv.o_vkidx;
    bv.vpair.slot_item = b + bv.o_vslots; bv.vpair.wave_key = b + bv.o_vslots + bv.v_slots;
    bv.vpair.n_uni = bv.v_uni; bv.vpair.n_slots = bv.v_slots;
    bv.vpa.gate_arr = reinterpret_cast<const int8_t*>(b + bv.o_gates);
}
// behind the ingest stage: items with an unknown key are decided (BBS_ST_UNKNOWN_KEY)
template <class J>
int keyed_gate(J* j, size_t n, const uint32_t* kidx, int8_t* status0) {
    return rt::launch<KeyGate>(j->stream(), KeyGateArgs{n, kidx, status0}, n) ? BBS_E_HIP : BBS_OK;
}
// the same place in a job that may bring its own keys: the context's key set, or the job's own (JobKeyGate, proof_gen:
// JobKeyStatusGate -- the device decides); unit: the line form of the job (not looked at by proof_gen's gate)
template <class C, class J>
int job_keyed_gate(J* j, size_t n, const JobForm<C>& jf, bool unit, int8_t* status0) {
    if (!jf.jk.on) return keyed_gate(j, n, jf.src.kidx, status0);
    // a cached job that hit a slot another job is still publishing: its main stream waits on the device, here, in front of the
    // first kernel that reads an entry (the host never waits)
    for (const auto& e : jf.jk.wait_events)
        if (rt::stream_wait(j->stream(), e->ev)) return BBS_E_HIP;
    return job_keys_gate<C>(j->stream(), jf.jk, unit, n, jf.src.kidx, status0);
}
template <class C, class J>
int paired_keyed_gate(J* j, size_t n, const PairedJobForm<C>& jf, int8_t* status0) { return job_keyed_gate<C>(j, n, jf, jf.unit, status0); }
#if !defined(BBS_HOST_TWIN)
// the keyed fused kernel over the slots of the pairing order (runtime.hpp launch_line_form)
template <class C>
inline int launch_pair_fused_keyed(rt::Stream& st, bool unit, const PairKeyedArgs<C>& ka) {
    return launch_line_form<PairDistKeyed, C>(st, unit, ka, pair6_threads(ka.n_slots));
}
#endif
// the pairing step of a keyed job on the main (aux = 0) or second stream, as add_pairing_stages: the fused kernel in both job
// forms.  pair->p is copied from *pa when the stage is launched.  pair = null: the job's real items (jf->pair) under the usual
// stage names; keyed batch verification passes its virtual items and its own names.
template <class C, class J>
void add_keyed_pairing_stages(J* j, PairedJobForm<C>* jf, const PairArgs<C>* pa, int aux, PairKeyedArgs<C>* pair = nullptr,
                              [[maybe_unused]] const char* nm = nullptr, [[maybe_unused]] const char* nm_final = nullptr) {
    if (!pair) pair = &jf->pair;
#ifdef BBS_HOST_TWIN
    j->stages.push_back({nm ? nm : "pair_miller_keyed", [j, pair, pa, aux]() {
        pair->p = *pa;
        return rt::launch<PairMillerKeyed<C>>(aux ? j->stream_aux() : j->stream(), *pair, pair->n_slots * 2);
    }, aux, 0});
    j->stages.push_back({nm_final ? nm_final : "pair_final_exp", [j, pa, aux]() { return rt::launch<PairFinal<C>>(aux ? j->stream_aux() : j->stream(), *pa, pa->n); }, aux, 0});
#else
    j->stages.push_back({nm ? nm : "pairing_6lane_keyed", [j, jf, pair, pa, aux]() {
        pair->p = *pa;
        // the key set the job holds and BP2's table on the device must agree (they do unless the form was switched under the job)
        if (jf->unit != j->ctx->dev_lines_unit) return -1;
        return launch_pair_fused_keyed<C>(aux ? j->stream_aux() : j->stream(), jf->unit, *pair);
    }, aux, 0});
#endif
}

// Keyed batch verification: the five stages of pippenger.hpp on the job's main stream, in front of the per-item keyed pairing
// step.  pa / pb: the two points of every item, Montgomery SoA [2N][n]; the items that take part are those with status ==
// ST_PAIRING.  No group (switch off, or no key reaches the threshold): nothing is added and the job is what it was.
// The job must have been planned (keyed_order) and bound (keyed_bind).
template <class C, class J>
int add_keyed_bv_stages(J* j, Ctx<C>* ctx, PairedJobForm<C>* jf, size_t n, const CtxConsts<C>* cc, const uint32_t* pa, const uint32_t* pb,
                        int negate_b, int8_t* status) {
    constexpr int N = C::FpP::N;
    constexpr int NW = 16, M = 2;
    KeyedBv<C>* bv = &jf->bv;
    if (!bv->G) return BBS_OK;
    const size_t NV = (size_t)NW * bv->G;
    int rc = BBS_OK;
    uint8_t* dig = j->template scratch<uint8_t>((size_t)NW * bv->n_pos + 4, rc);
    uint32_t* ppts = j->template scratch<uint32_t>((size_t)M * bv->n_pos * 2 * N, rc);
    uint32_t* seg_sums = j->template scratch<uint32_t>((size_t)3 * N * M * NW * bv->n_segs, rc);
    uint32_t* out = j->template scratch<uint32_t>((size_t)M * 2 * N * NV, rc);
    bv->verdicts = j->template scratch<int8_t>(NV, rc);
    if (rc) return rc;
    // pad positions are never written: their digits stay 0 (and their points the identity) for every run of the job
    if (rt::dmemset(dig, 0, (size_t)NW * bv->n_pos, j->stream()) || rt::dmemset(ppts, 0, (size_t)M * bv->n_pos * 2 * N * 4, j->stream())) return BBS_E_HIP;
    j->zero_on_reset.push_back({bv->verdicts, NV});
    RlcPrepArgs<C>& pr = bv->prep.r;
    pr.n = n; pr.n_pad = bv->n_pos; pr.pa = pa; pr.pb = pb; pr.canonical = 0; pr.gate_arr = status; pr.gate = ST_PAIRING;
    pr.dig = dig; pr.ppts = ppts;
    ctx->next_rlc_seed(pr.seed);
    PipSegArgs<C>& sg = bv->seg;
    sg.n_pos = bv->n_pos; sg.M = M; sg.NW = NW; sg.n_segs = bv->n_segs; sg.n_groups = bv->G;
    sg.ppts = ppts; sg.dig = dig; sg.seg_sums = seg_sums; sg.out = out;
    PairArgs<C>& ps = bv->vpa;
    ps.n = NV; ps.cc = cc; ps.pa = out; ps.pb = out + (size_t)2 * N * NV; ps.negate_b = negate_b; ps.canonical = 0;
    ps.gate = 1; ps.out = bv->verdicts; ps.fmiller = nullptr; ps.batch_ok = nullptr; ps.n_checks = 0;
#ifdef BBS_HOST_TWIN
    ps.fmiller = j->template scratch<uint32_t>((size_t)2 * 12 * N * NV, rc);      // (the fused device kernel keeps the Miller values in registers)
    if (rc) return rc;
#endif
    bv->dec.n = n; bv->dec.verdicts = bv->verdicts; bv->dec.status = status;
    j->stages.push_back({"keyed_rlc_prep", [j, bv]() { return rt::launch<KeyedRlcPrep<C>>(j->stream(), bv->prep, j->n); }});
#ifdef BBS_HOST_TWIN
    j->stages.push_back({"keyed_pip_windows", [j, bv]() { return rt::launch<PipGroupSumsHost<C>>(j->stream(), bv->seg, (size_t)bv->seg.M * bv->seg.NW * bv->seg.n_groups); }});
#else
    j->stages.push_back({"keyed_pip_windows", [j, bv]() { return rt::launch_pip_window_segs<C>(j->stream(), bv->seg); }});
#endif
    j->stages.push_back({"keyed_pip_group_sums", [j, bv]() { return rt::launch<PipGroupSums<C>>(j->stream(), bv->seg, (size_t)bv->seg.M * bv->seg.NW * bv->seg.n_groups); }});
    add_keyed_pairing_stages<C>(j, jf, &bv->vpa, 0, &bv->vpair, "keyed_rlc_pairing", "keyed_rlc_pair_final_exp");
    j->stages.push_back({"keyed_bv_decide", [j, bv]() { return rt::launch<KeyedBvDecide>(j->stream(), bv->dec, j->n); }});
    // bbs_job_bv_report: groups formed, groups whose 16 checks all passed (the verdicts read back on request), grouped items
    // bbs_job_bv_verdicts: the same flags as they are, entry g * 16 + w
    j->bv_verdicts = [j, bv](std::vector<int8_t>& v) {
        v.assign((size_t)16 * bv->G, 0);
        if (j->use() || rt::sync(j->stream())) return (int)BBS_E_HIP;
        return rt::d2h(v.data(), bv->verdicts, v.size(), j->stream()) ? (int)BBS_E_HIP : (int)BBS_OK;
    };
    j->bv_report = [j, bv](uint32_t* groups, uint32_t* passed, uint32_t* items) {
        std::vector<int8_t> v;
        if (const int rc = j->bv_verdicts(v)) return rc;
        uint32_t ok = 0;
        for (uint32_t g = 0; g < bv->G; g++) {
            bool all = true;
            for (int w = 0; w < 16; w++) all &= v[(size_t)g * 16 + w] == 1;
            ok += all ? 1u : 0u;
        }
        *groups = bv->G; *passed = ok; *items = bv->items;
        return (int)BBS_OK;
    };
    // a job-local key set: the groups of the keys KeyBuild refused (all their items gated, their checks over nothing) are left
    // out, so that the report is the one of a keyed job over the registered set, where such a key forms no group
    if (jf->jk.on) {
        const JobKeys<C>* jk = &jf->jk;
        j->bv_report = [j, bv, jk](uint32_t* groups, uint32_t* passed, uint32_t* items) {
            std::vector<int8_t> v, ks;
            if (const int rc = j->bv_verdicts(v)) return rc;
            if (const int rc = j->key_statuses(ks)) return rc;
            uint32_t G = 0, ok = 0, it = 0;
            for (uint32_t g = 0; g < bv->G; g++) {
                if (ks[jk->grp_key[g]] != 1) continue;
                bool all = true;
                for (int w = 0; w < 16; w++) all &= v[(size_t)g * 16 + w] == 1;
                G++; ok += all ? 1u : 0u; it += jk->grp_items[g];
            }
            *groups = G; *passed = ok; *items = it;
            return (int)BBS_OK;
        };
    }
    return BBS_OK;
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
