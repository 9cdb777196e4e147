// Host orchestration of key registration (template over the curve); instantiated by tu_key_*.hip.  runtime.hpp Ctx has the
// contract of add_keys, stages_key.hpp the device stage.
#pragma once
#include "job_form.hpp"
#include "host_codec.hpp"
#include "stages_key.hpp"

// What a launch of KeyBuild takes that depends on the curve and the line form alone: the twist constant, the stand-in point, the
// Frobenius constants, the Miller loop count; n_steps = the steps of the walk (the workspace is sized by it).
template <class C>
int key_build_consts(KeyBuildArgs<C>& a, bool want_unit, size_t& n_steps) {
    const std::vector<int> bits = miller_bits<C>();
    n_steps = bits.size() + (C::ID == 1 ? 2 : 0);
    for (int b : bits) n_steps += b ? 1 : 0;
    if (bits.size() > (size_t)KEY_MAX_BITS || n_steps > (size_t)MAX_LINES) return BBS_E_STATE;
    a.b2 = g2_b<C>();
    const G2Aff<C> gen = g2_generator<C>();
    a.gen_x = gen.x; a.gen_y = gen.y;
    a.frob_x = f2_from_consts<C>(C::K::FROB[0][2][0], C::K::FROB[0][2][1]);
    a.frob_y = f2_from_consts<C>(C::K::FROB[0][3][0], C::K::FROB[0][3][1]);
    a.want_unit = want_unit ? 1 : 0;
    a.n_bits = (int)bits.size();
    for (size_t k = 0; k < bits.size(); k++) a.bits[k] = (uint8_t)bits[k];
    return BBS_OK;
}

// One key by the host functions (host_g2.hpp, host_codec.hpp): the reference the device stage is compared with, and the path
// of every registration call (runtime.hpp KEY_BUILD_ON_DEVICE).  e is filled completely (zero behind the lines); the status is the stage's.  The line
// entries are stored as the representatives in [0, p), as the stage stores them.
template <class C>
int8_t Ctx<C>::host_key_entry(const uint8_t* rec, bool is_inf, const uint8_t* oct, KeyEntry<C>& e, uint8_t* rec_out, int8_t* inf_out,
                              G2Aff<C>* q_out) const {
    using P = typename C::FpP;
    std::memset(&e, 0, sizeof(e));
    e.hash = key_hash0();
    e.tab.q_is_identity = 1;
    if (rec_out) std::memset(rec_out, 0, 4 * FPB);
    if (inf_out) *inf_out = 0;
    G2Aff<C> q{};
    if (oct) {
        const int rc = codec::g2_decompress<C>(oct, q);
        if (rc == -1) return (int8_t)BBS_ST_NONCANONICAL;
        if (rc) return (int8_t)BBS_ST_NOT_ON_CURVE;
    } else {
        q.inf = is_inf;
        if (q.inf) { q.x = f2_zero<C>(); q.y = f2_zero<C>(); }
        else if (!fe_from_le_bytes<P>(rec, q.x.c0) || !fe_from_le_bytes<P>(rec + FPB, q.x.c1) ||
                 !fe_from_le_bytes<P>(rec + 2 * FPB, q.y.c0) || !fe_from_le_bytes<P>(rec + 3 * FPB, q.y.c1)) return (int8_t)BBS_ST_NOT_ON_CURVE;
    }
    if (!g2_on_curve<C>(q) || !g2_in_subgroup<C>(q) || !build_line_table<C>(q, e.tab, lines_unit())) {
        std::memset(&e.tab, 0, sizeof(e.tab));
        e.tab.q_is_identity = 1;
        return (int8_t)BBS_ST_NOT_ON_CURVE;
    }
    for (int s = 0; s < e.tab.n_lines; s++) { e.tab.e[s].c = f2_canon<C>(e.tab.e[s].c); e.tab.e[s].nl = f2_canon<C>(e.tab.e[s].nl); }
    domain_midstate(q, e.hash);
    if (q_out) *q_out = q;
    if (oct) {
        if (inf_out) *inf_out = q.inf ? 1 : 0;
        if (rec_out && !q.inf) {
            fe_to_le_bytes<P>(q.x.c0, rec_out); fe_to_le_bytes<P>(q.x.c1, rec_out + FPB);
            fe_to_le_bytes<P>(q.y.c0, rec_out + 2 * FPB); fe_to_le_bytes<P>(q.y.c1, rec_out + 3 * FPB);
        }
    }
    return 1;
}

// n entries into d_out (device memory of the context's device): by the KeyBuild stage, or on host threads and one upload.
// Synchronises the context's stream.  status / rec_out / inf_out: host arrays, the last two may be null.
template <class C>
int Ctx<C>::key_build(KeyEntry<C>* d_out, size_t n, const uint8_t* rec, const int8_t* is_inf, const uint8_t* oct, bool on_device,
                      int8_t* status, uint8_t* rec_out, int8_t* inf_out, G2Aff<C>* q_out, size_t* n_other_form) {
    if (n_other_form) *n_other_form = 0;
    if (!n) return BBS_OK;
    if ((q_out || n_other_form) && on_device) return BBS_E_STATE;      // the host copies of the keys and the forms that came out: host path only
    if (!on_device) {
        std::vector<KeyEntry<C>> host(n);
        auto one = [&](size_t k) {
            status[k] = host_key_entry(rec ? rec + k * 4 * FPB : nullptr, !oct && is_inf && is_inf[k] != 0, oct ? oct + k * 2 * FPB : nullptr,
                                       host[k], rec_out ? rec_out + k * 4 * FPB : nullptr, inf_out ? inf_out + k : nullptr, q_out ? q_out + k : nullptr);
        };
        const size_t nt = std::min<size_t>({(size_t)16, n, (size_t)std::max(1u, std::thread::hardware_concurrency())});
        if (nt <= 1) { for (size_t k = 0; k < n; k++) one(k); }
        else {
            std::vector<std::thread> th;
            for (size_t t = 0; t < nt; t++) th.emplace_back([&, t]() { for (size_t k = t; k < n; k += nt) one(k); });
            for (auto& x : th) x.join();
        }
        // tables that came out in the other form than the context's: keys without a unit form (add_keys rebuilds every table)
        if (n_other_form)
            for (size_t k = 0; k < n; k++) *n_other_form += (!host[k].tab.q_is_identity && (host[k].tab.unit != 0) != lines_unit()) ? 1 : 0;
        if (rt::h2d(d_out, host.data(), n * sizeof(KeyEntry<C>), stream) || rt::sync(stream)) return BBS_E_HIP;
        return BBS_OK;
    }
    // what follows the key in the domain prefix, the same for every key: built once (domain_midstate hashes the same bytes)
    std::vector<uint8_t> blob(sizeof(HashCtx));
    {
        const HashCtx h0 = key_hash0();
        std::memcpy(blob.data(), &h0, sizeof(h0));
        for (int k = 7; k >= 0; k--) blob.push_back((uint8_t)((uint64_t)L >> (8 * k)));
        uint8_t buf[FPB];
        for (const auto& g : gens) { g1_compress_host<C>(g, buf); blob.insert(blob.end(), buf, buf + FPB); }
        blob.insert(blob.end(), api_id.begin(), api_id.end());
    }
    const size_t in_bytes = n * (oct ? 2 : 4) * FPB;
    DevBuf d_in, d_inf, d_st, d_rec, d_io, d_ws, d_blob;
    KeyBuildArgs<C> a{};
    size_t n_steps = 0;
    if (const int rc = key_build_consts<C>(a, lines_unit(), n_steps)) return rc;
    if (d_in.alloc(in_bytes) || d_st.alloc(n) || d_blob.alloc(blob.size()) || d_ws.alloc(key_build_ws_words<C>(n_steps) * n * 4)) return BBS_E_NOMEM;
    if (oct ? (d_rec.alloc(n * 4 * FPB) || d_io.alloc(n)) : (is_inf && d_inf.alloc(n))) return BBS_E_NOMEM;
    auto fail = [&](int rc) { (void)rt::sync(stream); return rc; };      // the buffers must not go back while the stream uses them
    if (rt::h2d_async(d_in.p, oct ? oct : rec, in_bytes, stream) || rt::h2d_async(d_blob.p, blob.data(), blob.size(), stream)) return fail(BBS_E_HIP);
    if (d_inf.p && rt::h2d_async(d_inf.p, is_inf, n, stream)) return fail(BBS_E_HIP);
    if (rt::dmemset(d_out, 0, n * sizeof(KeyEntry<C>), stream)) return fail(BBS_E_HIP);
    a.n = n;
    a.rec = oct ? nullptr : d_in.as<uint32_t>();
    a.is_inf = d_inf.as<int8_t>();
    a.oct = oct ? d_in.as<uint32_t>() : nullptr;
    a.out = d_out;
    a.status = d_st.as<int8_t>();
    a.rec_out = d_rec.as<uint32_t>();
    a.inf_out = d_io.as<int8_t>();
    a.ws = d_ws.as<uint32_t>();
    a.hash0 = d_blob.as<HashCtx>();
    a.suffix = d_blob.as<uint8_t>() + sizeof(HashCtx);
    a.suffix_len = (uint32_t)(blob.size() - sizeof(HashCtx));
    if (rt::launch<KeyBuild<C>>(stream, a, n)) return fail(BBS_E_HIP);
    if (rt::d2h_async(status, d_st.p, n, stream)) return fail(BBS_E_HIP);
    if (oct && rec_out && rt::d2h_async(rec_out, d_rec.p, n * 4 * FPB, stream)) return fail(BBS_E_HIP);
    if (oct && inf_out && rt::d2h_async(inf_out, d_io.p, n, stream)) return fail(BBS_E_HIP);
    return rt::sync(stream) ? BBS_E_HIP : BBS_OK;       // (the workspace and the inputs go back with the locals, behind the synchronisation)
}

template <class C>
int Ctx<C>::add_keys(bool replace, size_t n, const uint8_t* rec, const int8_t* is_inf, const uint8_t* oct, int8_t* key_status,
                     uint8_t* rec_out, int8_t* inf_out, uint32_t* first_index) {
    if (n && !rec && !oct) return BBS_E_ARG;
    if (!gens_set) return BBS_E_STATE;
    if (use()) return BBS_E_HIP;
    const std::shared_ptr<const KeySet> old = replace ? nullptr : keys;
    const size_t n_old = old ? old->n : 0;
    if (n_old + n > 0xFFFFFFF0u) return BBS_E_ARG;
    if (!n) { if (first_index) *first_index = (uint32_t)n_old; return BBS_OK; }
    std::shared_ptr<KeySet> ks(new KeySet());
    ks->n = n_old + n;
    ks->unit = lines_unit();
    size_t n_other_form = 0;
    {
        static std::atomic<uint64_t> next_lineage{1};
        ks->lineage = old ? old->lineage : next_lineage.fetch_add(1);
    }
    ks->status.assign(ks->n, (int8_t)BBS_ST_NOT_ON_CURVE);
    {
        G2Aff<C> id{};
        id.inf = true; id.x = f2_zero<C>(); id.y = f2_zero<C>();
        ks->pk.assign(ks->n, id);
    }
    if (ks->d.alloc(ks->n * sizeof(KeyEntry<C>))) return BBS_E_NOMEM;
    if (n_old) {
        std::copy(old->status.begin(), old->status.end(), ks->status.begin());
        std::copy(old->pk.begin(), old->pk.end(), ks->pk.begin());
        if (rt::d2d_async(ks->d.p, old->d.p, n_old * sizeof(KeyEntry<C>), stream)) return BBS_E_HIP;
    }
    if (const int rc = key_build(ks->d.template as<KeyEntry<C>>() + n_old, n, rec, is_inf, oct, KEY_BUILD_ON_DEVICE,
                                 ks->status.data() + n_old, rec_out, inf_out, KEY_BUILD_ON_DEVICE ? nullptr : ks->pk.data() + n_old,
                                 KEY_BUILD_ON_DEVICE ? nullptr : &n_other_form)) {
        (void)rt::sync(stream);      // (the copy of the old entries must not outlive the buffer it writes)
        return rc;
    }
    static_assert(!KEY_BUILD_ON_DEVICE, "KeySet::pk is filled by the host path: decode the keys here before KeyBuild registers them");
    // keyed jobs of mixed counts: the rows of the old keys are copied, only the n new keys are hashed; a failure leaves the old
    // set and its rows
    std::shared_ptr<const KeyLenSet> kl;
    if (keyed_mixed_lengths) {
        const std::shared_ptr<const KeySet> cks = ks;
        const std::shared_ptr<const KeyLenSet> okl = key_lens;
        const bool reuse = n_old && okl && okl->of.get() == old.get() && okl->stride == (size_t)L + 1;
        if (const int rc = build_key_lens(cks, reuse ? okl : nullptr, reuse ? n_old : 0, kl)) return rc;
    }
    key_lens = kl;
    if (key_status) std::memcpy(key_status, ks->status.data() + n_old, n);
    if (first_index) *first_index = (uint32_t)n_old;
    keys = std::move(ks);
    // a new key without a unit form, or the key that had none was just replaced: every table of the context changes form
    if (n_other_form || lines_form_stale()) return rebuild_lines();
    return BBS_OK;
}

// Every line table of the context again -- BP2's, the public key's, the key set's (a new immutable set: jobs keep the one they
// hold) -- in the form asked for (unit_lines); where one of them has no unit form, all of them in the (c, nl) form.  Only the
// tables are rebuilt: statuses, host copies, midstates and the prefixes per (key, length) are carried over.  Synchronises the
// context's stream.  Setter-time work on the host, as registration is.
template <class C>
int Ctx<C>::rebuild_lines() {
    if (use()) return BBS_E_HIP;
    const std::shared_ptr<const KeySet> old = keys;
    for (int want = unit_lines ? 1 : 0;; want = 0) {
        bool same = true;
        if (!build_line_table<C>(g2_generator<C>(), hc.tab_bp2, want != 0)) return BBS_E_STATE;
        same &= hc.tab_bp2.unit == want;
        if (pk_set) {
            if (!build_line_table<C>(pk, hc.tab_pk, want != 0)) return BBS_E_STATE;
            same &= hc.tab_pk.q_is_identity || hc.tab_pk.unit == want;
        }
        std::shared_ptr<KeySet> ks;
        if (same && old && old->n) {
            std::vector<KeyEntry<C>> host(old->n);
            if (rt::d2h(host.data(), old->d.p, old->n * sizeof(KeyEntry<C>), stream) || rt::sync(stream)) return BBS_E_HIP;
            for (size_t k = 0; k < old->n && same; k++) {
                if (old->status[k] != 1 || old->pk[k].inf) continue;
                LineTable<C>& t = host[k].tab;
                if (!build_line_table<C>(old->pk[k], t, want != 0)) return BBS_E_STATE;
                for (int s = 0; s < t.n_lines; s++) { t.e[s].c = f2_canon<C>(t.e[s].c); t.e[s].nl = f2_canon<C>(t.e[s].nl); }
                same &= t.unit == want;
            }
            if (same) {
                ks.reset(new KeySet());
                ks->n = old->n; ks->status = old->status; ks->pk = old->pk; ks->lineage = old->lineage; ks->unit = want != 0;
                if (ks->d.alloc(ks->n * sizeof(KeyEntry<C>))) return BBS_E_NOMEM;
                if (rt::h2d(ks->d.p, host.data(), ks->n * sizeof(KeyEntry<C>), stream) || rt::sync(stream)) return BBS_E_HIP;
            }
        }
        if (!same && want) continue;                    // a key without a unit form: everything in the (c, nl) form
        consts_dirty = true;
        if (ks) {
            std::shared_ptr<const KeyLenSet> kl;
            if (keyed_mixed_lengths) {
                const std::shared_ptr<const KeySet> cks = ks;
                const std::shared_ptr<const KeyLenSet> okl = key_lens;
                const bool reuse = okl && okl->of.get() == old.get() && okl->stride == (size_t)L + 1;
                if (const int rc = build_key_lens(cks, reuse ? okl : nullptr, reuse ? old->n : 0, kl)) return rc;
            }
            key_lens = kl;
            keys = std::move(ks);
        }
        return BBS_OK;
    }
}

// The prefixes per (key, length) of the keys [n_old, ks->n) on up to 16 host threads (the generators are compressed once), the
// rows [0, n_old) copied device to device from `old`; one upload; synchronises the context's stream.  Registration-time work:
// no device kernel, as key_build's host path (DESIGN.md 8 "Registration").
template <class C>
int Ctx<C>::build_key_lens(const std::shared_ptr<const KeySet>& ks, const std::shared_ptr<const KeyLenSet>& old, size_t n_old,
                           std::shared_ptr<const KeyLenSet>& out) {
    if (use()) return BBS_E_HIP;
    std::shared_ptr<KeyLenSet> kl(new KeyLenSet());
    kl->of = ks;
    kl->stride = (size_t)L + 1;
    const size_t S = kl->stride, n_new = ks->n - n_old;
    if (kl->d.alloc(ks->n * S * sizeof(HashCtx))) return BBS_E_NOMEM;
    if (n_old && rt::d2d_async(kl->d.p, old->d.p, n_old * S * sizeof(HashCtx), stream)) return BBS_E_HIP;
    std::vector<HashCtx> host(n_new * S, key_hash0());
    const std::vector<uint8_t> cg = compressed_gens();
    auto one = [&](size_t k) {
        if (ks->status[n_old + k] != 1) return;
        for (size_t l = 0; l < S; l++) domain_midstate(ks->pk[n_old + k], host[k * S + l], (int)l, cg.data());
    };
    const size_t nt = std::min<size_t>({(size_t)16, n_new, (size_t)std::max(1u, std::thread::hardware_concurrency())});
    if (nt <= 1) { for (size_t k = 0; k < n_new; k++) one(k); }
    else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nt; t++) th.emplace_back([&, t]() { for (size_t k = t; k < n_new; k += nt) one(k); });
        for (auto& x : th) x.join();
    }
    const bool bad = n_new && rt::h2d(kl->d.template as<HashCtx>() + n_old * S, host.data(), host.size() * sizeof(HashCtx), stream);
    if (rt::sync(stream) || bad) return BBS_E_HIP;      // (the copy of the old rows must not outlive the buffer it writes)
    out = std::move(kl);
    return BBS_OK;
}

template <class C>
int Ctx<C>::set_keyed_mixed_lengths(int enabled) {
    std::lock_guard<std::mutex> g(mu);
    if (keyed_mixed_lengths == (enabled != 0)) return BBS_OK;
    if (!enabled) { keyed_mixed_lengths = false; key_lens.reset(); return BBS_OK; }
    std::shared_ptr<const KeyLenSet> kl;
    if (const auto ks = keys) {
        if (const int rc = build_key_lens(ks, nullptr, 0, kl)) return rc;       // (the switch stays off)
    }
    key_lens = kl;
    keyed_mixed_lengths = true;
    return BBS_OK;
}

// bbs_selftest_key_entries: the entries, statuses and (octet form) decoded records of n keys by path 0 = the host functions,
// one key at a time, or path 1 = the KeyBuild stage whatever the key count; the context's key set is not touched
template <class C>
int selftest_key_entries(Ctx<C>* ctx, size_t n, const uint8_t* rec, const int8_t* is_inf, const uint8_t* oct, int path,
                         uint8_t* entries_out, int8_t* status_out, uint8_t* rec_out) {
    constexpr size_t FPB = Ctx<C>::FPB;
    if (!ctx->gens_set) return BBS_E_STATE;
    if (ctx->use()) return BBS_E_HIP;
    if (path == 0) {
        KeyEntry<C> e;
        for (size_t k = 0; k < n; k++) {
            status_out[k] = ctx->host_key_entry(rec ? rec + k * 4 * FPB : nullptr, !oct && is_inf && is_inf[k] != 0, oct ? oct + k * 2 * FPB : nullptr,
                                                e, oct && rec_out ? rec_out + k * 4 * FPB : nullptr, nullptr);
            std::memcpy(entries_out + k * sizeof(e), &e, sizeof(e));
        }
        return BBS_OK;
    }
    DevBuf d;
    if (d.alloc(n * sizeof(KeyEntry<C>))) return BBS_E_NOMEM;
    if (const int rc = ctx->key_build(d.as<KeyEntry<C>>(), n, rec, is_inf, oct, true, status_out, oct ? rec_out : nullptr, nullptr)) return rc;
    if (rt::d2h(entries_out, d.p, n * sizeof(KeyEntry<C>), ctx->stream) || rt::sync(ctx->stream)) return BBS_E_HIP;
    return BBS_OK;
}

// ---- job-local key sets (job_form.hpp JobKeys) ------------------------------------------------------------------------------
// The keys of one job on the job's stream st, asynchronously: the entries cleared (KeyBuild wants them zeroed), KeyBuild in its
// octet form over the strings in the job's staging image, and -- stride != 0: a job of mixed counts -- KeyLenBuild into the job's
// own rows.  Nothing is copied back; nothing waits.  Every buffer comes from the job (alloc) and lives as long as it does.
template <class C> int job_keys_publish(Ctx<C>* ctx, rt::Stream& st, JobKeys<C>& jk, uint32_t stride);
// KeyLenBuild over the nk keys the job prepares, into jk.rows
template <class C>
int job_key_rows_launch(rt::Stream& st, const JobKeys<C>& jk, const typename Ctx<C>::KeyBlob& kb, size_t nk, uint32_t stride) {
    KeyLenBuildArgs<C> la{};
    la.n_keys = nk; la.stride = stride; la.oct = jk.d_oct; la.key_status = jk.status;
    la.cg = kb.cg(); la.api_id = kb.api(); la.api_len = (uint32_t)kb.api_len;
    la.hash0 = kb.hash0(); la.out = jk.rows;
    return rt::launch<KeyLenBuild<C>>(st, la, nk * stride) ? BBS_E_HIP : BBS_OK;
}
// What a launch of KeyDomainBuild takes that depends on the curve alone, and the launch over n strings
template <class C>
int key_domain_launch(rt::Stream& st, size_t n, const uint32_t* d_oct, KeyEntry<C>* entries, int8_t* status, const typename Ctx<C>::KeyBlob& kb) {
    KeyDomainBuildArgs<C> a{};
    a.b2 = g2_b<C>();
    const G2Aff<C> gen = g2_generator<C>();
    a.gen_x = gen.x; a.gen_y = gen.y;
    a.n = n; a.oct = d_oct; a.out = entries; a.status = status;
    a.hash0 = kb.hash0(); a.suffix = kb.suffix(); a.suffix_len = (uint32_t)kb.suffix_len();
    if (rt::dmemset(entries, 0, n * sizeof(KeyEntry<C>), st)) return BBS_E_HIP;
    return rt::launch<KeyDomainBuild<C>>(st, a, n) ? BBS_E_HIP : BBS_OK;
}
// The keys of a proof_gen job that is not cached (JobKeys::domain_only): KeyDomainBuild in place of KeyBuild, the rest as below.
template <class C>
int job_keys_prepare_domain(rt::Stream& st, JobKeys<C>& jk, const typename Ctx<C>::KeyBlob& kb, uint32_t stride, const std::function<void*(size_t)>& alloc) {
    const size_t nk = jk.n_keys;
    jk.status = static_cast<int8_t*>(alloc(nk));
    if (stride) jk.rows = static_cast<HashCtx*>(alloc(nk * stride * sizeof(HashCtx)));
    if (!jk.status || (stride && !jk.rows)) return BBS_E_NOMEM;
    if (!nk) return BBS_OK;
    if (const int rc = key_domain_launch<C>(st, nk, jk.d_oct, jk.entries, jk.status, kb)) return rc;
    return stride ? job_key_rows_launch<C>(st, jk, kb, nk, stride) : (int)BBS_OK;
}
template <class C>
int job_keys_prepare(Ctx<C>* ctx, rt::Stream& st, JobKeys<C>& jk, bool unit, uint32_t stride, const std::function<void*(size_t)>& alloc,
                     std::shared_ptr<const void>& blob_held) {
    // (a cached job: its misses only, hashed with what its generation of the cache was built under)
    const size_t nk = jk.n_build();
    std::shared_ptr<const typename Ctx<C>::KeyBlob> kb;
    if (jk.cache) kb = jk.cache->blob;
    else if (const int rc = ctx->sync_key_blob(kb)) return rc;
    blob_held = kb;
    // (proof_gen, uncached: the domain-only stage -- no workspace, no line form; a cached job's misses fill whole slots below)
    if (jk.domain_only && !jk.cache) return job_keys_prepare_domain<C>(st, jk, *kb, stride, alloc);
    KeyBuildArgs<C> a{};
    size_t n_steps = 0;
    if (const int rc = key_build_consts<C>(a, unit, n_steps)) return rc;
    jk.status = static_cast<int8_t*>(alloc(nk));
    uint32_t* ws = static_cast<uint32_t*>(alloc(key_build_ws_words<C>(n_steps) * nk * 4));
    if (stride) jk.rows = static_cast<HashCtx*>(alloc(nk * stride * sizeof(HashCtx)));
    if (!jk.status || !ws || (stride && !jk.rows)) return BBS_E_NOMEM;
    if (!nk) return BBS_OK;
    if (rt::dmemset(jk.entries, 0, nk * sizeof(KeyEntry<C>), st)) return BBS_E_HIP;
    a.n = nk;
    a.oct = jk.d_oct;
    a.out = jk.entries;
    a.status = jk.status;
    a.ws = ws;
    a.hash0 = kb->hash0();
    a.suffix = kb->suffix();
    a.suffix_len = (uint32_t)kb->suffix_len();
    if (rt::launch<KeyBuild<C>>(st, a, nk)) return BBS_E_HIP;
    if (stride)
        if (const int rc = job_key_rows_launch<C>(st, jk, *kb, nk, stride)) return rc;
    return jk.cache ? job_keys_publish<C>(ctx, st, jk, stride) : (int)BBS_OK;
}
// A cached job's misses into their slots (KeyCachePublish), ONE event behind the kernel, and only then -- under the context's
// mutex -- the slots become hits for the jobs planned from now on, carrying the event: a job on another stream that hits one
// before the event has completed waits for it on the device (job_form.hpp paired_keyed_gate).
template <class C>
int job_keys_publish(Ctx<C>* ctx, rt::Stream& st, JobKeys<C>& jk, uint32_t stride) {
    typename Ctx<C>::KeyCacheGen& gen = *jk.cache;
    const size_t m = jk.n_build();
    if (stride != gen.stride) return BBS_E_STATE;
    KeyCachePublishArgs<C> pa{};
    pa.n_miss = m; pa.stride = stride; pa.slot_of = jk.d_slot_of;
    pa.src_entries = jk.entries; pa.src_status = jk.status; pa.src_rows = jk.rows;
    pa.dst_entries = gen.entries.template as<KeyEntry<C>>(); pa.dst_status = gen.status.template as<int8_t>(); pa.dst_rows = gen.rows.template as<HashCtx>();
    if (rt::launch<KeyCachePublish<C>>(st, pa, KeyCachePublish<C>::lanes(m, stride))) return BBS_E_HIP;
    auto ev = std::make_shared<typename Ctx<C>::KeyCacheEvent>();
    ev->device = ctx->device;
    if (rt::event_create(&ev->ev)) return BBS_E_HIP;
    ev->ok = true;
    if (rt::event_record(ev->ev, st)) return BBS_E_HIP;
    std::lock_guard<std::mutex> g(ctx->mu);
    gen.book.commit(*jk.plan);
    for (const uint32_t s : jk.plan->miss_slot) gen.slot_event[s] = ev;
    return BBS_OK;
}
template <class C>
int job_keys_gate(rt::Stream& st, const JobKeys<C>& jk, bool unit, size_t n, const uint32_t* kidx, int8_t* status0) {
    if (jk.domain_only) return rt::launch<JobKeyStatusGate>(st, JobKeyStatusGateArgs{n, kidx, jk.use_status(), status0}, n) ? BBS_E_HIP : BBS_OK;
    JobKeyGateArgs<C> g{n, kidx, jk.use_entries(), jk.use_status(), unit ? 1 : 0, status0};
    return rt::launch<JobKeyGate<C>>(st, g, n) ? BBS_E_HIP : BBS_OK;
}

// bbs_selftest_key_domain_entries: the entries and statuses of n strings by the KeyDomainBuild stage, read back from the device;
// the context's key set is not touched
template <class C>
int selftest_key_domain_entries(Ctx<C>* ctx, size_t n, const uint8_t* oct, uint8_t* entries_out, int8_t* status_out) {
    constexpr size_t FPB = Ctx<C>::FPB;
    if (!ctx->gens_set) return BBS_E_STATE;
    if (ctx->use()) return BBS_E_HIP;
    if (!n) return BBS_OK;
    std::shared_ptr<const typename Ctx<C>::KeyBlob> kb;
    if (const int rc = ctx->sync_key_blob(kb)) return rc;
    DevBuf d_oct, d_entries, d_st;
    if (d_oct.alloc(n * 2 * FPB) || d_entries.alloc(n * sizeof(KeyEntry<C>)) || d_st.alloc(n)) return BBS_E_NOMEM;
    int rc = rt::h2d(d_oct.p, oct, n * 2 * FPB, ctx->stream) ? BBS_E_HIP : BBS_OK;
    if (!rc) rc = key_domain_launch<C>(ctx->stream, n, d_oct.as<uint32_t>(), d_entries.as<KeyEntry<C>>(), d_st.as<int8_t>(), *kb);
    if (!rc && (rt::sync(ctx->stream) || rt::d2h(entries_out, d_entries.p, n * sizeof(KeyEntry<C>), ctx->stream) ||
                rt::d2h(status_out, d_st.p, n, ctx->stream))) rc = BBS_E_HIP;
    (void)rt::sync(ctx->stream);                  // (the buffers go back with the locals, behind the synchronisation)
    return rc;
}

// bbs_selftest_job_key_cache_entries: what the current generation of the cache holds for n strings -- entry, status and (where
// the cache holds rows and rows_out is given) the L + 1 rows of each, behind the publishing kernels that wrote them.
// BBS_E_STATE: the cache is off, or one of the strings is not resident.
template <class C>
int selftest_job_key_cache_entries(Ctx<C>* ctx, size_t n, const uint8_t* oct, uint8_t* entries_out, int8_t* status_out, uint8_t* rows_out) {
    if (ctx->use()) return BBS_E_HIP;
    std::shared_ptr<typename Ctx<C>::KeyCacheGen> gen;
    std::vector<uint32_t> slots(n);
    std::vector<std::shared_ptr<typename Ctx<C>::KeyCacheEvent>> evs;
    {
        std::lock_guard<std::mutex> g(ctx->mu);
        gen = ctx->job_key_cache;
        if (!gen) return BBS_E_STATE;
        for (size_t k = 0; k < n; k++) {
            if (!gen->book.find_ready(oct + k * 2 * Ctx<C>::FPB, slots[k])) return BBS_E_STATE;
            if (gen->slot_event[slots[k]]) evs.push_back(gen->slot_event[slots[k]]);
        }
    }
    for (const auto& e : evs)
        if (rt::stream_wait(ctx->stream, e->ev)) return BBS_E_HIP;
    if (rt::sync(ctx->stream)) return BBS_E_HIP;
    const size_t rb = (size_t)gen->stride * sizeof(HashCtx);
    for (size_t k = 0; k < n; k++) {
        const size_t s = slots[k];
        if (rt::d2h(entries_out + k * sizeof(KeyEntry<C>), gen->entries.template as<KeyEntry<C>>() + s, sizeof(KeyEntry<C>), ctx->stream) ||
            rt::d2h(status_out + k, gen->status.template as<int8_t>() + s, 1, ctx->stream)) return BBS_E_HIP;
        if (rows_out && rb && rt::d2h(rows_out + k * rb, gen->rows.template as<uint8_t>() + s * rb, rb, ctx->stream)) return BBS_E_HIP;
    }
    return rt::sync(ctx->stream) ? BBS_E_HIP : BBS_OK;
}

// bbs_selftest_key_len_rows: the prefixes per (key, length) of n keys given as octets, [n][L + 1] HashCtx, by path 0 = the host
// functions registration uses (host_key_entry's decisions, domain_midstate per length) or path 1 = the stages a job with a
// job-local key set runs (job_keys_prepare: KeyBuild, KeyLenBuild); the context's key set is not touched
template <class C>
int selftest_key_len_rows(Ctx<C>* ctx, size_t n, const uint8_t* oct, int path, uint8_t* rows_out, int8_t* status_out) {
    constexpr size_t FPB = Ctx<C>::FPB;
    if (!ctx->gens_set) return BBS_E_STATE;
    if (ctx->use()) return BBS_E_HIP;
    const size_t S = (size_t)ctx->L + 1;
    if (!n) return BBS_OK;
    if (path == 0) {
        const std::vector<uint8_t> cg = ctx->compressed_gens();
        std::vector<HashCtx> rows(n * S, ctx->key_hash0());
        KeyEntry<C> e;
        for (size_t k = 0; k < n; k++) {
            G2Aff<C> q{};
            q.inf = true; q.x = f2_zero<C>(); q.y = f2_zero<C>();
            status_out[k] = ctx->host_key_entry(nullptr, false, oct + k * 2 * FPB, e, nullptr, nullptr, &q);
            if (status_out[k] != 1) continue;
            for (size_t l = 0; l < S; l++) ctx->domain_midstate(q, rows[k * S + l], (int)l, cg.data());
        }
        std::memcpy(rows_out, rows.data(), rows.size() * sizeof(HashCtx));
        return BBS_OK;
    }
    std::vector<std::unique_ptr<DevBuf>> bufs;
    auto alloc = [&](size_t b) -> void* {
        bufs.emplace_back(new DevBuf());
        return bufs.back()->alloc(std::max<size_t>(b, 1)) ? nullptr : bufs.back()->p;
    };
    JobKeys<C> jk;
    jk.on = true; jk.n_keys = n;
    jk.entries = static_cast<KeyEntry<C>*>(alloc(n * sizeof(KeyEntry<C>)));
    uint32_t* d_oct = static_cast<uint32_t*>(alloc(n * 2 * FPB));
    if (!jk.entries || !d_oct) return BBS_E_NOMEM;
    jk.d_oct = d_oct;
    std::shared_ptr<const void> held;
    int rc = rt::h2d(d_oct, oct, n * 2 * FPB, ctx->stream) ? BBS_E_HIP : BBS_OK;
    if (!rc) rc = job_keys_prepare<C>(ctx, ctx->stream, jk, ctx->lines_unit(), (uint32_t)S, alloc, held);
    if (!rc && (rt::sync(ctx->stream) || rt::d2h(rows_out, jk.rows, n * S * sizeof(HashCtx), ctx->stream) ||
                rt::d2h(status_out, jk.status, n, ctx->stream))) rc = BBS_E_HIP;
    (void)rt::sync(ctx->stream);                  // (the buffers go back with the locals, behind the synchronisation)
    return rc;
}
