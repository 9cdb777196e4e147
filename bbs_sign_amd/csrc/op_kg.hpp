// Host orchestration of batched key generation (template over the curve); instantiated by tu_kg_*.hip.  stages_kg.hpp has
// the two device stages.  Both calls are one-shot primitives in the pattern of h2s_batch (op_prim.hpp): they need a context
// for its curve, device and stream only -- no generators, no key -- and touch nothing of it.
// Secrets.  Every device buffer and every host staging buffer that held key material or secret keys is cleared before it
// goes back to the runtime's pools or to the allocator: the device buffers by rt::dmemset on the stream ahead of the final
// synchronisation, the host copies behind it (KgSecrets).  The caller's own input is `const` and stays the caller's business.
#pragma once
#include "runtime.hpp"
#include "stages_kg.hpp"

// memset that the compiler may not drop although the memory is released next
inline void kg_wipe(void* p, size_t b) {
    if (!b) return;
    std::memset(p, 0, b);
    __asm__ __volatile__("" : : "r"(p) : "memory");
}

// what a call must clear on every way out: device buffers (on the stream, then ONE synchronisation) and host memory
struct KgSecrets {
    rt::Stream& stream;
    std::vector<std::pair<void*, size_t>> dev, host;
    explicit KgSecrets(rt::Stream& s) : stream(s) {}
    int clear() {
        int rc = 0;
        for (auto& d : dev) if (d.first) rc |= rt::dmemset(d.first, 0, d.second, stream);
        rc |= rt::sync(stream);
        for (auto& h : host) kg_wipe(h.first, h.second);
        dev.clear(); host.clear();
        return rc;
    }
};

// The comb table of the G2 generator (stages_kg.hpp), built with the functions of host_g2.hpp and uploaded on first use under
// a lock; one per (curve, device), kept for the life of the process like the runtime's other per-device caches.
template <class C>
int kg_table(int dev, rt::Stream& stream, const uint32_t** out) {
    static std::mutex mu;
    static std::map<int, DevBuf*>* cache = new std::map<int, DevBuf*>();
    std::lock_guard<std::mutex> g(mu);
    auto it = cache->find(dev);
    if (it != cache->end()) { *out = it->second->template as<uint32_t>(); return BBS_OK; }
    constexpr int N = C::FpP::N;
    std::vector<uint32_t> tab(kg_table_words<C>());
    G2Aff<C> base = g2_generator<C>();
    uint32_t* p = tab.data();
    for (int w = 0; w < KG_WINDOWS; w++) {
        G2Aff<C> e = base;
        for (int d = 1; d <= KG_PER_WIN; d++) {
            if (e.inf) return BBS_E_STATE;
            for (int j = 0; j < N; j++) { p[j] = e.x.c0.v[j]; p[N + j] = e.x.c1.v[j]; p[2 * N + j] = e.y.c0.v[j]; p[3 * N + j] = e.y.c1.v[j]; }
            p += 4 * N;
            e = g2_add<C>(e, base);
        }
        base = e;                                      // [2^KG_WB] of this window's base
    }
    std::unique_ptr<DevBuf> b(new DevBuf());
    if (b->alloc(tab.size() * 4)) return BBS_E_NOMEM;
    if (rt::h2d(b->p, tab.data(), tab.size() * 4, stream)) return BBS_E_HIP;
    *out = b->template as<uint32_t>();
    (*cache)[dev] = b.release();
    return BBS_OK;
}

// the KgPublic stage over n scalars already on the device (d_sk: [8][n] words), results straight into the caller's arrays
template <class C>
static int kg_public_run(Ctx<C>* ctx, size_t n, const uint32_t* d_sk, int8_t* d_st, uint8_t* pk_affine_out, int8_t* inf_out, uint8_t* pk_octets_out) {
    constexpr size_t FPB = Ctx<C>::FPB;
    const uint32_t* table = nullptr;
    if (const int rc = kg_table<C>(ctx->device, ctx->stream, &table)) return rc;
    DevBuf d_rec, d_oct, d_inf;
    if ((pk_affine_out && d_rec.alloc(n * 4 * FPB)) || (pk_octets_out && d_oct.alloc(n * 2 * FPB)) || (inf_out && d_inf.alloc(n))) return BBS_E_NOMEM;
    KgPublicArgs<C> a{};
    a.n = n; a.sk = d_sk; a.table = table; a.status = d_st;
    a.rec = d_rec.as<uint32_t>(); a.oct = d_oct.as<uint32_t>(); a.inf = d_inf.as<int8_t>();
    if (rt::launch<KgPublic<C>>(ctx->stream, a, n)) { (void)rt::sync(ctx->stream); return BBS_E_HIP; }
    // (synchronous copies: the buffers go back behind them)
    if ((pk_affine_out && rt::d2h(pk_affine_out, d_rec.p, n * 4 * FPB, ctx->stream)) || (pk_octets_out && rt::d2h(pk_octets_out, d_oct.p, n * 2 * FPB, ctx->stream)) ||
        (inf_out && rt::d2h(inf_out, d_inf.p, n, ctx->stream)) || rt::sync(ctx->stream)) { (void)rt::sync(ctx->stream); return BBS_E_HIP; }
    return BBS_OK;
}

template <class C>
int key_gen_batch(Ctx<C>* ctx, size_t n, const uint8_t* km, const uint64_t* km_off, const uint8_t* ki, const uint64_t* ki_off,
                  const uint8_t* dst, size_t dst_len, uint8_t* sk32_out, uint8_t* pk_affine_out, uint8_t* pk_octets_out, int8_t* status) {
    constexpr size_t FPB = Ctx<C>::FPB;
    if (!n) return BBS_OK;
    if (!km || !km_off || !sk32_out || !status || (dst_len && !dst) || (ki && !ki_off)) return BBS_E_ARG;
    if (ctx->use()) return BBS_E_HIP;
    const bool with_pk = pk_affine_out || pk_octets_out;
    KgSecrets secrets(ctx->stream);
    BytePool kmp, kip;
    DevBuf d_kmo, d_kml, d_kio, d_kil, d_km, d_ki, d_sk, d_st;
    std::vector<uint32_t> w(n * 8);
    auto body = [&]() -> int {
        const bool km_ok = kmp.build(n, km, km_off);
        secrets.host.push_back({kmp.bytes.data(), kmp.bytes.size()});
        secrets.host.push_back({w.data(), w.size() * 4});
        if (!km_ok || !kip.build(n, ki, ki_off)) return BBS_E_ARG;
        if (d_kmo.alloc(n * 4) || d_kml.alloc(n * 4) || d_kio.alloc(n * 4) || d_kil.alloc(n * 4) || d_km.alloc(kmp.bytes.size()) ||
            d_ki.alloc(kip.bytes.size()) || d_sk.alloc(n * 32) || d_st.alloc(n)) return BBS_E_NOMEM;
        secrets.dev.push_back({d_km.p, kmp.bytes.size()});
        secrets.dev.push_back({d_sk.p, n * 32});
        if (rt::h2d(d_kmo.p, kmp.off.data(), n * 4, ctx->stream) || rt::h2d(d_kml.p, kmp.len.data(), n * 4, ctx->stream) ||
            rt::h2d(d_kio.p, kip.off.data(), n * 4, ctx->stream) || rt::h2d(d_kil.p, kip.len.data(), n * 4, ctx->stream) ||
            rt::h2d(d_km.p, kmp.bytes.data(), kmp.bytes.size(), ctx->stream) || rt::h2d(d_ki.p, kip.bytes.data(), kip.bytes.size(), ctx->stream) ||
            rt::dmemset(d_st.p, (uint8_t)ST_PENDING, n, ctx->stream)) return BBS_E_HIP;
        KgDeriveArgs a;
        std::memset(&a, 0, sizeof(a));
        a.n = n;
        a.km_off = d_kmo.as<uint32_t>(); a.km_len = d_kml.as<uint32_t>(); a.ki_off = d_kio.as<uint32_t>(); a.ki_len = d_kil.as<uint32_t>();
        a.km = d_km.as<uint8_t>(); a.ki = d_ki.as<uint8_t>();
        a.dst_too_long = dst_len > 255 ? 1 : 0;
        if (!a.dst_too_long && dst_len) std::memcpy(a.dst, dst, dst_len);
        a.dst_len = a.dst_too_long ? 0u : (uint32_t)dst_len;
        a.accepted = with_pk ? ST_PENDING : (int8_t)1;
        a.sk = d_sk.as<uint32_t>(); a.status = d_st.as<int8_t>();
        if (rt::launch<KgDerive<C>>(ctx->stream, a, n)) return BBS_E_HIP;
        if (with_pk) if (const int rc = kg_public_run<C>(ctx, n, d_sk.as<uint32_t>(), d_st.as<int8_t>(), pk_affine_out, nullptr, pk_octets_out)) return rc;
        if (rt::d2h(w.data(), d_sk.p, n * 32, ctx->stream) || rt::d2h(status, d_st.p, n, ctx->stream)) return BBS_E_HIP;
        if (!statuses_final(status, n)) return BBS_E_STATE;
        for (size_t i = 0; i < n; i++) {
            if (status[i] == 1) unpack_words_le(w, n, 0, i, 8, sk32_out + i * 32);
            else std::memset(sk32_out + i * 32, 0, 32);
        }
        return BBS_OK;
    };
    const int rc = body();
    const int crc = secrets.clear();
    if (rc) {                                          // nothing is delivered: no key of a call that failed can be read back
        kg_wipe(sk32_out, n * 32);
        if (pk_affine_out) std::memset(pk_affine_out, 0, n * 4 * FPB);
        if (pk_octets_out) std::memset(pk_octets_out, 0, n * 2 * FPB);
        return rc;
    }
    return crc ? BBS_E_HIP : BBS_OK;
}

template <class C>
int sk_to_pk_batch(Ctx<C>* ctx, size_t n, const uint8_t* sk32, uint8_t* pk_affine_out, int8_t* inf_out, uint8_t* pk_octets_out, int8_t* status) {
    constexpr size_t FPB = Ctx<C>::FPB;
    if (!n) return BBS_OK;
    if (!sk32 || !status || (!pk_affine_out && !pk_octets_out)) return BBS_E_ARG;
    if (ctx->use()) return BBS_E_HIP;
    KgSecrets secrets(ctx->stream);
    Soa S;
    DevBuf d_sk, d_st;
    auto body = [&]() -> int {
        S.init(8, n);
        for (size_t i = 0; i < n; i++) for (int k = 0; k < 8; k++) S.at(k, i) = le32(sk32 + i * 32 + 4 * k);
        const std::vector<uint32_t>& soa = S.soa();
        secrets.host.push_back({S.aos.data(), S.aos.size() * 4});
        secrets.host.push_back({S.v.data(), S.v.size() * 4});
        if (d_sk.alloc(n * 32) || d_st.alloc(n)) return BBS_E_NOMEM;
        secrets.dev.push_back({d_sk.p, n * 32});
        if (rt::h2d(d_sk.p, soa.data(), n * 32, ctx->stream) || rt::dmemset(d_st.p, (uint8_t)ST_PENDING, n, ctx->stream)) return BBS_E_HIP;
        if (const int rc = kg_public_run<C>(ctx, n, d_sk.as<uint32_t>(), d_st.as<int8_t>(), pk_affine_out, inf_out, pk_octets_out)) return rc;
        if (rt::d2h(status, d_st.p, n, ctx->stream)) return BBS_E_HIP;
        return statuses_final(status, n) ? BBS_OK : BBS_E_STATE;
    };
    const int rc = body();
    const int crc = secrets.clear();
    if (rc) {
        if (pk_affine_out) std::memset(pk_affine_out, 0, n * 4 * FPB);
        if (pk_octets_out) std::memset(pk_octets_out, 0, n * 2 * FPB);
        if (inf_out) std::memset(inf_out, 0, n);
        return rc;
    }
    return crc ? BBS_E_HIP : BBS_OK;
}

// Registration of secret keys for keyed sign (bbs_ctx_set_secret_keys / bbs_ctx_add_secret_keys; runtime.hpp SignSet, stages_sg.hpp
// SgScalarsIn).  The public halves of the whole call come from the KgPublic stage, as sk_to_pk_batch's do, and then go
// through add_keys like keys that arrive as records: a secret-registered key IS a public-registered key plus its row of the
// signing set, under the same index.  A scalar >= r is refused: BBS_ST_NONCANONICAL, a refused public entry, a zero row.
// Order: derive; build the new signing set (exactly n_old + n rows: the old rows copied device to device, zero rows for the
// public-only keys appended since, the new rows uploaded); then add_keys; the two pointers are swapped last, so a failure
// anywhere leaves both sets as they were and the set that was being built is cleared by its destructor.  Every buffer that
// held a secret -- the device scalars KgPublic read, the converted words, the rows' staging copy -- is cleared on every way out.
template <class C>
int add_secret_keys(Ctx<C>* ctx, bool replace, size_t n, const uint8_t* sk32, int8_t* key_status, uint8_t* pk_affine_out, int8_t* inf_out,
                    uint32_t* first_index) {
    constexpr size_t FPB = Ctx<C>::FPB;
    using SignSet = typename Ctx<C>::SignSet;
    if (n && (!sk32 || !key_status)) return BBS_E_ARG;
    if (!ctx->gens_set) return BBS_E_STATE;
    if (ctx->use()) return BBS_E_HIP;
    if (!n) {
        if (replace) ctx->drop_key_sets();
        else if (first_index) *first_index = (uint32_t)ctx->public_key_count();
        return BBS_OK;
    }
    const auto old_keys = replace ? nullptr : ctx->keys;
    const auto old_sign = replace ? nullptr : ctx->sign_keys;
    const size_t n_old = old_keys ? old_keys->n : 0;
    if (n_old + n > 0xFFFFFFF0u) return BBS_E_ARG;
    if (old_sign && (!old_keys || old_sign->lineage != old_keys->lineage || old_sign->n > n_old)) return BBS_E_STATE;
    KgSecrets secrets(ctx->stream);
    Soa S;
    DevBuf d_sk, d_st;
    std::vector<uint32_t> rows(n * 8, 0u);
    std::vector<uint8_t> rec(n * 4 * FPB, 0);
    std::vector<int8_t> inf(n, 0), st(n, 0), pub_st(n, 0);
    std::shared_ptr<SignSet> ss(new SignSet());
    uint32_t first = 0;
    auto body = [&]() -> int {
        S.init(8, n);
        secrets.host.push_back({S.aos.data(), S.aos.size() * 4});
        secrets.host.push_back({rows.data(), rows.size() * 4});
        for (size_t i = 0; i < n; i++) for (int k = 0; k < 8; k++) S.at(k, i) = le32(sk32 + i * 32 + 4 * k);
        const std::vector<uint32_t>& soa = S.soa();
        secrets.host.push_back({S.v.data(), S.v.size() * 4});
        if (d_sk.alloc(n * 32) || d_st.alloc(n)) return BBS_E_NOMEM;
        secrets.dev.push_back({d_sk.p, n * 32});
        if (rt::h2d(d_sk.p, soa.data(), n * 32, ctx->stream) || rt::dmemset(d_st.p, (uint8_t)ST_PENDING, n, ctx->stream)) return BBS_E_HIP;
        if (const int rc = kg_public_run<C>(ctx, n, d_sk.as<uint32_t>(), d_st.as<int8_t>(), rec.data(), inf.data(), nullptr)) return rc;
        if (rt::d2h(st.data(), d_st.p, n, ctx->stream)) return BBS_E_HIP;
        if (!statuses_final(st.data(), n)) return BBS_E_STATE;
        // the signing set: [0, old_sign->n) copied, [old_sign->n, n_old) public-only (zero), [n_old, n_old + n) this call's
        ss->n = n_old + n;
        ss->device = ctx->device;
        ss->has.assign(ss->n, 0);
        if (ss->d.alloc(ss->n * 32)) return BBS_E_NOMEM;
        if (rt::dmemset(ss->d.p, 0, ss->n * 32, ctx->stream)) return BBS_E_HIP;
        if (old_sign) {
            std::copy(old_sign->has.begin(), old_sign->has.end(), ss->has.begin());
            ss->n_secret = old_sign->n_secret;
            if (rt::d2d_async(ss->d.p, old_sign->d.p, old_sign->n * 32, ctx->stream)) return BBS_E_HIP;
        }
        for (size_t i = 0; i < n; i++) {
            if (st[i] != 1) {        // refused: a record no key has (0xFF.. is no field element), so that add_keys refuses it too
                std::memset(rec.data() + i * 4 * FPB, 0xFF, 4 * FPB);
                inf[i] = 0;
                continue;
            }
            for (int k = 0; k < 8; k++) rows[i * 8 + k] = S.at(k, i);
            ss->has[n_old + i] = 1;
            ss->n_secret++;
        }
        if (rt::h2d(ss->d.template as<uint32_t>() + n_old * 8, rows.data(), n * 32, ctx->stream) || rt::sync(ctx->stream)) return BBS_E_HIP;
        if (const int rc = ctx->add_keys(replace, n, rec.data(), inf.data(), nullptr, pub_st.data(), nullptr, nullptr, &first)) return rc;
        ss->lineage = ctx->keys->lineage;
        ctx->sign_keys = std::move(ss);
        return BBS_OK;
    };
    const int rc = body();
    if (rc) (void)rt::sync(ctx->stream);               // (a copy into the set that is given up must not outlive it)
    const int crc = secrets.clear();
    if (rc) return rc;
    for (size_t i = 0; i < n; i++) {
        const bool ok = st[i] == 1 && pub_st[i] == 1;
        key_status[i] = ok ? (int8_t)1 : st[i] != 1 ? st[i] : pub_st[i];
        if (!ok) { std::memset(rec.data() + i * 4 * FPB, 0, 4 * FPB); inf[i] = 0; }
    }
    if (pk_affine_out) std::memcpy(pk_affine_out, rec.data(), n * 4 * FPB);
    if (inf_out) std::memcpy(inf_out, inf.data(), n);
    if (first_index) *first_index = first;
    return crc ? BBS_E_HIP : BBS_OK;
}
