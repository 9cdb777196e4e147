// Device stages of sign.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// =============================================================================================
// sign
// =============================================================================================
template <class C>
struct SgArgs {
    size_t n;
    int L;
    const CtxConsts<C>* cc;
    uint32_t sk[8];           // canonical
    const uint32_t* msgs;     // [L][8][n]
    const uint32_t* hdr_off; const uint32_t* hdr_len; const uint8_t* hdr_bytes;
    int8_t* status;
    uint32_t* fscal;          // [L+2][8][n]
    uint32_t* partials;       // [NFIX][3N][n]
    uint32_t* out_a;          // [2NC][n] canonical
    uint32_t* out_e;          // [8][n] canonical
    uint32_t* out_rec;        // [n][2NC + 8]: the records A || e as the caller receives them (SgEmit)
    int oct_form;             // 1: out_rec holds n octet strings compress(A) || I2OSP(e, 32) instead (fp_bytes + 32 each)
};

// h: the domain prefix (the context's, or that of the item's own length in a mixed-length job); l: the item's message count
// (a.L unless the job is a mixed-length one); sk: the 8 canonical words of the item's secret key -- a.sk of the single-key
// stages (a kernel argument: scalar registers after inlining), the lane's own row of the signing set in the keyed ones
template <class C>
BBS_HD void sg_scalars_item(const SgArgs<C>& a, size_t i, const HashCtx& h, const uint32_t* sk, int l) {
    using R = typename C::FrP;
    const size_t n = a.n;
    Fr<C> dom = domain_from_header<C>(h, a.hdr_bytes + a.hdr_off[i], a.hdr_len[i]);
    // e = hash_to_scalar(sk || m_1 .. m_l || domain)   (sign.rs:90-118)
    Sha256 s;
    xmd48_begin(s);
    sha256_limbs_be8(s, sk);
    for (int j = 0; j < l; j++) {
        uint32_t m[8];
        soa_ld<8>(a.msgs + (size_t)j * 8 * n, n, i, m);
        sha256_limbs_be8(s, m);
    }
    sha256_fr_be<C>(s, dom);
    uint32_t okm[12];
    xmd48_finish(s, a.cc->hash.dst_h2s, a.cc->hash.dst_h2s_len, okm);
    Fr<C> e = fr_from_okm<C>(okm);
    Fr<C> ec = fe_to_canonical<R>(e);
    soa_st<8>(a.out_e, n, i, ec.v);
    Fr<C> skm = fe_from_limbs<R>(sk);
    Fr<C> spe = fe_add<R>(skm, e);
    if (fe_is_zero<R>(spe)) { a.status[i] = -20; return; }     // sign.rs:129 unwrap
    Fr<C> inv = fe_inv<R>(spe);                                 // Montgomery
    Fr<C> invc = fe_to_canonical<R>(inv);
    soa_st<8>(a.fscal, n, i, invc.v);
    Fr<C> di = fe_mul<R>(dom, invc);                            // (dom R) inv / R = dom*inv canonical
    soa_st<8>(a.fscal + (size_t)8 * n, n, i, di.v);
    for (int j = 0; j < l; j++) {
        Fr<C> m = fr_load_canon<C>(a.msgs + (size_t)j * 8 * n, n, i);
        Fr<C> mi = fe_mul<R>(inv, m);
        soa_st<8>(a.fscal + (size_t)(2 + j) * 8 * n, n, i, mi.v);
    }
}
template <class C>
struct SgScalars {
    static __host__ __device__ void run(const SgArgs<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;
        sg_scalars_item<C>(a, i, a.cc->hash, a.sk, a.L);
    }
};
// row k of the signing set (runtime.hpp SignSet: the 8 canonical words of sk_k, 32 bytes, 32-byte aligned).  The index
// diverges per lane, so the row is read with vector loads into the lane's registers; it is the caller's public key_index.
BBS_HD void sign_key_row(const uint32_t* sks, uint32_t k, uint32_t* sk) {
    const uint32_t* row = static_cast<const uint32_t*>(__builtin_assume_aligned(sks + (size_t)8 * k, 32));
    for (int j = 0; j < 8; j++) sk[j] = row[j];
}
// The derived forms, as PvScalarsIn (stages_pv.hpp).  core_sign meets the key in the domain, in the hash that gives e and in
// 1 / (sk + e): the keyed forms take the lane's own secret row where the single-key forms take a.sk; SgMsmPart .. SgEmit never
// see a key.  Mixed forms: e over the item's l messages, its scalars in fscal[2 .. 2 + l) and zeros WRITTEN for the bases
// behind them (also for an item that ends here with -20: nothing reads its scalars, and nothing stale stays behind).
template <class C, Form F>
struct SgScalarsIn {
    static __host__ __device__ void run(const FormArgs<C, SgArgs<C>>& f, size_t i) {
        if (f.a.status[i] != ST_PENDING) return;
        uint32_t row[8];
        const uint32_t* sk = f.a.sk;
        if constexpr (form_keyed(F)) { sign_key_row(f.d.sks, f.d.kidx[i], row); sk = row; }
        int l;
        const HashCtx& h = form_domain<F, C>(f.a.cc, f.d, i, f.a.L, l);
        sg_scalars_item<C>(f.a, i, h, sk, l);
        if constexpr (form_mixed(F)) mixed_zero_scalars(f.a.fscal, f.a.n, i, l, f.a.L);
    }
};

template <class C>
struct SgMsmPart {
    static constexpr int WAVES_PER_EU = MSM_WAVES;
    static __host__ __device__ void run(const SgArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int part = (int)(t / n);
        const size_t i = t - (size_t)part * n;
        if (a.status[i] != ST_PENDING) return;
        g1j_store<C>(a.partials + (size_t)part * 3 * N * n, n, i,
                     fixed_msm_chunk<C>(*a.cc, a.fscal, n, i, a.L + 2, part));
    }
};

template <class C>
struct SgCombine {
    static __host__ __device__ void run(const SgArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> acc = g1j_load<C>(a.partials, n, i);
        for (int f = 1; f < NFIX; f++) acc = g1j_add_i<C>(acc, g1j_load<C>(a.partials + (size_t)f * 3 * N * n, n, i));
        g1a_store_canon<C>(a.out_a, n, i, g1j_to_aff<C>(acc));
        a.status[i] = 1;
    }
};

// last stage of sign (lane per item): the signature record in the caller's layout (A affine || e, little-endian words,
// zeros unless the status is 1), so that delivery is one contiguous copy
template <class C>
struct SgEmit {
    static __host__ __device__ void run(const SgArgs<C>& a, size_t i) {
        constexpr int NC = C::FpP::NC, W = 2 * NC + 8;
        const size_t n = a.n;
        const bool ok = a.status[i] == 1;
        if (a.oct_form) {
            constexpr size_t NB = 4 * NC;
            uint8_t* o = reinterpret_cast<uint8_t*>(a.out_rec) + i * (NB + 32);
            if (!ok) { for (size_t k = 0; k < NB + 32; k++) o[k] = 0; return; }
            uint32_t pw[2 * NC], e[8];
            for (int k = 0; k < 2 * NC; k++) pw[k] = a.out_a[(size_t)k * n + i];
            for (int k = 0; k < 8; k++) e[k] = a.out_e[(size_t)k * n + i];
            g1_words_to_octets<C>(pw, pw + NC, o);
            words_be32(e, o + NB);
            return;
        }
        uint32_t* r = a.out_rec + i * (size_t)W;
        for (int k = 0; k < 2 * NC; k++) r[k] = ok ? a.out_a[(size_t)k * n + i] : 0u;
        for (int k = 0; k < 8; k++) r[2 * NC + k] = ok ? a.out_e[(size_t)k * n + i] : 0u;
    }
};

}  // namespace bbs
