// Device stages of verify.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// =============================================================================================
// verify
// =============================================================================================
constexpr int VF_NPARTS = 1 + NFIX;

template <class C>
struct VfArgs {
    size_t n;
    int L;
    const CtxConsts<C>* cc;
    int glv;
    const uint32_t* sig_a;    // [2NC][n] canonical
    const uint32_t* sig_e;    // [8][n]
    const uint32_t* msgs;     // [L][8][n]
    const uint32_t* hdr_off; const uint32_t* hdr_len; const uint8_t* hdr_bytes;
    int8_t* status;
    uint32_t* fscal;          // [L+2][8][n]
    uint32_t* partials;       // [VF_NPARTS][3N][n]
    uint32_t* aff;            // [2][2N][n] : A, e*A - B  (Montgomery)
    uint32_t* fmiller;
    uint32_t* vtab;           // [G1_TAB][2N][n] window table of e * A (g1.hpp TabHbm)
};

// stage 0 of verify (lane per item, once per upload): verify.rs:69-71's length check, range checks of the signature
// and the messages, transposition of the item-major staging image into the SoA arrays (see PvIngest)
template <class C>
struct VfIngestArgs {
    size_t n;
    int L, dst_too_long, has_sig;         // has_sig = 0: core_sign (no signature record, only messages)
    const uint32_t* rec;                  // n records A || e, little-endian words (has_sig, record form)
    // wire form (has_sig, oct != nullptr): n octet strings compress(A) || e big-endian; A has been decoded into sig_a by
    // VfOctDecode (codec_dev.hpp), its verdict is pcode[i]
    const uint8_t* oct;
    const int8_t* pcode;
    int msg_dst_too_long;                 // raw-message form: the reference's msg_to_scalars panics (DST > 255 bytes)
    const uint64_t *m_off, *hdr_off64;    // n + 1 entries each, rebased to 0
    const uint32_t* m;                    // messages, 8 words each
    uint32_t *sig_a, *sig_e, *msgs, *hdr_off, *hdr_len;
    int8_t* status0;
};
// MIXED (bbs_ctx_set_mixed_lengths, VfIngestMixed below; has_sig = 1 only): the item's own message count l may be anything in
// 0 .. L and is recorded in len[i]; l != L becomes l > L, nothing else changes
template <class C, bool MIXED>
struct VfIngestBody {
    static BBS_HD void run(const VfIngestArgs<C>& a, size_t i, uint32_t* len) {
        using P = typename C::FpP;
        using R = typename C::FrP;
        constexpr int NC = P::NC;
        const size_t n = a.n;
        a.hdr_off[i] = (uint32_t)a.hdr_off64[i];
        a.hdr_len[i] = (uint32_t)(a.hdr_off64[i + 1] - a.hdr_off64[i]);
        if constexpr (MIXED) len[i] = 0;
        if (a.has_sig && a.oct) {
            // the verdicts of bbs_signature_from_octets come first, in its order: the point's code, the identity, e >= r,
            // e = 0; only a decodable signature reaches core_verify's own checks
            constexpr size_t NB = 4 * NC;
            uint32_t e[8];
            be32_words(a.oct + i * (NB + 32) + NB, e);
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) any |= e[k];
            const int8_t c = a.pcode[i];
            int8_t pre = ST_PENDING;
            if (c < 0) pre = c;
            else if (c == 1) pre = -42;
            else if (!limbs_lt_mod<R>(e)) pre = -40;
            else if (!any) pre = -42;
            if (pre != ST_PENDING) {
#pragma unroll
                for (int k = 0; k < 8; k++) e[k] = 0;
            }
            soa_st<8>(a.sig_e, n, i, e);
            if (pre != ST_PENDING) { a.status0[i] = pre; return; }
        }
        const uint64_t l = a.m_off[i + 1] - a.m_off[i];
        // raw-message form: msg_to_scalars runs first in the reference's public functions (sign.rs:45, verify.rs:32)
        if (a.msg_dst_too_long && l > 0) { a.status0[i] = -23; return; }
        if (MIXED ? l > (uint64_t)a.L : l != (uint64_t)a.L) { a.status0[i] = -1; return; }   // InvalidMessageAndGeneratorsLength
        if constexpr (MIXED) len[i] = (uint32_t)l;
        if (a.dst_too_long) { a.status0[i] = -23; return; }
        bool ok = true;
        if (a.has_sig && !a.oct) {
            const uint32_t* sg = a.rec + i * (size_t)(2 * NC + 8);
            for (int c = 0; c < 2; c++) {
                uint32_t w[NC];
#pragma unroll
                for (int k = 0; k < NC; k++) w[k] = sg[c * NC + k];
                ok &= limbs_lt_mod<P>(w);
                soa_st<NC>(a.sig_a + (size_t)c * NC * n, n, i, w);
            }
            uint32_t e[8];
            soa_ld<8>(sg + 2 * NC, 1, 0, e);
            ok &= limbs_lt_mod<R>(e);
            soa_st<8>(a.sig_e, n, i, e);
        }
        for (uint64_t j = 0; j < l; j++) {
            uint32_t w[8];
            soa_ld<8>(a.m + (a.m_off[i] + j) * 8, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.msgs + (size_t)j * 8 * n, n, i, w);
        }
        a.status0[i] = ok ? ST_PENDING : (int8_t)-40;
    }
};
template <class C>
struct VfIngest {
    static __host__ __device__ void run(const VfIngestArgs<C>& a, size_t i) { VfIngestBody<C, false>::run(a, i, nullptr); }
};
template <class C>
struct VfIngestMixed {
    static __host__ __device__ void run(const MixedIngestArgs<VfIngestArgs<C>>& m, size_t i) { VfIngestBody<C, true>::run(m.a, i, m.len); }
};

// h: the domain prefix of the item's key (as pv_scalars_item); l: the item's message count (as pv_scalars_item)
template <class C>
BBS_HD void vf_scalars_item(const VfArgs<C>& a, size_t i, const HashCtx& h, int l) {
    using R = typename C::FrP;
    const size_t n = a.n;
    Fr<C> dom = fe_to_canonical<R>(domain_from_header<C>(h, a.hdr_bytes + a.hdr_off[i], a.hdr_len[i]));
    Fr<C> one = fe_zero<R>();
    one.v[0] = 1;
    soa_st<8>(a.fscal, n, i, one.v);
    soa_st<8>(a.fscal + (size_t)8 * n, n, i, dom.v);
    for (int j = 0; j < l; j++) {
        uint32_t m[8];
        soa_ld<8>(a.msgs + (size_t)j * 8 * n, n, i, m);
        soa_st<8>(a.fscal + (size_t)(2 + j) * 8 * n, n, i, m);
    }
}
template <class C>
struct VfScalars {
    static __host__ __device__ void run(const VfArgs<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;
        vf_scalars_item<C>(a, i, a.cc->hash, a.L);
    }
};
// the derived forms, as PvScalarsIn (stages_pv.hpp): the item's own prefix, its l messages, and in the mixed forms zeros
// WRITTEN for the bases behind them
template <class C, Form F>
struct VfScalarsIn {
    static __host__ __device__ void run(const FormArgs<C, VfArgs<C>>& f, size_t i) {
        if (f.a.status[i] != ST_PENDING) return;
        int l;
        const HashCtx& h = form_domain<F, C>(f.a.cc, f.d, i, f.a.L, l);
        vf_scalars_item<C>(f.a, i, h, l);
        if constexpr (form_mixed(F)) mixed_zero_scalars(f.a.fscal, f.a.n, i, l, f.a.L);
    }
};

// the multi-scalar multiplication as two kernels with their own budgets (round 5, as for proof_verify: PvVarMul / PvFixedChunk)
// lane per item: A on the curve?, its Montgomery copy, e * A (window table in HBM) -> partials[0]
template <class C>
struct VfVarMul {
    static constexpr int WAVES_PER_EU = chain_waves<C>(1);      // BN254: 264 - 268 registers -> 256
    static BBS_HD void run(const VfArgs<C>& a, size_t i) {
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Aff<C> A = g1a_load_canon_to_mont<C>(a.sig_a, n, i);
        if (!g1a_on_curve<C>(A)) { a.status[i] = -41; return; }
        g1a_store_mont<C>(a.aff, n, i, A);
        uint32_t k[8];
        soa_ld<8>(a.sig_e, n, i, k);
        G1Jac<C> r;
        g1_mul_aff_sel_hbm_inl<C>(A, k, a.glv != 0, a.vtab + i, n, r);
        g1j_store<C>(a.partials, n, i, r);
    }
};
// lane per (chunk, item): the fixed-base sum B over {P1, Q1, H_*} -> partials[1 + chunk]
template <class C>
struct VfFixedChunk {
    static __host__ __device__ void run(const VfArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int chunk = (int)(t / n);
        const size_t i = t - (size_t)chunk * n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> r;
        fixed_msm_chunk_to<C>(*a.cc, a.fscal, n, i, a.L + 2, chunk, r);
        g1j_store<C>(a.partials + (size_t)(1 + chunk) * 3 * N * n, n, i, r);
    }
};

template <class C>
struct VfCombine {
    static __host__ __device__ void run(const VfArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        auto part = [&](int p) { return g1j_load<C>(a.partials + (size_t)p * 3 * N * n, n, i); };
        G1Jac<C> b = part(1);
        for (int f = 1; f < NFIX; f++) b = g1j_add_i<C>(b, part(1 + f));
        G1Jac<C> x = g1j_add_i<C>(part(0), g1j_neg<C>(b));          // e*A - B
        g1a_store_mont<C>(a.aff + (size_t)2 * N * n, n, i, g1j_to_aff<C>(x));
        a.status[i] = ST_PAIRING;
    }
};

}  // namespace bbs
