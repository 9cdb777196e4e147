// Device stages of proof_gen.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// =============================================================================================
// proof_gen
// =============================================================================================
constexpr int PG_NVAR = 7;                  // 4 multiples of B, 3 multiples of A: the seven scalars of PgArgs::vscal
constexpr int PG_NPARTS = PG_NVAR + NFIX;   // + chunks of sum m~_j H_j (the split form: one lane per multiplication)
// Throughput form (round 4): Bbar = (r1 r2) B - (e r1 r2) A and T1 = (r1~ r2) B + (e~ r1 r2) A each on ONE shared doubling
// chain (g1_mul2_aff): five lanes and five chains of ~252 doublings per item instead of seven -- 14 % fewer instructions per
// proof, a 29 % longer longest lane.  The split form stays the layout of a job that is alone (bbs_ctx_set_latency_mode).
constexpr int PG_NVAR_JOINT = 5;            // D, Abar, Bbar (joint), T1 (joint), T2's multiple of B

template <class C>
struct PgArgs {
    size_t n;
    int L, Rmax;
    const CtxConsts<C>* cc;
    int glv;                  // see PvArgs
    const uint32_t* sig_a;    // [2NC][n] canonical
    const uint32_t* sig_e;    // [8][n]
    const uint32_t* msgs;     // [L][8][n]
    const uint32_t* dmask;    // [ceil(L/32)][n] disclosed slots
    const uint32_t* didx;     // [Rmax][n] sorted distinct disclosed indexes
    const uint32_t* rcount;   // [n] number of distinct disclosed indexes
    const uint32_t* rnd5;     // [5][8][n]  r1, r2, e~, r1~, r3~
    const uint32_t* mtilde;   // [L][8][n]  m~_j at undisclosed slots, 0 elsewhere
    const uint32_t* hdr_off; const uint32_t* hdr_len; const uint8_t* hdr_bytes;
    const uint32_t* ph_off;  const uint32_t* ph_len;  const uint8_t* ph_bytes;
    int8_t* status;
    // intermediates
    uint32_t* dom;            // [8][n] Montgomery
    uint32_t* fscal;          // [L+2][8][n]  B's scalars (1, domain, m_j)
    uint32_t* fscal2;         // [L+2][8][n]  (0, 0, m~_j)
    uint32_t* vscal;          // [PG_NVAR][8][n] canonical scalars of the variable-base parts
    int nvar;                 // PG_NVAR (split form) or PG_NVAR_JOINT
    uint32_t* vtab;           // [PG_NVAR][G1_TAB][2N][n] window tables of the variable-base parts: split form table k = part k;
                              // joint form tables 0, 1 = Bbar's chain (B, -A), 2, 3 = T1's (B, A), 4, 5, 6 = parts 0, 1, 4
    // comb form of the joint layout (g1.hpp g1_comb_sum_to): stage PgTables writes, per item, the tables of the 2^(64 j)
    // multiples of B and A -- [base 2][piece 4][entry 8][2N][n] -- and comb_ok[base * n + i] = 1; null: not used
    uint32_t* ctab;
    int8_t* comb_ok;
    uint32_t* bpart;          // [NFIX][3N][n]
    uint32_t* baff;           // [2][2N][n]  B, A (Montgomery affine)
    uint32_t* partials;       // [PG_NPARTS][3N][n]
    // outputs (canonical)
    uint32_t* out_pts;        // [3][2NC][n] a_bar, b_bar, d (canonical)
    uint32_t* out_sc;         // [4][8][n]   e^, r1^, r3^, c
    uint32_t* out_mhat;       // [L][8][n]   m^_j at undisclosed slots
    // what the caller receives (PgEmit): records [n][6NC + 32] (Abar, Bbar, D, e^, r1^, r3^, c), the m^ of the undisclosed
    // messages in ascending index order [n][L][8], and their number per item
    uint32_t* out_rec;
    uint32_t* out_mh;
    uint32_t* ucount;
    // 1: the wire form instead -- out_rec holds, at a stride of 3 fp_bytes + 32 (4 + max(L, 1)) bytes per item, the octet
    // string compress(Abar) || compress(Bbar) || compress(D) || e^ || r1^ || r3^ || m^_1 .. m^_U || c (scalars big-endian),
    // 3 fp_bytes + 32 (4 + U) bytes of it used; out_mh is not written
    int oct_form;
};

// stage 0 of proof_gen (lane per item, once per upload): the checks of proof_gen.rs:133-143 and :229-239 in the
// reference's order (the count of random scalars is a contract of this ABI and checked on the host), deduplication and
// sorting of the disclosed indexes (:151-161) through the bit mask, range checks, transposition (see PvIngest)
template <class C>
struct PgIngestArgs {
    size_t n;
    int L, dst_too_long;
    const uint32_t* rec;                  // n signature records A || e
    // wire form (oct != nullptr): n signature octet strings compress(A) || e big-endian; A has been decoded into sig_a by
    // VfOctDecode, its verdict is pcode[i] (as VfIngestArgs)
    const uint8_t* oct;
    const int8_t* pcode;
    int msg_dst_too_long;                 // raw-message form: the reference's msg_to_scalars panics (DST > 255 bytes)
    const uint64_t *m_off, *di_off, *rnd_off, *hdr_off64, *ph_off64;
    const uint32_t* m;                    // messages
    const uint64_t* di;                   // disclosed indexes, caller order, duplicates possible
    const uint32_t* rnd;                  // random scalars: r1, r2, e~, r1~, r3~, then m~_j for the undisclosed j ascending
    uint32_t *sig_a, *sig_e, *msgs, *dmask, *didx, *rcount, *rnd5, *mtilde, *hdr_off, *hdr_len, *ph_off, *ph_len;
    int8_t* status0;
};
// MIXED (bbs_ctx_set_mixed_lengths_gen, PgIngestMixed below): the item's own message count l may be anything in 0 .. L and is
// recorded in len[i] (0 for an item that is decided before or by the length check); l != L becomes l > L, nothing else changes
template <class C, bool MIXED>
struct PgIngestBody {
    static BBS_HD void run(const PgIngestArgs<C>& a, size_t i, uint32_t* len) {
        using P = typename C::FpP;
        using R = typename C::FrP;
        constexpr int NC = P::NC;
        const size_t n = a.n;
        a.hdr_off[i] = (uint32_t)a.hdr_off64[i];
        a.hdr_len[i] = (uint32_t)(a.hdr_off64[i + 1] - a.hdr_off64[i]);
        a.ph_off[i] = (uint32_t)a.ph_off64[i];
        a.ph_len[i] = (uint32_t)(a.ph_off64[i + 1] - a.ph_off64[i]);
        const uint64_t l = a.m_off[i + 1] - a.m_off[i], r = a.di_off[i + 1] - a.di_off[i];
        const uint64_t* idx = a.di + a.di_off[i];
        const int MW = ((a.L > 1 ? a.L : 1) + 31) / 32;
        for (int w = 0; w < MW; w++) a.dmask[(size_t)w * n + i] = 0;
        a.rcount[i] = 0;
        if constexpr (MIXED) len[i] = 0;
        if (a.oct) {
            // the verdicts of bbs_signature_from_octets first, in its order (see VfIngest)
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
            if (pre != ST_PENDING) { a.status0[i] = pre; return; }
            soa_st<8>(a.sig_e, n, i, e);
        }
        // raw-message form: msg_to_scalars runs first in the reference's public proof_gen (proof_gen.rs:95)
        if (a.msg_dst_too_long && l > 0) { a.status0[i] = -23; return; }
        if (r > l) { a.status0[i] = -2; return; }                          // InvalidDisclosedIndicesLength
        bool bad = false;
        for (uint64_t k = 0; k < r; k++) bad |= idx[k] >= l;
        if (bad) { a.status0[i] = -3; return; }                            // InvalidDisclosedIndex
        if (MIXED ? l > (uint64_t)a.L : l != (uint64_t)a.L) { a.status0[i] = -1; return; }   // proof_init: InvalidMessageAndGeneratorsLength
        if constexpr (MIXED) len[i] = (uint32_t)l;
        uint64_t distinct = 0;
        for (uint64_t k = 0; k < r; k++) {
            const size_t j = (size_t)idx[k];
            uint32_t* wp = a.dmask + (j >> 5) * n + i;
            const uint32_t w = *wp, bit = 1u << (j & 31);
            if (!(w & bit)) { *wp = w | bit; distinct++; }
        }
        // the random scalars were sized from the un-deduplicated length: a duplicate leaves fewer than 5 + undisclosed
        if (distinct != r) { a.status0[i] = -4; return; }
        if (a.dst_too_long) { a.status0[i] = -23; return; }
        bool ok = true;
        if (!a.oct) {
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
        const uint32_t* rs = a.rnd + a.rnd_off[i] * 8;
        for (int k = 0; k < 5; k++) {
            uint32_t w[8];
            soa_ld<8>(rs + 8 * k, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.rnd5 + (size_t)k * 8 * n, n, i, w);
        }
        uint32_t ku = 0, kd = 0;
        const uint32_t zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t j = 0; j < (size_t)l; j++) {
            uint32_t w[8];
            soa_ld<8>(a.m + (a.m_off[i] + j) * 8, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.msgs + j * 8 * n, n, i, w);
            if ((a.dmask[(j >> 5) * n + i] >> (j & 31)) & 1u) {
                a.didx[(size_t)kd * n + i] = (uint32_t)j;
                kd++;
                soa_st<8>(a.mtilde + j * 8 * n, n, i, zero);
            } else {
                soa_ld<8>(rs + 8 * (5 + ku), 1, 0, w);
                ok &= limbs_lt_mod<R>(w);
                soa_st<8>(a.mtilde + j * 8 * n, n, i, w);
                ku++;
            }
        }
        a.rcount[i] = kd;
        a.status0[i] = ok ? ST_PENDING : (int8_t)-40;
    }
};
template <class C>
struct PgIngest {
    static __host__ __device__ void run(const PgIngestArgs<C>& a, size_t i) { PgIngestBody<C, false>::run(a, i, nullptr); }
};
template <class C>
struct PgIngestMixed {
    static __host__ __device__ void run(const MixedIngestArgs<PgIngestArgs<C>>& m, size_t i) { PgIngestBody<C, true>::run(m.a, i, m.len); }
};
// the later stages of a mixed-length job that need the item's count and nothing else (PgFinalizeMixed, PgEmitMixed)
template <class A>
struct MixedLenArgs { A a; const uint32_t* len; };

// h: the domain prefix (the context's, or that of the item's own length in a mixed-length job); l: the item's message count
// (a.L unless the job is a mixed-length one)
template <class C>
BBS_HD void pg_scalars_item(const PgArgs<C>& a, size_t i, const HashCtx& h, int l) {
    using R = typename C::FrP;
    const size_t n = a.n;
    Fr<C> r2c = fr_load_canon<C>(a.rnd5 + (size_t)1 * 8 * n, n, i);
    Fr<C> dom = domain_from_header<C>(h, a.hdr_bytes + a.hdr_off[i], a.hdr_len[i]);
    soa_st<8>(a.dom, n, i, dom.v);
    Fr<C> domc = fe_to_canonical<R>(dom);
    Fr<C> one = fe_zero<R>();
    one.v[0] = 1;
    Fr<C> zero = fe_zero<R>();
    soa_st<8>(a.fscal, n, i, one.v);
    soa_st<8>(a.fscal + (size_t)8 * n, n, i, domc.v);
    soa_st<8>(a.fscal2, n, i, zero.v);
    soa_st<8>(a.fscal2 + (size_t)8 * n, n, i, zero.v);
    for (int j = 0; j < l; j++) {
        uint32_t m[8];
        soa_ld<8>(a.msgs + (size_t)j * 8 * n, n, i, m);
        soa_st<8>(a.fscal + (size_t)(2 + j) * 8 * n, n, i, m);
        soa_ld<8>(a.mtilde + (size_t)j * 8 * n, n, i, m);
        soa_st<8>(a.fscal2 + (size_t)(2 + j) * 8 * n, n, i, m);
    }
    // variable-base scalars (proof_gen.rs:254-258, restructured over B and A)
    Fr<C> r1 = fr_to_mont<C>(fr_load_canon<C>(a.rnd5, n, i));
    Fr<C> r2 = fr_to_mont<C>(r2c);
    Fr<C> et = fr_load_canon<C>(a.rnd5 + (size_t)2 * 8 * n, n, i);
    Fr<C> r1t = fr_load_canon<C>(a.rnd5 + (size_t)3 * 8 * n, n, i);
    Fr<C> r3t = fr_load_canon<C>(a.rnd5 + (size_t)4 * 8 * n, n, i);
    Fr<C> e = fr_load_canon<C>(a.sig_e, n, i);
    Fr<C> r1r2 = fe_mul<R>(r1, r2);                               // Montgomery
    Fr<C> v[PG_NVAR];
    v[0] = r2c;                                                   // D      = r2 * B
    v[1] = fe_to_canonical<R>(r1r2);                              // r1r2 * B
    v[2] = fe_mul<R>(r2, r1t);                                    // T1 part: (r1~ r2) * B
    v[3] = fe_mul<R>(r2, r3t);                                    // T2 part: (r3~ r2) * B
    v[4] = v[1];                                                  // Abar   = (r1 r2) * A
    v[5] = fe_mul<R>(r1r2, e);                                    // (e r1 r2) * A
    v[6] = fe_mul<R>(r1r2, et);                                   // (e~ r1 r2) * A
    for (int k = 0; k < PG_NVAR; k++) soa_st<8>(a.vscal + (size_t)k * 8 * n, n, i, v[k].v);
}
template <class C>
struct PgScalars {
    static __host__ __device__ void run(const PgArgs<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;
        pg_scalars_item<C>(a, i, a.cc->hash, a.L);
    }
};
// The derived forms, as PvScalarsIn (stages_pv.hpp).  A key enters a proof in calculate_domain alone (no pairing, no W), so
// this stage is all a keyed producing job has of its own.  Mixed forms: B's scalars and T2's for the item's l messages, and
// zeros WRITTEN for the bases H_{l+1} .. H_L in BOTH arrays (B's sum and T2's run over the same bases; the buffers come from
// the pools and hold what the last job left), so PgBPart runs unchanged.
template <class C, Form F>
struct PgScalarsIn {
    static __host__ __device__ void run(const FormArgs<C, PgArgs<C>>& f, size_t i) {
        if (f.a.status[i] != ST_PENDING) return;
        int l;
        const HashCtx& h = form_domain<F, C>(f.a.cc, f.d, i, f.a.L, l);
        pg_scalars_item<C>(f.a, i, h, l);
        if constexpr (form_mixed(F)) {
            mixed_zero_scalars(f.a.fscal, f.a.n, i, l, f.a.L);
            mixed_zero_scalars(f.a.fscal2, f.a.n, i, l, f.a.L);
        }
    }
};

// lane per (chunk, item): B = P1 + Q1*domain + sum H_j m_j
// lane per (sum, chunk, item): BOTH fixed-base sums of an item over {P1, Q1, H_*} -- B = P1 + Q1 domain + sum H_j m_j
// (scalars fscal; chunks -> bpart, summed by PgBCombine) and T2's sum H_j m~_j (scalars fscal2; chunks -> partials[nvar + f],
// summed by PgFinalize).  Both depend on the scalar stage only, so the second sum no longer rides in the kernel of the
// doubling chains (round 5): table look-ups and mixed additions, 246 registers, no scratch, two wavefronts per SIMD.
template <class C>
struct PgBPart {
    static __host__ __device__ void run(const PgArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int part = (int)(t / n);                        // 0 .. NFIX-1: B;  NFIX .. 2 NFIX-1: T2's sum
        const size_t i = t - (size_t)part * n;
        if (a.status[i] != ST_PENDING) return;
        const bool second = part >= NFIX;
        const int chunk = second ? part - NFIX : part;
        G1Jac<C> r;
        fixed_msm_chunk_to<C>(*a.cc, second ? a.fscal2 : a.fscal, n, i, a.L + 2, chunk, r);
        g1j_store<C>((second ? a.partials + (size_t)a.nvar * 3 * N * n : a.bpart) + (size_t)chunk * 3 * N * n, n, i, r);
    }
};

template <class C>
struct PgBCombine {
    static __host__ __device__ void run(const PgArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> acc = g1j_load<C>(a.bpart, n, i);
        for (int f = 1; f < NFIX; f++) acc = g1j_add_i<C>(acc, g1j_load<C>(a.bpart + (size_t)f * 3 * N * n, n, i));
        g1a_store_mont<C>(a.baff, n, i, g1j_to_aff<C>(acc));
        G1Aff<C> A = g1a_load_canon_to_mont<C>(a.sig_a, n, i);
        if (!g1a_on_curve<C>(A)) { a.status[i] = -41; return; }
        g1a_store_mont<C>(a.baff + (size_t)2 * N * n, n, i, A);
    }
};

// lane per (base, item), base 0 = B, 1 = A: the sub-bases 2^(64 j) P and their tables of odd multiples, true affine, for the comb
// (g1.hpp).  Anything unusual -- the identity, a point of small order (they exist only outside the prime-order subgroup), a
// degenerate step -- leaves comb_ok = 0 and the item's lanes take the joint chains instead: same group elements either way.
template <class C>
struct PgTables {
    static constexpr int WAVES_PER_EU = MSM_WAVES;
    static __host__ __device__ void run(const PgArgs<C>& a, size_t t) {
        using P = typename C::FpP;
        constexpr int N = P::N;
        const size_t n = a.n;
        const int base = (int)(t / n);
        const size_t i = t - (size_t)base * n;
        a.comb_ok[(size_t)base * n + i] = 0;
        if (a.status[i] != ST_PENDING) return;
        const G1Aff<C> p0 = g1a_load_mont<C>(a.baff + (size_t)base * 2 * N * n, n, i);
        if (g1a_is_inf<C>(p0)) return;
        // sub-bases: 2^(64 j) P for j < 4 -- or, under the GLV split (points known to be in the subgroup), P and 2^64 P only:
        // the other two are their images under the endomorphism
        const bool glv = C::K::HAS_GLV && a.glv != 0;
        const int n_sub = glv ? 2 : COMB_PIECES;
        G1Jac<C> q[COMB_PIECES - 1];
        G1Jac<C> cur = g1j_from_aff<C>(p0);
#pragma unroll 1
        for (int j = 0; j < n_sub - 1; j++) {
#pragma unroll 1
            for (int d = 0; d < 64; d++) cur = g1j_dbl<C>(cur);
            if (g1j_is_inf<C>(cur)) return;
            q[j] = cur;
        }
        for (int j = n_sub - 1; j < COMB_PIECES - 1; j++) q[j] = g1j_inf<C>();
        // the sub-bases in affine form go straight to entry 0 of their tables (HBM), where the table builder picks them up:
        // no array of them in this lane's frame (scratch x hardware queues is a budget, DESIGN.md 5 rule 6)
        uint32_t* tb = a.ctab + (size_t)base * comb_table_words(N) * n + i;
        TabHbm<C>{tb, n}.st(0, p0);
        g1j_batch_to_aff_emit<C, COMB_PIECES - 1>(q, [&](int k, const G1Aff<C>& s) { TabHbm<C>{tb + (size_t)(k + 1) * G1_TAB * 2 * N * n, n}.st(0, s); });
        Fp<C> zc[COMB_PIECES];
        bool ok = true;
#pragma unroll 1
        for (int j = 0; j < n_sub; j++) {
            TabHbm<C> tab{tb + (size_t)j * G1_TAB * 2 * N * n, n};
            ok = g1_odd_table<C>(tab.ld(0), tab, zc[j]) && ok;
        }
        if (!ok) return;
        // entries (x', y') of table j are the Jacobian points (x', y', zc_j): to true affine with ONE inversion for the scales
        Fp<C> pre[COMB_PIECES];
        Fp<C> acc = fe_one<P>();
#pragma unroll 1
        for (int j = 0; j < n_sub; j++) { pre[j] = acc; acc = fe_mul<P>(acc, zc[j]); }
        Fp<C> inv = fe_inv<P>(acc);
#pragma unroll 1
        for (int j = n_sub - 1; j >= 0; j--) {
            const Fp<C> zi = fe_mul<P>(inv, pre[j]);
            inv = fe_mul<P>(inv, zc[j]);
            const Fp<C> zi2 = fe_sqr<P>(zi), zi3 = fe_mul<P>(zi2, zi);
            TabHbm<C> tab{tb + (size_t)j * G1_TAB * 2 * N * n, n};
#pragma unroll 1
            for (int e = 0; e < G1_TAB; e++) {
                const G1Aff<C> v = tab.ld(e);
                tab.st(e, G1Aff<C>{fe_mul<P>(v.x, zi2), fe_mul<P>(v.y, zi3)});
            }
        }
        if constexpr (C::K::HAS_GLV) {
            if (glv) {                               // tables 2, 3 = phi of tables 0, 1: (beta x, y)
                const Fp<C> beta = glv_beta<C>();
#pragma unroll 1
                for (int j = 0; j < 2; j++) {
                    TabHbm<C> src{tb + (size_t)j * G1_TAB * 2 * N * n, n}, dst{tb + (size_t)(2 + j) * G1_TAB * 2 * N * n, n};
#pragma unroll 1
                    for (int e = 0; e < G1_TAB; e++) {
                        const G1Aff<C> v = src.ld(e);
                        dst.st(e, G1Aff<C>{fe_mul<P>(v.x, beta), v.y});
                    }
                }
            }
        }
        a.comb_ok[(size_t)base * n + i] = 1;
    }
};

// lane per (part < nvar, item): the variable-base parts -- multiples of B and of the signature point A.  A kernel of its own
// (round 5: the fixed-base chunks are in PgBPart), window tables in HBM, the multiplication routines inlined.
template <class C>
struct PgVarPart {
    static BBS_HD void run(const PgArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        constexpr size_t TW = (size_t)G1_TAB * 2 * N;
        const size_t n = a.n;
        const int part = (int)(t / n);
        const size_t i = t - (size_t)part * n;
        if (a.status[i] != ST_PENDING) return;
        uint32_t* out = a.partials + (size_t)part * 3 * N * n;
        auto scalar = [&](int k, uint32_t* dst) { soa_ld<8>(a.vscal + (size_t)k * 8 * n, n, i, dst); };
        G1Jac<C> r;
        if (a.nvar == PG_NVAR) {
            // split form: part k multiplies B (k < 4) or A by scalar k
            const G1Aff<C> p = g1a_load_mont<C>(a.baff + (size_t)(part < 4 ? 0 : 1) * 2 * N * n, n, i);
            uint32_t k[8];
            scalar(part, k);
            g1_mul_aff_sel_hbm_inl<C>(p, k, a.glv != 0, a.vtab + (size_t)part * TW * n + i, n, r);
        } else if (a.ctab && a.comb_ok[i] && a.comb_ok[n + i]) {
            // comb form: every multiple of B and A from the tables of their 2^(64 j) multiples, 60 doublings per chain.
            // part 0: D = v0 B; 1: Abar = v4 A; 2: Bbar = v1 B - v5 A; 3: T1 = v2 B + v6 A; 4: T2's v3 B
            const uint32_t* tB = a.ctab + i;
            const uint32_t* tA = a.ctab + comb_table_words(N) * n + i;
            uint32_t k0[8], k1[8];
            if (part == 2 || part == 3) {
                scalar(part == 2 ? 1 : 2, k0);
                scalar(part == 2 ? 5 : 6, k1);
                CombTerm tm[2];
                bool done = false;
                if constexpr (C::K::HAS_GLV) {
                    if (a.glv) { comb_recode_glv<C>(k0, false, tB, tm[0]); comb_recode_glv<C>(k1, part == 2, tA, tm[1]); done = true; }
                }
                if (!done) { comb_recode(k0, false, tB, tm[0]); comb_recode(k1, part == 2, tA, tm[1]); }
                g1_comb_sum_to<C, 2>(tm, n, r);
            } else {
                scalar(part == 0 ? 0 : (part == 1 ? 4 : 3), k0);
                CombTerm tm[1];
                bool done = false;
                if constexpr (C::K::HAS_GLV) {
                    if (a.glv) { comb_recode_glv<C>(k0, false, part == 1 ? tA : tB, tm[0]); done = true; }
                }
                if (!done) comb_recode(k0, false, part == 1 ? tA : tB, tm[0]);
                g1_comb_sum_to<C, 1>(tm, n, r);
            }
        } else if (part == 2 || part == 3) {
            // joint form: Bbar = v1 B + v5 (-A) (part 2), T1 = v2 B + v6 A (part 3) -- one doubling chain each; if a table hits an
            // exceptional case (B or A the identity or of small order) the two products one by one on the generic chain
            const G1Aff<C> B = g1a_load_mont<C>(a.baff, n, i);
            G1Aff<C> A = g1a_load_mont<C>(a.baff + (size_t)2 * N * n, n, i);
            if (part == 2) A = g1a_neg<C>(A);
            uint32_t kb[8], ka[8];
            scalar(part == 2 ? 1 : 2, kb);
            scalar(part == 2 ? 5 : 6, ka);
            uint32_t* tabs = a.vtab + (size_t)(part - 2) * 2 * TW * n + i;
            TabHbm<C>{tabs, n}.st(0, B);
            TabHbm<C>{tabs + TW * n, n}.st(0, A);
            bool done = false;
            if constexpr (C::K::HAS_GLV) {
                if (a.glv) done = g1_mul2_tabs_fast<C, true>(kb, ka, tabs, n, r);
            }
            if (!a.glv) done = g1_mul2_tabs_fast<C, false>(kb, ka, tabs, n, r);
            if (!done) {
                const G1Jac<C> x = g1_mul_aff_naf<C>(B, kb);
                r = g1j_add_i<C>(x, g1_mul_aff_naf<C>(A, ka));
            }
        } else {
            // joint form, single multiplications: D = v0 B (part 0), Abar = v4 A (part 1), T2's v3 B (part 4)
            const G1Aff<C> p = g1a_load_mont<C>(a.baff + (size_t)(part == 1 ? 1 : 0) * 2 * N * n, n, i);
            uint32_t k[8];
            scalar(part == 0 ? 0 : (part == 1 ? 4 : 3), k);
            const int slot = part == 0 ? 4 : (part == 1 ? 5 : 6);
            g1_mul_aff_sel_hbm_inl<C>(p, k, a.glv != 0, a.vtab + (size_t)slot * TW * n + i, n, r);
        }
        g1j_store<C>(out, n, i, r);
    }
};

// l: the item's message count (a.L unless the job is a mixed-length one): m^ for the undisclosed j < l
template <class C>
BBS_HD void pg_finalize_item(const PgArgs<C>& a, size_t i, int l) {
    using R = typename C::FrP;
    constexpr int N = C::FpP::N;
    const size_t n = a.n;
    auto part = [&](int p) { return g1j_load<C>(a.partials + (size_t)p * 3 * N * n, n, i); };
    G1Jac<C> pj[5];
    if (a.nvar == PG_NVAR) {
        pj[0] = part(4);                                              // Abar
        pj[1] = g1j_add_i<C>(part(1), g1j_neg<C>(part(5)));             // Bbar = r1r2 B - e r1r2 A
        pj[2] = part(0);                                              // D
        pj[3] = g1j_add_i<C>(part(6), part(2));                         // T1
        pj[4] = part(3);                                              // T2
    } else {
        pj[0] = part(1); pj[1] = part(2); pj[2] = part(0); pj[3] = part(3); pj[4] = part(4);      // the joint chains' own sums
    }
    for (int f = 0; f < NFIX; f++) pj[4] = g1j_add_i<C>(pj[4], part(a.nvar + f));
    G1Aff<C> pa[5];
    g1j_batch_to_aff<C, 5>(pj, pa);
    // challenge (proof_gen.rs:272-328), disclosed indexes sorted + deduplicated (:151-161)
    Sha256 s;
    xmd48_begin(s);
    const uint32_t Rn = a.rcount[i];
    sha256_u64be(s, Rn);
    for (uint32_t k = 0; k < Rn; k++) {
        const uint32_t idx = a.didx[(size_t)k * n + i];
        sha256_u64be(s, idx);
        uint32_t m[8];
        soa_ld<8>(a.msgs + (size_t)idx * 8 * n, n, i, m);
        sha256_limbs_be8(s, m);
    }
    for (int p = 0; p < 5; p++) sha256_g1_compressed<C>(s, pa[p]);
    Fr<C> dom;
    soa_ld<8>(a.dom, n, i, dom.v);
    sha256_fr_be<C>(s, dom);
    sha256_u64be(s, a.ph_len[i]);
    sha256_bytes(s, a.ph_bytes + a.ph_off[i], a.ph_len[i]);
    uint32_t okm[12];
    xmd48_finish(s, a.cc->hash.dst_h2s, a.cc->hash.dst_h2s_len, okm);
    Fr<C> c = fr_from_okm<C>(okm);                                // Montgomery
    // proof_finalize (proof_gen.rs:331-365)
    Fr<C> r2 = fr_to_mont<C>(fr_load_canon<C>(a.rnd5 + (size_t)1 * 8 * n, n, i));
    if (fe_is_zero<R>(r2)) { a.status[i] = -21; return; }         // :346 unwrap
    Fr<C> r3 = fe_inv<R>(r2);
    Fr<C> r1 = fr_to_mont<C>(fr_load_canon<C>(a.rnd5, n, i));
    Fr<C> et = fr_to_mont<C>(fr_load_canon<C>(a.rnd5 + (size_t)2 * 8 * n, n, i));
    Fr<C> r1t = fr_to_mont<C>(fr_load_canon<C>(a.rnd5 + (size_t)3 * 8 * n, n, i));
    Fr<C> r3t = fr_to_mont<C>(fr_load_canon<C>(a.rnd5 + (size_t)4 * 8 * n, n, i));
    Fr<C> e = fr_to_mont<C>(fr_load_canon<C>(a.sig_e, n, i));
    Fr<C> o[4];
    o[0] = fe_to_canonical<R>(fe_add<R>(et, fe_mul<R>(e, c)));
    o[1] = fe_to_canonical<R>(fe_sub<R>(r1t, fe_mul<R>(r1, c)));
    o[2] = fe_to_canonical<R>(fe_sub<R>(r3t, fe_mul<R>(r3, c)));
    o[3] = fe_to_canonical<R>(c);
    for (int k = 0; k < 4; k++) soa_st<8>(a.out_sc + (size_t)k * 8 * n, n, i, o[k].v);
    for (int j = 0; j < l; j++) {
        const uint32_t dm = a.dmask[(size_t)(j >> 5) * n + i];
        if ((dm >> (j & 31)) & 1u) continue;
        Fr<C> m = fr_load_canon<C>(a.msgs + (size_t)j * 8 * n, n, i);       // canonical
        Fr<C> mt = fr_load_canon<C>(a.mtilde + (size_t)j * 8 * n, n, i);   // canonical
        // m~ + m*c : mont_mul(c_mont, m_canon) = m*c canonical ; add canonical values mod r
        Fr<C> mh = fe_add<R>(mt, fe_mul<R>(c, m));
        soa_st<8>(a.out_mhat + (size_t)j * 8 * n, n, i, mh.v);
    }
    for (int p = 0; p < 3; p++) g1a_store_canon<C>(a.out_pts + (size_t)p * 2 * C::FpP::NC * n, n, i, pa[p]);
    a.status[i] = 1;
}
template <class C>
struct PgFinalize {
    static __host__ __device__ void run(const PgArgs<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;
        pg_finalize_item<C>(a, i, a.L);
    }
};
template <class C>
struct PgFinalizeMixed {
    static __host__ __device__ void run(const MixedLenArgs<PgArgs<C>>& m, size_t i) {
        if (m.a.status[i] != ST_PENDING) return;
        pg_finalize_item<C>(m.a, i, (int)m.len[i]);
    }
};

// last stage of proof_gen (lane per item): the proof in the caller's layout, zeros / no commitments unless the status is 1
// l: the item's message count (a.L unless the job is a mixed-length one): commitments for the undisclosed j < l only; the
// strides stay those of L.  A plain inline function, not BBS_HD: forced inlining merges the body into the kernel before it is
// optimised on its own, which moved PgEmit on BLS12-381 from 46 to 50 registers; left to the ordinary inliner (the body is
// small: it is inlined into both kernels) PgEmit keeps the code it had.
template <class C>
__host__ __device__ inline void pg_emit_item(const PgArgs<C>& a, size_t i, int l) {
    constexpr int NC = C::FpP::NC, W = 6 * NC + 32;
    const size_t n = a.n;
    const bool ok = a.status[i] == 1;
    if (a.oct_form) {
        constexpr size_t NB = 4 * NC;
        const size_t stride = 3 * NB + 32 * (size_t)(4 + (a.L > 1 ? a.L : 1));
        uint8_t* o = reinterpret_cast<uint8_t*>(a.out_rec) + i * stride;
        uint32_t u = 0;
        if (ok) {
            for (int p = 0; p < 3; p++) {
                uint32_t pw[2 * NC];
                for (int k = 0; k < 2 * NC; k++) pw[k] = a.out_pts[((size_t)p * 2 * NC + k) * n + i];
                g1_words_to_octets<C>(pw, pw + NC, o + (size_t)p * NB);
            }
            uint32_t w[8];
            for (int q = 0; q < 3; q++) {
                for (int k = 0; k < 8; k++) w[k] = a.out_sc[((size_t)q * 8 + k) * n + i];
                words_be32(w, o + 3 * NB + 32 * (size_t)q);
            }
            for (int j = 0; j < l; j++) {
                const uint32_t dm = a.dmask[(size_t)(j >> 5) * n + i];
                if ((dm >> (j & 31)) & 1u) continue;
                for (int k = 0; k < 8; k++) w[k] = a.out_mhat[((size_t)j * 8 + k) * n + i];
                words_be32(w, o + 3 * NB + 96 + 32 * (size_t)u);
                u++;
            }
            for (int k = 0; k < 8; k++) w[k] = a.out_sc[((size_t)3 * 8 + k) * n + i];
            words_be32(w, o + 3 * NB + 96 + 32 * (size_t)u);
        }
        a.ucount[i] = ok ? u : 0xFFFFFFFFu;          // no string at all for a failed item
        return;
    }
    uint32_t* r = a.out_rec + i * (size_t)W;
    for (int k = 0; k < 6 * NC; k++) r[k] = ok ? a.out_pts[(size_t)k * n + i] : 0u;
    for (int k = 0; k < 32; k++) r[6 * NC + k] = ok ? a.out_sc[(size_t)k * n + i] : 0u;
    uint32_t u = 0;
    if (ok) {
        uint32_t* m = a.out_mh + i * (size_t)(a.L > 1 ? a.L : 1) * 8;
        for (int j = 0; j < l; j++) {
            const uint32_t dm = a.dmask[(size_t)(j >> 5) * n + i];
            if ((dm >> (j & 31)) & 1u) continue;
            for (int k = 0; k < 8; k++) m[(size_t)u * 8 + k] = a.out_mhat[((size_t)j * 8 + k) * n + i];
            u++;
        }
    }
    a.ucount[i] = u;
}
template <class C>
struct PgEmit {
    static __host__ __device__ void run(const PgArgs<C>& a, size_t i) { pg_emit_item<C>(a, i, a.L); }
};
// (a failed item has len = 0 or a count it never uses: nothing is counted or written for it)
template <class C>
struct PgEmitMixed {
    static __host__ __device__ void run(const MixedLenArgs<PgArgs<C>>& m, size_t i) { pg_emit_item<C>(m.a, i, (int)m.len[i]); }
};

}  // namespace bbs
