// Device stages of proof_verify.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// =============================================================================================
// proof_verify
// =============================================================================================
constexpr int PV_NVAR = 2;                    // (c*Bbar + e^*Abar + r1^*D) jointly, r3^*D
constexpr int PV_NVAR_SPLIT = 4;              // latency mode: c*Bbar, e^*Abar, r1^*D, r3^*D each on its own lane
constexpr int PV_NPARTS = PV_NVAR + NFIX;
constexpr int PV_NPARTS_MAX = PV_NVAR_SPLIT + NFIX;
// throughput form only (nvar = PV_NVAR): two more terms of T1, behind the fixed-base chunks.  Identity unless the joint chain
// of an item could not be used (a proof point that is the identity or of small order): then T1's three products are computed
// one by one and land in slots 0, PV_T1_EXTRA, PV_T1_EXTRA + 1; PvChallenge adds them up in either case.
constexpr int PV_T1_EXTRA = PV_NVAR + NFIX;
static_assert(PV_T1_EXTRA + 2 <= PV_NPARTS_MAX, "partial-sum slots");

template <class C>
struct PvArgs {
    size_t n;
    int L, Rmax;
    const CtxConsts<C>* cc;
    int glv;                  // inputs vouched to be in G1: GLV split for the variable-base terms (BLS12-381)
    int nvar;                 // PV_NVAR (throughput: T1 as one joint chain) or PV_NVAR_SPLIT (latency: bbs_ctx_set_latency_mode)
    // batch verification, throughput form: PvChallenge also prepares the combination (RlcPrep of pippenger.hpp) -- null otherwise
    uint8_t* bv_dig; uint32_t* bv_ppts; size_t bv_n_pad; uint32_t bv_seed[8];
    // inputs (canonical limbs, SoA)
    const uint32_t* pts;      // [3][2NC][n] a_bar, b_bar, d (canonical words)
    const uint32_t* sc;       // [4][8][n]   e_cap, r1_cap, r3_cap, challenge
    const uint32_t* slots;    // [L][8][n]   slot j: disclosed message m_j or commitment m^_j
    const uint32_t* dmask;    // [ceil(L/32)][n]
    const uint32_t* didx;     // [Rmax][n]   disclosed indexes in caller order
    const uint32_t* rcount;   // [n]
    const uint32_t* hdr_off; const uint32_t* hdr_len; const uint8_t* hdr_bytes;
    const uint32_t* ph_off;  const uint32_t* ph_len;  const uint8_t* ph_bytes;
    int8_t* status;           // [n]; ST_PENDING = to compute, ST_PAIRING = pairing pending, else final
    // intermediates
    uint32_t* dom;            // [8][n] domain, Montgomery
    uint32_t* fscal;          // [L+2][8][n] canonical fixed-base scalars
    uint32_t* partials;       // [nvar + NFIX][3N][n] Jacobian
    uint32_t* aff;            // [5][2N][n] Montgomery affine: a_bar, b_bar, d, T1, T2
    uint32_t* fmiller;        // [2][12N][n]
    uint32_t* vtab;           // [4][G1_TAB][2N][n] window tables: three of the joint multiplication, one of D * r3^ (g1.hpp)
    FixTreeWork<C> fixwk;     // pts0 != nullptr: the fixed-base sum as one tree of affine additions per item (chunk 0's lane)
};

// stage 0 (lane per item, once per upload): the work the reference does before any arithmetic, on the raw batch as the
// C ABI receives it (item-major records, ragged arrays with 64-bit offsets) -- proof_verify_init's checks in the
// reference's order (src/proof_verify.rs:139-150), the duplicate test behind its out-of-bounds panic (:177-179), range
// checks of every scalar and coordinate (arkworks' types cannot hold a non-canonical value), and the transposition
// into the SoA arrays the later stages read.  Reads are strided by the record size, writes are coalesced.
template <class C>
struct PvIngestArgs {
    size_t n;
    int L, dst_too_long;
    const uint32_t* rec;                  // n records a_bar || b_bar || d || e^ || r1^ || r3^ || c, little-endian words
    const uint64_t *cm_off, *dm_off, *di_off, *hdr_off64, *ph_off64;   // n + 1 entries each, rebased to start at 0
    const uint32_t* cm;                   // commitments, 8 words each
    const uint32_t* dm;                   // disclosed messages, 8 words each
    const uint64_t* di;                   // disclosed indexes
    uint32_t *pts, *sc, *slots, *dmask, *didx, *rcount, *hdr_off, *hdr_len, *ph_off, *ph_len;   // PvArgs arrays
    int8_t* status0;                      // ST_PENDING or the reference's Err / panic / a non-canonical input
};

// MIXED (bbs_ctx_set_mixed_lengths, PvIngestMixed below): the item's own count l = commitments + disclosed indexes may be
// anything in 0 .. L and is recorded in len[i]; every check is made against l as before, only l != L becomes l > L
template <class C, bool MIXED>
struct PvIngestBody {
    static BBS_HD void run(const PvIngestArgs<C>& a, size_t i, uint32_t* len) {
        using P = typename C::FpP;
        using R = typename C::FrP;
        constexpr int NC = P::NC;
        constexpr int RECW = 6 * NC + 32;
        const size_t n = a.n;
        a.hdr_off[i] = (uint32_t)a.hdr_off64[i];
        a.hdr_len[i] = (uint32_t)(a.hdr_off64[i + 1] - a.hdr_off64[i]);
        a.ph_off[i] = (uint32_t)a.ph_off64[i];
        a.ph_len[i] = (uint32_t)(a.ph_off64[i + 1] - a.ph_off64[i]);
        const uint64_t u = a.cm_off[i + 1] - a.cm_off[i], r = a.di_off[i + 1] - a.di_off[i], rm = a.dm_off[i + 1] - a.dm_off[i];
        const uint64_t l = u + r;
        if constexpr (MIXED) len[i] = l > (uint64_t)a.L ? 0u : (uint32_t)l;
        const uint64_t* idx = a.di + a.di_off[i];
        const int MW = ((a.L > 1 ? a.L : 1) + 31) / 32;
        for (int w = 0; w < MW; w++) a.dmask[(size_t)w * n + i] = 0;
        a.rcount[i] = 0;
        int8_t st = ST_PENDING;
        bool bad = false;
        for (uint64_t k = 0; k < r; k++) bad |= idx[k] >= l;
        if (bad) st = -3;                                      // InvalidDisclosedIndex
        else if (rm != r) st = -6;                             // InvalidIndicesAndMessagesLength
        else if (MIXED ? l > (uint64_t)a.L : l != (uint64_t)a.L) st = -1;   // InvalidMessageAndGeneratorsLength
        else if (a.dst_too_long) st = -23;
        else {
            // duplicates make the undisclosed set larger than `commitments`: the reference indexes
            // proof.commitments[i] out of bounds (proof_verify.rs:177-179) and panics
            uint64_t distinct = 0;
            for (uint64_t k = 0; k < r; k++) {
                const size_t j = (size_t)idx[k];
                uint32_t* wp = a.dmask + (j >> 5) * n + i;
                const uint32_t w = *wp, bit = 1u << (j & 31);
                if (!(w & bit)) { *wp = w | bit; distinct++; }
            }
            if (distinct != r) st = -22;
        }
        if (st != ST_PENDING) { a.status0[i] = st; return; }
        bool ok = true;
        const uint32_t* pf = a.rec + i * (size_t)RECW;
        for (int c = 0; c < 6; c++) {                          // six coordinates
            uint32_t w[NC];
#pragma unroll
            for (int k = 0; k < NC; k++) w[k] = pf[c * NC + k];
            ok &= limbs_lt_mod<P>(w);
            soa_st<NC>(a.pts + (size_t)c * NC * n, n, i, w);
        }
        for (int c = 0; c < 4; c++) {
            uint32_t w[8];
            soa_ld<8>(pf + 6 * NC + 8 * c, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.sc + (size_t)c * 8 * n, n, i, w);
        }
        // slots: disclosed messages at their index, commitments at the sorted undisclosed indexes
        for (uint64_t k = 0; k < r; k++) {
            const size_t j = (size_t)idx[k];
            uint32_t w[8];
            soa_ld<8>(a.dm + (a.dm_off[i] + k) * 8, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.slots + j * 8 * n, n, i, w);
            a.didx[(size_t)k * n + i] = (uint32_t)j;
        }
        uint64_t cu = 0;
        for (size_t j = 0; j < (size_t)l; j++) {
            if ((a.dmask[(j >> 5) * n + i] >> (j & 31)) & 1u) continue;
            uint32_t w[8];
            soa_ld<8>(a.cm + (a.cm_off[i] + cu) * 8, 1, 0, w);
            ok &= limbs_lt_mod<R>(w);
            soa_st<8>(a.slots + j * 8 * n, n, i, w);
            cu++;
        }
        a.rcount[i] = (uint32_t)r;
        a.status0[i] = ok ? ST_PENDING : (int8_t)-40;
    }
};
template <class C>
struct PvIngest {
    static __host__ __device__ void run(const PvIngestArgs<C>& a, size_t i) { PvIngestBody<C, false>::run(a, i, nullptr); }
};
template <class C>
struct PvIngestMixed {
    static __host__ __device__ void run(const MixedIngestArgs<PvIngestArgs<C>>& m, size_t i) { PvIngestBody<C, true>::run(m.a, i, m.len); }
};

// stage 1 (lane per item): domain, fixed-base scalars.  h: the domain prefix of the item's key (the context's, or its key-set
// entry in a keyed job: stages_common.hpp form_domain); l: the item's message count (a.L unless the job is a mixed-length one)
template <class C>
BBS_HD void pv_scalars_item(const PvArgs<C>& a, size_t i, const HashCtx& h, int l) {
    using R = typename C::FrP;
    const size_t n = a.n;
    Fr<C> dom = domain_from_header<C>(h, a.hdr_bytes + a.hdr_off[i], a.hdr_len[i]);
    soa_st<8>(a.dom, n, i, dom.v);
    Fr<C> c_canon = fr_load_canon<C>(a.sc + (size_t)3 * 8 * n, n, i);
    Fr<C> c_m = fr_to_mont<C>(c_canon);
    // P1 * c
    soa_st<8>(a.fscal, n, i, c_canon.v);
    // Q1 * (domain * c) : mont_mul(dom_mont, c_canon) = dom*c canonical... dom is Montgomery:
    Fr<C> dc = fe_mul<R>(dom, c_canon);                 // (dom*R)*c/R = dom*c canonical
    soa_st<8>(a.fscal + (size_t)1 * 8 * n, n, i, dc.v);
    for (int j = 0; j < l; j++) {
        Fr<C> s = fr_load_canon<C>(a.slots + (size_t)j * 8 * n, n, i);
        const uint32_t m = a.dmask[(size_t)(j >> 5) * n + i];
        if ((m >> (j & 31)) & 1u) s = fe_mul<R>(c_m, s);    // (c*R)*m/R = c*m canonical
        soa_st<8>(a.fscal + (size_t)(2 + j) * 8 * n, n, i, s.v);
    }
}
template <class C>
struct PvScalars {
    static __host__ __device__ void run(const PvArgs<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;
        pv_scalars_item<C>(a, i, a.cc->hash, a.L);
    }
};
// The derived forms (stages_common.hpp Form): the item's prefix and count from the job's DomainSrc.  In the two mixed forms the
// item's scalars fill fscal[2 .. 2 + l) and the scalars of the bases H_{l+1} .. H_L are WRITTEN as zero (the buffers come from
// the pools and hold anything): a zero scalar biased by K has the digit 0 in every window (fixed_digit), so the fixed-base
// kernels add nothing for those bases and run unchanged.  DESIGN.md 8 "Job forms".
template <class C, Form F>
struct PvScalarsIn {
    static __host__ __device__ void run(const FormArgs<C, PvArgs<C>>& f, size_t i) {
        if (f.a.status[i] != ST_PENDING) return;
        int l;
        const HashCtx& h = form_domain<F, C>(f.a.cc, f.d, i, f.a.L, l);
        pv_scalars_item<C>(f.a, i, h, l);
        if constexpr (form_mixed(F)) mixed_zero_scalars(f.a.fscal, f.a.n, i, l, f.a.L);
    }
};

// stage 2: the multi-scalar multiplication, as THREE kernels with their own register and scratch budgets (round 5; one
// kernel with four branch bodies -- 428 registers, 2.7 KB of scratch per lane -- charged that budget to the 512 of its 640
// wavefronts that only look up table entries and add them).  Every part writes its Jacobian partial sum to
// partials[part], part = 0: T1's chain, 1 .. nvar-1: single variable-base multiplications, nvar + f: fixed-base chunk f.
//
// stage 2a (lane per item): the on-curve checks of the proof's three points, their Montgomery copies, and -- throughput form
// -- T1 = c*Bbar + e^*Abar + r1^*D (proof_verify.rs:163-164) on one shared doubling chain.  (Latency form: T1's three terms are
// parts 0 .. 2 of PvVarMul, summed by PvChallenge, and this stage only checks and converts.)  The only stage that can decide
// -41 (a point off the curve); the other two may run beside it on other streams and need not see that verdict: what they
// compute for such an item is never read (PvChallenge runs behind all three and skips it).
template <class C>
struct PvT1Chain {
    static constexpr int WAVES_PER_EU = chain_waves<C>(T1_WAVES);
    static BBS_HD void run(const PvArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        constexpr int NC = C::FpP::NC;
        constexpr size_t TW = (size_t)G1_TAB * 2 * N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        const bool joint = a.nvar == PV_NVAR;
        {
            // Abar, Bbar, D: on the curve?  Montgomery copies for the challenge stage (and batch verification); in the
            // throughput form also entry 0 of their window tables (tables 1, 0, 2: the chain's order is Bbar, Abar, D)
            bool on = true;
#pragma unroll 1
            for (int k = 0; k < 3; k++) {
                const G1Aff<C> p = g1a_load_canon_to_mont<C>(a.pts + (size_t)k * 2 * NC * n, n, i);
                on = g1a_on_curve<C>(p) && on;
                g1a_store_mont<C>(a.aff + (size_t)k * 2 * N * n, n, i, p);
                if (joint) TabHbm<C>{a.vtab + (size_t)(k == 0 ? 1 : (k == 1 ? 0 : 2)) * TW * n + i, n}.st(0, p);
            }
            if (!on) { a.status[i] = -41; return; }
        }
        if (!joint) return;
        uint32_t kc[8], ke[8], k1[8];
        soa_ld<8>(a.sc + (size_t)3 * 8 * n, n, i, kc);
        soa_ld<8>(a.sc, n, i, ke);
        soa_ld<8>(a.sc + (size_t)1 * 8 * n, n, i, k1);
        uint32_t* const x0 = a.partials + (size_t)PV_T1_EXTRA * 3 * N * n;
        uint32_t* const x1 = a.partials + (size_t)(PV_T1_EXTRA + 1) * 3 * N * n;
        G1Jac<C> r;
        bool done = false;
        if constexpr (C::K::HAS_GLV) {
            if (a.glv) done = g1_mul3_tabs_fast<C, true>(kc, ke, k1, a.vtab + i, n, r);
        }
        if (!a.glv) done = g1_mul3_tabs_fast<C, false>(kc, ke, k1, a.vtab + i, n, r);
        if (done) {
            g1j_store<C>(a.partials, n, i, r);
            r = g1j_inf<C>();
            g1j_store<C>(x0, n, i, r);
            g1j_store<C>(x1, n, i, r);
        } else {
            // a table hit an exceptional case (a proof point that is the identity or of small order, i.e. outside the
            // prime-order subgroup): the three products one by one on the generic double-and-add chain, which is right for
            // any on-curve point; PvChallenge sums the three slots.  Rare by construction, so its speed is of no concern,
            // but its frame is: a windowed multiplication here would add 0.9 KB to the kernel's scratch.
#pragma unroll 1
            for (int k = 0; k < 3; k++) {
                const G1Aff<C> p = g1a_load_mont<C>(a.aff + (size_t)(k == 0 ? 1 : (k == 1 ? 0 : 2)) * 2 * N * n, n, i);
                const uint32_t* kk = k == 0 ? kc : (k == 1 ? ke : k1);
                g1j_store<C>(k == 0 ? a.partials : (k == 1 ? x0 : x1), n, i, g1_mul_aff_naf<C>(p, kk));
            }
        }
    }
};
// stage 2b (lane per (part, item)): single variable-base multiplications -- r3^*D, the variable-base term of T2
// (proof_verify.rs:175-182), always (part nvar - 1); in the latency form also T1's three terms c*Bbar, e^*Abar, r1^*D (parts
// 0, 1, 2).  Window tables in HBM (a private table is 0.9 KB of scratch per lane of the whole kernel, and scratch x hardware
// queues is a budget: DESIGN.md 5 rule 6).  Reads the points in canonical form, as the ingest stage left them.
template <class C>
struct PvVarMul {
    static constexpr int WAVES_PER_EU = chain_waves<C>(VARMUL_WAVES);
    static __host__ __device__ int first_part(const PvArgs<C>& a) { return a.nvar == PV_NVAR ? 1 : 0; }
    static BBS_HD void run(const PvArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        constexpr int NC = C::FpP::NC;
        const size_t n = a.n;
        const int rel = (int)(t / n);
        const int part = first_part(a) + rel;
        const size_t i = t - (size_t)rel * n;
        if (a.status[i] != ST_PENDING) return;
        const bool last = part == a.nvar - 1;
        const int pt = last ? 2 : (part == 0 ? 1 : (part == 1 ? 0 : 2));   // point: D | Bbar, Abar, D
        const int sc = last ? 2 : (part == 0 ? 3 : (part == 1 ? 0 : 1));   // scalar: r3^ | c, e^, r1^
        G1Aff<C> p = g1a_load_canon_to_mont<C>(a.pts + (size_t)pt * 2 * NC * n, n, i);
        uint32_t k[8];
        soa_ld<8>(a.sc + (size_t)sc * 8 * n, n, i, k);
        const int slot = last ? 3 : part;                                   // vtab slot 3 is D * r3^ in both forms
        G1Jac<C> r;
        g1_mul_aff_sel_hbm_inl<C>(p, k, a.glv != 0, a.vtab + (size_t)slot * G1_TAB * 2 * N * n + i, n, r);
        g1j_store<C>(a.partials + (size_t)part * 3 * N * n, n, i, r);
    }
};
// stages 2a + 2b as ONE launch (lane per (unit, item); unit 0 = stage 2a, the others stage 2b): for a job that keeps
// everything on one stream (batch verification's throughput form), where two launches would run one after the other
template <class C>
struct PvChains {
    static constexpr int WAVES_PER_EU = chain_waves<C>(T1_WAVES < VARMUL_WAVES ? T1_WAVES : VARMUL_WAVES);
    static __host__ __device__ size_t units(const PvArgs<C>& a) { return (size_t)1 + (size_t)(a.nvar - PvVarMul<C>::first_part(a)); }
    static BBS_HD void run(const PvArgs<C>& a, size_t t) {
        if (t < a.n) PvT1Chain<C>::run(a, t);
        else PvVarMul<C>::run(a, t - a.n);
    }
};
// stage 2c (lane per (chunk, item)): the NFIX chunks of the fixed-base sum over {P1, Q1, H_*}: table look-ups and mixed
// additions with inlined multipliers, nothing else -- no scratch, two wavefronts per SIMD.
template <class C>
struct PvFixedChunk {
    static __host__ __device__ void run(const PvArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int chunk = (int)(t / n);
        const size_t i = t - (size_t)chunk * n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> r;
        fixed_msm_chunk_to<C>(*a.cc, a.fscal, n, i, a.L + 2, chunk, r);
        g1j_store<C>(a.partials + (size_t)(a.nvar + chunk) * 3 * N * n, n, i, r);
    }
};
// the same sum as ONE tree of affine additions per item (bbs_ctx_set_fixed_base_tree; lane per item): the result is chunk 0's
// partial sum, the other chunks are the identity
template <class C>
struct PvFixedTree {
    static __host__ __device__ void run(const PvArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> r = g1j_inf<C>();
        for (int f = 1; f < NFIX; f++) g1j_store<C>(a.partials + (size_t)(a.nvar + f) * 3 * N * n, n, i, r);
        fixed_msm_tree_to<C>(*a.cc, a.fscal, n, i, a.L + 2, a.fixwk, r);
        g1j_store<C>(a.partials + (size_t)a.nvar * 3 * N * n, n, i, r);
    }
};

// stage 3 (lane per item): combine parts, normalise, challenge hash, compare
template <class C>
struct PvChallenge {
    static constexpr int WAVES_PER_EU = chain_waves<C>(1);      // BN254: 264 - 268 registers -> 256
    static __host__ __device__ void run(const PvArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        auto part = [&](int p) { return g1j_load<C>(a.partials + (size_t)p * 3 * N * n, n, i); };
        G1Jac<C> t1 = part(0);
        for (int p = 1; p < a.nvar - 1; p++) t1 = g1j_add_i<C>(t1, part(p));       // latency mode: the three terms of T1
        if (a.nvar == PV_NVAR) {                                                  // throughput form: identities unless the joint chain was not usable
            t1 = g1j_add_i<C>(t1, part(PV_T1_EXTRA));
            t1 = g1j_add_i<C>(t1, part(PV_T1_EXTRA + 1));
        }
        G1Jac<C> t2 = part(a.nvar - 1);
        for (int f = 0; f < NFIX; f++) t2 = g1j_add_i<C>(t2, part(a.nvar + f));
        G1Aff<C> T1, T2;
        g1j_to_aff2<C>(t1, t2, T1, T2);
        // challenge (proof_gen.rs:272-328)
        Sha256 s;
        xmd48_begin(s);
        const uint32_t R = a.rcount[i];
        sha256_u64be(s, R);
        for (uint32_t k = 0; k < R; k++) {
            const uint32_t idx = a.didx[(size_t)k * n + i];
            sha256_u64be(s, idx);
            uint32_t m[8];
            soa_ld<8>(a.slots + (size_t)idx * 8 * n, n, i, m);
            sha256_limbs_be8(s, m);
        }
        for (int p = 0; p < 3; p++) sha256_g1_compressed<C>(s, g1a_load_mont<C>(a.aff + (size_t)p * 2 * N * n, n, i));
        sha256_g1_compressed<C>(s, T1);
        sha256_g1_compressed<C>(s, T2);
        Fr<C> dom;
        soa_ld<8>(a.dom, n, i, dom.v);
        sha256_fr_be<C>(s, dom);
        sha256_u64be(s, a.ph_len[i]);
        sha256_bytes(s, a.ph_bytes + a.ph_off[i], a.ph_len[i]);
        uint32_t okm[12];
        xmd48_finish(s, a.cc->hash.dst_h2s, a.cc->hash.dst_h2s_len, okm);
        Fr<C> chal = fe_to_canonical<typename C::FrP>(fr_from_okm<C>(okm));
        Fr<C> c = fr_load_canon<C>(a.sc + (size_t)3 * 8 * n, n, i);
        // proof_verify.rs:108-110: mismatch -> Ok(false) before any pairing
        a.status[i] = fe_eq<typename C::FrP>(chal, c) ? ST_PAIRING : (int8_t)0;
    }
    // batch verification, throughput form: every lane -- also those that left run() early -- then prepares its item's part
    // of the combination (digits of rho_i, the two points item-major); see RlcPrep in pippenger.hpp
    static __host__ __device__ void run_with_bv_prep(const PvArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        run(a, i);
        const size_t n = a.n;
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        G1Aff<C> p = g1a_inf<C>(), q = g1a_inf<C>();
        if (a.status[i] == ST_PAIRING) {
            p = g1a_load_mont<C>(a.aff, n, i);
            q = g1a_load_mont<C>(a.aff + (size_t)2 * N * n, n, i);
            Sha256 s;
            sha256_init(s);
            for (int k = 0; k < 8; k++) sha256_word(s, a.bv_seed[k]);
            sha256_u64be(s, (uint64_t)i);
            sha256_final(s, h);
        }
        for (int w = 0; w < 16; w++) a.bv_dig[(size_t)w * a.bv_n_pad + i] = (uint8_t)(h[w >> 2] >> (8 * (w & 3)));
        g1a_store_mont<C>(a.bv_ppts + i * 2 * N, 1, 0, p);
        g1a_store_mont<C>(a.bv_ppts + (n + i) * 2 * N, 1, 0, q);
    }
};
template <class C>
struct PvChallengeBv {
    static constexpr int WAVES_PER_EU = chain_waves<C>(1);      // BN254: 264 - 268 registers -> 256
    static __host__ __device__ void run(const PvArgs<C>& a, size_t i) { PvChallenge<C>::run_with_bv_prep(a, i); }
};

// proof_verify runs the pairing concurrently with the MSM/challenge stages (the pairing needs only
// the proof's own points); this joins the two results.  proof_verify.rs:108-115: challenge
// mismatch -> Ok(false), otherwise the pairing boolean.
struct PvFinishArgs { size_t n; int8_t* status; const int8_t* pair_ok; };
struct PvFinish {
    static __host__ __device__ void run(const PvFinishArgs& a, size_t i) {
        if (a.status[i] == ST_PAIRING) a.status[i] = a.pair_ok[i] == 1 ? 1 : 0;
    }
};

}  // namespace bbs
