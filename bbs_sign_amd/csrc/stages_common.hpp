// Device stages, shared part: constants, the context constants in HBM, SoA and hashing helpers, the fixed-base sum
// (chunk and tree form), normalisation and octet helpers.  See stages.hpp for the work split.
#pragma once
#include "pairing.hpp"
#include "pairing_dist.hpp"
#include "sha256.hpp"

namespace bbs {

constexpr int NFIX = 8;          // fixed-base chunks per MSM (one lane each)
constexpr int MAX_DST = 255;
// Internal per-item states.  Neither is a value the C ABI may return: an item that no kernel has decided stays at one of
// them and bbs_job_fetch_status / bbs_job_wait then fail with BBS_E_STATE instead of reporting Ok(true) (fail closed).
constexpr int8_t ST_PENDING = -128;   // accepted by validation, nothing computed yet
constexpr int8_t ST_PAIRING = -127;   // every check before the pairing passed: the pairing product decides
// Wavefronts per SIMD the kernels are compiled for (register caps).  Decided values: the retired alternatives -- the pairing
// check as two kernels with two wavefronts per SIMD for the final exponentiation (profiles/r04_d_ab_split_pairing_two_waves.log),
// MSM stages at 2 and 3 (no gain, spills) -- are listed in DESIGN.md "Retired experiments".
constexpr int PAIR_WAVES = 1;         // every six-lane pairing kernel, PairFinalDist included (its own value was the retired experiment)
constexpr int MSM_WAVES = 1;          // multi-scalar-multiplication stages
// The doubling-chain kernels of proof_verify capped at 256 registers, so that two of their wavefronts -- or one and a
// wavefront of a fixed-base chunk kernel (246) -- share a SIMD (profiles/r05_i_*): BLS12-381 T1 chain 300 -> 256 (97 spilled)
// gains, the single multiplication (354, 251 spilled) does not and stays at one; BN254's kernels (244 - 268) are all capped.
constexpr int T1_WAVES = 2;
constexpr int VARMUL_WAVES = 1;       // BLS12-381; BN254: 2 (chain_waves below)
constexpr int BN_CHAIN_WAVES = 2;
template <class C> constexpr int chain_waves(int bls_default) { return C::FpP::N <= 10 ? BN_CHAIN_WAVES : bls_default; }

// ---- context constants resident in HBM ------------------------------------------------------
struct HashCtx {
    uint32_t dom_mid[8];         // SHA-256 state after Z_pad || domain prefix, at a block boundary
    uint64_t dom_mid_total;
    uint8_t dom_tail[64];
    uint32_t dom_tail_len;
    uint8_t dst_h2s[256];        // api_id || "H2S_"
    uint32_t dst_h2s_len;
};

template <class C>
struct CtxConsts {
    HashCtx hash;
    G1Aff<C> p1;                 // Montgomery form
    int L;                       // number of message generators
    int n_bases;                 // L + 2 : P1, Q1, H_1..H_L
    int win_bits;                // c
    int n_windows;               // W = ceil(256 / c)
    uint32_t fix_bias[8];        // K = sum over w < W - 1 of 2^(c w + c - 1): signed-digit recoding of the fixed-base scalars
    const uint32_t* tables;      // [base][window][|digit| - 1][fix_tab_stride] affine Montgomery, |digit| in 1 .. 2^(c-1)
    uint32_t frob[3][6][2][C::FpP::N];   // xi^(m (p^k - 1)/6), Montgomery (for the lane-sliced Fp12)
    MillerSchedule sched;
    LineTable<C> tab_pk;         // lines of W = pk
    LineTable<C> tab_bp2;        // lines of BP2
};

// Words from one entry of the fixed-base window tables to the next.  An entry is 2N words (x, y); BLS12-381's 112 bytes are
// padded to 128 (round 5): the tables are read at random, one entry per mixed addition, and an unaligned 112-byte entry
// straddles two 128-byte lines in 7 cases of 8 -- the counters showed 2 x 205 MB fetched per 4096-item batch for 203 MB of
// entries (profiles/r05_p_pmc.csv before the change).  Aligned, an entry is one line and seven 16-byte loads.  BN254's 80
// bytes stay packed (16-byte aligned; padding them to 128 would cost 60 % more table memory).  A/B: profiles/r05_h_ab_table_entries_padded.log.
template <class C>
constexpr int fix_tab_stride() { return 2 * C::FpP::N == 28 ? 32 : 2 * C::FpP::N; }
// one entry (16-byte loads: every entry starts on a 16-byte boundary)
template <class C>
BBS_HD void fix_tab_load(const uint32_t* e, G1Aff<C>& q) {
    constexpr int N = C::FpP::N;
    static_assert((2 * N) % 4 == 0 && fix_tab_stride<C>() % 4 == 0, "table entries are whole 16-byte groups");
    uint32_t w[2 * N];
#pragma unroll
    for (int g = 0; g < 2 * N / 4; g++) {
        const uint4 v = reinterpret_cast<const uint4*>(e)[g];
        w[4 * g] = v.x; w[4 * g + 1] = v.y; w[4 * g + 2] = v.z; w[4 * g + 3] = v.w;
    }
#pragma unroll
    for (int j = 0; j < N; j++) { q.x.v[j] = w[j]; q.y.v[j] = w[N + j]; }
}

// ---- SoA helpers ----------------------------------------------------------------------------
template <int NW>
BBS_HD void soa_ld(const uint32_t* base, size_t n, size_t i, uint32_t* out) {
#pragma unroll
    for (int w = 0; w < NW; w++) out[w] = base[(size_t)w * n + i];
}
template <int NW>
BBS_HD void soa_st(uint32_t* base, size_t n, size_t i, const uint32_t* v) {
#pragma unroll
    for (int w = 0; w < NW; w++) base[(size_t)w * n + i] = v[w];
}

template <class C>
BBS_HD Fr<C> fr_load_canon(const uint32_t* base, size_t n, size_t i) {   // canonical limbs, no conversion
    Fr<C> r;
    soa_ld<8>(base, n, i, r.v);
    return r;
}
template <class C>
BBS_HD Fr<C> fr_to_mont(const Fr<C>& canon) { return fe_from_limbs<typename C::FrP>(canon.v); }

// canonical affine point: 2 * NC 32-bit words per item (x then y)
template <class C>
BBS_HD G1Aff<C> g1a_load_canon_to_mont(const uint32_t* base, size_t n, size_t i) {
    constexpr int NC = C::FpP::NC;
    uint32_t w[2 * NC];
    soa_ld<2 * NC>(base, n, i, w);
    G1Aff<C> p;
    p.x = fe_from_words<typename C::FpP>(w);
    p.y = fe_from_words<typename C::FpP>(w + NC);
    return p;
}
template <class C>
BBS_HD G1Aff<C> g1a_load_mont(const uint32_t* base, size_t n, size_t i) {
    constexpr int N = C::FpP::N;
    G1Aff<C> p;
    soa_ld<N>(base, n, i, p.x.v);
    soa_ld<N>(base + (size_t)N * n, n, i, p.y.v);
    return p;
}
template <class C>
BBS_HD void g1a_store_mont(uint32_t* base, size_t n, size_t i, const G1Aff<C>& p) {
    constexpr int N = C::FpP::N;
    soa_st<N>(base, n, i, p.x.v);
    soa_st<N>(base + (size_t)N * n, n, i, p.y.v);
}
template <class C>
BBS_HD void g1a_store_canon(uint32_t* base, size_t n, size_t i, const G1Aff<C>& p) {
    constexpr int NC = C::FpP::NC;
    uint32_t x[NC], y[NC];
    fe_to_words<typename C::FpP>(p.x, x);
    fe_to_words<typename C::FpP>(p.y, y);
    soa_st<NC>(base, n, i, x);
    soa_st<NC>(base + (size_t)NC * n, n, i, y);
}
template <class C>
BBS_HD G1Jac<C> g1j_load(const uint32_t* base, size_t n, size_t i) {
    constexpr int N = C::FpP::N;
    G1Jac<C> p;
    soa_ld<N>(base, n, i, p.x.v);
    soa_ld<N>(base + (size_t)N * n, n, i, p.y.v);
    soa_ld<N>(base + (size_t)2 * N * n, n, i, p.z.v);
    return p;
}
template <class C>
BBS_HD void g1j_store(uint32_t* base, size_t n, size_t i, const G1Jac<C>& p) {
    constexpr int N = C::FpP::N;
    soa_st<N>(base, n, i, p.x.v);
    soa_st<N>(base + (size_t)N * n, n, i, p.y.v);
    soa_st<N>(base + (size_t)2 * N * n, n, i, p.z.v);
}

// ---- job forms ----------------------------------------------------------------------------------
// The scalar stage is the only stage that knows a job's form: where item i's domain prefix comes from and how many messages
// it has.  Single: the context's prefix, L.  Mixed (bbs_ctx_set_mixed_lengths, .._gen): item i has its own count l = len[i]
// <= L (written by the MIXED ingest bodies; 0 for an item decided before or by the length check) and starts from the prefix of
// that length, pref[l] (runtime.hpp LenSet).  Keyed (bbs_*_keyed_*): the midstate of the item's key-set entry, L.  KeyedMixed
// (bbs_ctx_set_keyed_mixed_lengths): the prefix of THAT key and THAT length, pref[kidx * stride + l] (runtime.hpp KeyLenSet,
// stride = L + 1).  DESIGN.md 8 has the table; job_form.hpp decides and binds the form on the host.
enum class Form { Single, Mixed, Keyed, KeyedMixed };
constexpr bool form_mixed(Form f) { return f == Form::Mixed || f == Form::KeyedMixed; }
constexpr bool form_keyed(Form f) { return f == Form::Keyed || f == Form::KeyedMixed; }
// what a key set holds per key (keyed.hpp): the only two things of a verification that depend on the key
template <class C>
struct KeyEntry {
    LineTable<C> tab;            // lines of W = this key
    HashCtx hash;                // domain prefix midstate with this key (dst_h2s as the context's)
};
template <class C>
struct DomainSrc {
    const HashCtx* pref; uint32_t stride;                  // Mixed: [L + 1]; KeyedMixed: [n_keys][stride]
    const KeyEntry<C>* keys; const uint32_t* kidx;         // Keyed, KeyedMixed: [n] key of item i
    const uint32_t* len;                                   // Mixed, KeyedMixed: [n]
    const uint32_t* sks;                                   // keyed sign only: rows of the signing set
};
// the arguments of a scalar stage in a derived form: its fixed-length neighbour's plus the source of the domains
template <class C, class A>
struct FormArgs { A a; DomainSrc<C> d; };
template <class A>
struct MixedIngestArgs { A a; uint32_t* len; };
// Item i's prefix and (l) its count.  Only a pending item is looked at: KEY_NONE (decided by KeyGate) and l > L (decided at
// ingest, len = 0) never index anything.  In every derived form the index diverges per lane, so the 368 bytes of the HashCtx
// are read with vector loads through a per-lane pointer: the struct is returned and passed on BY REFERENCE, never copied into
// a local (368 B of scratch per lane).
template <Form F, class C>
BBS_HD const HashCtx& form_domain(const CtxConsts<C>* cc, const DomainSrc<C>& d, size_t i, int L, int& l) {
    if constexpr (form_mixed(F)) l = (int)d.len[i]; else l = L;
    if constexpr (F == Form::Single) return cc->hash;
    else if constexpr (F == Form::Mixed) return d.pref[l];
    else if constexpr (F == Form::Keyed) return d.keys[d.kidx[i]].hash;
    else return d.pref[(size_t)d.kidx[i] * d.stride + (size_t)l];
}
// the scalars of the bases H_{l+1} .. H_L of an item with l messages: written as zero, never assumed
BBS_HD void mixed_zero_scalars(uint32_t* fscal, size_t n, size_t i, int l, int L) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = l; j < L; j++) soa_st<8>(fscal + (size_t)(2 + j) * 8 * n, n, i, z);
}

// ---- hashing helpers ------------------------------------------------------------------------
// ark-serialize compressed G1 absorbed into a hash (core_utilities.rs:39-47, proof_gen.rs:304-311)
template <class C>
__host__ __device__ inline void sha256_g1_compressed(Sha256& s, const G1Aff<C>& p) {
    using P = typename C::FpP;
    constexpr int N = P::NC;                     // canonical words
    const bool inf = g1a_is_inf<C>(p);
    struct { uint32_t v[P::NC]; } x, yw;
    fe_to_words<P>(p.x, x.v);
    fe_to_words<P>(p.y, yw.v);
    const bool ybig = words_gt_half<P>(yw.v);
    if constexpr (C::ID == 0) {
        // 48 bytes big-endian, flags in the first byte
        uint32_t flags = inf ? 0xC0000000u : (0x80000000u | (ybig ? 0x20000000u : 0u));
#pragma unroll
        for (int i = N - 1; i >= 0; i--) {
            uint32_t w = inf ? 0u : x.v[i];
            if (i == N - 1) w |= flags;
            sha256_word(s, w);
        }
    } else {
        // 32 bytes little-endian, flags in the last byte
        uint32_t flags = inf ? 0x40u : (ybig ? 0x80u : 0u);
#pragma unroll
        for (int i = 0; i < N; i++) {
            uint32_t l = inf ? 0u : x.v[i];
            uint32_t w = (l << 24) | ((l & 0xff00u) << 8) | ((l >> 8) & 0xff00u) | (l >> 24);   // bswap
            if (i == N - 1) w |= flags;
            sha256_word(s, w);
        }
    }
}

// calculate_domain (core_utilities.rs:24-63) from the cached prefix midstate
template <class C>
__host__ __device__ inline Fr<C> domain_from_header(const HashCtx& h, const uint8_t* hdr, uint32_t hdr_len) {
    Sha256 s;
    sha256_init_mid(s, h.dom_mid, h.dom_mid_total);
    sha256_bytes(s, h.dom_tail, h.dom_tail_len);
    sha256_u64be(s, hdr_len);
    sha256_bytes(s, hdr, hdr_len);
    uint32_t okm[12];
    xmd48_finish(s, h.dst_h2s, h.dst_h2s_len, okm);
    return fr_from_okm<C>(okm);
}

// ---- multi-scalar multiplication parts --------------------------------------------------------
// one chunk of the fixed-base sum: terms are (base k, window w) pairs, flattened index t = k*W + w,
// chunk f of NFIX handles t in [f*T/NFIX, (f+1)*T/NFIX).
// (result through `out`, the accumulator a plain local: where this function is not inlined, a named return value is
// the caller's memory and every addition of the loop would start with a scratch round trip -- DESIGN.md 5 rule 7b)
// SIGNED digits (round 3): a table holds 2^(c-1) entries per (base, window) instead of 2^c - 1 -- half the memory, half the
// build time, the same number of additions.  The scalar s < r < 2^255 is biased once, sb = s + K with
// K = sum_{w < W-1} 2^(c w + c - 1) (no carry chain between windows: one 256-bit addition per scalar); window w < W - 1 then
// contributes the digit  ((sb >> c w) mod 2^c) - 2^(c-1)  in [-2^(c-1), 2^(c-1) - 1], the top window  sb >> c (W - 1)  in
// [0, 2^(c-1)] (it holds at most c - 1 bits of s plus the carry), and  sum_w digit_w 2^(c w) = sb - K = s.  A negative
// digit adds the NEGATED table entry (y -> -y).
template <class C>
BBS_HD void fixed_bias_scalar(const CtxConsts<C>& cc, uint32_t* sc) {
    uint64_t cy = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { cy += (uint64_t)sc[j] + cc.fix_bias[j]; sc[j] = (uint32_t)cy; cy >>= 32; }
}
// window w of a biased scalar: |digit| (0 = nothing to add) and its sign
BBS_HD uint32_t fixed_digit(const uint32_t* sb, int w, int c, int W, bool& neg) {
    const int bit = w * c;
    const int li = bit >> 5, sh = bit & 31;
    uint64_t two = sb[li];
    if (li + 1 < 8) two |= (uint64_t)sb[li + 1] << 32;
    const uint32_t half = 1u << (c - 1);
    uint32_t raw = (uint32_t)(two >> sh);
    if (w == W - 1) {
        // top window: the 256 - c (W - 1) <= c remaining bits (nothing is loaded from beyond bit 256).  A canonical scalar
        // gives raw <= 2^(c-1); clamped so that a non-canonical one could never index past the table
        neg = false;
        return raw > half ? half : raw;
    }
    raw &= (half << 1) - 1u;
    neg = raw < half;
    return neg ? half - raw : raw - half;
}

template <class C>
__host__ __device__ inline void fixed_msm_chunk_to(const CtxConsts<C>& cc, const uint32_t* fscal, size_t n, size_t i,
                                                   int n_terms, int chunk, G1Jac<C>& out) {
    constexpr int N = C::FpP::N;
    const int W = cc.n_windows, c = cc.win_bits;
    const int T = n_terms * W;
    const int t0 = (int)(((long long)T * chunk) / NFIX), t1 = (int)(((long long)T * (chunk + 1)) / NFIX);
    const size_t per_win = (size_t)1 << (c - 1);
    G1Jac<C> acc = g1j_inf<C>();
    int k_cur = -1;
    uint32_t sc[8];
    // table entry of term t (false: digit 0, nothing to add)
    auto fetch = [&](int t, G1Aff<C>& q) -> bool {
        const int k = t / W, w = t - k * W;
        if (k != k_cur) { soa_ld<8>(fscal + (size_t)k * 8 * n, n, i, sc); fixed_bias_scalar<C>(cc, sc); k_cur = k; }
        bool neg;
        const uint32_t d = fixed_digit(sc, w, c, W, neg);
        if (d == 0) return false;
        fix_tab_load<C>(cc.tables + (((size_t)k * W + w) * per_win + (d - 1)) * fix_tab_stride<C>(), q);
        q.y = fe_select<typename C::FpP>(neg, fe_neg<typename C::FpP>(q.y), q.y);
        return true;
    };
    // the entry of term t + 1 is requested before the addition of term t: the (random, HBM) table read of one
    // term overlaps the ~11 multiplications of the previous one -- with one wavefront per SIMD nothing else hides it
    G1Aff<C> qn = g1a_inf<C>();
    bool hn = t0 < t1 ? fetch(t0, qn) : false;
    for (int t = t0; t < t1; t++) {
        const G1Aff<C> q = qn;
        const bool h = hn;
        hn = t + 1 < t1 ? fetch(t + 1, qn) : false;
        if (h) acc = g1j_add_aff<C>(acc, q);
    }
    out = acc;
}
template <class C>
BBS_HD G1Jac<C> fixed_msm_chunk(const CtxConsts<C>& cc, const uint32_t* fscal, size_t n, size_t i, int n_terms, int chunk) {
    G1Jac<C> r;
    fixed_msm_chunk_to<C>(cc, fscal, n, i, n_terms, chunk, r);
    return r;
}

// ---- the fixed-base sum as a tree of AFFINE additions (bbs_ctx_set_fixed_base_tree) -------------------------------------
// All T = n_terms * W table entries of an item are summed by ONE lane, pairwise, level by level.  The slopes of a level
// share one inversion (Montgomery's trick: prefix products on the way up, one fe_inv, back-substitution on the way
// down): 5M + 1S per addition instead of the 7M + 4S of a mixed Jacobian addition, ceil(log2 T) inversions per item.
// The points of a level live in HBM work arrays of the job ([slot][2N words][n items]: coalesced over the items of a
// wavefront); (0, 0) is the identity.  Every exceptional case of affine addition is resolved per pair: an identity
// operand (digit 0), equal points (doubling, slope 3x^2 / 2y -- caller-supplied generators may repeat), opposite points
// (identity).  The result is the same group element as the sum of the NFIX chunks of fixed_msm_chunk.
template <class C>
struct FixTreeWork {
    uint32_t* pts0;     // [T][2N][n]
    uint32_t* pts1;     // [ceil(T/2)][2N][n]
    uint32_t* pre;      // [floor(T/2)][N][n]   prefix products of a level
};

template <class C>
__host__ __device__ inline void fixed_msm_tree_to(const CtxConsts<C>& cc, const uint32_t* fscal, size_t n, size_t i, int n_terms,
                                                  const FixTreeWork<C>& wk, G1Jac<C>& out) {
    using P = typename C::FpP;
    constexpr int N = P::N;
    const int W = cc.n_windows, c = cc.win_bits;
    const int T = n_terms * W;
    const size_t per_win = (size_t)1 << (c - 1);
    auto ld = [&](const uint32_t* a, int slot) {
        G1Aff<C> q;
        const uint32_t* b = a + (size_t)slot * 2 * N * n + i;
#pragma unroll
        for (int j = 0; j < N; j++) { q.x.v[j] = b[(size_t)j * n]; q.y.v[j] = b[(size_t)(N + j) * n]; }
        return q;
    };
    auto st = [&](uint32_t* a, int slot, const G1Aff<C>& q) {
        uint32_t* b = a + (size_t)slot * 2 * N * n + i;
#pragma unroll
        for (int j = 0; j < N; j++) { b[(size_t)j * n] = q.x.v[j]; b[(size_t)(N + j) * n] = q.y.v[j]; }
    };
    // level 0: the table entries themselves (digit 0 -> identity).  The reads are random 112-byte HBM accesses and nothing
    // depends on them but the store behind them: four are in flight at a time (a load -> store chain per entry would pay
    // the full memory latency 442 times per item)
    {
        auto entry = [&](int t, bool& neg) -> const uint32_t* {
            const int k = t / W, w = t - k * W;
            uint32_t sc[8];
            soa_ld<8>(fscal + (size_t)k * 8 * n, n, i, sc);
            fixed_bias_scalar<C>(cc, sc);
            const uint32_t d = fixed_digit(sc, w, c, W, neg);
            return d ? cc.tables + (((size_t)k * W + w) * per_win + (d - 1)) * fix_tab_stride<C>() : nullptr;
        };
        constexpr int G = 4;
        for (int t0 = 0; t0 < T; t0 += G) {
            G1Aff<C> q[G];
#pragma unroll
            for (int g = 0; g < G; g++) {
                q[g] = g1a_inf<C>();
                bool neg = false;
                const uint32_t* e = t0 + g < T ? entry(t0 + g, neg) : nullptr;
                if (e) {
                    fix_tab_load<C>(e, q[g]);
                    q[g].y = fe_select<P>(neg, fe_neg<P>(q[g].y), q[g].y);
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++) if (t0 + g < T) st(wk.pts0, t0 + g, q[g]);
        }
    }
    // what a pair needs: the denominator of its slope (1 when the result needs none), and how to finish it
    struct Pair { Fp<C> den, dy; bool trivial, dbl, pinf, qinf; };
    auto classify = [&](const G1Aff<C>& p, const G1Aff<C>& q) {
        Pair r;
        r.pinf = g1a_is_inf<C>(p); r.qinf = g1a_is_inf<C>(q);
        const Fp<C> dx = fe_sub<P>(q.x, p.x);
        r.dy = fe_sub<P>(q.y, p.y);
        const bool same_x = fe_is_zero<P>(dx), same_y = fe_is_zero<P>(r.dy);
        r.trivial = r.pinf | r.qinf | (same_x & !same_y);            // the other operand, or P + (-P) = identity
        r.dbl = !r.pinf & !r.qinf & same_x & same_y;                 // P + P (y != 0: no point of order two on these curves)
        r.den = fe_select<P>(r.trivial, fe_one<P>(), fe_select<P>(r.dbl, fe_dbl<P>(p.y), dx));
        return r;
    };
    uint32_t* src = wk.pts0;
    uint32_t* dst = wk.pts1;
    int m = T;
    while (m > 1) {
        const int h = m >> 1;
        // up: prefix products of the denominators (pre[j] = product of den_0 .. den_{j-1})
        Fp<C> acc = fe_one<P>();
        {
            G1Aff<C> pn = ld(src, 0), qn = ld(src, 1);
            for (int j = 0; j < h; j++) {
                const G1Aff<C> p = pn, q = qn;
                if (j + 1 < h) { pn = ld(src, 2 * j + 2); qn = ld(src, 2 * j + 3); }     // requested one pair ahead
                const Pair pr = classify(p, q);
                uint32_t* b = wk.pre + (size_t)j * N * n + i;
#pragma unroll
                for (int l = 0; l < N; l++) b[(size_t)l * n] = acc.v[l];
                acc = fe_mul_i<P>(acc, pr.den);
            }
        }
        Fp<C> inv = fe_inv<P>(acc);                                   // never zero: every den is non-zero by construction
        // down: slope of pair j = num_j * inv(den_j), inv(den_j) = pre[j] * inv(den_0 .. den_j)
        {
            G1Aff<C> pn = ld(src, 2 * h - 2), qn = ld(src, 2 * h - 1);
            Fp<C> pren;
            { const uint32_t* b = wk.pre + (size_t)(h - 1) * N * n + i;
#pragma unroll
              for (int l = 0; l < N; l++) pren.v[l] = b[(size_t)l * n]; }
            for (int j = h - 1; j >= 0; j--) {
                const G1Aff<C> p = pn, q = qn;
                const Fp<C> pre_j = pren;
                if (j > 0) {
                    pn = ld(src, 2 * j - 2); qn = ld(src, 2 * j - 1);
                    const uint32_t* b = wk.pre + (size_t)(j - 1) * N * n + i;
#pragma unroll
                    for (int l = 0; l < N; l++) pren.v[l] = b[(size_t)l * n];
                }
                const Pair pr = classify(p, q);
                const Fp<C> inv_j = fe_mul_i<P>(inv, pre_j);
                inv = fe_mul_i<P>(inv, pr.den);
                Fp<C> num = pr.dy;
                if (pr.dbl) num = fe_scale<P, 3>(fe_sqr_i<P>(p.x));
                const Fp<C> lam = fe_mul_i<P>(num, inv_j);
                G1Aff<C> r;
                r.x = fe_lin<P, 1, -1, -1>(fe_sqr_i<P>(lam), p.x, q.x);
                r.y = fe_sub<P>(fe_mul_i<P>(lam, fe_sub<P>(p.x, r.x)), p.y);
                const G1Aff<C> other = pr.pinf ? q : (pr.qinf ? p : g1a_inf<C>());
                r.x = fe_select<P>(pr.trivial, other.x, r.x);
                r.y = fe_select<P>(pr.trivial, other.y, r.y);
                st(dst, j, r);
            }
        }
        if (m & 1) st(dst, h, ld(src, m - 1));
        m = h + (m & 1);
        uint32_t* t = src; src = dst; dst = t;
    }
    out = T > 0 ? g1j_from_aff<C>(ld(src, 0)) : g1j_inf<C>();
}

// shared inversion for two Jacobian points -> affine (Montgomery trick), identities preserved
template <class C>
__host__ __device__ inline void g1j_to_aff2(const G1Jac<C>& a, const G1Jac<C>& b, G1Aff<C>& oa, G1Aff<C>& ob) {
    using P = typename C::FpP;
    const bool ia = g1j_is_inf<C>(a), ib = g1j_is_inf<C>(b);
    Fp<C> za = ia ? fe_one<P>() : a.z, zb = ib ? fe_one<P>() : b.z;
    Fp<C> inv = fe_inv<P>(fe_mul<P>(za, zb));
    Fp<C> zai = fe_mul<P>(inv, zb), zbi = fe_mul<P>(inv, za);
    Fp<C> zai2 = fe_sqr<P>(zai), zbi2 = fe_sqr<P>(zbi);
    oa = ia ? g1a_inf<C>() : G1Aff<C>{fe_mul<P>(a.x, zai2), fe_mul<P>(fe_mul<P>(a.y, zai2), zai)};
    ob = ib ? g1a_inf<C>() : G1Aff<C>{fe_mul<P>(b.x, zbi2), fe_mul<P>(fe_mul<P>(b.y, zbi2), zbi)};
}

// n-point batch normalisation (one inversion), identities preserved
// emit(k, affine point k), k = K-1 .. 0 (one shared inversion; a caller that stores the points elsewhere needs no array of them)
template <class C, int K, class Emit>
__host__ __device__ inline void g1j_batch_to_aff_emit(const G1Jac<C>* in, Emit emit) {
    using P = typename C::FpP;
    Fp<C> pre[K];
    Fp<C> acc = fe_one<P>();
    for (int k = 0; k < K; k++) {
        pre[k] = acc;
        if (!g1j_is_inf<C>(in[k])) acc = fe_mul<P>(acc, in[k].z);
    }
    Fp<C> inv = fe_inv<P>(acc);
    for (int k = K - 1; k >= 0; k--) {
        if (g1j_is_inf<C>(in[k])) { emit(k, g1a_inf<C>()); continue; }
        Fp<C> zi = fe_mul<P>(inv, pre[k]);
        inv = fe_mul<P>(inv, in[k].z);
        Fp<C> zi2 = fe_sqr<P>(zi);
        emit(k, G1Aff<C>{fe_mul<P>(in[k].x, zi2), fe_mul<P>(fe_mul<P>(in[k].y, zi2), zi)});
    }
}
template <class C, int K>
__host__ __device__ inline void g1j_batch_to_aff(const G1Jac<C>* in, G1Aff<C>* out) {
    g1j_batch_to_aff_emit<C, K>(in, [&](int k, const G1Aff<C>& p) { out[k] = p; });
}

// 32 big-endian bytes (any alignment) -> 8 little-endian words
BBS_HD void be32_words(const uint8_t* b, uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint8_t* q = b + 28 - 4 * k;
        w[k] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
    }
}

// 8 little-endian words -> 32 big-endian bytes (I2OSP(x, 32))
BBS_HD void words_be32(const uint32_t* w, uint8_t* b) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t v = w[7 - k];
        b[4 * k] = (uint8_t)(v >> 24); b[4 * k + 1] = (uint8_t)(v >> 16); b[4 * k + 2] = (uint8_t)(v >> 8); b[4 * k + 3] = (uint8_t)v;
    }
}
// compressed G1 octets from CANONICAL affine words (x: NC words, y: NC words; all zero = identity), the formats of
// codec_dev.hpp: BLS12-381 48 bytes big-endian with flags 0x80 / 0x40 / 0x20 in byte 0, BN254 32 bytes little-endian with
// flags 0x80 (y is the larger root) / 0x40 (identity) in the last byte
template <class C>
BBS_HD void g1_words_to_octets(const uint32_t* xw, const uint32_t* yw, uint8_t* out) {
    using P = typename C::FpP;
    constexpr int NC = P::NC, NB = 4 * NC;
    uint32_t any = 0;
#pragma unroll
    for (int k = 0; k < NC; k++) any |= xw[k] | yw[k];
    const bool inf = any == 0;
    const bool ybig = !inf && words_gt_half<P>(yw);
    if constexpr (C::ID == 0) {
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const uint32_t v = xw[NC - 1 - k];
            out[4 * k] = (uint8_t)(v >> 24); out[4 * k + 1] = (uint8_t)(v >> 16); out[4 * k + 2] = (uint8_t)(v >> 8); out[4 * k + 3] = (uint8_t)v;
        }
        out[0] |= (uint8_t)(0x80u | (inf ? 0x40u : 0u) | (ybig ? 0x20u : 0u));
    } else {
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const uint32_t v = xw[k];
            out[4 * k] = (uint8_t)v; out[4 * k + 1] = (uint8_t)(v >> 8); out[4 * k + 2] = (uint8_t)(v >> 16); out[4 * k + 3] = (uint8_t)(v >> 24);
        }
        out[NB - 1] |= (uint8_t)((inf ? 0x40u : 0u) | (ybig ? 0x80u : 0u));
    }
}

}  // namespace bbs
