// Fixed-base table construction, the unit-parity primitives (hash_to_scalar, multi-scalar multiplication) and the
// self-tests of the six-lane Fp12 code.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// =============================================================================================
// fixed-base table construction (once per generator set)
// =============================================================================================
template <class C>
struct TabArgs {
    int n_bases, win_bits, n_windows;
    const uint32_t* bases;    // [n_bases][2N] Montgomery affine (AoS)
    uint32_t* winbase;        // [n_bases][W][2N] : 2^(c*w) * G_k
    uint32_t* tables;         // [n_bases][W][2^(c-1)][fix_tab_stride]
};

// lane per base: the W window bases by repeated doubling
template <class C>
struct TabWinBase {
    static __host__ __device__ void run(const TabArgs<C>& a, size_t k) {
        constexpr int N = C::FpP::N;
        G1Aff<C> b;
        for (int j = 0; j < N; j++) { b.x.v[j] = a.bases[k * 2 * N + j]; b.y.v[j] = a.bases[k * 2 * N + N + j]; }
        for (int w = 0; w < a.n_windows; w++) {
            uint32_t* o = a.winbase + ((size_t)k * a.n_windows + w) * 2 * N;
            for (int j = 0; j < N; j++) { o[j] = b.x.v[j]; o[N + j] = b.y.v[j]; }
            G1Jac<C> t = g1j_from_aff<C>(b);
            for (int d = 0; d < a.win_bits; d++) t = g1j_dbl<C>(t);
            b = g1j_to_aff<C>(t);
        }
    }
};

// lane per table entry (k, w, d): d * winbase[k][w], affine
template <class C>
struct TabEntry {
    static __host__ __device__ void run(const TabArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t per_win = (size_t)1 << (a.win_bits - 1);        // |digit| = 1 .. 2^(c-1) (signed digits)
        const size_t kw = t / per_win;
        const uint32_t d = (uint32_t)(t - kw * per_win) + 1;
        const uint32_t* bsrc = a.winbase + kw * 2 * N;
        G1Aff<C> b;
        for (int j = 0; j < N; j++) { b.x.v[j] = bsrc[j]; b.y.v[j] = bsrc[N + j]; }
        G1Jac<C> r = g1j_inf<C>();
        for (int i = a.win_bits - 1; i >= 0; i--) {
            r = g1j_dbl<C>(r);
            if ((d >> i) & 1u) r = g1j_add_aff<C>(r, b);
        }
        G1Aff<C> o = g1j_to_aff<C>(r);
        uint32_t* dst = a.tables + t * fix_tab_stride<C>();
        for (int j = 0; j < N; j++) { dst[j] = o.x.v[j]; dst[N + j] = o.y.v[j]; }
        for (int j = 2 * N; j < fix_tab_stride<C>(); j++) dst[j] = 0;
    }
};

// =============================================================================================
// unit-parity primitives
// =============================================================================================
struct H2sArgs {
    size_t n;
    const uint32_t* off; const uint32_t* len; const uint8_t* bytes;
    uint8_t dst[256];
    uint32_t dst_len;
    uint32_t* out;            // [8][n] canonical
};

template <class C>
struct H2sItem {
    static __host__ __device__ void run(const H2sArgs& a, size_t i) {
        Sha256 s;
        xmd48_begin(s);
        sha256_bytes(s, a.bytes + a.off[i], a.len[i]);
        uint32_t okm[12];
        xmd48_finish(s, a.dst, a.dst_len, okm);
        Fr<C> r = fe_to_canonical<typename C::FrP>(fr_from_okm<C>(okm));
        soa_st<8>(a.out, a.n, i, r.v);
    }
};

template <class C>
struct MsmArgs {
    size_t n;
    int n_fixed, n_var;
    int glv;                  // see PvArgs
    const CtxConsts<C>* cc;
    const uint32_t* fscal;    // [n_fixed][8][n]
    const uint32_t* vpts;     // [n_var][2NC][n] canonical
    const uint32_t* vscal;    // [n_var][8][n]
    int8_t* status;
    uint32_t* partials;       // [n_var + NFIX][3N][n]
    uint32_t* out;            // [2NC][n] canonical
    FixTreeWork<C> fixwk;     // see PvArgs
    uint32_t* vtab;           // [n_var][G1_TAB][2N][n] window tables of the variable-base terms
};

// lane per (variable-base term, item)
template <class C>
struct MsmVarMul {
    static constexpr int WAVES_PER_EU = chain_waves<C>(1);      // BN254: 264 - 268 registers -> 256
    static BBS_HD void run(const MsmArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int part = (int)(t / n);
        const size_t i = t - (size_t)part * n;
        if (a.status[i] != ST_PENDING) return;
        uint32_t* out = a.partials + (size_t)part * 3 * N * n;
        G1Aff<C> p = g1a_load_canon_to_mont<C>(a.vpts + (size_t)part * 2 * C::FpP::NC * n, n, i);
        G1Jac<C> r = g1j_inf<C>();
        if (!g1a_on_curve<C>(p)) { a.status[i] = -41; g1j_store<C>(out, n, i, r); return; }
        uint32_t k[8];
        soa_ld<8>(a.vscal + (size_t)part * 8 * n, n, i, k);
        g1_mul_aff_sel_hbm_inl<C>(p, k, a.glv != 0, a.vtab + (size_t)part * G1_TAB * 2 * N * n + i, n, r);
        g1j_store<C>(out, n, i, r);
    }
};
// lane per (chunk, item)
template <class C>
struct MsmFixedChunk {
    static __host__ __device__ void run(const MsmArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int chunk = (int)(t / n);
        const size_t i = t - (size_t)chunk * n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> r;
        fixed_msm_chunk_to<C>(*a.cc, a.fscal, n, i, a.n_fixed, chunk, r);
        g1j_store<C>(a.partials + (size_t)(a.n_var + chunk) * 3 * N * n, n, i, r);
    }
};
// the fixed-base sum as one tree of affine additions per item (bbs_ctx_set_fixed_base_tree; lane per item)
template <class C>
struct MsmFixedTree {
    static __host__ __device__ void run(const MsmArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> r = g1j_inf<C>();
        for (int f = 1; f < NFIX; f++) g1j_store<C>(a.partials + (size_t)(a.n_var + f) * 3 * N * n, n, i, r);
        fixed_msm_tree_to<C>(*a.cc, a.fscal, n, i, a.n_fixed, a.fixwk, r);
        g1j_store<C>(a.partials + (size_t)a.n_var * 3 * N * n, n, i, r);
    }
};

template <class C>
struct MsmCombine {
    static __host__ __device__ void run(const MsmArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.status[i] != ST_PENDING) return;
        G1Jac<C> acc = g1j_inf<C>();
        for (int p = 0; p < a.n_var + NFIX; p++) acc = g1j_add_i<C>(acc, g1j_load<C>(a.partials + (size_t)p * 3 * N * n, n, i));
        g1a_store_canon<C>(a.out, n, i, g1j_to_aff<C>(acc));
        a.status[i] = 1;
    }
};

#if !defined(BBS_HOST_TWIN)
// self-test: one Fp12 operation per item computed by the one-lane code (on the host) and by the six-lane code, the items laid
// out over the wavefronts as PairDist lays them out: wave = t / 64, group = (t % 64) / 6, item = wave * 10 + group
template <class C>
struct SelfTestArgs {
    int op;
    size_t n;
    const CtxConsts<C>* cc;
    const uint32_t* b;      // [n][12] Fp (tower order c0.c0.c0, c0.c0.c1, c0.c1.c0 ... ), Montgomery; OP 6: the point (b[0], b[1])
    const int8_t* active;   // [n]: an item that is not active is left by its six lanes before any exchange (a gated item of PairDist)
    int line_table;         // OP 6: 0 = tab_pk, 1 = tab_bp2
    int line_index;         //       the entry of that table
    uint32_t* out_dist;     // [n][12] Fp: the operand x as prepared by the host (already cyclotomic for OP 10, 11), then the result
    int8_t* flag;           // [n]: 1 once the item's result is stored; OP 12: the boolean of d_is_one
};
template <class C, int OP>
struct SelfTestDist {
    static __device__ void run(const SelfTestArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const int lane = (int)(t & 63);
        const int grp = lane / GRP;                 // (pair6_group, written out for this kernel's registers: profiles/pair_body_ab.log)
        if (grp >= GRP_PER_WAVE) return;
        const size_t i = pair6_item(t >> 6, grp);
        if (i >= a.n) return;
        if (!a.active[i]) return;
        const Lane6 L = pair6_lanes(lane, grp);
        // w-basis coefficient m of a tower-ordered array: g_m = (e[2k], e[2k+1]) with k = (m & 1) * 3 + (m >> 1)
        const int k = (L.m & 1) * 3 + (L.m >> 1);
        uint32_t* xd = a.out_dist + i * 12 * N;
        const uint32_t* yd = a.b + i * 12 * N;
        Fp2<C> gx, gy;
        for (int j = 0; j < N; j++) {
            gx.c0.v[j] = xd[(2 * k) * N + j]; gx.c1.v[j] = xd[(2 * k + 1) * N + j];
            gy.c0.v[j] = yd[(2 * k) * N + j]; gy.c1.v[j] = yd[(2 * k + 1) * N + j];
        }
        G1Aff<C> P;
        for (int j = 0; j < N; j++) { P.x.v[j] = yd[j]; P.y.v[j] = yd[N + j]; }
        const uint32_t* ft = &a.cc->frob[0][0][0][0];
        Fp2<C> rd;
        if constexpr (OP == 0) rd = d_mul<C>(L, gx, gy);
        else if constexpr (OP == 1) rd = d_frob<C, 1>(L, gx, ft);
        else if constexpr (OP == 2) rd = d_frob<C, 2>(L, gx, ft);
        else if constexpr (OP == 3) rd = d_frob<C, 3>(L, gx, ft);
        else if constexpr (OP == 4) rd = d_inv<C>(L, gx);
        else if constexpr (OP == 5) rd = d_conj<C>(L, gx);
        else if constexpr (OP == 6) {                      // (the table's form: uniform over the launch)
            const LineTable<C>& tab = a.line_table ? a.cc->tab_bp2 : a.cc->tab_pk;
            rd = tab.unit ? d_mul_line<C, true>(L, gx, tab.e[a.line_index], P) : d_mul_line<C, false>(L, gx, tab.e[a.line_index], P);
        }
        else if constexpr (OP == 7) rd = d_final_exp<C>(L, gx, ft);
        else if constexpr (OP == 10) rd = d_cyclo_sqr<C>(L, gx);
        else if constexpr (OP == 8) rd = d_sqr<C>(L, gx);
        else if constexpr (OP == 11) rd = d_pow_x<C>(L, gx);
        else rd = gx;
        int8_t flag = 1;
        if constexpr (OP == 12) flag = d_is_one<C>(L, gx) ? 1 : 0;
        for (int j = 0; j < N; j++) { xd[(2 * k) * N + j] = rd.c0.v[j]; xd[(2 * k + 1) * N + j] = rd.c1.v[j]; }
        if (L.m == 0) a.flag[i] = flag;
    }
};
#endif

}  // namespace bbs
