// Device stages of the pairing check: the one-lane stages of the CPU-side test build and the six-lane kernels.
#pragma once
#include "stages_common.hpp"

namespace bbs {

// generic pairing stages: e(Pa, pk) * e(Pb, BP2) == 1 for items whose status is 2
template <class C>
struct PairArgs {
    size_t n;
    const CtxConsts<C>* cc;
    const uint32_t* pa;       // [2N][n] Montgomery affine
    const uint32_t* pb;       // [2N][n]
    int negate_b;             // use -Pb (e(P, -Q) = e(-P, Q))
    int canonical;            // pa/pb hold canonical limbs (converted here) instead of Montgomery
    const int8_t* gate_arr;   // item i is processed iff gate_arr[i] == gate
    int gate;
    int8_t* out;              // result 1 / 0 per item (may alias the status array)
    uint32_t* fmiller;        // one-lane stages: [2][12N][n] (f12_store); six-lane kernels: fmiller_slot
    // batch verification: this launch is the per-item FALLBACK behind the combined checks -- if all n_checks of them passed
    // (batch_ok[k] == 1), every gated item's product is 1 (error 2^-128) and the lane only writes that; null otherwise
    const int8_t* batch_ok;
    int n_checks;
};
template <class C>
BBS_HD bool pair_batch_passed(const PairArgs<C>& a) {
    if (!a.batch_ok) return false;
    int ok = 1;
    for (int k = 0; k < a.n_checks; k++) ok &= (a.batch_ok[k] == 1);
    return ok != 0;
}

template <class C>
BBS_HD G1Aff<C> pair_load_point(const PairArgs<C>& a, const uint32_t* base, size_t i) {
    return a.canonical ? g1a_load_canon_to_mont<C>(base, a.n, i) : g1a_load_mont<C>(base, a.n, i);
}

// Fp12 <-> 12 Fp in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, .., c1.c2.c1), no pointer casts
template <class C>
BBS_HD void f12_to_array(const Fp12<C>& f, Fp<C>* e) {
    e[0] = f.c0.c0.c0; e[1] = f.c0.c0.c1; e[2] = f.c0.c1.c0; e[3] = f.c0.c1.c1; e[4] = f.c0.c2.c0; e[5] = f.c0.c2.c1;
    e[6] = f.c1.c0.c0; e[7] = f.c1.c0.c1; e[8] = f.c1.c1.c0; e[9] = f.c1.c1.c1; e[10] = f.c1.c2.c0; e[11] = f.c1.c2.c1;
}
template <class C>
BBS_HD Fp12<C> f12_from_array(const Fp<C>* e) {
    Fp12<C> f;
    f.c0.c0.c0 = e[0]; f.c0.c0.c1 = e[1]; f.c0.c1.c0 = e[2]; f.c0.c1.c1 = e[3]; f.c0.c2.c0 = e[4]; f.c0.c2.c1 = e[5];
    f.c1.c0.c0 = e[6]; f.c1.c0.c1 = e[7]; f.c1.c1.c0 = e[8]; f.c1.c1.c1 = e[9]; f.c1.c2.c0 = e[10]; f.c1.c2.c1 = e[11];
    return f;
}
template <class C>
BBS_HD void f12_store(uint32_t* base, size_t n, size_t i, const Fp12<C>& f) {
    constexpr int N = C::FpP::N;
    Fp<C> e[12];
    f12_to_array<C>(f, e);
#pragma unroll
    for (int k = 0; k < 12; k++) soa_st<N>(base + (size_t)k * N * n, n, i, e[k].v);
}
template <class C>
BBS_HD Fp12<C> f12_load(const uint32_t* base, size_t n, size_t i) {
    constexpr int N = C::FpP::N;
    Fp<C> e[12];
#pragma unroll
    for (int k = 0; k < 12; k++) soa_ld<N>(base + (size_t)k * N * n, n, i, e[k].v);
    return f12_from_array<C>(e);
}

// the one-lane Miller loop of ONE pair (a pair whose point or table is the identity contributes 1)
template <class C>
BBS_HD Fp12<C> miller_one_pair(const LineTable<C>& tab, const G1Aff<C>& P, const MillerSchedule& sched) {
    Fp12<C> f = f12_one<C>();
    if (g1a_is_inf<C>(P) | (tab.q_is_identity != 0)) return f;
    int li = 0;
    for (int k = 0; k < sched.n_ops; k++) {
        if (sched.op[k] == 0) f = f12_sqr<C>(f);
        else f = f12_mul_line<C>(f, tab.e[li++], P, tab.unit != 0);
    }
    if constexpr (C::K::X_NEG) f = f12_conj<C>(f);
    return f;
}

// lane per (pair, item)
template <class C>
struct PairMiller {
    static __host__ __device__ void run(const PairArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        const int pair = (int)(t / n);
        const size_t i = t - (size_t)pair * n;
        if (a.gate_arr[i] != a.gate) return;
        if (pair_batch_passed<C>(a)) return;
        G1Aff<C> P = pair_load_point<C>(a, pair == 0 ? a.pa : a.pb, i);
        if (pair == 1 && a.negate_b) P = g1a_neg<C>(P);
        const LineTable<C>& tab = pair == 0 ? a.cc->tab_pk : a.cc->tab_bp2;
        f12_store<C>(a.fmiller + (size_t)pair * 12 * N * n, n, i, miller_one_pair<C>(tab, P, a.cc->sched));
    }
};

// lane per item
template <class C>
struct PairFinal {
    static __host__ __device__ void run(const PairArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        const size_t n = a.n;
        if (a.gate_arr[i] != a.gate) return;
        if (pair_batch_passed<C>(a)) { a.out[i] = 1; return; }
        Fp12<C> f = f12_mul<C>(f12_load<C>(a.fmiller, n, i), f12_load<C>(a.fmiller + (size_t)12 * N * n, n, i));
        a.out[i] = f12_is_one<C>(final_exponentiation<C>(f)) ? 1 : 0;
    }
};

// canonical affine inputs -> Montgomery, on-curve check, status 2 (pairing pending)
template <class C>
struct PairPrep {
    const uint32_t* pa_c; const uint32_t* pb_c; uint32_t* pa; uint32_t* pb; int8_t* status; size_t n;
    static __host__ __device__ void run(const PairPrep<C>& a, size_t i) {
        if (a.status[i] != ST_PENDING) return;     // flagged by validation
        G1Aff<C> p = g1a_load_canon_to_mont<C>(a.pa_c, a.n, i), q = g1a_load_canon_to_mont<C>(a.pb_c, a.n, i);
        if (!g1a_on_curve<C>(p) || !g1a_on_curve<C>(q)) { a.status[i] = -41; return; }
        g1a_store_mont<C>(a.pa, a.n, i, p);
        g1a_store_mont<C>(a.pb, a.n, i, q);
        a.status[i] = ST_PAIRING;
    }
};

#if !defined(BBS_HOST_TWIN)
// =============================================================================================
// wavefront-cooperative pairing check (pairing_dist.hpp): six lanes per item, Miller loop of both
// pairs (shared squarings) and the final exponentiation fused in one kernel, nothing spilled to HBM.
// Thread index: wave = t / 64 ; group = (t % 64) / 6 ; item = wave * 10 + group.
// UNIT: the form of BOTH line tables (pairing.hpp "Unit form"), picked by the host per job.
// =============================================================================================
// The product of one item on its six lanes: e(Pa, W) * e(Pb, BP2) == 1, W's lines in *tw.  Both bodies of PairDistKeyed call it
// with a key-set entry's table (keyed.hpp); PairDist below is the same body with tw = &cc->tab_pk, written out for its registers.
// Every lane of the group returns the boolean.
template <class C, bool UNIT>
__device__ __forceinline__ bool pair6_product_is_one(const Lane6& L, const CtxConsts<C>* cc, const LineTable<C>* tw, const G1Aff<C>& Pa,
                                                     const G1Aff<C>& Pb) {
    const bool skipA = g1a_is_inf<C>(Pa) | (tw->q_is_identity != 0);
    const bool skipB = g1a_is_inf<C>(Pb) | (cc->tab_bp2.q_is_identity != 0);
    Fp2<C> f = d_one<C>(L);
    if (!(skipA & skipB)) {
        // the Miller accumulator is its own variable, never handed by reference to a non-inlined function: that
        // would make it a memory object and put a scratch store / load of it around every step of the loop
        Fp2<C> m = d_one<C>(L);
        int li = 0;
        const int nops = cc->sched.n_ops;
        for (int k = 0; k < nops; k++) {
            if (cc->sched.op[k] == 0) {
                m = d_sqr<C>(L, m);
            } else {
                if (!skipA) m = d_mul_line<C, UNIT>(L, m, tw->e[li], Pa);
                if (!skipB) m = d_mul_line<C, UNIT>(L, m, cc->tab_bp2.e[li], Pb);
                li++;
            }
        }
        if constexpr (C::K::X_NEG) m = d_conj<C>(L, m);
        const Fp2<C> mf = m;
        f = d_final_exp<C>(L, mf, &cc->frob[0][0][0][0]);
    }
    return d_is_one<C>(L, f);
}

template <class C, bool UNIT>
struct PairDist {
    static constexpr int WAVES_PER_EU = PAIR_WAVES;
    static __device__ void run(const PairArgs<C>& a, size_t t) {
        const int lane = (int)(t & 63);
        const int grp = pair6_group(lane);
        if (grp < 0) return;
        const size_t i = pair6_item(t >> 6, grp);
        if (i >= a.n) return;
        if (a.gate_arr[i] != a.gate) return;
        const Lane6 L = pair6_lanes(lane, grp);
        if (pair_batch_passed<C>(a)) { if (L.m == 0) a.out[i] = 1; return; }
        G1Aff<C> Pa = pair_load_point<C>(a, a.pa, i);
        G1Aff<C> Pb = pair_load_point<C>(a, a.pb, i);
        if (a.negate_b) Pb = g1a_neg<C>(Pb);
        // pair6_product_is_one's body with W = cc->tab_pk, written out: no form of the call leaves the registers of this kernel
        // and of PairDistKeyed both as they are (profiles/pair_body_ab.log, section 2).  A change to either body goes into both.
        const CtxConsts<C>* cc = a.cc;
        const bool skipA = g1a_is_inf<C>(Pa) | (cc->tab_pk.q_is_identity != 0);
        const bool skipB = g1a_is_inf<C>(Pb) | (cc->tab_bp2.q_is_identity != 0);
        Fp2<C> f = d_one<C>(L);
        if (!(skipA & skipB)) {
            Fp2<C> m = d_one<C>(L);
            int li = 0;
            const int nops = cc->sched.n_ops;
            for (int k = 0; k < nops; k++) {
                if (cc->sched.op[k] == 0) {
                    m = d_sqr<C>(L, m);
                } else {
                    if (!skipA) m = d_mul_line<C, UNIT>(L, m, cc->tab_pk.e[li], Pa);
                    if (!skipB) m = d_mul_line<C, UNIT>(L, m, cc->tab_bp2.e[li], Pb);
                    li++;
                }
            }
            if constexpr (C::K::X_NEG) m = d_conj<C>(L, m);
            const Fp2<C> mf = m;
            f = d_final_exp<C>(L, mf, &cc->frob[0][0][0][0]);
        }
        const bool one = d_is_one<C>(L, f);
        if (L.m == 0) a.out[i] = one ? 1 : 0;
    }
};

// The Miller values between PairMillerHalf and PairFinalDist: fmiller is [pair][lane m][2N][n], lane m = w-basis coefficient m =
// the tower's Fp2 number (m & 1) * 3 + (m >> 1); limb j of c0 at row j, of c1 at row N + j (coalesced over the items' lanes m)
template <class C>
BBS_HD size_t fmiller_slot(size_t n, int pair, int m, int row, size_t i) {
    return (((size_t)pair * GRP + m) * 2 * C::FpP::N + row) * n + i;
}
template <class C>
BBS_HD void fmiller_store(uint32_t* fm, size_t n, int pair, int m, size_t i, const Fp2<C>& g) {
    constexpr int N = C::FpP::N;
    uint32_t* o = fm + fmiller_slot<C>(n, pair, m, 0, i);
#pragma unroll
    for (int j = 0; j < N; j++) { o[(size_t)j * n] = g.c0.v[j]; o[(size_t)(N + j) * n] = g.c1.v[j]; }
}
template <class C>
BBS_HD Fp2<C> fmiller_load(const uint32_t* fm, size_t n, int pair, int m, size_t i) {
    constexpr int N = C::FpP::N;
    const uint32_t* p = fm + fmiller_slot<C>(n, pair, m, 0, i);
    Fp2<C> g;
#pragma unroll
    for (int j = 0; j < N; j++) { g.c0.v[j] = p[(size_t)j * n]; g.c1.v[j] = p[(size_t)(N + j) * n]; }
    return g;
}

// ---- latency form (round 3): the two Miller loops of an item on SEPARATE six-lane groups ------------------------------
// PairDist runs both pairs of an item on one group (63 shared squarings + 2 x 68 line products) and then the final
// exponentiation: 410 wavefronts of ~4.9 ms for a 4096-item batch on a chip of 1024 SIMDs.  When a batch has the chip to
// itself that is the critical path.  Here wavefront 2 v runs the loop of pair 0 = (Pa, pk) and wavefront 2 v + 1 the loop
// of pair 1 = (+-Pb, BP2) of the same ten items (the line table is uniform per wavefront: scalar loads), each 63
// squarings + 68 line products (0.66 of the joint loop), the two values are handed over in HBM ([pair][coefficient]
// [2N][n], coalesced over the items' lanes m) and PairFinalDist multiplies them and runs the final exponentiation:
// 820 wavefronts x 0.66 + 410 wavefronts x 1 instead of 410 x 2: 17 % more wave-time, a critical path ~0.8 ms shorter.
template <class C, bool UNIT>
struct PairMillerHalf {
    static constexpr int WAVES_PER_EU = PAIR_WAVES;
    static __device__ void run(const PairArgs<C>& a, size_t t) {
        const int lane = (int)(t & 63);
        const int grp = pair6_group(lane);
        if (grp < 0) return;
        const size_t wave = t >> 6;
        const int pair = (int)(wave & 1);
        const size_t i = pair6_item(wave >> 1, grp);
        if (i >= a.n) return;
        if (a.gate_arr[i] != a.gate) return;
        if (pair_batch_passed<C>(a)) return;                   // PairFinalDist writes the verdict
        const Lane6 L = pair6_lanes(lane, grp);
        G1Aff<C> P = pair_load_point<C>(a, pair ? a.pb : a.pa, i);
        if (pair && a.negate_b) P = g1a_neg<C>(P);
        const CtxConsts<C>* cc = a.cc;
        const LineTable<C>& tab = pair ? cc->tab_bp2 : cc->tab_pk;
        const bool skip = g1a_is_inf<C>(P) | (tab.q_is_identity != 0);
        Fp2<C> m = d_one<C>(L);
        if (!skip) {
            int li = 0;
            const int nops = cc->sched.n_ops;
            for (int k = 0; k < nops; k++) {
                if (cc->sched.op[k] == 0) m = d_sqr<C>(L, m);
                else m = d_mul_line<C, UNIT>(L, m, tab.e[li++], P);
            }
            if constexpr (C::K::X_NEG) m = d_conj<C>(L, m);
        }
        // fmiller_store, written out: through the helper this kernel takes more registers and, on BN254, loses its second
        // wavefront per SIMD (profiles/pair_body_ab.log, section 2)
        constexpr int N = C::FpP::N;
        uint32_t* o = a.fmiller + ((size_t)pair * GRP + L.m) * 2 * N * a.n + i;
#pragma unroll
        for (int j = 0; j < N; j++) { o[(size_t)j * a.n] = m.c0.v[j]; o[(size_t)(N + j) * a.n] = m.c1.v[j]; }
    }
};
template <class C>
struct PairFinalDist {
    static constexpr int WAVES_PER_EU = PAIR_WAVES;
    static __device__ void run(const PairArgs<C>& a, size_t t) {
        const int lane = (int)(t & 63);
        const int grp = pair6_group(lane);
        if (grp < 0) return;
        const size_t i = pair6_item(t >> 6, grp);
        if (i >= a.n) return;
        if (a.gate_arr[i] != a.gate) return;
        const Lane6 L = pair6_lanes(lane, grp);
        if (pair_batch_passed<C>(a)) { if (L.m == 0) a.out[i] = 1; return; }
        const Fp2<C> mf = d_mul<C>(L, fmiller_load<C>(a.fmiller, a.n, 0, L.m, i), fmiller_load<C>(a.fmiller, a.n, 1, L.m, i));
        const Fp2<C> f = d_final_exp<C>(L, mf, &a.cc->frob[0][0][0][0]);
        const bool one = d_is_one<C>(L, f);
        if (L.m == 0) a.out[i] = one ? 1 : 0;
    }
};
#endif

}  // namespace bbs
