// Two-pair optimal-ate pairing product check  e(P_a, Q_a) * e(P_b, Q_b) == 1  with BOTH G2
// arguments fixed per issuer key, so their Miller-loop line coefficients are precomputed once
// (host, at bbs_ctx_set_pk) and the per-item device work is: evaluate lines at P, sparse-multiply
// into one shared accumulator f, one shared final exponentiation.
//
// Replaces (boolean-identically) the two full `E::pairing` calls + GT multiplication + `== ONE`
// at /root/reference/src/proof_verify.rs:112-115 and src/verify.rs:88-92.  A pair whose G1 or G2
// argument is the identity contributes 1 (ark-ec skips it; pinned by
// src/tests/bbs_over_bls_tests.rs:119-133,156-169).
//
// Line table entry k holds (c, nl) in Fp2: the line through T and T' (tangent when equal) on the
// twist is  y - yT = lam (x - xT);  c = lam*xT - yT,  nl = -lam.  Evaluated at P = (xP, yP) and
// scaled by a factor the final exponentiation kills it is
//   M-type twist (BLS12-381):  c + (nl*xP) v + yP v w
//   D-type twist (BN254)    :  yP + (nl*xP + c v) w
//
// Unit form.  c lies in Fp2, so the final exponentiation kills it as well: where every c of a table is invertible the
// builder scales each line by 1/c and the constant term becomes a constant of Fp --
//   M-type twist:  k + (k (nl/c)*xP) v + (k (1/c)*yP) v w
//   D-type twist:  k (1/c)*yP + (k (nl/c)*xP + k v) w
// -- with k = R^-1, R the Montgomery radix: the internal form of k is the integer 1, so the entries (nl/c) k and (1/c) k are
// stored as the PLAIN residues of nl/c and 1/c, and the constant term times g is g's own limbs in the low columns of a dot
// product (tower.hpp f2acc_init_rinv): no multiplication and no reduction of its own.  That is one Fp2 product fewer per line
// in the six-lane kernel (pairing_dist.hpp d_mul_line).  c = 0 is a line through the
// twist's origin; it cannot be excluded for a caller's key, so a table that meets one keeps the form above (unit = 0).
// Every table a job reads has the same form (runtime.hpp Ctx::rebuild_lines), the kernels take it as a template parameter.
#pragma once
#include "g1.hpp"

namespace bbs {

#define FP typename C::FpP

constexpr int MAX_MILLER_OPS = 256;    // schedule bytes: 0 = square f, 1 = multiply by next line
constexpr int MAX_LINES = 128;

// unit = 0: (c, nl) in the internal (Montgomery) form.  unit = 1: c holds 1/c and nl holds nl/c as plain residues in [0, p) --
// read as internal forms they are (1/c) R^-1 and (nl/c) R^-1; the constant term R^-1 is not stored.
template <class C>
struct LineEntry {
    Fp2<C> c, nl;
};

template <class C>
struct LineTable {
    LineEntry<C> e[MAX_LINES];
    int n_lines;
    int q_is_identity;     // pair contributes 1
    int unit;              // form of every entry (0 for a table without lines)
};

struct MillerSchedule {
    uint8_t op[MAX_MILLER_OPS];
    int n_ops;
};

template <class C>
BBS_HD Fp12<C> f12_mul_line(const Fp12<C>& f, const LineEntry<C>& le, const G1Aff<C>& P, bool unit) {
    Fp2<C> lx = f2_mul_fp<C>(le.nl, P.x);
    if (unit) {
        const Fp2<C> ly = f2_mul_fp<C>(le.c, P.y);
        if constexpr (C::K::TWIST_M) return f12_mul_by_line_M_unit<C>(f, lx, ly);
        else return f12_mul_by_line_D_unit<C>(f, lx, ly);
    }
    if constexpr (C::K::TWIST_M) {
        return f12_mul_by_line_M<C>(f, le.c, lx, P.y);
    } else {
        return f12_mul_by_line_D<C>(f, lx, le.c, P.y);
    }
}

// f^|x| by square-and-multiply (f in the cyclotomic subgroup; plain squarings for now)
template <class C>
BBS_HD_NOINLINE Fp12<C> f12_pow_xabs(const Fp12<C>& f) {
    Fp12<C> r = f;
    const uint64_t x = C::K::X_ABS;
    int top = 63;
    while (!((x >> top) & 1)) top--;
    for (int i = top - 1; i >= 0; i--) {
        r = f12_sqr<C>(r);
        if ((x >> i) & 1) r = f12_mul<C>(r, f);
    }
    return r;
}

// f^x for the signed curve parameter, f unitary (inverse == conjugate)
template <class C>
BBS_HD Fp12<C> f12_pow_x(const Fp12<C>& f) {
    Fp12<C> r = f12_pow_xabs<C>(f);
    if constexpr (C::K::X_NEG) r = f12_conj<C>(r);
    return r;
}

// f^((p^12-1)/r * m) with m = 3 (BLS12-381) or 1 (BN254); gcd(m, r) = 1 so "== 1" is unchanged.
template <class C>
BBS_HD_NOINLINE Fp12<C> final_exponentiation(const Fp12<C>& f_in) {
    // easy part: f^((p^6-1)(p^2+1))
    Fp12<C> f = f12_mul<C>(f12_conj<C>(f_in), f12_inv<C>(f_in));
    f = f12_mul<C>(f12_frob<C, 2>(f), f);
    if constexpr (C::ID == 0) {
        // 3*(p^4-p^2+1)/r = (x-1)^2 (x+p) (x^2+p^2-1) + 3
        Fp12<C> a = f12_mul<C>(f12_pow_x<C>(f), f12_conj<C>(f));          // f^(x-1)
        a = f12_mul<C>(f12_pow_x<C>(a), f12_conj<C>(a));                   // f^((x-1)^2)
        Fp12<C> b = f12_mul<C>(f12_pow_x<C>(a), f12_frob<C, 1>(a));        // a^(x+p)
        Fp12<C> c = f12_pow_x<C>(f12_pow_x<C>(b));                         // b^(x^2)
        c = f12_mul<C>(c, f12_frob<C, 2>(b));
        c = f12_mul<C>(c, f12_conj<C>(b));                                 // b^(x^2+p^2-1)
        Fp12<C> f3 = f12_mul<C>(f12_sqr<C>(f), f);
        return f12_mul<C>(c, f3);
    } else {
        // Devegili-Scott-Dahab: (p^4-p^2+1)/r = l0 + l1 p + l2 p^2 + p^3 via
        // y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36
        Fp12<C> fu = f12_pow_x<C>(f);
        Fp12<C> fu2 = f12_pow_x<C>(fu);
        Fp12<C> fu3 = f12_pow_x<C>(fu2);
        Fp12<C> y0 = f12_mul<C>(f12_mul<C>(f12_frob<C, 1>(f), f12_frob<C, 2>(f)), f12_frob<C, 3>(f));
        Fp12<C> y1 = f12_conj<C>(f);
        Fp12<C> y2 = f12_frob<C, 2>(fu2);
        Fp12<C> y3 = f12_conj<C>(f12_frob<C, 1>(fu));
        Fp12<C> y4 = f12_conj<C>(f12_mul<C>(fu, f12_frob<C, 1>(fu2)));
        Fp12<C> y5 = f12_conj<C>(fu2);
        Fp12<C> y6 = f12_conj<C>(f12_mul<C>(fu3, f12_frob<C, 1>(fu3)));
        Fp12<C> t0 = f12_sqr<C>(y6);
        t0 = f12_mul<C>(t0, y4);
        t0 = f12_mul<C>(t0, y5);
        Fp12<C> t1 = f12_mul<C>(y3, y5);
        t1 = f12_mul<C>(t1, t0);
        t0 = f12_mul<C>(t0, y2);
        t1 = f12_sqr<C>(t1);
        t1 = f12_mul<C>(t1, t0);
        t1 = f12_sqr<C>(t1);
        t0 = f12_mul<C>(t1, y1);
        t1 = f12_mul<C>(t1, y0);
        t0 = f12_sqr<C>(t0);
        return f12_mul<C>(t0, t1);
    }
}

// Miller loop over two pairs sharing the squarings.  skipA / skipB: the pair contributes 1.
template <class C>
BBS_HD_NOINLINE Fp12<C> miller_loop2(const MillerSchedule* sched, const LineTable<C>* ta, const G1Aff<C>& Pa,
                                     bool skipA, const LineTable<C>* tb, const G1Aff<C>& Pb, bool skipB) {
    Fp12<C> f = f12_one<C>();
    int li = 0;
    const int n = sched->n_ops;
    for (int k = 0; k < n; k++) {
        if (sched->op[k] == 0) {
            f = f12_sqr<C>(f);
        } else {
            if (!skipA) f = f12_mul_line<C>(f, ta->e[li], Pa, ta->unit != 0);
            if (!skipB) f = f12_mul_line<C>(f, tb->e[li], Pb, tb->unit != 0);
            li++;
        }
    }
    if constexpr (C::K::X_NEG) f = f12_conj<C>(f);
    return f;
}

template <class C>
BBS_HD bool pairing_product2_is_one(const MillerSchedule* sched, const LineTable<C>* ta, const G1Aff<C>& Pa,
                                    const LineTable<C>* tb, const G1Aff<C>& Pb) {
    const bool skipA = g1a_is_inf<C>(Pa) | (ta->q_is_identity != 0);
    const bool skipB = g1a_is_inf<C>(Pb) | (tb->q_is_identity != 0);
    if (skipA & skipB) return true;
    Fp12<C> f = miller_loop2<C>(sched, ta, Pa, skipA, tb, Pb, skipB);
    return f12_is_one<C>(final_exponentiation<C>(f));
}

#undef FP
}  // namespace bbs
