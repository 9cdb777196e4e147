// Key registration on the device (not yet used by bbs_ctx_add_public_keys* / bbs_ctx_set_public_keys, which prepare keys on host
// threads until the stage has been timed against them: runtime.hpp KEY_BUILD_ON_DEVICE; bbs_selftest_key_entries runs it): ONE stage prepares a
// key of the context's key set (keyed.hpp) -- decode (affine record or compressed octets), on-twist test, subgroup test
// [r]Q = infinity, the Miller-loop line table of W = Q and the domain midstate -- one lane per key, and writes the KeyEntry in
// place into the set's device array.  Every DECISION is the host code's (host_g2.hpp g2_on_curve / g2_in_subgroup /
// build_line_table, host_codec.hpp g2_decompress), the arithmetic is not:
//   * the subgroup test walks [r]Q in Jacobian coordinates with the exact group law (T = infinity, T = Q and T = -Q are handled),
//     so its result is the point g2_mul computes in affine coordinates and the decision is g2_in_subgroup's;
//   * the line walk is Jacobian too: a step keeps the numerators of its entry (c, nl) and its one denominator, all
//     denominators of a key are inverted with ONE f2_inv (Montgomery's trick) and a second pass finishes the entries.  The
//     host walk takes an Fp2 inversion per step.  The entries are equal as field elements; the stage stores the representative
//     in [0, p) of every coordinate (the 28-bit limb form is not unique: a value may be stored as v or v + p).
//   * the unit form (pairing.hpp; a.want_unit; entries times R^-1) needs 1/c = d / cn of every step: the product that is inverted runs over d cn
//     (a zero cn counts as 1), and 1/d or 1/cn comes out of 1/(d cn) by one more product.  A key that meets cn = 0 keeps
//     the (c, nl) form -- by selects, its lane stays with the wavefront -- and reports unit = 0, as build_line_table does.
// Refusals of the line walk.  build_line_table refuses when T is the identity or the line is vertical; for a key that passed
// the subgroup test (order exactly r) neither can happen: T = [k]Q with 1 < k < r at every addition, so T != +-Q, T is never
// the identity or of order two, and on BN254 the Frobenius steps meet [6x+2]Q = +-[p]Q or [6x+2+p]Q = +-[p^2]Q for no key
// (6x + 2 + p - p^2 + p^3 = 0 mod r).  The stage refuses a key whose walk meets a zero denominator; that is reachable only
// for a key the subgroup test has refused already.
// Convergence.  A refused or identity key does not leave the wavefront (a noinline helper reached by part of a
// wavefront): it walks the generator instead and its result is dropped by a select at the end.  The branches that remain are
// on the bits of r and of the Miller loop count, the same for every lane.
// The per-step values live in a workspace in global memory laid out [word][key] (a wavefront's accesses coalesce), never in
// the kernel's frame; op_key.hpp key_build sizes it per call by the steps of the walk.
// KeyDomainBuild, behind KeyBuild, is the same stage without the line table, for the jobs that read a key's midstate alone.
#pragma once
#include "keyed.hpp"

namespace bbs {

constexpr int KEY_MAX_BITS = 72;             // Miller loop bits after the leading one: 63 (BLS12-381), 64 (BN254)

template <class C>
struct KeyBuildArgs {
    size_t n;
    const uint32_t* rec;         // record form: [n][4 NC] words of the affine records (little-endian), or null
    const int8_t* is_inf;        // record form: identity flags, or null = none
    const uint32_t* oct;         // octet form: [n][2 NC] words holding the n compressed strings; null = record form
    KeyEntry<C>* out;            // [n] entries, ZEROED by the caller, at their place in the key set
    int8_t* status;              // [n] 1 accepted / BBS_ST_NOT_ON_CURVE / BBS_ST_NONCANONICAL (octet form only)
    uint32_t* rec_out;           // octet form: [n][4 NC] decoded records (zero for a refused key or the identity)
    int8_t* inf_out;             // octet form: [n] 1 = the identity encoding
    uint32_t* ws;                // workspace, key_build_ws_words<C>(steps of the walk) * n words, [word][key]
    const uint8_t* suffix;       // what the domain prefix holds behind the key: I2OSP(L, 8) || compress(Q1, H_i..) || api_id
    uint32_t suffix_len;
    const HashCtx* hash0;        // dst_h2s of the context, dom_* zero
    Fp2<C> b2, gen_x, gen_y, frob_x, frob_y;     // twist constant, the generator (stand-in point), Frobenius constants (BN254)
    int want_unit;               // the context's line form: entries (1/c, nl/c) where every c of the key is invertible
    int n_bits;
    uint8_t bits[KEY_MAX_BITS];  // Miller loop count, most significant bit first, the leading one dropped (miller_bits)
};

// workspace words per key: the denominator d, the factor d cn of the inverted product and the running product of every step
// of the line walk (n_steps = Miller loop bits + the ones among them + the two Frobenius steps of BN254: 68 steps, 22848
// bytes on BLS12-381)
template <class C>
constexpr size_t key_build_ws_words(size_t n_steps) { return n_steps * 3 * 2 * C::FpP::N; }

// The point and root helpers are inlined into the kernel (their operands stay in registers) and are ordinary functions in a host
// compilation, where one copy of each keeps the translation unit small.
#if defined(__HIP_DEVICE_COMPILE__)
#define BBS_KB_HD BBS_HD
#else
#define BBS_KB_HD __host__ __device__ inline __attribute__((noinline))
#endif

template <class C>
struct G2Jac { Fp2<C> x, y, z; };      // z = 0: the identity

template <class C> BBS_HD Fp2<C> f2_select(bool c, const Fp2<C>& a, const Fp2<C>& b) {
    return {fe_select<typename C::FpP>(c, a.c0, b.c0), fe_select<typename C::FpP>(c, a.c1, b.c1)};
}
template <class C> BBS_HD Fp2<C> f2_canon(const Fp2<C>& a) {
    if constexpr (C::FpP::W == 28) return {r28::canon<typename C::FpP>(a.c0), r28::canon<typename C::FpP>(a.c1)};
    else return a;
}
template <class C> BBS_HD void kb_ws_store(const KeyBuildArgs<C>& a, size_t t, int slot, const Fp2<C>& v) {
    constexpr int N = C::FpP::N;
    uint32_t* p = a.ws + (size_t)slot * 2 * N * a.n + t;
    for (int j = 0; j < N; j++) { p[(size_t)j * a.n] = v.c0.v[j]; p[(size_t)(N + j) * a.n] = v.c1.v[j]; }
}
template <class C> BBS_HD Fp2<C> kb_ws_load(const KeyBuildArgs<C>& a, size_t t, int slot) {
    constexpr int N = C::FpP::N;
    const uint32_t* p = a.ws + (size_t)slot * 2 * N * a.n + t;
    Fp2<C> v;
    for (int j = 0; j < N; j++) { v.c0.v[j] = p[(size_t)j * a.n]; v.c1.v[j] = p[(size_t)(N + j) * a.n]; }
    return v;
}

// 2T (a = 0), any T: the identity and points of order two give z = 0
template <class C>
BBS_KB_HD G2Jac<C> g2j_dbl(const G2Jac<C>& T) {
    const Fp2<C> A = f2_sqr<C>(T.x), B = f2_sqr<C>(T.y), Cc = f2_sqr<C>(B);
    const Fp2<C> D = f2_dbl<C>(f2_dbl<C>(f2_mul<C>(T.x, B)));
    const Fp2<C> E = f2_add<C>(f2_dbl<C>(A), A);
    G2Jac<C> r;
    r.x = f2_sub<C>(f2_sqr<C>(E), f2_dbl<C>(D));
    r.y = f2_sub<C>(f2_mul<C>(E, f2_sub<C>(D, r.x)), f2_dbl<C>(f2_dbl<C>(f2_dbl<C>(Cc))));
    r.z = f2_dbl<C>(f2_mul<C>(T.y, T.z));
    return r;
}
// T + Q, Q = (qx, qy) affine and not the identity, Q2 = 2Q: exact for every T (the identity, Q, -Q)
template <class C>
BBS_KB_HD G2Jac<C> g2j_add_affine(const G2Jac<C>& T, const Fp2<C>& qx, const Fp2<C>& qy, const G2Jac<C>& Q2) {
    const bool t_inf = f2_is_zero<C>(T.z);
    const Fp2<C> ZZ = f2_sqr<C>(T.z);
    const Fp2<C> H = f2_sub<C>(f2_mul<C>(qx, ZZ), T.x);
    const Fp2<C> R = f2_sub<C>(f2_mul<C>(qy, f2_mul<C>(T.z, ZZ)), T.y);
    const Fp2<C> HH = f2_sqr<C>(H), HHH = f2_mul<C>(H, HH), V = f2_mul<C>(T.x, HH);
    G2Jac<C> r;
    r.x = f2_sub<C>(f2_sub<C>(f2_sqr<C>(R), HHH), f2_dbl<C>(V));
    r.y = f2_sub<C>(f2_mul<C>(R, f2_sub<C>(V, r.x)), f2_mul<C>(T.y, HHH));
    r.z = f2_mul<C>(T.z, H);                                          // T = -Q: H = 0, the identity
    const bool same = (!t_inf) & f2_is_zero<C>(H) & f2_is_zero<C>(R);      // T = Q
    const Fp2<C> one = f2_one<C>();
    r.x = f2_select<C>(t_inf, qx, f2_select<C>(same, Q2.x, r.x));
    r.y = f2_select<C>(t_inf, qy, f2_select<C>(same, Q2.y, r.y));
    r.z = f2_select<C>(t_inf, one, f2_select<C>(same, Q2.z, r.z));
    return r;
}

// a^((p + 1) / 4) and whether it is a root (host_codec.hpp fe_sqrt)
template <class P>
BBS_KB_HD bool kb_fe_sqrt(const Fe<P>& a, Fe<P>& out) {
    uint32_t e[P::NC];
    uint64_t c = 1;
    for (int i = 0; i < P::NC; i++) { c += P::MODC[i]; e[i] = (uint32_t)c; c >>= 32; }
    for (int i = 0; i < P::NC; i++) e[i] = (e[i] >> 2) | ((i + 1 < P::NC ? e[i + 1] : (uint32_t)c) << 30);
    Fe<P> r = fe_one<P>();
    for (int i = P::NC - 1; i >= 0; i--)
        for (int b = 31; b >= 0; b--) {
            r = fe_sqr<P>(r);
            if ((e[i] >> b) & 1) r = fe_mul<P>(r, a);                  // (the exponent is the same for every lane)
        }
    out = r;
    return fe_eq<P>(fe_sqr<P>(r), a);
}
// host_codec.hpp f2_sqrt without a branch on the value: the three candidates in its order, the first that is a root wins
template <class C>
BBS_KB_HD bool kb_f2_sqrt(const Fp2<C>& a, Fp2<C>& out) {
    using P = typename C::FpP;
    Fe<P> s;
    const bool norm_ok = kb_fe_sqrt<P>(fe_add<P>(fe_sqr<P>(a.c0), fe_sqr<P>(a.c1)), s);
    uint32_t two[P::NC] = {2};
    const Fe<P> inv2 = fe_inv<P>(fe_from_words<P>(two));
    bool found = false;
    out = f2_zero<C>();
    for (int k = 0; k < 2; k++) {
        const Fe<P> sg = k ? fe_neg<P>(s) : s;
        const Fe<P> t = fe_mul<P>(fe_add<P>(a.c0, sg), inv2);
        Fe<P> x0;
        const bool r0 = kb_fe_sqrt<P>(t, x0);
        const Fp2<C> cand = {x0, fe_mul<P>(a.c1, fe_inv<P>(fe_dbl<P>(x0)))};
        const bool ok = norm_ok & r0 & !fe_is_zero<P>(x0) & f2_eq<C>(f2_sqr<C>(cand), a);
        out = f2_select<C>(ok & !found, cand, out);
        found |= ok;
    }
    Fe<P> x1;
    const bool r1 = kb_fe_sqrt<P>(fe_neg<P>(a.c0), x1);
    const bool imag = norm_ok & fe_is_zero<P>(a.c1) & r1;
    const Fp2<C> ci = {fe_zero<P>(), x1};
    out = f2_select<C>(imag & !found, ci, out);
    found |= imag;
    const bool zero = f2_is_zero<C>(a);
    out = f2_select<C>(zero, f2_zero<C>(), out);
    return found | zero;
}

template <class P>
BBS_HD bool kb_fe_gt_half(const Fe<P>& a) {
    uint32_t c[P::NC];
    fe_to_words<P>(a, c);
    return words_gt_half<P>(c);
}
BBS_HD uint32_t kb_bswap(uint32_t l) { return (l << 24) | ((l & 0xff00u) << 8) | ((l >> 8) & 0xff00u) | (l >> 24); }

// one step of the line walk: the entry's numerators go to the key's entry, its denominator, the factor d cn and the running
// product of the factors to the workspace; T moves on.  dbl: the tangent at T; otherwise the line through T and (qx, qy).
template <class C>
BBS_KB_HD void kb_line_step(const KeyBuildArgs<C>& a, size_t t, int s, bool dbl, G2Jac<C>& T, const Fp2<C>& qx, const Fp2<C>& qy,
                         Fp2<C>& prod, bool& degenerate, bool& c_zero) {
    const Fp2<C> ZZ = f2_sqr<C>(T.z);
    Fp2<C> cn, nn, d;
    G2Jac<C> r;
    if (dbl) {
        // lambda = 3 X^2 / (2 Y Z);  c = lambda x - y = (3 X^3 - 2 Y^2) / (2 Y Z^3);  nl = -3 X^2 Z^2 / (2 Y Z^3)
        const Fp2<C> A = f2_sqr<C>(T.x), B = f2_sqr<C>(T.y), Cc = f2_sqr<C>(B);
        const Fp2<C> E = f2_add<C>(f2_dbl<C>(A), A);
        const Fp2<C> D = f2_dbl<C>(f2_dbl<C>(f2_mul<C>(T.x, B)));
        cn = f2_sub<C>(f2_mul<C>(E, T.x), f2_dbl<C>(B));
        nn = f2_neg<C>(f2_mul<C>(E, ZZ));
        r.z = f2_dbl<C>(f2_mul<C>(T.y, T.z));
        d = f2_mul<C>(r.z, ZZ);
        r.x = f2_sub<C>(f2_sqr<C>(E), f2_dbl<C>(D));
        r.y = f2_sub<C>(f2_mul<C>(E, f2_sub<C>(D, r.x)), f2_dbl<C>(f2_dbl<C>(f2_dbl<C>(Cc))));
    } else {
        // lambda = R / (Z H), H = qx Z^2 - X, R = qy Z^3 - Y;  c = lambda qx - qy (the line passes through Q as well)
        const Fp2<C> H = f2_sub<C>(f2_mul<C>(qx, ZZ), T.x);
        const Fp2<C> R = f2_sub<C>(f2_mul<C>(qy, f2_mul<C>(T.z, ZZ)), T.y);
        const Fp2<C> HH = f2_sqr<C>(H), HHH = f2_mul<C>(H, HH), V = f2_mul<C>(T.x, HH);
        r.z = f2_mul<C>(T.z, H);
        d = r.z;
        cn = f2_sub<C>(f2_mul<C>(R, qx), f2_mul<C>(qy, r.z));
        nn = f2_neg<C>(R);
        r.x = f2_sub<C>(f2_sub<C>(f2_sqr<C>(R), HHH), f2_dbl<C>(V));
        r.y = f2_sub<C>(f2_mul<C>(R, f2_sub<C>(V, r.x)), f2_mul<C>(T.y, HHH));
    }
    const bool dz = f2_is_zero<C>(d);
    degenerate |= dz;
    d = f2_select<C>(dz, f2_one<C>(), d);                              // (keeps the product invertible; the key is refused)
    const bool cz = f2_is_zero<C>(cn);                                 // a line through the twist's origin: no unit form
    c_zero |= cz;
    const Fp2<C> dc = f2_mul<C>(d, f2_select<C>(cz, f2_one<C>(), cn));
    a.out[t].tab.e[s].c = cn;
    a.out[t].tab.e[s].nl = nn;
    kb_ws_store<C>(a, t, 3 * s, d);
    kb_ws_store<C>(a, t, 3 * s + 1, dc);
    kb_ws_store<C>(a, t, 3 * s + 2, prod);                            // the product of the factors BEFORE this step
    prod = f2_mul<C>(prod, dc);
    T = r;
}

template <class C>
struct KeyBuild {
    static __host__ __device__ __forceinline__ void run(const KeyBuildArgs<C>& a, size_t t) {      // (inlined: no copy of the arguments, no frame of its own)
        using P = typename C::FpP;
        constexpr int NC = P::NC;
        // ---- 1. decode
        Fp2<C> qx = f2_zero<C>(), qy = f2_zero<C>();
        bool inf = false, noncanon = false, refused = false;
        if (a.oct) {                                                   // (the same form for every key of a call)
            uint32_t w0[NC], w1[NC];                                   // x.c0, x.c1 as canonical little-endian words
            const uint32_t* o = a.oct + t * 2 * NC;
            bool ybig;
            if constexpr (C::ID == 0) {                                // big-endian x.c1 || x.c0, flags in the first byte
                for (int i = 0; i < NC; i++) { w1[i] = kb_bswap(o[NC - 1 - i]); w0[i] = kb_bswap(o[2 * NC - 1 - i]); }
                const uint32_t fl = w1[NC - 1] >> 24;
                noncanon |= !(fl & 0x80);
                inf = (fl & 0x40) != 0; ybig = (fl & 0x20) != 0;
                w1[NC - 1] &= 0x1FFFFFFFu;
            } else {                                                   // little-endian x.c0 || x.c1, flags in the last byte
                for (int i = 0; i < NC; i++) { w0[i] = o[i]; w1[i] = o[NC + i]; }
                const uint32_t fl = w1[NC - 1] >> 24;
                inf = (fl & 0x40) != 0; ybig = (fl & 0x80) != 0;
                w1[NC - 1] &= 0x3FFFFFFFu;
            }
            uint32_t any = 0;
            for (int i = 0; i < NC; i++) any |= w0[i] | w1[i];
            noncanon |= inf ? ((any != 0) | ybig) : (!limbs_lt_mod<P>(w0) | !limbs_lt_mod<P>(w1));
            if (inf | noncanon) for (int i = 0; i < NC; i++) { w0[i] = 0; w1[i] = 0; }
            qx = {fe_from_words<P>(w0), fe_from_words<P>(w1)};
            const Fp2<C> rhs = f2_add<C>(f2_mul<C>(f2_sqr<C>(qx), qx), a.b2);
            Fp2<C> y;
            const bool root = kb_f2_sqrt<C>(rhs, y);
            const bool big = fe_is_zero<P>(y.c1) ? kb_fe_gt_half<P>(y.c0) : kb_fe_gt_half<P>(y.c1);
            qy = f2_select<C>(big != ybig, f2_neg<C>(y), y);
            refused = noncanon | (!inf & !root);
        } else {
            const uint32_t* r = a.rec + t * 4 * NC;
            inf = a.is_inf && a.is_inf[t] != 0;
            uint32_t w[4][NC];
            bool lt = true;
            for (int k = 0; k < 4; k++) {
                for (int i = 0; i < NC; i++) w[k][i] = inf ? 0u : r[k * NC + i];
                lt &= limbs_lt_mod<P>(w[k]);
            }
            refused = !lt;
            if (refused) for (int k = 0; k < 4; k++) for (int i = 0; i < NC; i++) w[k][i] = 0;
            qx = {fe_from_words<P>(w[0]), fe_from_words<P>(w[1])};
            qy = {fe_from_words<P>(w[2]), fe_from_words<P>(w[3])};
        }
        // ---- 2. on the twist?  (a refused or identity key goes on with the generator: its lane stays with the wavefront)
        refused |= !inf & !f2_eq<C>(f2_sqr<C>(qy), f2_add<C>(f2_mul<C>(f2_sqr<C>(qx), qx), a.b2));
        const bool stand_in = inf | refused;
        const Fp2<C> wx = f2_select<C>(stand_in, a.gen_x, qx), wy = f2_select<C>(stand_in, a.gen_y, qy);
        // ---- 3. [r]Q = identity?  (g2_mul's loop: 256 bits of r, most significant first)
        {
            const G2Jac<C> Q1 = {wx, wy, f2_one<C>()};
            const G2Jac<C> Q2 = g2j_dbl<C>(Q1);
            G2Jac<C> T = {f2_zero<C>(), f2_zero<C>(), f2_zero<C>()};
#pragma unroll 1
            for (int i = 255; i >= 0; i--) {
                T = g2j_dbl<C>(T);
                if ((C::FrP::MOD[i >> 5] >> (i & 31)) & 1) T = g2j_add_affine<C>(T, wx, wy, Q2);
            }
            refused |= !f2_is_zero<C>(T.z);
        }
        // ---- 4. line table: the walk ...
        int ns = 0;
        bool degenerate = false, c_zero = false;
        Fp2<C> prod = f2_one<C>();
        {
            G2Jac<C> T = {wx, wy, f2_one<C>()};
#pragma unroll 1
            for (int k = 0; k < a.n_bits; k++) {
                kb_line_step<C>(a, t, ns++, true, T, wx, wy, prod, degenerate, c_zero);
                if (a.bits[k]) kb_line_step<C>(a, t, ns++, false, T, wx, wy, prod, degenerate, c_zero);
            }
            if constexpr (C::ID == 1) {                                // Q1 = frob(Q), Q2 = -frob(frob(Q))  (g2_frob_D)
                const Fp2<C> x1 = f2_mul<C>(f2_conj<C>(wx), a.frob_x), y1 = f2_mul<C>(f2_conj<C>(wy), a.frob_y);
                const Fp2<C> x2 = f2_mul<C>(f2_conj<C>(x1), a.frob_x), y2 = f2_neg<C>(f2_mul<C>(f2_conj<C>(y1), a.frob_y));
                kb_line_step<C>(a, t, ns++, false, T, x1, y1, prod, degenerate, c_zero);
                kb_line_step<C>(a, t, ns++, false, T, x2, y2, prod, degenerate, c_zero);
            }
        }
        refused |= degenerate;
        // ... one inversion, and the entries from the last to the first
        const bool table = !stand_in & !refused;
        const bool unit = (a.want_unit != 0) & !c_zero;
        {
            Fp2<C> inv = f2_inv<C>(prod);
#pragma unroll 1
            for (int s = ns - 1; s >= 0; s--) {
                const Fp2<C> d = kb_ws_load<C>(a, t, 3 * s), dc = kb_ws_load<C>(a, t, 3 * s + 1), before = kb_ws_load<C>(a, t, 3 * s + 2);
                const Fp2<C> dci = f2_mul<C>(inv, before);             // 1 / (d cn)
                inv = f2_mul<C>(inv, dc);
                LineEntry<C>& e = a.out[t].tab.e[s];
                // (c, nl) = (cn, nn) / d: times cn / (d cn);  (1/c, nl/c) = (d, nn) / cn: times d / (d cn)
                const Fp2<C> cn1 = f2_select<C>(f2_is_zero<C>(e.c), f2_one<C>(), e.c);
                // (the unit form stores plain residues: times R^-1, whose internal form is the integer 1)
                const Fp2<C> di = f2_mul_fp<C>(f2_mul<C>(f2_select<C>(unit, d, cn1), dci), fe_select<typename C::FpP>(unit, f2_rinv<C>().c0, fe_one<typename C::FpP>()));
                const Fp2<C> c = f2_canon<C>(f2_mul<C>(f2_select<C>(unit, d, e.c), di)), nl = f2_canon<C>(f2_mul<C>(e.nl, di));
                e.c = f2_select<C>(table, c, f2_zero<C>());
                e.nl = f2_select<C>(table, nl, f2_zero<C>());
            }
        }
        KeyEntry<C>& o = a.out[t];
        o.tab.n_lines = table ? ns : 0;
        o.tab.q_is_identity = table ? 0 : 1;
        o.tab.unit = (table & unit) ? 1 : 0;
        // ---- 5. domain midstate: Z_pad || compress(pk) || suffix  (g2_compress; the identity has its own encoding)
        uint32_t xw0[NC], xw1[NC];
        fe_to_words<P>(qx.c0, xw0);
        fe_to_words<P>(qx.c1, xw1);
        const bool largest = fe_is_zero<P>(qy.c1) ? kb_fe_gt_half<P>(qy.c0) : kb_fe_gt_half<P>(qy.c1);
        Sha256 s;
        xmd48_begin(s);
        if constexpr (C::ID == 0) {
            const uint32_t fl = inf ? 0xC0000000u : (0x80000000u | (largest ? 0x20000000u : 0u));
            for (int i = NC - 1; i >= 0; i--) sha256_word(s, (inf ? 0u : xw1[i]) | (i == NC - 1 ? fl : 0u));
            for (int i = NC - 1; i >= 0; i--) sha256_word(s, inf ? 0u : xw0[i]);
        } else {
            const uint32_t fl = inf ? 0x40000000u : (largest ? 0x80000000u : 0u);
            for (int i = 0; i < NC; i++) sha256_word(s, kb_bswap(inf ? 0u : xw0[i]));
            for (int i = 0; i < NC; i++) sha256_word(s, kb_bswap((inf ? 0u : xw1[i]) | (i == NC - 1 ? fl : 0u)));
        }
        sha256_bytes(s, a.suffix, a.suffix_len);
        o.hash = *a.hash0;
        if (!refused) {
            for (int k = 0; k < 8; k++) o.hash.dom_mid[k] = s.h[k];
            o.hash.dom_mid_total = s.total - s.fill;
            o.hash.dom_tail_len = s.fill;
            // (the block buffer is zero behind its `fill` bytes, as the entry is: all 64 bytes, no indexed read of s.w)
            for (int k = 0; k < 64; k++) o.hash.dom_tail[k] = (uint8_t)(s.w[k >> 2] >> ((3 - (k & 3)) * 8));
        }
        a.status[t] = (int8_t)(noncanon ? BBS_ST_NONCANONICAL : refused ? BBS_ST_NOT_ON_CURVE : 1);
        if (a.oct) {
            uint32_t yw0[NC], yw1[NC];
            fe_to_words<P>(qy.c0, yw0);
            fe_to_words<P>(qy.c1, yw1);
            const bool put = !inf & !refused;
            if (a.rec_out) {
                uint32_t* ro = a.rec_out + t * 4 * NC;
                for (int i = 0; i < NC; i++) {
                    ro[i] = put ? xw0[i] : 0u; ro[NC + i] = put ? xw1[i] : 0u;
                    ro[2 * NC + i] = put ? yw0[i] : 0u; ro[3 * NC + i] = put ? yw1[i] : 0u;
                }
            }
            if (a.inf_out) a.inf_out[t] = (int8_t)((inf & !refused) ? 1 : 0);
        }
    }
};

// ---- the domain-only key stage (bbs_*proof_gen*_with_keys_*; job_form.hpp JobKeys::domain_only) ------------------------------
// proof_gen meets the key in calculate_domain alone: of a KeyEntry it reads `hash`.  This stage prepares a key for such a job:
// steps 1, 2, 3 and 5 of KeyBuild::run in its octet form -- decode, on-twist test, [r]Q = identity, domain midstate -- and
// nothing of step 4: no line walk, no workspace, no Miller loop count, no line form, no f2_inv.  `hash` and the status are, bit
// for bit, what KeyBuild writes for the same string (the two bodies are kept side by side; KeyBuild's is left as it was so that
// its code does not move); `tab` is that of a key without a table -- n_lines = 0, q_is_identity = 1, unit = 0, entries zero
// as the caller cleared them -- so PgScalars reads the entry unchanged and no pairing kernel must ever be given it.
// Convergence as KeyBuild's: a refused or identity key walks the generator, its result is dropped by a select; the branches
// that remain are on the bits of r.
template <class C>
struct KeyDomainBuildArgs {
    size_t n;
    const uint32_t* oct;         // [n][2 NC] words holding the n compressed strings
    KeyEntry<C>* out;            // [n] entries, ZEROED by the caller
    int8_t* status;              // [n] 1 accepted / BBS_ST_NOT_ON_CURVE / BBS_ST_NONCANONICAL
    const uint8_t* suffix;       // as KeyBuildArgs
    uint32_t suffix_len;
    const HashCtx* hash0;
    Fp2<C> b2, gen_x, gen_y;     // twist constant, the generator (stand-in point)
};
template <class C>
struct KeyDomainBuild {
    static __host__ __device__ __forceinline__ void run(const KeyDomainBuildArgs<C>& a, size_t t) {
        using P = typename C::FpP;
        constexpr int NC = P::NC;
        // ---- 1. decode (KeyBuild's octet form)
        uint32_t w0[NC], w1[NC];                                       // x.c0, x.c1 as canonical little-endian words
        const uint32_t* oc = a.oct + t * 2 * NC;
        bool inf, ybig, noncanon = false;
        if constexpr (C::ID == 0) {                                    // big-endian x.c1 || x.c0, flags in the first byte
            for (int i = 0; i < NC; i++) { w1[i] = kb_bswap(oc[NC - 1 - i]); w0[i] = kb_bswap(oc[2 * NC - 1 - i]); }
            const uint32_t fl = w1[NC - 1] >> 24;
            noncanon |= !(fl & 0x80);
            inf = (fl & 0x40) != 0; ybig = (fl & 0x20) != 0;
            w1[NC - 1] &= 0x1FFFFFFFu;
        } else {                                                       // little-endian x.c0 || x.c1, flags in the last byte
            for (int i = 0; i < NC; i++) { w0[i] = oc[i]; w1[i] = oc[NC + i]; }
            const uint32_t fl = w1[NC - 1] >> 24;
            inf = (fl & 0x40) != 0; ybig = (fl & 0x80) != 0;
            w1[NC - 1] &= 0x3FFFFFFFu;
        }
        uint32_t any = 0;
        for (int i = 0; i < NC; i++) any |= w0[i] | w1[i];
        noncanon |= inf ? ((any != 0) | ybig) : (!limbs_lt_mod<P>(w0) | !limbs_lt_mod<P>(w1));
        if (inf | noncanon) for (int i = 0; i < NC; i++) { w0[i] = 0; w1[i] = 0; }
        const Fp2<C> qx = {fe_from_words<P>(w0), fe_from_words<P>(w1)};
        const Fp2<C> rhs = f2_add<C>(f2_mul<C>(f2_sqr<C>(qx), qx), a.b2);
        Fp2<C> y;
        const bool root = kb_f2_sqrt<C>(rhs, y);
        const bool big = fe_is_zero<P>(y.c1) ? kb_fe_gt_half<P>(y.c0) : kb_fe_gt_half<P>(y.c1);
        const Fp2<C> qy = f2_select<C>(big != ybig, f2_neg<C>(y), y);
        bool refused = noncanon | (!inf & !root);
        // ---- 2. on the twist?  (a refused or identity key goes on with the generator: its lane stays with the wavefront)
        refused |= !inf & !f2_eq<C>(f2_sqr<C>(qy), rhs);
        const bool stand_in = inf | refused;
        const Fp2<C> wx = f2_select<C>(stand_in, a.gen_x, qx), wy = f2_select<C>(stand_in, a.gen_y, qy);
        // ---- 3. [r]Q = identity?  (g2_mul's loop: 256 bits of r, most significant first)
        {
            const G2Jac<C> Q1 = {wx, wy, f2_one<C>()};
            const G2Jac<C> Q2 = g2j_dbl<C>(Q1);
            G2Jac<C> T = {f2_zero<C>(), f2_zero<C>(), f2_zero<C>()};
#pragma unroll 1
            for (int i = 255; i >= 0; i--) {
                T = g2j_dbl<C>(T);
                if ((C::FrP::MOD[i >> 5] >> (i & 31)) & 1) T = g2j_add_affine<C>(T, wx, wy, Q2);
            }
            refused |= !f2_is_zero<C>(T.z);
        }
        // ---- 5. domain midstate: Z_pad || compress(pk) || suffix.  For a key that is not refused compress(pk) is the input
        // string itself (decoding is canonical): the words of x as decoded, the sign flag recomputed from the y that was chosen
        const bool largest = fe_is_zero<P>(qy.c1) ? kb_fe_gt_half<P>(qy.c0) : kb_fe_gt_half<P>(qy.c1);
        Sha256 s;
        xmd48_begin(s);
        if constexpr (C::ID == 0) {
            const uint32_t fl = inf ? 0xC0000000u : (0x80000000u | (largest ? 0x20000000u : 0u));
            for (int i = NC - 1; i >= 0; i--) sha256_word(s, (inf ? 0u : w1[i]) | (i == NC - 1 ? fl : 0u));
            for (int i = NC - 1; i >= 0; i--) sha256_word(s, inf ? 0u : w0[i]);
        } else {
            const uint32_t fl = inf ? 0x40000000u : (largest ? 0x80000000u : 0u);
            for (int i = 0; i < NC; i++) sha256_word(s, kb_bswap(inf ? 0u : w0[i]));
            for (int i = 0; i < NC; i++) sha256_word(s, kb_bswap((inf ? 0u : w1[i]) | (i == NC - 1 ? fl : 0u)));
        }
        sha256_bytes(s, a.suffix, a.suffix_len);
        KeyEntry<C>& o = a.out[t];
        o.tab.n_lines = 0;
        o.tab.q_is_identity = 1;
        o.tab.unit = 0;
        o.hash = *a.hash0;
        if (!refused) {
            for (int k = 0; k < 8; k++) o.hash.dom_mid[k] = s.h[k];
            o.hash.dom_mid_total = s.total - s.fill;
            o.hash.dom_tail_len = s.fill;
            for (int k = 0; k < 64; k++) o.hash.dom_tail[k] = (uint8_t)(s.w[k >> 2] >> ((3 - (k & 3)) * 8));
        }
        a.status[t] = (int8_t)(noncanon ? BBS_ST_NONCANONICAL : refused ? BBS_ST_NOT_ON_CURVE : 1);
    }
};

#undef BBS_KB_HD

// ---- job-local key sets (bbs_*_with_keys_*; job_form.hpp JobKeys) ------------------------------------------------------------
// The keys of ONE job, prepared by KeyBuild (octet form) on the job's main stream in front of its ingest kernel.  The host
// planned the job without knowing which keys come out accepted: every index < n_keys has its slot in the pairing order and in
// the groups of keyed batch verification.  This gate, behind KeyBuild and the ingest kernel and in front of everything that
// reads an entry, decides the items whose key the job does not have -- an index >= n_keys (KEY_NONE, set by the host), a key
// KeyBuild refused, and an accepted key (not the identity) whose table came out in another form than the job's: unit == 0 in a
// unit-form job, a walk that met c = 0.  No key of order r is known to reach that; the job fails closed there
// (BBS_ST_UNKNOWN_KEY), registration -- which moves the whole context to the (c, nl) form -- serves such a key.
// A decided item keeps its slot; the pairing kernels and the combination leave it out by its status, as every decided item.
template <class C>
struct JobKeyGateArgs {
    size_t n;
    const uint32_t* kidx;        // [n] key of item i, KEY_NONE: index >= n_keys
    const KeyEntry<C>* keys;     // [n_keys] as KeyBuild left them
    const int8_t* key_status;    // [n_keys] KeyBuild's codes
    int unit;                    // line form of the job
    int8_t* status0;
};
template <class C>
struct JobKeyGate {
    static __host__ __device__ void run(const JobKeyGateArgs<C>& a, size_t i) {
        const uint32_t k = a.kidx[i];
        bool ok = k != KEY_NONE;
        if (ok) ok = a.key_status[k] == 1;
        if (ok) {
            const LineTable<C>& t = a.keys[k].tab;
            ok = t.q_is_identity != 0 || (t.unit != 0) == (a.unit != 0);
        }
        if (!ok) a.status0[i] = (int8_t)BBS_ST_UNKNOWN_KEY;
    }
};
// The same gate for a job that reads the `hash` of an entry alone (proof_gen: it never pairs).  No key is refused for the form
// of its table: the entry may have none (KeyDomainBuild), or one in either form (a slot of the job-local key cache).
struct JobKeyStatusGateArgs {
    size_t n;
    const uint32_t* kidx;        // [n] key of item i, KEY_NONE: index >= n_keys
    const int8_t* key_status;    // [n_keys] the key stage's codes
    int8_t* status0;
};
struct JobKeyStatusGate {
    static __host__ __device__ void run(const JobKeyStatusGateArgs& a, size_t i) {
        const uint32_t k = a.kidx[i];
        if (k == KEY_NONE || a.key_status[k] != 1) a.status0[i] = (int8_t)BBS_ST_UNKNOWN_KEY;
    }
};

// The prefixes per (key, length) of a job-local key set under bbs_ctx_set_keyed_mixed_lengths: what Ctx::build_key_lens hashes
// on host threads, one lane per (key, l), 0 <= l < stride = L + 1, into the job's own rows.  For an accepted key compress(pk) is
// the input string itself (decoding is canonical, the identity included), so the lane hashes bytes only:
//     Z_pad || octets || I2OSP(l, 8) || compress(Q1, H_1 .. H_l) || api_id
// and keeps midstate, total, tail and tail length as step 5 of KeyBuild does.  Rows of a refused key stay at hash0.
// Lanes of one wavefront hash different lengths.  The message is read as a function of the word index and the compression
// function is inlined in the one loop over blocks: no out-of-line helper is reached by part of a wavefront.
// Everything in front of api_id is whole words (FPB, 8 and 64 are multiples of 4).
template <class C>
struct KeyLenBuildArgs {
    size_t n_keys;
    uint32_t stride;             // L + 1
    const uint32_t* oct;         // [n_keys][2 NC] words of the compressed strings, as KeyBuild reads them
    const int8_t* key_status;    // [n_keys] KeyBuild's codes
    const uint8_t* cg;           // compress(Q1) || compress(H_1) || .. || compress(H_L), 4-byte aligned
    const uint8_t* api_id;
    uint32_t api_len;
    const HashCtx* hash0;
    HashCtx* out;                // [n_keys][stride]
};
template <class C>
struct KeyLenBuild {
    static __host__ __device__ void run(const KeyLenBuildArgs<C>& a, size_t t) {
        constexpr uint32_t NC = C::FpP::NC;
        const size_t k = t / a.stride;
        const uint32_t l = (uint32_t)(t - k * a.stride);
        HashCtx& o = a.out[t];
        o = *a.hash0;
        if (a.key_status[k] != 1) return;
        const uint32_t* ow = a.oct + k * 2 * NC;
        const uint32_t* gw = reinterpret_cast<const uint32_t*>(a.cg);
        // word j of the message (big-endian), zero behind its end
        const uint32_t w_key = 16, w_len = w_key + 2 * NC, w_gen = w_len + 2, w_api = w_gen + (l + 1) * NC;
        const uint32_t total = 4 * w_api + a.api_len;
        auto word = [&](uint32_t j) -> uint32_t {
            if (j < w_key) return 0u;
            if (j < w_len) return kb_bswap(ow[j - w_key]);
            if (j < w_gen) return j == w_len ? 0u : l;
            if (j < w_api) return kb_bswap(gw[j - w_gen]);
            uint32_t v = 0;
            for (uint32_t b = 0; b < 4; b++) {
                const uint32_t at = 4 * (j - w_api) + b;
                v = (v << 8) | (at < a.api_len ? (uint32_t)a.api_id[at] : 0u);
            }
            return v;
        };
        uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
        const uint32_t n_blocks = total / 64;
#pragma unroll 1
        for (uint32_t b = 0; b < n_blocks; b++) {
            uint32_t w[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) w[i] = word(16 * b + i);
            sha256_compress_body(h, w);
        }
        for (int i = 0; i < 8; i++) o.dom_mid[i] = h[i];
        o.dom_mid_total = (uint64_t)n_blocks * 64;
        o.dom_tail_len = total - n_blocks * 64;
        for (uint32_t i = 0; i < 16; i++) {                              // (words behind the end are zero, as the entry is)
            const uint32_t v = word(16 * n_blocks + i);
            for (uint32_t b = 0; b < 4; b++) o.dom_tail[4 * i + b] = (uint8_t)(v >> ((3 - b) * 8));
        }
    }
};

// ---- the job-local key cache (bbs_ctx_set_job_key_cache; job_form.hpp, key_cache.hpp) ------------------------------------------
// Behind KeyBuild (and KeyLenBuild) of a cached job, which prepared the job's MISSES into arrays of the job: miss t -- its
// entry, its status byte, its `stride` rows -- is copied into slot slot_of[t] of the cache's arrays, all of it (no slot is
// cleared beforehand).  One lane per unit of U bytes, U = 16 where the two structures are whole multiples of 16 bytes (they
// are: the assertion below says so for the curve at hand), else 4.  The lanes [t * per_key, (t + 1) * per_key) belong to key t:
// first the units of the entry, then those of the rows, the last lane the status byte -- consecutive lanes take consecutive
// units of one key, so the loads and stores of a wavefront coalesce.  Neither KeyBuild nor KeyLenBuild knows of the cache.
template <class C>
struct KeyCachePublishArgs {
    size_t n_miss;
    uint32_t stride;             // rows per key (0: the cache holds no rows)
    const uint32_t* slot_of;     // [n_miss], distinct, < capacity (in the job's staging image)
    const KeyEntry<C>* src_entries;
    const int8_t* src_status;
    const HashCtx* src_rows;     // [n_miss][stride]
    KeyEntry<C>* dst_entries;    // the cache's arrays, [capacity]
    int8_t* dst_status;
    HashCtx* dst_rows;           // [capacity][stride]
};
template <class C>
struct KeyCachePublish {
    static constexpr bool WIDE = sizeof(KeyEntry<C>) % 16 == 0 && sizeof(HashCtx) % 16 == 0;
    static constexpr size_t U = WIDE ? 16 : 4;
    static_assert(sizeof(KeyEntry<C>) % U == 0 && sizeof(HashCtx) % U == 0, "KeyCachePublish copies whole units");
    static_assert(alignof(KeyEntry<C>) >= 4 && alignof(HashCtx) >= 4, "KeyCachePublish reads words");
    struct alignas(WIDE ? 16 : 4) Unit { uint32_t w[WIDE ? 4 : 1]; };
    static constexpr size_t E_UNITS = sizeof(KeyEntry<C>) / U, R_UNITS = sizeof(HashCtx) / U;
    static size_t lanes(size_t n_miss, uint32_t stride) { return n_miss * (E_UNITS + (size_t)stride * R_UNITS + 1); }
    static __host__ __device__ void run(const KeyCachePublishArgs<C>& a, size_t i) {
        const size_t row_units = (size_t)a.stride * R_UNITS, per_key = E_UNITS + row_units + 1;
        const size_t t = i / per_key, u = i - t * per_key;
        const size_t s = a.slot_of[t];
        if (u < E_UNITS) {
            reinterpret_cast<Unit*>(a.dst_entries + s)[u] = reinterpret_cast<const Unit*>(a.src_entries + t)[u];
        } else if (u < E_UNITS + row_units) {
            const size_t r = u - E_UNITS;
            reinterpret_cast<Unit*>(a.dst_rows + s * a.stride)[r] = reinterpret_cast<const Unit*>(a.src_rows + t * a.stride)[r];
        } else {
            a.dst_status[s] = a.src_status[t];
        }
    }
};

}  // namespace bbs
