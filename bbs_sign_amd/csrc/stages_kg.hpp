// Batched key generation on the device (bbs_key_gen_batch, bbs_sk_to_pk_batch; op_kg.hpp has the host side): two stages, one
// lane per item each, because their register budgets differ.
//   KgDerive   SecretKey::key_gen (src/key_gen.rs:46-81): sk = hash_to_scalar(key_material || I2OSP(len(key_info), 2) ||
//              key_info, key_dst), with the statuses of bbs_key_gen in its order of checks.
//   KgPublic   sk_to_pk (src/key_gen.rs:83-90): pk = sk * BP2 by a fixed-base comb of the G2 generator, one f2_inv per lane
//              to go affine, then the record and the compressed octets (host_g2.hpp g2_compress).
// The comb.  T[w][d - 1] = [d * 2^(KG_WB w)] BP2 for d = 1 .. 2^KG_WB - 1, affine, Montgomery limbs, built once per (curve,
// device) on the host (op_kg.hpp kg_table).  The scalar is cut into KG_WINDOWS digits of KG_WB bits; window w adds its
// digit's entry to the accumulator: KG_WINDOWS mixed additions and no doubling.  A zero digit adds the window's first entry
// and drops the sum by a select; an identity accumulator is handled by select too.
// The accumulator never meets +- its addend.  Before window w the accumulator is [a] BP2 with a = k mod 2^(KG_WB w), and the
// addend is [b] BP2 with b = d * 2^(KG_WB w), 1 <= d: a < 2^(KG_WB w) <= b, so a != b, and 0 < a + b <= k < r, so a != -b mod
// r (BP2 has order r).  The kernel does not rely on that silently: a lane that meets H = 0 with a live accumulator, or ends
// with z = 0 for a scalar that is not zero, is REFUSED -- zero outputs and a status left at ST_PENDING, for which the call
// returns BBS_E_STATE (fail closed); no wrong key is emitted.
// Convergence (stages_key.hpp).  A refused item does not leave its wavefront: KgDerive hashes what it has
// (a key_info refused for its length is read up to 65535 bytes and no further), KgPublic walks the scalar 1 instead, and a
// select at the end drops the result.  Every output word of every item is written, refused items included.
// Timing.  NOTHING is claimed about timing side channels: the table index is a secret digit and the hash loops run as long as
// the item's input (the reference's arkworks multiplication is not constant-time either).
#pragma once
#include "stages_common.hpp"
#include "stages_key.hpp"

namespace bbs {

// The window is 8 bits: 32 windows x 255 entries, 1.83 MB on BLS12-381 and 1.31 MB on BN254 (inside the 4 MB L2), 32 additions
// per key.  Measured against 4 bits (64 x 15 entries, 215 KB / 154 KB, 64 additions) on the MI355X at 4096 keys: the stage
// takes 1.36 ms instead of 2.44 ms on BLS12-381 and 0.80 ms instead of 1.37 ms on BN254 (DESIGN.md 8 "Key generation");
// the price is the one-off table build on the host, 8160 affine additions instead of 960.  -DBBS_KG_WB=4 builds the other width.
#ifndef BBS_KG_WB
#define BBS_KG_WB 8
#endif
constexpr int KG_WB = BBS_KG_WB;                 // comb window, bits: 4 or 8
constexpr int KG_WINDOWS = 256 / KG_WB;
constexpr int KG_PER_WIN = (1 << KG_WB) - 1;     // entries per window: the digits 1 .. 2^KG_WB - 1
static_assert(KG_WB == 4 || KG_WB == 8, "a digit must not straddle two words of the scalar; 16 bits would be a 235 MB table");

// words of the comb table: [KG_WINDOWS][KG_PER_WIN][x.c0, x.c1, y.c0, y.c1][N]
template <class C>
constexpr size_t kg_table_words() { return (size_t)KG_WINDOWS * KG_PER_WIN * 4 * C::FpP::N; }

struct KgDeriveArgs {
    size_t n;
    const uint32_t* km_off; const uint32_t* km_len;      // [n] key_material of item i: km[km_off[i] .. + km_len[i])
    const uint32_t* ki_off; const uint32_t* ki_len;      // [n] key_info likewise
    const uint8_t* km; const uint8_t* ki;
    uint8_t dst[256];            // key_dst, one for the call (as MsgHashArgs::dst)
    uint32_t dst_len;
    int dst_too_long;            // key_dst has more than 255 bytes: dst is empty and every item that passed the length checks is refused
    int8_t accepted;             // what an accepted item's status becomes: 1, or ST_PENDING when KgPublic follows and decides
    uint32_t* sk;                // [8][n] canonical words; zero for a refused item
    int8_t* status;              // [n]
};

template <class C>
struct KgDerive {
    static __host__ __device__ void run(const KgDeriveArgs& a, size_t i) {
        const uint32_t km_len = a.km_len[i], ki_len = a.ki_len[i];
        const bool km_short = km_len < 32, ki_long = ki_len > 65535;
        Sha256 s;
        xmd48_begin(s);
        sha256_bytes(s, a.km + a.km_off[i], km_len);
        sha256_byte(s, (ki_len >> 8) & 0xff);
        sha256_byte(s, ki_len & 0xff);
        sha256_bytes(s, a.ki + a.ki_off[i], ki_long ? 65535u : ki_len);
        uint32_t okm[12];
        xmd48_finish(s, a.dst, a.dst_len, okm);
        const Fr<C> r = fe_to_canonical<typename C::FrP>(fr_from_okm<C>(okm));
        uint32_t any = 0;
        for (int k = 0; k < 8; k++) any |= r.v[k];
        const int8_t st = (int8_t)(km_short ? BBS_ST_INVALID_KEY_MATERIAL_LENGTH : ki_long ? BBS_ST_INVALID_KEY_INFO_LENGTH :
                                   a.dst_too_long ? BBS_ST_PANIC_DST_TOO_LONG : !any ? BBS_ST_INVALID_SECRET_KEY : a.accepted);
        uint32_t out[8];
        for (int k = 0; k < 8; k++) out[k] = st == a.accepted ? r.v[k] : 0u;
        soa_st<8>(a.sk, a.n, i, out);
        a.status[i] = st;
    }
};

template <class C>
struct KgPublicArgs {
    size_t n;
    const uint32_t* sk;          // [8][n] words of the scalars
    const uint32_t* table;       // kg_table_words<C>() words
    int8_t* status;              // [n] ST_PENDING on entry for an item to decide; any other value is kept and its outputs are zero
    uint32_t* rec;               // [n][4 NC] words x.c0, x.c1, y.c0, y.c1 (little-endian), or null
    uint32_t* oct;               // [n][2 NC] words holding the compressed strings, or null
    int8_t* inf;                 // [n] 1 = the identity key (sk = 0), or null
};

#if defined(__HIP_DEVICE_COMPILE__)
#define BBS_KG_HD BBS_HD
#else
#define BBS_KG_HD __host__ __device__ inline __attribute__((noinline))
#endif

template <class C>
BBS_KG_HD Fp2<C> kg_table_load(const uint32_t* p) {
    constexpr int N = C::FpP::N;
    Fp2<C> v;
    for (int j = 0; j < N; j++) { v.c0.v[j] = p[j]; v.c1.v[j] = p[N + j]; }
    return v;
}

// T + (qx, qy) when `take`, T otherwise; (qx, qy) affine and not the identity.  Exact for T = the identity; T = +-(qx, qy)
// (H = 0 with a live T) is not computed but reported in `degenerate` (see the header: it cannot happen)
template <class C>
BBS_KG_HD void kg_add(G2Jac<C>& T, const Fp2<C>& qx, const Fp2<C>& qy, bool take, bool& degenerate) {
    const bool t_inf = f2_is_zero<C>(T.z);
    const Fp2<C> ZZ = f2_sqr<C>(T.z);
    const Fp2<C> H = f2_sub<C>(f2_mul<C>(qx, ZZ), T.x);
    const Fp2<C> R = f2_sub<C>(f2_mul<C>(qy, f2_mul<C>(T.z, ZZ)), T.y);
    const Fp2<C> HH = f2_sqr<C>(H), HHH = f2_mul<C>(H, HH), V = f2_mul<C>(T.x, HH);
    G2Jac<C> r;
    r.x = f2_sub<C>(f2_sub<C>(f2_sqr<C>(R), HHH), f2_dbl<C>(V));
    r.y = f2_sub<C>(f2_mul<C>(R, f2_sub<C>(V, r.x)), f2_mul<C>(T.y, HHH));
    r.z = f2_mul<C>(T.z, H);
    degenerate |= take & !t_inf & f2_is_zero<C>(H);
    const Fp2<C> one = f2_one<C>();
    T.x = f2_select<C>(take, f2_select<C>(t_inf, qx, r.x), T.x);
    T.y = f2_select<C>(take, f2_select<C>(t_inf, qy, r.y), T.y);
    T.z = f2_select<C>(take, f2_select<C>(t_inf, one, r.z), T.z);
}

template <class C>
struct KgPublic {
    static __host__ __device__ __forceinline__ void run(const KgPublicArgs<C>& a, size_t t) {
        using P = typename C::FpP;
        constexpr int N = P::N, NC = P::NC;
        const int8_t st_in = a.status[t];
        const bool live = st_in == ST_PENDING;
        // ---- 1. the scalar: canonical?  (a lane that is not live or not canonical walks the scalar 1)
        uint32_t k[8];
        soa_ld<8>(a.sk, a.n, t, k);
        const bool canon = limbs_lt_mod<typename C::FrP>(k);
        uint32_t any = 0;
        for (int j = 0; j < 8; j++) any |= k[j];
        const bool stand_in = !live | !canon;
        // ---- 2. the comb: one mixed addition per window, no doubling
        G2Jac<C> T = {f2_zero<C>(), f2_zero<C>(), f2_zero<C>()};
        bool degenerate = false;
#pragma unroll 1
        for (int j = 0; j < 8; j++) {
            const uint32_t word = stand_in ? (j == 0 ? 1u : 0u) : a.sk[(size_t)j * a.n + t];
#pragma unroll 1
            for (int b = 0; b < 32 / KG_WB; b++) {
                const int w = j * (32 / KG_WB) + b;
                const uint32_t d = (word >> (KG_WB * b)) & (uint32_t)KG_PER_WIN;
                const uint32_t* e = a.table + ((size_t)w * KG_PER_WIN + (d ? d - 1 : 0)) * 4 * N;
                const Fp2<C> qx = kg_table_load<C>(e), qy = kg_table_load<C>(e + 2 * N);
                kg_add<C>(T, qx, qy, d != 0, degenerate);
            }
        }
        // ---- 3. affine, canonical
        const bool z0 = f2_is_zero<C>(T.z);
        const Fp2<C> zi = f2_inv<C>(f2_select<C>(z0, f2_one<C>(), T.z)), zi2 = f2_sqr<C>(zi);
        const Fp2<C> x = f2_canon<C>(f2_mul<C>(T.x, zi2)), y = f2_canon<C>(f2_mul<C>(T.y, f2_mul<C>(zi, zi2)));
        const bool inf = !stand_in & !any;                             // sk = 0: the identity key
        const bool failed = !stand_in & (degenerate | (z0 & (any != 0)));     // fail closed: the item stays undecided
        const bool put = !stand_in & !inf & !failed;
        uint32_t xw0[NC], xw1[NC], yw0[NC], yw1[NC];
        fe_to_words<P>(x.c0, xw0); fe_to_words<P>(x.c1, xw1);
        fe_to_words<P>(y.c0, yw0); fe_to_words<P>(y.c1, yw1);
        const bool largest = fe_is_zero<P>(y.c1) ? kb_fe_gt_half<P>(y.c0) : kb_fe_gt_half<P>(y.c1);
        // ---- 4. outputs: every word, whatever the status
        if (a.rec) {
            uint32_t* ro = a.rec + t * 4 * NC;
            for (int i = 0; i < NC; i++) {
                ro[i] = put ? xw0[i] : 0u; ro[NC + i] = put ? xw1[i] : 0u;
                ro[2 * NC + i] = put ? yw0[i] : 0u; ro[3 * NC + i] = put ? yw1[i] : 0u;
            }
        }
        if (a.oct) {
            uint32_t* o = a.oct + t * 2 * NC;
            if constexpr (C::ID == 0) {                                // big-endian x.c1 || x.c0, flags in the first byte
                const uint32_t fl = inf ? 0xC0000000u : put ? (0x80000000u | (largest ? 0x20000000u : 0u)) : 0u;
                for (int i = 0; i < NC; i++) {
                    o[NC - 1 - i] = kb_bswap((put ? xw1[i] : 0u) | (i == NC - 1 ? fl : 0u));
                    o[2 * NC - 1 - i] = kb_bswap(put ? xw0[i] : 0u);
                }
            } else {                                                   // little-endian x.c0 || x.c1, flags in the last byte
                const uint32_t fl = inf ? 0x40000000u : (put & largest) ? 0x80000000u : 0u;
                for (int i = 0; i < NC; i++) {
                    o[i] = put ? xw0[i] : 0u;
                    o[NC + i] = (put ? xw1[i] : 0u) | (i == NC - 1 ? fl : 0u);
                }
            }
        }
        if (a.inf) a.inf[t] = (int8_t)(inf ? 1 : 0);
        a.status[t] = !live ? st_in : !canon ? (int8_t)BBS_ST_NONCANONICAL : failed ? ST_PENDING : (int8_t)1;
    }
};

#undef BBS_KG_HD

}  // namespace bbs
