// Seeded random scalars on the device (bbs_ctx_set_seeded_random_scalars, bbs_seeded_random_scalars_batch):
// seeded_random_scalars(seed, dst, count) of the reference (src/utils/core_utilities.rs:84-100) = expand_message(seed, dst,
// 48 * count) cut into 48-byte pieces, each through FromOkm.  One lane per item: the chain b_1 .. b_ell is sequential (every
// b_i hashes b_{i-1}); 48 bytes are one and a half hash values, so a scalar straddles two of them and three b_i make two scalars.
#pragma once
#include "stages_common.hpp"

namespace bbs {

constexpr uint32_t DRAW_MAX_COUNT = (XMD_MAX_ELL * 32) / 48;      // 170: ell = ceil(48 * count / 32) <= 255

// what a draw needs of its DST; a DST of more than 255 bytes is refused before any item reads this (dst_len = 0 then)
struct DrawDst {
    uint8_t dst[256];
    uint32_t dst_len;
    XmdTail tail;
};
inline void draw_dst_build(DrawDst& d, const uint8_t* dst, size_t dst_len) {
    std::memset(&d, 0, sizeof(d));
    if (dst_len > 255) dst_len = 0;
    if (dst_len) std::memcpy(d.dst, dst, dst_len);
    d.dst_len = (uint32_t)dst_len;
    xmd_tail_build(d.tail, d.dst, d.dst_len);
}

// count (1 .. DRAW_MAX_COUNT) canonical scalars, 8 little-endian words each, to out[0 .. 8 * count).  The seed is
// seed[0 .. seed_len), followed by I2OSP(index, 8) when `indexed` (the job-seed shape).  Lanes of a wavefront leave the loop
// at different trip counts: inside it the compression function, the Montgomery multiplier and the canonical conversion are
// each reached from one place.
template <class C>
BBS_HD void draw_scalars(const DrawDst& d, const uint8_t* seed, uint32_t seed_len, bool indexed, uint64_t index, uint32_t count, uint32_t* out) {
    using R = typename C::FrP;
    Sha256 s;
    xmd_begin(s);
    sha256_bytes(s, seed, seed_len);
    if (indexed) sha256_u64be(s, index);
    uint32_t b0[8], b[8], okm[12];
    xmd_b0(s, 48 * count, d.dst, d.dst_len, b0);
#pragma unroll
    for (int j = 0; j < 8; j++) b[j] = 0;
#pragma unroll
    for (int j = 0; j < 12; j++) okm[j] = 0;
    const uint32_t ell = xmd_ell(48 * count);
    uint32_t phase = 0;           // bytes of the scalar under way that earlier b_i supplied: 0, 32 (phase 1) or 16 (phase 2)
    for (uint32_t i = 1; i <= ell; i++) {
        xmd_next(d.tail, b0, b, i);
        if (phase == 0) {
#pragma unroll
            for (int j = 0; j < 8; j++) okm[j] = b[j];
            phase = 1;
            continue;
        }
        if (phase == 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) okm[8 + j] = b[j];
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++) okm[4 + j] = b[j];
        }
        const Fr<C> r = fe_to_canonical<R>(fr_from_okm<C>(okm));
#pragma unroll
        for (int j = 0; j < 8; j++) out[j] = r.v[j];
        out += 8;
        if (phase == 1) {
#pragma unroll
            for (int j = 0; j < 4; j++) okm[j] = b[4 + j];
            phase = 2;
        } else phase = 0;
    }
}

// ---- the primitive: counts given by the caller ----------------------------------------------------------------------------
struct DrawArgs {
    size_t n;
    const uint8_t* seeds;
    const uint64_t* seed_off;     // n + 1, bytes
    const uint32_t* counts;
    const uint64_t* out_off;      // n + 1, scalars: the running sum of the counts
    int dst_too_long;
    DrawDst d;
    uint32_t* out;                // [out_off[n]][8] canonical
    int8_t* status;
};
template <class C>
struct DrawItem {
    static __host__ __device__ void run(const DrawArgs& a, size_t i) {
        const uint32_t count = a.counts[i];
        // (expand_message looks at ell before it looks at the DST: utilities_helper.rs:46-52)
        if (count > DRAW_MAX_COUNT) { a.status[i] = (int8_t)BBS_ST_PANIC_ELL_TOO_BIG; return; }
        if (a.dst_too_long) { a.status[i] = (int8_t)BBS_ST_PANIC_DST_TOO_LONG; return; }
        draw_scalars<C>(a.d, a.seeds + a.seed_off[i], (uint32_t)(a.seed_off[i + 1] - a.seed_off[i]), false, 0, count, a.out + a.out_off[i] * 8);
        a.status[i] = 1;
    }
};

// ---- proof_gen: stage PgDraw, once per upload, in front of PgIngest ---------------------------------------------------------
// Item i's 5 + l_i - r_i scalars (r_i before deduplication, as the reference sizes them: proof_gen.rs:145-149) go to
// out[sc_off[i] ..): the array and the offsets PgIngest is given as rnd / rnd_off.  The reference draws BEFORE proof_init's
// checks (:229-239) and after everything that decides an item earlier, so an item that is decided earlier draws nothing and its
// seed is not read: a signature that does not decode (wire form), msg_to_scalars' refusal, r > l, a disclosed index >= l, an
// unknown key.  A draw that the reference's expand_message refuses (utilities_helper.rs:46-52) leaves its code in dcode[i];
// PgDrawGate puts it in front of whatever PgIngest found for that item (all of which the reference would have found later).
template <class C>
struct PgDrawArgs {
    size_t n;
    const uint8_t* oct;           // wire form: see PgIngestArgs
    const int8_t* pcode;
    int msg_dst_too_long;
    const uint32_t* kidx;         // keyed jobs: KEY_NONE = decided by KeyGate; nullptr otherwise
    const uint64_t *m_off, *di_off;
    const uint64_t* di;
    const uint8_t* seeds;         // per-item seeds, or the 32-byte job seed
    const uint64_t* seed_off;     // n + 1, bytes; unused with a job seed
    int job_seed;                 // item i's seed is seeds[0 .. 32) || I2OSP(i, 8)
    int dst_too_long;
    DrawDst d;
    const uint64_t* sc_off;       // n + 1, scalars
    uint32_t* out;
    int8_t* dcode;                // 0, -23 or -24
};
template <class C>
struct PgDraw {
    static __host__ __device__ void run(const PgDrawArgs<C>& a, size_t i) {
        using R = typename C::FrP;
        a.dcode[i] = 0;
        if (a.kidx && a.kidx[i] == 0xFFFFFFFFu) return;                       // KEY_NONE
        if (a.oct) {                                                            // the verdicts PgIngest gives first
            constexpr size_t NB = 4 * C::FpP::NC;
            uint32_t e[8];
            be32_words(a.oct + i * (NB + 32) + NB, e);
            uint32_t any = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) any |= e[k];
            const int8_t c = a.pcode[i];
            if (c < 0 || c == 1 || !limbs_lt_mod<R>(e) || !any) return;
        }
        const uint64_t l = a.m_off[i + 1] - a.m_off[i], r = a.di_off[i + 1] - a.di_off[i];
        if (a.msg_dst_too_long && l > 0) return;
        if (r > l) return;
        const uint64_t* idx = a.di + a.di_off[i];
        bool bad = false;
        for (uint64_t k = 0; k < r; k++) bad |= idx[k] >= l;
        if (bad) return;
        const uint64_t count = 5 + l - r;
        if (count > DRAW_MAX_COUNT) { a.dcode[i] = (int8_t)BBS_ST_PANIC_ELL_TOO_BIG; return; }
        if (a.dst_too_long) { a.dcode[i] = (int8_t)BBS_ST_PANIC_DST_TOO_LONG; return; }
        // (the host sized out from the same l and r: sc_off[i + 1] - sc_off[i] == count here)
        const bool js = a.job_seed != 0;
        const uint8_t* seed = js ? a.seeds : a.seeds + a.seed_off[i];
        const uint32_t seed_len = js ? 32u : (uint32_t)(a.seed_off[i + 1] - a.seed_off[i]);
        draw_scalars<C>(a.d, seed, seed_len, js, (uint64_t)i, (uint32_t)count, a.out + a.sc_off[i] * 8);
    }
};
struct PgDrawGateArgs { size_t n; const int8_t* dcode; int8_t* status0; };
struct PgDrawGate {
    static __host__ __device__ void run(const PgDrawGateArgs& a, size_t i) {
        if (a.dcode[i] != 0) a.status0[i] = a.dcode[i];
    }
};

}  // namespace bbs
