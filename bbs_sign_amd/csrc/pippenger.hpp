// Large-n variable-base multi-scalar multiplication  S = sum_i k_i * P_i  by the bucket (Pippenger) method,
// and the random-linear-combination batch check built on it.
//
// The per-item multi-scalar multiplications of the four core operations (stages.hpp) have at most 38 terms and
// fixed bases: they use window tables.  THIS file is the other shape: thousands of per-item points, one sum.
// Used by
//   * bbs_g1_msm_pippenger (unit parity against the oracle's sum), and
//   * batch verification: instead of n two-pairing products e(Abar_i, W) e(Bbar_i, -BP2) == 1
//     (src/proof_verify.rs:112-115) one checks  e(sum rho_i Abar_i, W) e(sum rho_i Bbar_i, -BP2) == 1  for secret
//     random 128-bit rho_i; the left side equals prod_i t_i^rho_i where t_i is item i's own pairing product, an
//     r-th root of unity after the final exponentiation, so a batch that passes has every t_i = 1 except with
//     probability 2^-128 (cofactor components of a point never reach GT: the final exponentiation removes them).
//     A batch that fails is re-checked item by item with the exact kernel, so the booleans are the reference's.
//
// Host-twin stages (lane-per-work-unit functors; window c = 8 bits, digits in HBM as bytes) -- the device runs the
// workgroup-cooperative kernel k_pip_window further down instead of the first three:
//   PipBuckets : lane per (point set, window, bucket b): scans the window's n digits (every lane of a wavefront
//                reads the same words -> one broadcast load per 4 items), claims its slice of the window's index
//                list (offset = number of smaller non-zero digits), fills it, then sums its points with mixed
//                additions -- no atomics, no conflicts, every lane of a wavefront in the same loop.
//   PipSegments: lane per 16 buckets: running sums  sum_b (b - 16 s) B_b  and  sum_b B_b, then  + 16 s * (sum B_b).
//   PipWindows : lane per window: adds its 16 segments and shifts by 2^(8 w).
//   PipFinal   : lane per point set: adds the windows, one inversion, affine Montgomery out.
// Batch verification does not need the one 128-bit combination: the 16 windows are 16 INDEPENDENT 8-bit
// combinations (digit bytes of a hash are independent and uniform), each checked by its own pairing product; a bad
// item survives one of them with probability <= 1/256 and all of them with 2^-128.  So PipWindowSums (no shifts)
// writes 16 affine sums per point set and the 16 checks run side by side in two wavefronts of the pairing kernel --
// no 120 doublings, no final addition chain.
#pragma once
#include "stages.hpp"

namespace bbs {

constexpr int PIP_C = 8;             // window bits
constexpr int PIP_NB = 1 << PIP_C;   // buckets per window (bucket 0 unused)
constexpr int PIP_SEG = 16;          // buckets per segment

template <class C>
struct PipArgs {
    size_t n;                 // points per set
    size_t n_pad;             // n rounded up to a multiple of 4: length of a digit row
    int M;                    // point sets sharing the digits (1 or 2)
    int NW;                   // windows = scalar bits / 8
    const uint32_t* ppts;     // [M][n][2N] Montgomery affine, item-major, (0,0) = identity
    const uint8_t* dig;       // [NW][n_pad] window digits, 0 = no contribution
    uint32_t* list;           // [M][NW][n] item indexes grouped by bucket
    uint32_t* buckets;        // [3N][M*NW*256] Jacobian
    uint32_t* segs;           // [3N][M*NW*16]
    uint32_t* wins;           // [3N][M*NW]
    uint32_t* out;            // [M][2N] Montgomery affine sums
};

template <class C>
struct PipBuckets {
    static __host__ __device__ void run(const PipArgs<C>& a, size_t t) {
        const size_t T = (size_t)a.M * a.NW * PIP_NB;
        const uint32_t b = (uint32_t)(t & (PIP_NB - 1));
        const size_t mw = t >> PIP_C;
        const int m = (int)(mw / (size_t)a.NW);
        const int w = (int)(mw - (size_t)m * a.NW);
        if (b == 0) { g1j_store<C>(a.buckets, T, t, g1j_inf<C>()); return; }
        const uint32_t* dw = reinterpret_cast<const uint32_t*>(a.dig + (size_t)w * a.n_pad);
        const size_t nq = a.n_pad >> 2;
        uint32_t lower = 0, cnt = 0;
        for (size_t q = 0; q < nq; q++) {
            const uint32_t word = dw[q];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t d = (word >> (8 * k)) & 0xffu;
                lower += ((d - 1u) < (b - 1u)) ? 1u : 0u;        // 0 < d < b
                cnt += (d == b) ? 1u : 0u;
            }
        }
        uint32_t* lst = a.list + mw * a.n + lower;
        uint32_t pos = 0;
        for (size_t q = 0; q < nq && pos < cnt; q++) {
            const uint32_t word = dw[q];
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (((word >> (8 * k)) & 0xffu) == b) lst[pos++] = (uint32_t)(4 * q + k);
        }
        const uint32_t* pts = a.ppts + (size_t)m * a.n * 2 * C::FpP::N;
        G1Jac<C> acc = g1j_inf<C>();
        for (uint32_t k = 0; k < cnt; k++) acc = g1j_add_aff<C>(acc, g1a_load_mont<C>(pts + (size_t)lst[k] * 2 * C::FpP::N, 1, 0));
        g1j_store<C>(a.buckets, T, t, acc);
    }
};

template <class C>
struct PipSegments {
    static __host__ __device__ void run(const PipArgs<C>& a, size_t t) {
        const size_t T = (size_t)a.M * a.NW * PIP_NB, TS = (size_t)a.M * a.NW * (PIP_NB / PIP_SEG);
        const uint32_t s = (uint32_t)(t % (PIP_NB / PIP_SEG));
        const size_t base = (t / (PIP_NB / PIP_SEG)) * PIP_NB + (size_t)s * PIP_SEG;
        G1Jac<C> run = g1j_inf<C>(), acc = g1j_inf<C>();
        for (int b = PIP_SEG - 1; b >= 1; b--) {
            run = g1j_add<C>(run, g1j_load<C>(a.buckets, T, base + b));
            acc = g1j_add<C>(acc, run);                      // acc = sum_b (b - 16 s) B_b
        }
        run = g1j_add<C>(run, g1j_load<C>(a.buckets, T, base));
        if (s) {                                             // + 16 s * sum_b B_b
            G1Jac<C> sr = g1j_inf<C>();
            for (int bit = 3; bit >= 0; bit--) {
                sr = g1j_dbl<C>(sr);
                if ((s >> bit) & 1u) sr = g1j_add<C>(sr, run);
            }
            for (int k = 0; k < 4; k++) sr = g1j_dbl<C>(sr);
            acc = g1j_add<C>(acc, sr);
        }
        g1j_store<C>(a.segs, TS, t, acc);
    }
};

template <class C>
struct PipWindows {
    static __host__ __device__ void run(const PipArgs<C>& a, size_t t) {
        const size_t TS = (size_t)a.M * a.NW * (PIP_NB / PIP_SEG), TW = (size_t)a.M * a.NW;
        const int w = (int)(t % (size_t)a.NW);
        G1Jac<C> acc = g1j_inf<C>();
        for (int s = 0; s < PIP_NB / PIP_SEG; s++) acc = g1j_add<C>(acc, g1j_load<C>(a.segs, TS, t * (PIP_NB / PIP_SEG) + s));
        for (int k = 0; k < PIP_C * w; k++) acc = g1j_dbl<C>(acc);
        g1j_store<C>(a.wins, TW, t, acc);
    }
};

template <class C>
struct PipFinal {
    static __host__ __device__ void run(const PipArgs<C>& a, size_t m) {
        constexpr int N = C::FpP::N;
        const size_t TW = (size_t)a.M * a.NW;
        G1Jac<C> acc = g1j_inf<C>();
        for (int w = 0; w < a.NW; w++) acc = g1j_add<C>(acc, g1j_load<C>(a.wins, TW, m * a.NW + w));
        g1a_store_mont<C>(a.out + m * 2 * N, 1, 0, g1j_to_aff<C>(acc));
    }
};

// batch verification: window sums without the 2^(8 w) shift, normalised: out[m] is an SoA array of NW affine points
// ([2N][NW], Montgomery), i.e. NW "items" for the pairing stage
template <class C>
struct PipWindowSums {
    static __host__ __device__ void run(const PipArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t TS = (size_t)a.M * a.NW * (PIP_NB / PIP_SEG);
        const size_t m = t / (size_t)a.NW, w = t - m * (size_t)a.NW;
        G1Jac<C> acc = g1j_inf<C>();
        for (int s = 0; s < PIP_NB / PIP_SEG; s++) acc = g1j_add<C>(acc, g1j_load<C>(a.segs, TS, t * (PIP_NB / PIP_SEG) + s));
        g1a_store_mont<C>(a.out + m * 2 * N * a.NW, (size_t)a.NW, w, g1j_to_aff<C>(acc));
    }
};

// =============================================================================================
// Workgroup-cooperative bucket accumulation (round 3; device only -- the lane functors above remain the host twin's path)
// =============================================================================================
// One workgroup of 256 threads (four wavefronts = one per SIMD of a compute unit) per (point set m, window w, tile of
// PIP_TILE items); thread b OWNS bucket b.
//   1. the tile's digit bytes of window w are staged ONCE into LDS (coalesced 16-byte loads);
//   2. bucket membership by wavefront ballots: for every 64 digits the eight ballots B_j of their bits are formed, and
//      thread b's members are the lanes in  AND_j (b_j ? B_j : ~B_j)  -- 16 mask operations per 64 items instead of 64
//      byte compares; a first pass counts (popcount), an exclusive scan over the 256 counts (wavefront shuffles + one
//      LDS hop between the four wavefronts) gives every bucket its slice of an index list in LDS, a second pass fills
//      it in item order (deterministic: no atomics);
//   3. thread b sums the points of its slice (mixed additions; points read as 16-byte vectors from an item-major copy);
//   4. sum_b b * B_b  =  sum_{b >= 1} T_b  with the suffix sums T_b = sum_{j >= b} B_j: a Hillis-Steele scan and a tree
//      reduction over the 256 threads, the points moved between lanes with wavefront shuffles and between the four
//      wavefronts through LDS -- 19 Jacobian additions deep instead of the 48 of the segment / window-sum stages;
//   5. thread 0 stores the tile's window sum (Jacobian).  Window sums are linear in the bucket contents, so tiles simply
//      add up: PipTileSums (lane per window) adds the tiles and normalises (or shifts, for the plain MSM).
// HBM traffic per workgroup: PIP_TILE digit bytes + its points once (112 B each on BLS12-381) -- the algorithmic minimum.
constexpr int PIP_TILE = 4096;
constexpr int PIP_WG = 256;           // (k_pip_window_seg further down is k_pip_window's twin over a segment table: keep the two in step)

template <class C>
struct PipCoopArgs {
    size_t n, n_pad;
    int M, NW, n_tiles;
    const uint32_t* ppts;     // [M][n][2N] Montgomery affine, ITEM-major (one point = 2N consecutive words), (0,0) = identity
    const uint8_t* dig;       // [NW][n_pad]
    uint32_t* tile_sums;      // [3N][M*NW*n_tiles] Jacobian (SoA over the work units)
    uint32_t* out_aff;        // n_tiles == 1 only, or null: the window sum normalised straight into [M][2N][NW] (no PipTileSums launch)
};

#if !defined(BBS_HOST_TWIN)
template <class C>
__device__ __forceinline__ G1Jac<C> g1j_shfl_down(const G1Jac<C>& p, int delta) {
    G1Jac<C> r;
#pragma unroll
    for (int j = 0; j < C::FpP::N; j++) {
        r.x.v[j] = (uint32_t)__shfl_down((int)p.x.v[j], delta, 64);
        r.y.v[j] = (uint32_t)__shfl_down((int)p.y.v[j], delta, 64);
        r.z.v[j] = (uint32_t)__shfl_down((int)p.z.v[j], delta, 64);
    }
    return r;
}
template <class C>
__device__ __forceinline__ void g1j_to_lds(uint32_t* s, const G1Jac<C>& p) {
#pragma unroll
    for (int j = 0; j < C::FpP::N; j++) { s[j] = p.x.v[j]; s[C::FpP::N + j] = p.y.v[j]; s[2 * C::FpP::N + j] = p.z.v[j]; }
}
template <class C>
__device__ __forceinline__ G1Jac<C> g1j_from_lds(const uint32_t* s) {
    G1Jac<C> p;
#pragma unroll
    for (int j = 0; j < C::FpP::N; j++) { p.x.v[j] = s[j]; p.y.v[j] = s[C::FpP::N + j]; p.z.v[j] = s[2 * C::FpP::N + j]; }
    return p;
}

template <class C>
__global__ void __launch_bounds__(PIP_WG) k_pip_window(PipCoopArgs<C> a) {
    constexpr int N = C::FpP::N;
    __shared__ __attribute__((aligned(16))) uint8_t s_dig[PIP_TILE];
    __shared__ uint16_t s_list[PIP_TILE];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_pt[4][3 * N];
    const int b = (int)threadIdx.x, lane = b & 63, wv = b >> 6;
    const size_t unit = blockIdx.x;                          // (m * NW + w) * n_tiles + tile
    const int tile = (int)(unit % (size_t)a.n_tiles);
    const size_t mw = unit / (size_t)a.n_tiles;
    const int w = (int)(mw % (size_t)a.NW), m = (int)(mw / (size_t)a.NW);
    const size_t i0 = (size_t)tile * PIP_TILE;
    const int n_t = (int)((a.n - i0) < (size_t)PIP_TILE ? (a.n - i0) : (size_t)PIP_TILE);
    // 1. digits -> LDS (the row is padded to a multiple of 4 and a tile starts at a multiple of 4096: 4-byte loads are aligned)
    {
        const uint8_t* row = a.dig + (size_t)w * a.n_pad + i0;
        uint32_t* s32 = reinterpret_cast<uint32_t*>(s_dig);
        for (int q = b; q < PIP_TILE / 4; q += PIP_WG) {
            uint32_t v = 0;
            if (4 * q < n_t) {
                v = *reinterpret_cast<const uint32_t*>(row + 4 * q);
                const int rem = n_t - 4 * q;
                if (rem < 4) v &= (1u << (8 * rem)) - 1u;
            }
            s32[q] = v;
        }
    }
    __syncthreads();
    const int n_chunks = (n_t + 63) >> 6;
    // membership mask of bucket b among the 64 digits of chunk q (every wavefront forms the same eight ballots)
    auto members = [&](int q) -> uint64_t {
        const uint32_t d = s_dig[q * 64 + lane];
        uint64_t mk = ~(uint64_t)0;
#pragma unroll
        for (int j = 0; j < PIP_C; j++) {
            const uint64_t bj = __ballot((d >> j) & 1u);
            mk &= ((b >> j) & 1) ? bj : ~bj;
        }
        return b ? mk : (uint64_t)0;                         // digit 0 contributes nothing
    };
    // 2a. counts
    uint32_t cnt = 0;
    for (int q = 0; q < n_chunks; q++) cnt += (uint32_t)__popcll(members(q));
    // 2b. exclusive scan of the 256 counts: inclusive scan inside the wavefront, wavefront totals through LDS
    uint32_t inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t start = inc - cnt;
    for (int k = 0; k < wv; k++) start += s_wave[k];
    // 2c. fill (item order)
    {
        uint32_t pos = start;
        for (int q = 0; q < n_chunks; q++) {
            uint64_t mk = members(q);
            while (mk) {
                const int l = __ffsll((unsigned long long)mk) - 1;
                mk &= mk - 1;
                s_list[pos++] = (uint16_t)(q * 64 + l);
            }
        }
    }
    __syncthreads();
    // 3. bucket sum
    G1Jac<C> acc = g1j_inf<C>();
    {
        const uint32_t* pts = a.ppts + ((size_t)m * a.n + i0) * (2 * N);
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* e = reinterpret_cast<const uint4*>(pts + (size_t)s_list[start + k] * (2 * N));
            uint32_t wds[2 * N];
            static_assert((2 * N) % 4 == 0, "a point is a whole number of 16-byte vectors");
#pragma unroll
            for (int v = 0; v < (2 * N) / 4; v++) { const uint4 t = e[v]; wds[4 * v] = t.x; wds[4 * v + 1] = t.y; wds[4 * v + 2] = t.z; wds[4 * v + 3] = t.w; }
            G1Aff<C> pnt;
#pragma unroll
            for (int j = 0; j < N; j++) { pnt.x.v[j] = wds[j]; pnt.y.v[j] = wds[N + j]; }
            acc = g1j_add_aff<C>(acc, pnt);
        }
    }
    // 4a. suffix sums T_b = sum_{j >= b} B_j: inside the wavefront by shuffles ...
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const G1Jac<C> o = g1j_shfl_down<C>(acc, off);
        if (lane + off < 64) acc = g1j_add<C>(acc, o);
    }
    // ... then + everything held by the wavefronts above (their totals are in their lane 0)
    if (lane == 0) g1j_to_lds<C>(s_pt[wv], acc);
    __syncthreads();
    {
        G1Jac<C> above = g1j_inf<C>();
        for (int k = 3; k > wv; k--) above = g1j_add<C>(above, g1j_from_lds<C>(s_pt[k]));
        acc = g1j_add<C>(acc, above);
    }
    __syncthreads();
    // 4b. sum_{b >= 1} T_b: bucket 0 holds nothing of its own, its suffix sum is not a term
    if (b == 0) acc = g1j_inf<C>();
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {
        const G1Jac<C> o = g1j_shfl_down<C>(acc, off);
        if (lane < off) acc = g1j_add<C>(acc, o);
    }
    if (lane == 0) g1j_to_lds<C>(s_pt[wv], acc);
    __syncthreads();
    // 5. thread 0: the tile's window sum
    if (b == 0) {
        for (int k = 1; k < 4; k++) acc = g1j_add<C>(acc, g1j_from_lds<C>(s_pt[k]));
        if (a.out_aff && a.n_tiles == 1) g1a_store_mont<C>(a.out_aff + (size_t)m * 2 * N * a.NW, (size_t)a.NW, (size_t)w, g1j_to_aff<C>(acc));
        else g1j_store<C>(a.tile_sums, (size_t)a.M * a.NW * a.n_tiles, unit, acc);
    }
}
#endif

// lane per (m, w): add the tiles' window sums.  shift = 0: normalise into the SoA array of NW affine points per set the
// combined pairing checks read (batch verification: the windows are independent 8-bit combinations); shift = 1: the plain
// MSM -- multiply window w by 2^(8 w) and leave it Jacobian in `wins` for PipFinal.
template <class C>
struct PipTileSumArgs {
    int M, NW, n_tiles, shift;
    const uint32_t* tile_sums;   // [3N][M*NW*n_tiles]
    uint32_t* out;               // [M][2N][NW] Montgomery affine (shift = 0)
    uint32_t* wins;              // [3N][M*NW] (shift = 1)
};
template <class C>
struct PipTileSums {
    static __host__ __device__ void run(const PipTileSumArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t TU = (size_t)a.M * a.NW * a.n_tiles, TW = (size_t)a.M * a.NW;
        const size_t m = t / (size_t)a.NW, w = t - m * (size_t)a.NW;
        G1Jac<C> acc = g1j_inf<C>();
        for (int k = 0; k < a.n_tiles; k++) acc = g1j_add<C>(acc, g1j_load<C>(a.tile_sums, TU, t * a.n_tiles + k));
        if (a.shift) {
            for (size_t k = 0; k < (size_t)PIP_C * w; k++) acc = g1j_dbl<C>(acc);
            g1j_store<C>(a.wins, TW, t, acc);
        } else {
            g1a_store_mont<C>(a.out + m * 2 * N * a.NW, (size_t)a.NW, w, g1j_to_aff<C>(acc));
        }
    }
};

// ---- batch verification glue ------------------------------------------------------------------
// lane per item, in front of the bucket stage: the item's two points in Montgomery form, item-major, and its sixteen
// digit bytes  rho_i = first 128 bits of SHA-256(seed || I2OSP(i, 8)).  An item takes part iff gate_arr[i] == gate and
// (canonical inputs) both points are on the curve; otherwise its digits are 0 and it contributes nothing.
//   verify      : gate = the status after VfCombine (ST_PAIRING), points = A and e A - B (Montgomery, computed).
//   proof_verify: gate = the status the ingest stage left (ST_PENDING = structurally valid), points = the proof's own
//                 Abar, Bbar (canonical) -- the combination does not wait for the challenge stage: it runs on the job's
//                 second stream beside the MSM chain, as the per-item pairing does.  An item whose challenge does not
//                 match is then part of the combination although its status is already Ok(false): harmless when its
//                 pairing product is 1 (a tampered commitment / scalar), and when it is not, the combined check fails
//                 and the per-item kernel decides every item still pending -- the booleans are the reference's either way.
template <class C>
struct RlcPrepArgs {
    size_t n, n_pad;
    const uint32_t* pa;       // [2NC][n] canonical words or [2N][n] Montgomery limbs
    const uint32_t* pb;
    int canonical;
    const int8_t* gate_arr;
    int gate;
    uint32_t seed[8];         // secret per-batch seed
    uint8_t* dig;             // [16][n_pad]
    uint32_t* ppts;           // [2][n][2N]
};
template <class C>
struct RlcPrep {
    static __host__ __device__ void run(const RlcPrepArgs<C>& a, size_t i) {
        constexpr int N = C::FpP::N;
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        G1Aff<C> p = g1a_inf<C>(), q = g1a_inf<C>();
        bool in = a.gate_arr[i] == (int8_t)a.gate;
        if (in) {
            if (a.canonical) {
                p = g1a_load_canon_to_mont<C>(a.pa, a.n, i);
                q = g1a_load_canon_to_mont<C>(a.pb, a.n, i);
                in = g1a_on_curve<C>(p) && g1a_on_curve<C>(q);
            } else {
                p = g1a_load_mont<C>(a.pa, a.n, i);
                q = g1a_load_mont<C>(a.pb, a.n, i);
            }
        }
        if (in) {
            Sha256 s;
            sha256_init(s);
            for (int k = 0; k < 8; k++) sha256_word(s, a.seed[k]);
            sha256_u64be(s, (uint64_t)i);
            sha256_final(s, h);
        } else {
            p = g1a_inf<C>(); q = g1a_inf<C>();
        }
        for (int w = 0; w < 16; w++) a.dig[(size_t)w * a.n_pad + i] = (uint8_t)(h[w >> 2] >> (8 * (w & 3)));
        g1a_store_mont<C>(a.ppts + i * 2 * N, 1, 0, p);
        g1a_store_mont<C>(a.ppts + (a.n + i) * 2 * N, 1, 0, q);
    }
};

// =============================================================================================
// Keyed batch verification: one combination PER ISSUER KEY (bbs_ctx_set_keyed_batch_verification)
// =============================================================================================
// The argument of the head of this file, applied per key: for key k the library checks
//   e(sum rho_i Abar_i, W_k) e(sum rho_i Bbar_i, -BP2) == 1   over the items i presented under k,
// again as 16 independent 8-bit combinations.  The host (job_form.hpp keyed_bv_plan) sorts the grouped items by key into the
// BV ORDER: every group's run starts at a multiple of 4 (pad positions keep digit 0), and is cut into SEGMENTS of at most
// PIP_TILE items.  Stages, all on the job's main stream:
//   keyed_rlc_prep       : KeyedRlcPrep, RlcPrep's logic with the digits and the item-major points written at the item's
//                          POSITION in the bv order; rho_i stays SHA-256(seed || i) of the ITEM index;
//   keyed_pip_windows    : k_pip_window_seg, k_pip_window's algorithm with the tile taken from the segment table -- one
//                          workgroup per (set, window, segment); host twin: PipGroupSumsHost, double-and-add per group;
//   keyed_pip_group_sums : PipGroupSums, lane per (set, window, group): adds the group's segment sums and normalises into the
//                          SoA arrays the group's 16 VIRTUAL items read (entry g * 16 + w of [2N][16 G] per set);
//   keyed_rlc_pairing    : the existing keyed pairing step over the virtual items (virtual item g * 16 + w under group g's key);
//   keyed_bv_decide      : KeyedBvDecide, lane per item: pending, grouped and all 16 verdicts of its group 1 -> Ok(true).
// The per-item keyed pairing kernel follows and finds those items decided; the items of a group that failed, and the items
// of keys below the threshold, get their own product as before.  A failing key costs its own group, not the batch.
constexpr uint32_t BV_NONE = 0xFFFFFFFFu;     // pos_of_item / item_group of an item that belongs to no group

template <class C>
struct PipSegArgs {
    size_t n_pos;             // positions of the bv order (a multiple of 4): length of a digit row and of a point set
    int M, NW;
    uint32_t n_segs, n_groups;
    const uint32_t* segs;     // [n_segs][3] first position, items (<= PIP_TILE), group
    const uint32_t* grp_seg;  // [n_groups][2] first segment, segments
    const uint32_t* grp_run;  // [n_groups][2] first position (a multiple of 4), items
    const uint32_t* ppts;     // [M][n_pos][2N] Montgomery affine, item-major, (0,0) = identity
    const uint8_t* dig;       // [NW][n_pos]
    uint32_t* seg_sums;       // [3N][M*NW*n_segs] Jacobian (SoA over the work units (m * NW + w) * n_segs + segment)
    uint32_t* out;            // [M][2N][NW*n_groups] Montgomery affine: entry g * NW + w = window w of group g
};

template <class C>
struct KeyedRlcPrepArgs {
    RlcPrepArgs<C> r;             // n = items (stride of pa / pb), n_pad = n_pos, dig [16][n_pos], ppts [2][n_pos][2N]
    const uint32_t* pos_of_item;  // [n] position in the bv order, BV_NONE: not grouped
};
template <class C>
struct KeyedRlcPrep {
    static __host__ __device__ void run(const KeyedRlcPrepArgs<C>& ka, size_t i) {
        constexpr int N = C::FpP::N;
        const RlcPrepArgs<C>& a = ka.r;
        const uint32_t pos = ka.pos_of_item[i];
        if (pos == BV_NONE) return;
        uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        G1Aff<C> p = g1a_inf<C>(), q = g1a_inf<C>();
        bool in = a.gate_arr[i] == (int8_t)a.gate;
        if (in) {
            if (a.canonical) {
                p = g1a_load_canon_to_mont<C>(a.pa, a.n, i);
                q = g1a_load_canon_to_mont<C>(a.pb, a.n, i);
                in = g1a_on_curve<C>(p) && g1a_on_curve<C>(q);
            } else {
                p = g1a_load_mont<C>(a.pa, a.n, i);
                q = g1a_load_mont<C>(a.pb, a.n, i);
            }
        }
        if (in) {
            Sha256 s;
            sha256_init(s);
            for (int k = 0; k < 8; k++) sha256_word(s, a.seed[k]);
            sha256_u64be(s, (uint64_t)i);
            sha256_final(s, h);
        } else {
            p = g1a_inf<C>(); q = g1a_inf<C>();
        }
        for (int w = 0; w < 16; w++) a.dig[(size_t)w * a.n_pad + pos] = (uint8_t)(h[w >> 2] >> (8 * (w & 3)));
        g1a_store_mont<C>(a.ppts + (size_t)pos * 2 * N, 1, 0, p);
        g1a_store_mont<C>(a.ppts + (a.n_pad + (size_t)pos) * 2 * N, 1, 0, q);
    }
};

// host twin of k_pip_window_seg: lane per (set, window, group), sum of digit * P over the group's run by double-and-add --
// slow and obviously right.  The sum goes to the group's first segment, the identity to its other segments.
template <class C>
struct PipGroupSumsHost {
    static __host__ __device__ void run(const PipSegArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t TU = (size_t)a.M * a.NW * a.n_segs;
        const size_t g = t % a.n_groups, mw = t / a.n_groups;
        const size_t w = mw % (size_t)a.NW, m = mw / (size_t)a.NW;
        const uint32_t first = a.grp_run[2 * g], cnt = a.grp_run[2 * g + 1];
        G1Jac<C> acc = g1j_inf<C>();
        for (uint32_t k = 0; k < cnt; k++) {
            const uint32_t d = a.dig[w * a.n_pos + first + k];
            if (!d) continue;
            const G1Aff<C> P = g1a_load_mont<C>(a.ppts + (m * a.n_pos + first + k) * 2 * N, 1, 0);
            G1Jac<C> r = g1j_inf<C>();
            for (int bit = PIP_C - 1; bit >= 0; bit--) {
                r = g1j_dbl<C>(r);
                if ((d >> bit) & 1u) r = g1j_add_aff<C>(r, P);
            }
            acc = g1j_add<C>(acc, r);
        }
        const uint32_t s0 = a.grp_seg[2 * g], ns = a.grp_seg[2 * g + 1];
        for (uint32_t s = 0; s < ns; s++) g1j_store<C>(a.seg_sums, TU, mw * a.n_segs + s0 + s, s ? g1j_inf<C>() : acc);
    }
};

// lane per (set, window, group): the group's segment sums added and normalised for the group's virtual item of that window
template <class C>
struct PipGroupSums {
    static __host__ __device__ void run(const PipSegArgs<C>& a, size_t t) {
        constexpr int N = C::FpP::N;
        const size_t TU = (size_t)a.M * a.NW * a.n_segs, NV = (size_t)a.NW * a.n_groups;
        const size_t g = t % a.n_groups, mw = t / a.n_groups;
        const size_t w = mw % (size_t)a.NW, m = mw / (size_t)a.NW;
        const uint32_t s0 = a.grp_seg[2 * g], ns = a.grp_seg[2 * g + 1];
        G1Jac<C> acc = g1j_inf<C>();
        for (uint32_t s = 0; s < ns; s++) acc = g1j_add<C>(acc, g1j_load<C>(a.seg_sums, TU, mw * a.n_segs + s0 + s));
        g1a_store_mont<C>(a.out + m * 2 * N * NV, NV, g * (size_t)a.NW + w, g1j_to_aff<C>(acc));
    }
};

// lane per item, behind the groups' 16 combined checks: a pending item of a group whose checks all passed is Ok(true)
struct KeyedBvDecideArgs {
    size_t n;
    const uint32_t* item_group;   // [n] group of item i, BV_NONE: none
    const int8_t* verdicts;       // [16 G] verdict of virtual item g * 16 + w (0: failed or never ran)
    int8_t* status;
};
struct KeyedBvDecide {
    static __host__ __device__ void run(const KeyedBvDecideArgs& a, size_t i) {
        const uint32_t g = a.item_group[i];
        if (g == BV_NONE || a.status[i] != ST_PAIRING) return;
        bool all = true;
        for (int w = 0; w < 16; w++) all &= a.verdicts[(size_t)g * 16 + w] == 1;
        if (all) a.status[i] = 1;
    }
};

#if !defined(BBS_HOST_TWIN)
// k_pip_window with the tile taken from the segment table: one workgroup per (point set m, window w, segment); thread b owns
// bucket b.  A segment starts at a multiple of 4 of its digit row (runs start at multiples of 4, PIP_TILE is one) and a row
// is n_pos = a multiple of 4 long, so the 4-byte digit loads are aligned and stay inside the row.  Steps 1 - 4 are
// k_pip_window's; step 5 always stores the segment's window sum Jacobian (PipGroupSums adds a group's segments).
template <class C>
__global__ void __launch_bounds__(PIP_WG) k_pip_window_seg(PipSegArgs<C> a) {
    constexpr int N = C::FpP::N;
    static_assert(PIP_TILE % 4 == 0, "a segment starts at a multiple of 4");
    __shared__ __attribute__((aligned(16))) uint8_t s_dig[PIP_TILE];
    __shared__ uint16_t s_list[PIP_TILE];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_pt[4][3 * N];
    const int b = (int)threadIdx.x, lane = b & 63, wv = b >> 6;
    const size_t unit = blockIdx.x;                          // (m * NW + w) * n_segs + segment
    const uint32_t seg = (uint32_t)(unit % (size_t)a.n_segs);
    const size_t mw = unit / (size_t)a.n_segs;
    const int w = (int)(mw % (size_t)a.NW), m = (int)(mw / (size_t)a.NW);
    const size_t i0 = a.segs[3 * seg];
    // (the host builds the table inside the order; a segment that is not ends at the row's end and is never longer than a tile)
    size_t n_seg = a.segs[3 * seg + 1];
    if (n_seg > (size_t)PIP_TILE) n_seg = PIP_TILE;
    if (n_seg > (i0 < a.n_pos ? a.n_pos - i0 : 0)) n_seg = i0 < a.n_pos ? a.n_pos - i0 : 0;
    const int n_t = (int)n_seg;
    // 1. digits -> LDS: the 64-digit chunks the segment reaches into, zeros behind its last item
    {
        const uint8_t* row = a.dig + (size_t)w * a.n_pos + i0;
        uint32_t* s32 = reinterpret_cast<uint32_t*>(s_dig);
        for (int q = b; 4 * q < ((n_t + 63) & ~63); q += PIP_WG) {
            uint32_t v = 0;
            if (4 * q < n_t) {
                v = *reinterpret_cast<const uint32_t*>(row + 4 * q);
                const int rem = n_t - 4 * q;
                if (rem < 4) v &= (1u << (8 * rem)) - 1u;
            }
            s32[q] = v;
        }
    }
    __syncthreads();
    const int n_chunks = (n_t + 63) >> 6;
    auto members = [&](int q) -> uint64_t {
        const uint32_t d = s_dig[q * 64 + lane];
        uint64_t mk = ~(uint64_t)0;
#pragma unroll
        for (int j = 0; j < PIP_C; j++) {
            const uint64_t bj = __ballot((d >> j) & 1u);
            mk &= ((b >> j) & 1) ? bj : ~bj;
        }
        return b ? mk : (uint64_t)0;                         // digit 0 contributes nothing
    };
    // 2a. counts
    uint32_t cnt = 0;
    for (int q = 0; q < n_chunks; q++) cnt += (uint32_t)__popcll(members(q));
    // 2b. exclusive scan of the 256 counts
    uint32_t inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t start = inc - cnt;
    for (int k = 0; k < wv; k++) start += s_wave[k];
    // 2c. fill (item order)
    {
        uint32_t pos = start;
        for (int q = 0; q < n_chunks; q++) {
            uint64_t mk = members(q);
            while (mk) {
                const int l = __ffsll((unsigned long long)mk) - 1;
                mk &= mk - 1;
                s_list[pos++] = (uint16_t)(q * 64 + l);
            }
        }
    }
    __syncthreads();
    // 3. bucket sum
    G1Jac<C> acc = g1j_inf<C>();
    {
        const uint32_t* pts = a.ppts + ((size_t)m * a.n_pos + i0) * (2 * N);
        for (uint32_t k = 0; k < cnt; k++) {
            const uint4* e = reinterpret_cast<const uint4*>(pts + (size_t)s_list[start + k] * (2 * N));
            uint32_t wds[2 * N];
            static_assert((2 * N) % 4 == 0, "a point is a whole number of 16-byte vectors");
#pragma unroll
            for (int v = 0; v < (2 * N) / 4; v++) { const uint4 t = e[v]; wds[4 * v] = t.x; wds[4 * v + 1] = t.y; wds[4 * v + 2] = t.z; wds[4 * v + 3] = t.w; }
            G1Aff<C> pnt;
#pragma unroll
            for (int j = 0; j < N; j++) { pnt.x.v[j] = wds[j]; pnt.y.v[j] = wds[N + j]; }
            acc = g1j_add_aff<C>(acc, pnt);
        }
    }
    // 4a. suffix sums T_b = sum_{j >= b} B_j
#pragma unroll 1
    for (int off = 1; off < 64; off <<= 1) {
        const G1Jac<C> o = g1j_shfl_down<C>(acc, off);
        if (lane + off < 64) acc = g1j_add<C>(acc, o);
    }
    if (lane == 0) g1j_to_lds<C>(s_pt[wv], acc);
    __syncthreads();
    {
        G1Jac<C> above = g1j_inf<C>();
        for (int k = 3; k > wv; k--) above = g1j_add<C>(above, g1j_from_lds<C>(s_pt[k]));
        acc = g1j_add<C>(acc, above);
    }
    __syncthreads();
    // 4b. sum_{b >= 1} T_b
    if (b == 0) acc = g1j_inf<C>();
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {
        const G1Jac<C> o = g1j_shfl_down<C>(acc, off);
        if (lane < off) acc = g1j_add<C>(acc, o);
    }
    if (lane == 0) g1j_to_lds<C>(s_pt[wv], acc);
    __syncthreads();
    // 5. thread 0: the segment's window sum
    if (b == 0) {
        for (int k = 1; k < 4; k++) acc = g1j_add<C>(acc, g1j_from_lds<C>(s_pt[k]));
        g1j_store<C>(a.seg_sums, (size_t)a.M * a.NW * a.n_segs, unit, acc);
    }
}
#endif

// generic digits for the unit-parity primitive: 256-bit canonical scalars -> 32 byte digits
struct PipDigitArgs { size_t n, n_pad; const uint32_t* scal; /* [8][n] */ const int8_t* status; uint8_t* dig; /* [32][n_pad] */ };
struct PipDigits {
    static __host__ __device__ void run(const PipDigitArgs& a, size_t i) {
        for (int w = 0; w < 32; w++) {
            const uint32_t l = a.scal[(size_t)(w >> 2) * a.n + i];
            a.dig[(size_t)w * a.n_pad + i] = a.status[i] != 1 ? 0 : (uint8_t)(l >> (8 * (w & 3)));
        }
    }
};

// canonical affine points -> Montgomery, on-curve check (status -41, the item then contributes nothing)
template <class C>
struct PipPrep {
    const uint32_t* pts_c; uint32_t* pts; int8_t* status; size_t n;     // pts: [n][2N] item-major
    static __host__ __device__ void run(const PipPrep<C>& a, size_t i) {
        G1Aff<C> p = g1a_inf<C>();
        if (a.status[i] == ST_PENDING) {
            p = g1a_load_canon_to_mont<C>(a.pts_c, a.n, i);
            if (!g1a_on_curve<C>(p)) { a.status[i] = -41; p = g1a_inf<C>(); }
            else a.status[i] = 1;
        }
        g1a_store_mont<C>(a.pts + i * 2 * C::FpP::N, 1, 0, p);
    }
};

}  // namespace bbs
