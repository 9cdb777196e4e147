// Keyed verification (bbs_ctx_set_public_keys, bbs_*_keyed_*): every item of a batch names one key of the context's KEY SET
// instead of the context's single public key.  Only two things of a verification depend on the key: the Miller-loop line
// table of W = pk and the midstate of the domain hash.  A key-set entry (stages_common.hpp KeyEntry) holds both; everything else (the fixed-base window
// tables, BP2's line table, the Frobenius constants) stays in CtxConsts and is shared by all keys.
//
// Pairing order.  The six-lane pairing kernel (PairDist) reads W's line entries with SCALAR loads: the table is the same
// for the ten items of a wavefront.  The host sorts a keyed batch by key (stable counting sort) into a slot -> item map:
//   * first, whole wavefronts of ONE key (floor(c / 10) per key with c items): the key-uniform body -- the key is made
//     wave-uniform with readfirstlane, the line loads stay scalar, the body is PairDist's plus the slot -> item lookup;
//   * then the c mod 10 remaining items of every key, packed ten per wavefront: the mixed body -- each six-lane group
//     reads its own key's lines with vector loads.
// ONE launch covers both (PairDistKeyed picks the body per wavefront): as two launches on the job's pairing stream the
// mixed wavefronts waited for the whole uniform launch, a second wavefront-time on the job's critical path (measured: 0.70
// of the single-key rate on the headline loop).
// Items keep their own index for points, gate and output; the slot map only decides which lanes compute which item.
// DESIGN.md 8 has the layout and the measured registers and times.
#pragma once
#include "stages.hpp"

namespace bbs {

constexpr uint32_t KEY_NONE = 0xFFFFFFFFu;     // item whose key index is unknown or names a refused key
constexpr int KEY_SLOTS_PER_WAVE = 10;         // == GRP_PER_WAVE (pairing_dist.hpp)

// items with KEY_NONE are decided at ingest: BBS_ST_UNKNOWN_KEY, never computed (runs behind the ingest stage)
struct KeyGateArgs { size_t n; const uint32_t* kidx; int8_t* status0; };
struct KeyGate {
    static __host__ __device__ void run(const KeyGateArgs& a, size_t i) {
        if (a.kidx[i] == KEY_NONE) a.status0[i] = (int8_t)BBS_ST_UNKNOWN_KEY;
    }
};

// The domain of a keyed item: the scalar stages in their Keyed / KeyedMixed forms (stages_common.hpp DomainSrc, form_domain;
// stages_*.hpp *ScalarsIn), instantiated from the keyed translation units only.
//
// Keyed sign (bbs_*sign*_keyed_*): item i under key kidx[i] of the context's key set AND its signing set (stages_sg.hpp
// sign_key_row).  The gate decides every item that has no secret row before the scalar stage runs: KEY_NONE as KeyGate does,
// KEY_NO_SECRET (an accepted key that was registered public-only) as BBS_ST_NO_SECRET_KEY -- neither ever indexes the signing
// set, a midstate or a prefix.
constexpr uint32_t KEY_NO_SECRET = 0xFFFFFFFEu;
struct SignKeyGate {
    static __host__ __device__ void run(const KeyGateArgs& a, size_t i) {
        const uint32_t k = a.kidx[i];
        if (k == KEY_NONE) a.status0[i] = (int8_t)BBS_ST_UNKNOWN_KEY;
        else if (k == KEY_NO_SECRET) a.status0[i] = (int8_t)BBS_ST_NO_SECRET_KEY;
    }
};

// the keyed pairing step: e(Pa, W_key(i)) * e(+-Pb, BP2) == 1 for the items of the slots [0, n_slots)
template <class C>
struct PairKeyedArgs {
    PairArgs<C> p;               // points, gate, output of the job (batch_ok unused: keyed jobs do not batch-verify)
    const KeyEntry<C>* keys;
    const uint32_t* kidx;        // [n] key of item i
    const uint32_t* slot_item;   // [n_slots] pairing order: slot -> item
    const uint32_t* wave_key;    // [n_uni / 10] key of uniform wavefront w
    size_t n_uni;                // slots [0, n_uni): key-uniform wavefronts (a multiple of 10); [n_uni, n_slots): mixed
    size_t n_slots;
};
template <class C>
BBS_HD uint32_t pair_keyed_key(const PairKeyedArgs<C>& ka, size_t s, size_t i) {
    return s < ka.n_uni ? ka.wave_key[s / KEY_SLOTS_PER_WAVE] : ka.kidx[i];
}

// host twin: one lane per (pair, slot), same item / key lookup as the device kernels; PairFinal follows per item
template <class C>
struct PairMillerKeyed {
    static __host__ __device__ void run(const PairKeyedArgs<C>& ka, size_t t) {
        constexpr int N = C::FpP::N;
        const PairArgs<C>& a = ka.p;
        const size_t n = a.n, ns = ka.n_slots;
        const int pair = (int)(t / ns);
        const size_t s = t - (size_t)pair * ns;
        const size_t i = ka.slot_item[s];
        if (a.gate_arr[i] != a.gate) return;
        G1Aff<C> P = pair_load_point<C>(a, pair == 0 ? a.pa : a.pb, i);
        if (pair == 1 && a.negate_b) P = g1a_neg<C>(P);
        const LineTable<C>& tab = pair == 0 ? ka.keys[pair_keyed_key<C>(ka, s, i)].tab : a.cc->tab_bp2;
        f12_store<C>(a.fmiller + (size_t)pair * 12 * N * n, n, i, miller_one_pair<C>(tab, P, a.cc->sched));
    }
};

#if !defined(BBS_HOST_TWIN)
static_assert(KEY_SLOTS_PER_WAVE == GRP_PER_WAVE, "the host cuts the pairing order into wavefronts of GRP_PER_WAVE items");
// PairDist over a slot map.  UNIFORM: every slot of the wavefront has the key wave_key[wave] -- read once, made
// wave-uniform, so W's line entries are scalar loads exactly as in PairDist.  Mixed: each six-lane group reads the lines of
// its own item's key (vector loads).
template <class C, bool UNIT, bool UNIFORM>
__device__ __forceinline__ void pair_dist_keyed(const PairKeyedArgs<C>& ka, size_t t) {
    const PairArgs<C>& a = ka.p;
    const int lane = (int)(t & 63);
    const int grp = pair6_group(lane);
    if (grp < 0) return;
    const size_t s = pair6_item(t >> 6, grp);
    if (s >= ka.n_slots) return;
    const size_t i = ka.slot_item[s];
    if (a.gate_arr[i] != a.gate) return;
    const Lane6 L = pair6_lanes(lane, grp);
    const LineTable<C>* tw;
    if constexpr (UNIFORM) tw = &ka.keys[__builtin_amdgcn_readfirstlane(ka.wave_key[t >> 6])].tab;
    else tw = &ka.keys[ka.kidx[i]].tab;
    G1Aff<C> Pa = pair_load_point<C>(a, a.pa, i);
    G1Aff<C> Pb = pair_load_point<C>(a, a.pb, i);
    if (a.negate_b) Pb = g1a_neg<C>(Pb);
    const bool one = pair6_product_is_one<C, UNIT>(L, a.cc, tw, Pa, Pb);
    if (L.m == 0) a.out[i] = one ? 1 : 0;
}
// UNIT: the form of every table of the key set and of BP2's (one form per context: runtime.hpp Ctx::rebuild_lines)
template <class C, bool UNIT>
struct PairDistKeyed {
    static constexpr int WAVES_PER_EU = PAIR_WAVES;
    static __device__ void run(const PairKeyedArgs<C>& ka, size_t t) {
        if ((t >> 6) * GRP_PER_WAVE < ka.n_uni) pair_dist_keyed<C, UNIT, true>(ka, t);     // (uniform over the wavefront)
        else pair_dist_keyed<C, UNIT, false>(ka, t);
    }
};
#endif

}  // namespace bbs
