#pragma once
#include "job_form.hpp"
// ---- inputs of the four upload templates: one field per pointer of the C ABI, named as in include/bbs_sign_amd.h.  A field
// that is left null selects the form (core / octets / wire / keyed); the upload functions deduce it from that alone.
struct PvIn {
    const uint8_t* proofs_fixed = nullptr;      // core form: n records, with commitments / commit_off
    const uint8_t* commitments = nullptr;
    const uint64_t* commit_off = nullptr;
    const uint8_t* disclosed_msgs = nullptr;    // scalars; ignored when the messages come as raw bytes
    const uint64_t* dmsg_off = nullptr;         // disclosed messages per item, in messages (msg_item_off of the wire exports)
    const uint64_t* disclosed_idx = nullptr;
    const uint64_t* didx_off = nullptr;
    const uint8_t* headers = nullptr;
    const uint64_t* hdr_off = nullptr;
    const uint8_t* ph = nullptr;
    const uint64_t* ph_off = nullptr;
    // proof_octets / oct_off != nullptr: the wire form (bbs_proof_verify_octets_*): proofs_fixed / commitments / commit_off are
    // ignored, the proofs come as octet strings and are decoded on the device (codec_dev.hpp PvOctDecode / PvOctIngest)
    const uint8_t* proof_octets = nullptr;
    const uint64_t* oct_off = nullptr;
    // msg_byte_off != nullptr (wire form only): the disclosed messages arrive as RAW BYTES -- message t of the batch is
    // msg_bytes[msg_byte_off[t] .. msg_byte_off[t + 1]), dmsg_off counts messages per item as before, disclosed_msgs is
    // ignored -- and are mapped to scalars on the device (msg_to_scalars, interface_utilities.rs:76-88)
    const uint8_t* msg_bytes = nullptr;
    const uint64_t* msg_byte_off = nullptr;
    const uint32_t* key_index = nullptr;        // KEYED only: item i is verified under key key_index[i] of the context's key set
    // KEYED only, bbs_*_with_keys_*: the key set is THIS call's -- n_keys compressed strings, prepared by the job (job_form.hpp JobKeys)
    bool job_keys = false;
    size_t n_keys = 0;
    const uint8_t* pk_octets = nullptr;
};
struct VfIn {
    const uint8_t* signatures = nullptr;        // n records A || e
    const uint8_t* messages = nullptr;          // scalars; ignored when the messages come as raw bytes
    const uint64_t* msg_off = nullptr;          // messages per item, in messages (msg_item_off of the wire exports)
    const uint8_t* headers = nullptr;
    const uint64_t* hdr_off = nullptr;
    // signature_octets != nullptr: the wire form -- n strings compress(A) || e instead of the records `signatures`
    const uint8_t* signature_octets = nullptr;
    // msg_byte_off != nullptr: the messages arrive as RAW BYTES (message t of the batch = msg_bytes[msg_byte_off[t] ..
    // msg_byte_off[t + 1]), msg_off counts messages per item, messages is ignored) and are hashed to scalars on the device
    const uint8_t* msg_bytes = nullptr;
    const uint64_t* msg_byte_off = nullptr;
    const uint32_t* key_index = nullptr;        // KEYED only, as PvIn
    bool job_keys = false;                      // KEYED only, as PvIn
    size_t n_keys = 0;
    const uint8_t* pk_octets = nullptr;
};
struct SgIn {
    const uint8_t* messages = nullptr;
    const uint64_t* msg_off = nullptr;
    const uint8_t* headers = nullptr;
    const uint64_t* hdr_off = nullptr;
    // msg_byte_off != nullptr: raw messages, hashed to scalars on the device (see VfIn)
    const uint8_t* msg_bytes = nullptr;
    const uint64_t* msg_byte_off = nullptr;
    const uint32_t* key_index = nullptr;        // KEYED only: item i is signed under key key_index[i] of the context's signing set
};
struct PgIn {
    const uint8_t* signatures = nullptr;
    const uint8_t* messages = nullptr;
    const uint64_t* msg_off = nullptr;
    const uint64_t* disclosed_idx = nullptr;
    const uint64_t* didx_off = nullptr;
    const uint8_t* random_scalars = nullptr;
    const uint64_t* rnd_off = nullptr;
    const uint8_t* headers = nullptr;
    const uint64_t* hdr_off = nullptr;
    const uint8_t* ph = nullptr;
    const uint64_t* ph_off = nullptr;
    // signature_octets != nullptr: the signatures arrive as octet strings compress(A) || e (decoded and subgroup-checked on the
    // device, `signatures` ignored); msg_byte_off != nullptr: the messages arrive as raw bytes (see VfIn)
    const uint8_t* signature_octets = nullptr;
    const uint8_t* msg_bytes = nullptr;
    const uint64_t* msg_byte_off = nullptr;
    const uint32_t* key_index = nullptr;        // KEYED only: item i is derived under key key_index[i] of the context's key set
    bool job_keys = false;                      // KEYED only, as PvIn (bbs_*proof_gen*_with_keys_*)
    size_t n_keys = 0;
    const uint8_t* pk_octets = nullptr;
};
// declarations of the per-operation templates (defined in op_*.hpp, instantiated in tu_*.hip)
template <class C, bool KEYED = false> int pv_upload(Ctx<C>*, size_t, const PvIn&, bbs_job**);
template <class C, bool KEYED = false> int vf_upload(Ctx<C>*, size_t, const VfIn&, bbs_job**);
template <class C, bool KEYED = false> int sg_upload(Ctx<C>*, size_t, const SgIn&, bbs_job**);
template <class C, bool KEYED = false> int pg_upload(Ctx<C>*, size_t, const PgIn&, bbs_job**);
template <class C> int h2s_batch(Ctx<C>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*);
template <class C> int seeded_scalars_batch(Ctx<C>*, size_t, const uint8_t*, const uint64_t*, const uint32_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
template <class C> int msm_batch(Ctx<C>*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
template <class C> int selftest_f12(Ctx<C>*, int, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
template <class C> int selftest_f12_batch(Ctx<C>*, int, size_t, const uint8_t*, const uint8_t*, const int8_t*, int, int, uint8_t*, uint8_t*, int8_t*);
template <class C> int selftest_pairing_split(Ctx<C>*, size_t, const uint8_t*, const uint8_t*, int, const int8_t*, const uint8_t*, uint8_t*, uint8_t*, int8_t*);
template <class C> int pairing_batch(Ctx<C>*, size_t, const uint8_t*, const uint8_t*, int8_t*);
template <class C> int msm_pippenger(Ctx<C>*, size_t, const uint8_t*, const uint8_t*, uint8_t*, int*, int8_t*);
template <class C> int g1_decompress_batch(Ctx<C>*, size_t, const uint8_t*, uint8_t*, int8_t*);
template <class C> int signatures_from_octets_batch(Ctx<C>*, size_t, const uint8_t*, uint8_t*, int8_t*);
template <class C> int proofs_from_octets_batch(Ctx<C>*, size_t, const uint8_t*, const uint64_t*, uint8_t*, uint8_t*, uint64_t*, int8_t*);
template <class C> int selftest_key_entries(Ctx<C>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
extern template int pv_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const PvIn&, bbs_job**);
extern template int pv_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const PvIn&, bbs_job**);
extern template int pv_upload<BnCurve>(Ctx<BnCurve>*, size_t, const PvIn&, bbs_job**);
extern template int pv_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const PvIn&, bbs_job**);
extern template int vf_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const VfIn&, bbs_job**);
extern template int vf_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const VfIn&, bbs_job**);
extern template int vf_upload<BnCurve>(Ctx<BnCurve>*, size_t, const VfIn&, bbs_job**);
extern template int vf_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const VfIn&, bbs_job**);
extern template int sg_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const SgIn&, bbs_job**);
extern template int sg_upload<BnCurve>(Ctx<BnCurve>*, size_t, const SgIn&, bbs_job**);
extern template int sg_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const SgIn&, bbs_job**);
extern template int sg_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const SgIn&, bbs_job**);
extern template int pg_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const PgIn&, bbs_job**);
extern template int pg_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const PgIn&, bbs_job**);
extern template int pg_upload<BnCurve>(Ctx<BnCurve>*, size_t, const PgIn&, bbs_job**);
extern template int pg_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const PgIn&, bbs_job**);
extern template int Ctx<BlsCurve>::set_generators(const uint8_t*, size_t, const uint8_t*, size_t);
extern template int h2s_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*);
extern template int seeded_scalars_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint32_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
extern template int msm_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
extern template int pairing_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, int8_t*);
extern template int msm_pippenger<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, uint8_t*, int*, int8_t*);
extern template int g1_decompress_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int signatures_from_octets_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int proofs_from_octets_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, uint8_t*, uint8_t*, uint64_t*, int8_t*);
extern template int Ctx<BnCurve>::set_generators(const uint8_t*, size_t, const uint8_t*, size_t);
extern template int h2s_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*);
extern template int seeded_scalars_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint64_t*, const uint32_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
extern template int msm_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
extern template int pairing_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, int8_t*);
extern template int msm_pippenger<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, uint8_t*, int*, int8_t*);
extern template int g1_decompress_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int signatures_from_octets_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int proofs_from_octets_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint64_t*, uint8_t*, uint8_t*, uint64_t*, int8_t*);
extern template int selftest_f12<BlsCurve>(Ctx<BlsCurve>*, int, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
extern template int selftest_f12<BnCurve>(Ctx<BnCurve>*, int, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
extern template int selftest_f12_batch<BlsCurve>(Ctx<BlsCurve>*, int, size_t, const uint8_t*, const uint8_t*, const int8_t*, int, int, uint8_t*, uint8_t*, int8_t*);
extern template int selftest_pairing_split<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, int, const int8_t*, const uint8_t*, uint8_t*, uint8_t*, int8_t*);
extern template int selftest_f12_batch<BnCurve>(Ctx<BnCurve>*, int, size_t, const uint8_t*, const uint8_t*, const int8_t*, int, int, uint8_t*, uint8_t*, int8_t*);
extern template int selftest_pairing_split<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, int, const int8_t*, const uint8_t*, uint8_t*, uint8_t*, int8_t*);
extern template int Ctx<BlsCurve>::add_keys(bool, size_t, const uint8_t*, const int8_t*, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
extern template int Ctx<BlsCurve>::set_keyed_mixed_lengths(int);
extern template int Ctx<BlsCurve>::rebuild_lines();
extern template int selftest_key_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
extern template int Ctx<BnCurve>::add_keys(bool, size_t, const uint8_t*, const int8_t*, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
extern template int Ctx<BnCurve>::set_keyed_mixed_lengths(int);
extern template int Ctx<BnCurve>::rebuild_lines();
extern template int selftest_key_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
template <class C> int selftest_segmented_sums(Ctx<C>*, size_t, const uint8_t*, const uint8_t*, size_t, const uint64_t*, const uint64_t*, uint8_t*);
extern template int selftest_segmented_sums<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, size_t, const uint64_t*, const uint64_t*, uint8_t*);
extern template int selftest_segmented_sums<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, size_t, const uint64_t*, const uint64_t*, uint8_t*);
template <class C> int key_gen_batch(Ctx<C>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*, int8_t*);
template <class C> int sk_to_pk_batch(Ctx<C>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*, int8_t*);
template <class C> int add_secret_keys(Ctx<C>*, bool, size_t, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
extern template int add_secret_keys<BlsCurve>(Ctx<BlsCurve>*, bool, size_t, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
extern template int add_secret_keys<BnCurve>(Ctx<BnCurve>*, bool, size_t, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
extern template int key_gen_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*, int8_t*);
extern template int sk_to_pk_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*, int8_t*);
extern template int key_gen_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*, int8_t*);
extern template int sk_to_pk_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*, int8_t*);
template <class C> int selftest_key_len_rows(Ctx<C>*, size_t, const uint8_t*, int, uint8_t*, int8_t*);
extern template int selftest_key_len_rows<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, int, uint8_t*, int8_t*);
extern template int selftest_key_len_rows<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, int, uint8_t*, int8_t*);
template <class C> int selftest_job_key_cache_entries(Ctx<C>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*);
extern template int selftest_job_key_cache_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*);
extern template int selftest_job_key_cache_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*);
template <class C> int selftest_key_domain_entries(Ctx<C>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int selftest_key_domain_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
extern template int selftest_key_domain_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
