// explicit instantiation: key registration for BnCurve
#include "op_key.hpp"
template int8_t Ctx<BnCurve>::host_key_entry(const uint8_t*, bool, const uint8_t*, KeyEntry<BnCurve>&, uint8_t*, int8_t*, G2Aff<BnCurve>*) const;
template int Ctx<BnCurve>::key_build(KeyEntry<BnCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, bool, int8_t*, uint8_t*, int8_t*, G2Aff<BnCurve>*, size_t*);
template int Ctx<BnCurve>::rebuild_lines();
template int Ctx<BnCurve>::add_keys(bool, size_t, const uint8_t*, const int8_t*, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
template int Ctx<BnCurve>::build_key_lens(const std::shared_ptr<const Ctx<BnCurve>::KeySet>&, const std::shared_ptr<const Ctx<BnCurve>::KeyLenSet>&, size_t,
                                               std::shared_ptr<const Ctx<BnCurve>::KeyLenSet>&);
template int Ctx<BnCurve>::set_keyed_mixed_lengths(int);
template int selftest_key_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
template int job_keys_prepare<BnCurve>(Ctx<BnCurve>*, rt::Stream&, JobKeys<BnCurve>&, bool, uint32_t, const std::function<void*(size_t)>&, std::shared_ptr<const void>&);
template int job_keys_gate<BnCurve>(rt::Stream&, const JobKeys<BnCurve>&, bool, size_t, const uint32_t*, int8_t*);
template int selftest_key_len_rows<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, int, uint8_t*, int8_t*);
template int selftest_job_key_cache_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*);
template int selftest_key_domain_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
