// explicit instantiation: key registration for BlsCurve
#include "op_key.hpp"
template int8_t Ctx<BlsCurve>::host_key_entry(const uint8_t*, bool, const uint8_t*, KeyEntry<BlsCurve>&, uint8_t*, int8_t*, G2Aff<BlsCurve>*) const;
template int Ctx<BlsCurve>::key_build(KeyEntry<BlsCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, bool, int8_t*, uint8_t*, int8_t*, G2Aff<BlsCurve>*, size_t*);
template int Ctx<BlsCurve>::rebuild_lines();
template int Ctx<BlsCurve>::add_keys(bool, size_t, const uint8_t*, const int8_t*, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
template int Ctx<BlsCurve>::build_key_lens(const std::shared_ptr<const Ctx<BlsCurve>::KeySet>&, const std::shared_ptr<const Ctx<BlsCurve>::KeyLenSet>&, size_t,
                                               std::shared_ptr<const Ctx<BlsCurve>::KeyLenSet>&);
template int Ctx<BlsCurve>::set_keyed_mixed_lengths(int);
template int selftest_key_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
template int job_keys_prepare<BlsCurve>(Ctx<BlsCurve>*, rt::Stream&, JobKeys<BlsCurve>&, bool, uint32_t, const std::function<void*(size_t)>&, std::shared_ptr<const void>&);
template int job_keys_gate<BlsCurve>(rt::Stream&, const JobKeys<BlsCurve>&, bool, size_t, const uint32_t*, int8_t*);
template int selftest_key_len_rows<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, int, uint8_t*, int8_t*);
template int selftest_job_key_cache_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*);
template int selftest_key_domain_entries<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
