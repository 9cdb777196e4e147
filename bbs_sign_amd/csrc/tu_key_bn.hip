// explicit instantiation: key registration for BnCurve
#include "op_key.hpp"
template int8_t Ctx<BnCurve>::host_key_entry(const uint8_t*, bool, const uint8_t*, KeyEntry<BnCurve>&, uint8_t*, int8_t*) const;
template int Ctx<BnCurve>::key_build(KeyEntry<BnCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, bool, int8_t*, uint8_t*, int8_t*);
template int Ctx<BnCurve>::add_keys(bool, size_t, const uint8_t*, const int8_t*, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
template int selftest_key_entries<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const int8_t*, const uint8_t*, int, uint8_t*, int8_t*, uint8_t*);
