// explicit instantiation: batched key generation for BlsCurve
#include "op_kg.hpp"
template int key_gen_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*, int8_t*);
template int sk_to_pk_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*, int8_t*);
template int add_secret_keys<BlsCurve>(Ctx<BlsCurve>*, bool, size_t, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
