// explicit instantiation: batched key generation for BnCurve
#include "op_kg.hpp"
template int key_gen_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*, uint8_t*, uint8_t*, int8_t*);
template int sk_to_pk_batch<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*, uint8_t*, int8_t*);
template int add_secret_keys<BnCurve>(Ctx<BnCurve>*, bool, size_t, const uint8_t*, int8_t*, uint8_t*, int8_t*, uint32_t*);
