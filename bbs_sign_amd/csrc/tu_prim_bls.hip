// explicit instantiation: prim for BlsCurve
#include "op_prim.hpp"
template int Ctx<BlsCurve>::set_generators(const uint8_t*, size_t, const uint8_t*, size_t);
template int h2s_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint8_t*, size_t, uint8_t*);
template int seeded_scalars_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, const uint32_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
template int msm_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, size_t, const uint8_t*, const uint8_t*, size_t, uint8_t*, int8_t*);
template int pairing_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, int8_t*);
template int selftest_f12<BlsCurve>(Ctx<BlsCurve>*, int, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*);
template int selftest_f12_batch<BlsCurve>(Ctx<BlsCurve>*, int, size_t, const uint8_t*, const uint8_t*, const int8_t*, int, int, uint8_t*, uint8_t*, int8_t*);
template int selftest_pairing_split<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, int, const int8_t*, const uint8_t*, uint8_t*, uint8_t*, int8_t*);
template int msm_pippenger<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, uint8_t*, int*, int8_t*);
template int proofs_from_octets_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint64_t*, uint8_t*, uint8_t*, uint64_t*, int8_t*);
template int g1_decompress_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
template int signatures_from_octets_batch<BlsCurve>(Ctx<BlsCurve>*, size_t, const uint8_t*, uint8_t*, int8_t*);
