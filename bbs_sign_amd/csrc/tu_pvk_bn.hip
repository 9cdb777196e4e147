// explicit instantiation: keyed proof_verify for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_pv.hpp"
template int pv_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint64_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, bbs_job**, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, const uint32_t*);
