// explicit instantiation: keyed verify for BlsCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_vf.hpp"
template int vf_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const uint8_t*, const uint8_t*, const uint64_t*, const uint8_t*, const uint64_t*, bbs_job**, const uint8_t*, const uint8_t*, const uint64_t*, const uint32_t*);
