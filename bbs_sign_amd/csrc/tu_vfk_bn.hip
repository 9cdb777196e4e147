// explicit instantiation: keyed verify for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_vf.hpp"
template int vf_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const VfIn&, bbs_job**);
template int selftest_segmented_sums<BnCurve>(Ctx<BnCurve>*, size_t, const uint8_t*, const uint8_t*, size_t, const uint64_t*, const uint64_t*, uint8_t*);
