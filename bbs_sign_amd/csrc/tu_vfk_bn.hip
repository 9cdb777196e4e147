// explicit instantiation: keyed verify for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_vf.hpp"
template int vf_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const VfIn&, bbs_job**);
