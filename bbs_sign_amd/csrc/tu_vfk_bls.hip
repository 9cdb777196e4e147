// explicit instantiation: keyed verify for BlsCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_vf.hpp"
template int vf_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const VfIn&, bbs_job**);
