// explicit instantiation: vf for BnCurve
#include "op_vf.hpp"
template int vf_upload<BnCurve>(Ctx<BnCurve>*, size_t, const VfIn&, bbs_job**);
