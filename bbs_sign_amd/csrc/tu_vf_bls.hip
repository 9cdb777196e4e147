// explicit instantiation: vf for BlsCurve
#include "op_vf.hpp"
template int vf_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const VfIn&, bbs_job**);
