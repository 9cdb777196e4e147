// explicit instantiation: pv for BlsCurve
#include "op_pv.hpp"
template int pv_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const PvIn&, bbs_job**);
