// explicit instantiation: pv for BnCurve
#include "op_pv.hpp"
template int pv_upload<BnCurve>(Ctx<BnCurve>*, size_t, const PvIn&, bbs_job**);
