// explicit instantiation: sg for BnCurve
#include "op_sg.hpp"
template int sg_upload<BnCurve>(Ctx<BnCurve>*, size_t, const SgIn&, bbs_job**);
