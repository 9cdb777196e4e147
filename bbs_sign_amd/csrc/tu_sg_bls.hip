// explicit instantiation: sg for BlsCurve
#include "op_sg.hpp"
template int sg_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const SgIn&, bbs_job**);
