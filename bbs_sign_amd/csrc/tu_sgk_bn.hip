// explicit instantiation: keyed sign for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_sg.hpp"
template int sg_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const SgIn&, bbs_job**);
