// explicit instantiation: keyed sign for BlsCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_sg.hpp"
template int sg_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const SgIn&, bbs_job**);
