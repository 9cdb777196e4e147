// explicit instantiation: keyed proof_verify for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_pv.hpp"
template int pv_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const PvIn&, bbs_job**);
