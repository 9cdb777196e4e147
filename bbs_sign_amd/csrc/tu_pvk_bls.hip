// explicit instantiation: keyed proof_verify for BlsCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_pv.hpp"
template int pv_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const PvIn&, bbs_job**);
