// explicit instantiation: keyed proof_gen for BnCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_pg.hpp"
template int pg_upload<BnCurve, true>(Ctx<BnCurve>*, size_t, const PgIn&, bbs_job**);
