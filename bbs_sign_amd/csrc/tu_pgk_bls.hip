// explicit instantiation: keyed proof_gen for BlsCurve (keyed.hpp; its own unit so that the build stays parallel)
#include "op_pg.hpp"
template int pg_upload<BlsCurve, true>(Ctx<BlsCurve>*, size_t, const PgIn&, bbs_job**);
