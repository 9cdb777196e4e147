// explicit instantiation: pg for BlsCurve
#include "op_pg.hpp"
template int pg_upload<BlsCurve>(Ctx<BlsCurve>*, size_t, const PgIn&, bbs_job**);
