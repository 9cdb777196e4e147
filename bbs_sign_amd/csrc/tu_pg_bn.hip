// explicit instantiation: pg for BnCurve
#include "op_pg.hpp"
template int pg_upload<BnCurve>(Ctx<BnCurve>*, size_t, const PgIn&, bbs_job**);
