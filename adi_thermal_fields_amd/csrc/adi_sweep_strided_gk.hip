// adi_sweep_strided_gk.hip -- the GENERAL kernels of the strided-axis sweeps (adi_strided_general.hpp) that carry the deferred
// interface correction of a slab decomposition (adi_sweep_corrected, SweepScal::c_*: the axis-1 sweep of a slab adds the
// rank-two update of the sharded-axis solve to every value it loads).  Only these instantiations
// contain corr_apply; the ordinary sweeps of adi_sweep_strided.hip / _gc.hip are compiled without it.  8 / 16 rows per
// thread, never fused; the source of the coefficients is decided at run time here (a slab-only path).
#include "adi_strided_general.hpp"

namespace adi {

void strided_general_corr(int m, bool has_dir, bool has_q, const StridedPlan &P, unsigned ggrid, const StridedCall &c)
{
    by_rows(RowsGeneralBuilt(), m, [&](auto M) {
        by_variant(has_dir, has_q, [&](auto dir, auto q) {
            launch_strided_general_t<M.value, dir.value, q.value, false, 0, true>(P, ggrid, c);
        });
    });
}

}  // namespace adi
