// adi_sweep_strided_gc.hip -- the GENERAL kernels of the strided-axis sweeps (adi_strided_general.hpp) for packs built from
// per-face SCALARS (SweepScal::fconst, h_face_consts of include/adi_hip.h): the Robin coefficient / Neumann flux of a row
// exposed along the sweep axis follows from its flags byte, and these instantiations contain no load of coeff / qflux at
// all.  8 / 16 rows per thread, with and without the explicit stage folded in (they drain what the FAST kernels of
// adi_sweep_strided_fc.hip queue: surface tiles, Dirichlet cells).  A translation unit of its own: the build stays parallel.
#include "adi_strided_general.hpp"

namespace adi {

void strided_general_fc(int m, bool has_dir, bool has_q, bool fuse, const StridedPlan &P, unsigned ggrid, const StridedCall &c)
{
    by_rows(RowsGeneralBuilt(), m, [&](auto M) {
        by_variant(has_dir, has_q, [&](auto dir, auto q) {
            by_bool(fuse, [&](auto f) { launch_strided_general_t<M.value, dir.value, q.value, f.value, 1, false>(P, ggrid, c); });
        });
    });
}

}  // namespace adi
