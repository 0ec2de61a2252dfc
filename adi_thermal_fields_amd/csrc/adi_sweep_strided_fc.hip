// adi_sweep_strided_fc.hip -- the FAST kernels of the strided-axis sweeps (adi_strided_fast.hpp) for packs built from per-face
// SCALARS (SweepScal::fconst, h_face_consts of include/adi_hip.h): the Robin coefficient / Neumann flux of a row exposed
// along the sweep axis follows from its flags byte, so these instantiations contain no load of coeff / qflux at all.  On a
// curved solid such a load can only be issued once the flags have arrived -- a second memory latency in every wave that
// holds a surface row -- and even its presence behind a run-time branch cost the 512^3 ellipsoid 0.02 ms per strided sweep.
// 8 / 16 / 32 rows per thread, no Dirichlet cells, with and without the explicit stage folded in; a translation unit of its
// own so that the build stays parallel.
#include "adi_strided_fast.hpp"

namespace adi {

void strided_fast_fc(int mf, bool has_q, bool fuse, const StridedPlan &P, const StridedCall &c)
{
    const StridedCall v = without_dir(c, has_q);
    by_rows(RowsFast(), mf, [&](auto m) {
        by_bool(has_q, [&](auto q) {
            // (32 rows per thread are never fused)
            by_bool(fuse && m.value <= kFuseMaxRows, [&](auto f) {
                launch_strided_fast_t<m.value, false, q.value, (f.value && m.value <= kFuseMaxRows), true>(P, v);
            });
        });
    });
}

}  // namespace adi
