// adi_sweep_strided_y.hip -- the FAST kernel of the strided-axis sweeps (adi_strided_fast.hpp) with 18, 22, 26 and 30 rows per
// thread: lines of 288 / 352 / 416 / 480 rows (16 segments) and 576 / 704 / 832 / 960 rows (32 segments); with
// adi_sweep_strided_x.hip (20 / 24 / 28 rows) every multiple of 32 rows from 256 to 512 is an exact fit of the unfused strided
// sweeps too -- the lengths the padded extents (adi_recommended_dims) round ragged lines up to.
#include "adi_strided_fast.hpp"

namespace adi {

void strided_fast_exact2(int mf, bool has_dir, bool has_q, const StridedPlan &P, const StridedCall &c)
{
    launch_strided_exact(RowsFastY(), mf, has_dir, has_q, P, c);
}

}  // namespace adi
