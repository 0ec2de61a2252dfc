// adi_sweep_strided_x.hip -- the FAST kernel of the strided-axis sweeps (adi_strided_fast.hpp) with 20, 24 and 28 rows per
// thread: lines of 320 / 384 / 448 rows (16 segments, 256-thread workgroups) and 640 / 768 / 896 rows (32 segments).  With 16
// or 32 rows per thread those lines fill 20 - 28 of 32 segment slots and the rest of every workgroup is padding (strided_plan).
// A translation unit of its own so that the build stays parallel.
#include "adi_strided_fast.hpp"

namespace adi {

void strided_fast_exact(int mf, bool has_dir, bool has_q, const StridedPlan &P, const StridedCall &c)
{
    launch_strided_exact(RowsFastX(), mf, has_dir, has_q, P, c);
}

}  // namespace adi
