// adi_sweep_strided_fy.hip -- the FUSED explicit + axis-0 FAST kernel (adi_strided_fast.hpp, FUSE = true) with 9, 11, 13 and 15
// rows per thread: lines of 144 / 176 / 208 / 240 rows (16 segments) and 288 / 352 / 416 / 480 rows (32 segments); with
// adi_sweep_strided_fx.hip every multiple of 16 from 128 to 256 rows and every multiple of 32 from 256 to 512 is an exact fit,
// which is what the padded extents (adi_recommended_dims) round ragged lines up to.  Why these row counts, and what the unit
// instantiates (RowsFusedY of adi_cart_host.hpp; no Dirichlet cells, FC or not): see adi_sweep_strided_fx.hip.
#include "adi_strided_fast.hpp"

namespace adi {

void strided_fast_fused_exact_odd(int mf, bool has_q, const StridedPlan &P, const StridedCall &c)
{
    launch_strided_fused_exact(RowsFusedY(), mf, has_q, P, c);
}

}  // namespace adi
