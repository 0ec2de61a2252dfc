// adi_sweep_strided_fx.hip -- the FUSED explicit + axis-0 FAST kernel (adi_strided_fast.hpp, FUSE = true) with 10, 12 and 14
// rows per thread: lines of 160 / 192 / 224 rows (16 segments) and 320 / 384 / 448 rows (32 segments).  The fused kernel holds
// at most 16 rows per thread (its loader hands the k-halo columns round the 16 lanes of a DPP row and it sits at the 128-VGPR
// budget), so with 16 rows those lines fill 10 - 14 of 16 (20 - 28 of 32) segment slots of every workgroup: 127 - 164 Gcell/s
// against 195 - 200 at 256 / 512 rows.  No Dirichlet cells (those tiles would go to the GENERAL kernel anyway); with and without
// the coefficients taken from the flags (FC).  A translation unit of its own so that the build stays parallel.
#include "adi_strided_fast.hpp"

namespace adi {

void strided_fast_fused_exact(int mf, bool has_q, const StridedPlan &P, const StridedCall &c)
{
    launch_strided_fused_exact(RowsFusedX(), mf, has_q, P, c);
}

}  // namespace adi
