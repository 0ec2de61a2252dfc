// adi_goldak_dev.hpp -- the pieces of Goldak's double ellipsoid every evaluator of the library shares (adi_source.hip, the
// Cartesian step; adi_scan_eval.hpp, the scan path; adi_cyl_source_dev.hpp, the cylindrical step), written once for the host
// and the device, fp64, no contraction.  q = amp * exp(-E), E the sum of one exponent term per axis, q = 0 exactly where
// E > ADI_SOURCE_E_CUT (include/adi_hip.h).  Host-only code may include this header without the HIP runtime.
#pragma once
#include <math.h>

#include "../../include/adi_hip.h"

#if defined(__HIPCC__)
#define ADI_GOLDAK_HD __host__ __device__ inline
#else
#define ADI_GOLDAK_HD inline
#endif

namespace adi {

// exponent term of one axis for offset o: 3 o^2 / L^2 with L the half-length of that axis (role- and side-dependent)
ADI_GOLDAK_HD double goldak_eterm(double o, double len)
{
#pragma clang fp contract(off)
    return 3.0 * (o * o) / (len * len);
}

// amplitude 6 sqrt(3) f eta P / (a b c pi^1.5) of the side with fraction f and length cl
ADI_GOLDAK_HD double goldak_amp(double f, double eta, double P, double a, double b, double cl)
{
#pragma clang fp contract(off)
    return (6.0 * sqrt(3.0) * f * eta * P) / (a * b * cl * pow(M_PI, 1.5));
}

// t_n + dt/2 of a parameter block: t_n = t0 + n*dt, computed from the integer counter (no accumulation, no fused
// multiply-add: the host's t0 + i*dt gives the same double)
ADI_GOLDAK_HD double goldak_tmid(double t0, double dt, unsigned long long n)
{
#pragma clang fp contract(off)
    const double tn = t0 + (double)n * dt;
    return tn + 0.5 * dt;
}

}  // namespace adi
