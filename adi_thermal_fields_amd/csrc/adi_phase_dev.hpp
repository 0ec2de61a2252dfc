// adi_phase_dev.hpp -- the latent-heat law as the kernels take it, shared by adi_phase.hip (one law for the grid) and
// adi_matmap_phase.hip (one law per material): the record, the host constants of include/adi_hip.h ("Latent heat") and the clamp.
#pragma once
#include <math.h>

#include "adi_brick_dev.hpp"

namespace adi {

// the law as the kernels take it: the host constants of the header, each one fp64 operation
struct PhaseLaw {
    double cp, L, Ts, Tl;
    double dT, Hs, Hl, cm;
};

__device__ __forceinline__ double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// ADI_OK and the law as the kernels take it, or the first rule of the header the arguments break
inline int make_phase_law(const char *who, const adi_phase_change &s, double cp, PhaseLaw *w)
{
#pragma clang fp contract(off)
    ADI_REQUIRE(isfinite(s.latent_heat) && isfinite(s.T_solidus) && isfinite(s.T_liquidus),
                "%s: latent_heat, T_solidus or T_liquidus not finite", who);
    ADI_REQUIRE(s.latent_heat > 0.0, "%s: latent_heat must be > 0", who);
    ADI_REQUIRE(s.T_liquidus > s.T_solidus, "%s: T_liquidus must be above T_solidus", who);
    ADI_REQUIRE(isfinite(cp) && cp > 0.0, "%s: cp must be finite and > 0", who);
    w->cp = cp; w->L = s.latent_heat; w->Ts = s.T_solidus; w->Tl = s.T_liquidus;
    w->dT = w->Tl - w->Ts;
    w->Hs = cp * w->Ts;
    const double hl = cp * w->Tl;
    w->Hl = hl + w->L;
    const double r = w->L / w->dT;
    w->cm = cp + r;
    ADI_REQUIRE(isfinite(w->dT) && isfinite(w->Hl) && isfinite(w->cm), "%s: the law overflows fp64", who);
    return ADI_OK;
}

}  // namespace adi
