// adi_surface_loss.hip -- temperature-dependent surface loss of the Cartesian step: the C entry of the kernel and launcher of
// adi_surface_loss_dev.hpp.
#include "adi_surface_loss_dev.hpp"

using namespace adi;

extern "C" {

int adi_surface_loss_update(const adi_surface_loss *h_law, double Tinf, const double *d_T, const uint8_t *d_flags,
                            const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, double dx, double rho,
                            double cp, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream)
{
    return launch_surface_loss("adi_surface_loss_update", NoRatio(), h_law, Tinf, d_T, d_flags, d_bricks, nx, ny, nz, plane_stride,
                               dx, rho, cp, d_coeff, k_begin, k_end, full, stream);
}

}  // extern "C"
