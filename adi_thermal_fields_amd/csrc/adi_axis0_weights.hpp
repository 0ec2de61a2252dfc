// adi_axis0_weights.hpp -- the weights of the uniform axis-0 line of the slab decomposition, on the host (no HIP call):
//     w = c * tridiag(-tg, 1+2tg, -tg)^-1 e_0   (n x n),   tg = theta * gam,
// c = 1 for the dot products of pass A (adi_axis0_dots_setup), c = tg for the decaying homogeneous solution of the deferred
// form (adi_axis0_deferred_setup).  Both entries upload what this builds; adi_axis0_weights_host shows it to a CPU test.
#pragma once
#include <vector>

namespace adi {

// Thomas on c * e_0 in long double, rounded to double.  reach != nullptr: entries <= tol are stored as exactly 0 and *reach
// is the number of entries kept (w decreases monotonically: exactly 0 beyond its reach); reach == nullptr: nothing is cut.
inline void axis0_weights(int n, double theta, double gam, bool times_tg, double *w, double tol = 0.0, int *reach = nullptr)
{
    const long double tg = (long double)theta * (long double)gam, b = 1.0L + 2.0L * tg;
    const long double c = times_tg ? tg : 1.0L;
    std::vector<long double> cp(n), x(n);
    long double piv = b;
    cp[0] = -tg / piv; x[0] = c / piv;
    for (int i = 1; i < n; ++i) {
        piv = b + tg * cp[i - 1];
        cp[i] = -tg / piv;
        x[i] = (tg * x[i - 1]) / piv;
    }
    for (int i = n - 2; i >= 0; --i) x[i] -= cp[i] * x[i + 1];
    for (int i = 0; i < n; ++i) w[i] = (double)x[i];
    if (reach == nullptr) return;
    *reach = 0;
    for (int i = 0; i < n; ++i) {
        if (w[i] > tol) *reach = i + 1; else w[i] = 0.0;
    }
}

}  // namespace adi
