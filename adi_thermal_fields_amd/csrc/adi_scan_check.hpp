// adi_scan_check.hpp -- the argument checks every entry point that takes a scan path's segment table shares (adi_scan.hip,
// adi_bead.hip): what can be said of a path without its table, the rules of a host table, and the grid.  Host code; each
// returns ADI_OK or ADI_ERR_ARG with the message set, `fn` naming the entry.
#pragma once
#include <cmath>

#include "adi_common.hpp"
#include "adi_scan_eval.hpp"

namespace adi {

inline int scan_check_path(int K, double t_end, const char *fn)
{
    ADI_REQUIRE(K >= 1, "%s: a path needs at least one segment (K = %d)", fn, K);
    ADI_REQUIRE(K <= ADI_SCAN_MAX_SEGMENTS, "%s: K = %d segments, at most %d", fn, K, ADI_SCAN_MAX_SEGMENTS);
    ADI_REQUIRE(std::isfinite(t_end), "%s: non-finite t_end", fn);
    return ADI_OK;
}

// the host table: finite, t_begin ascending, t_end after the last begin, unit directions, speed >= 0, power >= 0
inline int scan_check_rows(const double *tab, int K, double t_end, const char *fn)
{
    ADI_REQUIRE(tab != nullptr, "%s: null segment table", fn);
    for (int k = 0; k < K; ++k) {
        const double *s = tab + (long)k * kScanCols;
        for (int c = 0; c < kScanCols; ++c) ADI_REQUIRE(std::isfinite(s[c]), "%s: segment %d: non-finite entry", fn, k);
        ADI_REQUIRE(scan_t_next(tab, K, t_end, k) > s[0],
                    k + 1 < K ? "%s: segment %d: t_begin does not ascend" : "%s: segment %d: t_end is not after the last t_begin",
                    fn, k);
        ADI_REQUIRE(fabs(hypot(s[4], s[5]) - 1.0) <= 1e-12, "%s: segment %d: the direction is not a unit vector", fn, k);
        ADI_REQUIRE(s[6] >= 0.0, "%s: segment %d: speed < 0", fn, k);
        ADI_REQUIRE(s[7] >= 0.0, "%s: segment %d: power < 0", fn, k);
    }
    return ADI_OK;
}

inline int scan_check_grid(int nx, int ny, int nz, double dx, const char *fn)
{
    ADI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "%s: bad grid %d x %d x %d", fn, nx, ny, nz);
    ADI_REQUIRE(std::isfinite(dx) && dx > 0.0, "%s: bad dx", fn);
    return ADI_OK;
}

}  // namespace adi
