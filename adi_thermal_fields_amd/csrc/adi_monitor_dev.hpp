// adi_monitor_dev.hpp -- what the two kernels of the field monitor (adi_monitor.hip) and its host side share: the regions as
// they travel by value, and the plan a record is launched from -- every argument rule of adi_monitor_record, the brick boxes
// of the regions, their offsets in the partial buffer and the launch box.  The plan is host arithmetic alone (no HIP call),
// so a stand-alone program can run it under a sanitizer (scripts/monitor_plan_check.hip).
#pragma once
#include "adi_history_dev.hpp"

namespace adi {

constexpr int kMonRegions = ADI_MONITOR_MAX_REGIONS;
constexpr int kMonWords = ADI_MONITOR_PARTIAL_WORDS;    // per (region, brick): sum_T, sum_wT, sum_extra, key_min, key_max, cells
static_assert(ADI_MONITOR_REGION_WORDS == 6 && ADI_MONITOR_PARTIAL_WORDS == 6, "monitor row layout");

struct MonRegions {
    int n;
    int lo[kMonRegions][3], hi[kMonRegions][3];   // cells, half open
    int blo[kMonRegions][3], bn[kMonRegions][3];  // the region's brick box: first brick, bricks per axis
    long off[kMonRegions];                        // (region, brick) records ahead of the region's in the partial buffer
};

struct MonWeights {
    double w[ADI_MATMAP_MAX];
};

struct MonPlan {
    Lay L;
    MonRegions R;
    int box_lo[3], box_n[3];     // the launch box in bricks: the bounding box of the regions' brick boxes
    long records;                // (region, brick) records in all
    long row_words;
};

inline int monitor_plan(int nx, int ny, int nz, long plane_stride, int nreg, const int *h_regions, int nprobe,
                        const int *h_probes, long partial_words, long capacity, MonPlan *P)
{
    ADI_REQUIRE(nreg >= 1 && nreg <= ADI_MONITOR_MAX_REGIONS, "adi_monitor_record: %d regions (1 to %d)", nreg,
                ADI_MONITOR_MAX_REGIONS);
    ADI_REQUIRE(nprobe >= 0 && nprobe <= ADI_MONITOR_MAX_PROBES, "adi_monitor_record: %d probes (0 to %d)", nprobe,
                ADI_MONITOR_MAX_PROBES);
    ADI_REQUIRE(h_regions != nullptr && (nprobe == 0 || h_probes != nullptr), "adi_monitor_record: null argument");
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "adi_monitor_record: capacity %ld is not in [1, 2^31)", capacity);
    if (int rc = make_lay(nx, ny, nz, plane_stride, &P->L)) return rc;
    const int n[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a)
        ADI_REQUIRE((n[a] + kBrick - 1) / kBrick <= 65535, "adi_monitor_record: box of %d x %d x %d is too large", nx, ny, nz);
    P->R.n = nreg;
    long off = 0;
    int blo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, bhi[3] = {-1, -1, -1};
    for (int r = 0; r < kMonRegions; ++r) {
        for (int a = 0; a < 3; ++a) {
            if (r < nreg) {
                const int lo = h_regions[6 * r + 2 * a], hi = h_regions[6 * r + 2 * a + 1];
                ADI_REQUIRE(lo < hi, "adi_monitor_record: region %d is empty along axis %d: [%d, %d)", r, a, lo, hi);
                ADI_REQUIRE(lo >= 0 && hi <= n[a], "adi_monitor_record: region %d leaves the box along axis %d: [%d, %d)", r, a,
                            lo, hi);
                P->R.lo[r][a] = lo; P->R.hi[r][a] = hi;
                P->R.blo[r][a] = lo / kBrick;
                P->R.bn[r][a] = (hi - 1) / kBrick - lo / kBrick + 1;
                if (P->R.blo[r][a] < blo[a]) blo[a] = P->R.blo[r][a];
                if ((hi - 1) / kBrick > bhi[a]) bhi[a] = (hi - 1) / kBrick;
            } else {
                P->R.lo[r][a] = 0; P->R.hi[r][a] = 0; P->R.blo[r][a] = 0; P->R.bn[r][a] = 0;
            }
        }
        P->R.off[r] = off;
        off += (long)P->R.bn[r][0] * P->R.bn[r][1] * P->R.bn[r][2];
    }
    for (int q = 0; q < nprobe; ++q)
        for (int a = 0; a < 3; ++a)
            ADI_REQUIRE(h_probes[3 * q + a] >= 0 && h_probes[3 * q + a] < n[a],
                        "adi_monitor_record: probe %d lies outside the box along axis %d: %d", q, a, h_probes[3 * q + a]);
    P->records = off;
    ADI_REQUIRE(partial_words >= off * kMonWords, "adi_monitor_record: %ld words of partials, %ld needed", partial_words,
                off * kMonWords);
    for (int a = 0; a < 3; ++a) { P->box_lo[a] = blo[a]; P->box_n[a] = bhi[a] - blo[a] + 1; }
    P->row_words = (long)nprobe + (long)ADI_MONITOR_REGION_WORDS * nreg;
    return ADI_OK;
}

}  // namespace adi
