// monitor_plan_check.hip -- the host side of the field monitor on its own: the argument rules and the offset arithmetic of
// monitor_plan (csrc/adi_monitor_dev.hpp), walked over good and bad arguments by a program with its own main.  It makes no
// HIP call and needs no GPU; it is meant to be built with the host sanitizers and run on the CPU:
//
//     hipcc -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//           -I include -I adi_thermal_fields_amd/csrc scripts/monitor_plan_check.hip -o monitor_plan_check && ./monitor_plan_check
//
// Every (region, brick) record and every row word the plan hands out is written into buffers of exactly the size the caller
// is told to allocate, so an offset past the end is a sanitizer report, and the records of all regions must tile the partial
// buffer without a gap or an overlap.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "adi_hip.h"
#include "adi_common.hpp"
#include "adi_monitor_dev.hpp"

namespace adi {
static char g_err[512];
int set_err(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace adi

using namespace adi;

static int failures = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        if (!(cond)) { printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the good path: every record exactly once, every row word inside the log
static void walk(int nx, int ny, int nz, const std::vector<int> &regions, const std::vector<int> &probes, long capacity)
{
    const int nreg = (int)regions.size() / 6, nprobe = (int)probes.size() / 3;
    MonPlan P;
    long need = 0;
    for (int r = 0; r < nreg; ++r) {
        long nb = 1;
        for (int a = 0; a < 3; ++a) nb *= (regions[6 * r + 2 * a + 1] - 1) / 16 - regions[6 * r + 2 * a] / 16 + 1;
        need += nb;
    }
    EXPECT(monitor_plan(nx, ny, nz, 0, nreg, regions.data(), nprobe, nprobe ? probes.data() : nullptr, need * kMonWords - 1, capacity,
                        &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(nx, ny, nz, 0, nreg, regions.data(), nprobe, nprobe ? probes.data() : nullptr, need * kMonWords, capacity,
                        &P) == ADI_OK);
    EXPECT(P.records == need && P.row_words == nprobe + 6L * nreg);
    std::vector<unsigned char> hit((size_t)need * kMonWords, 0);
    for (int bi = P.box_lo[0]; bi < P.box_lo[0] + P.box_n[0]; ++bi)
        for (int bj = P.box_lo[1]; bj < P.box_lo[1] + P.box_n[1]; ++bj)
            for (int bk = P.box_lo[2]; bk < P.box_lo[2] + P.box_n[2]; ++bk)
                for (int r = 0; r < P.R.n; ++r) {
                    const MonRegions &R = P.R;
                    if (bi < R.blo[r][0] || bi >= R.blo[r][0] + R.bn[r][0] || bj < R.blo[r][1] || bj >= R.blo[r][1] + R.bn[r][1] ||
                        bk < R.blo[r][2] || bk >= R.blo[r][2] + R.bn[r][2])
                        continue;
                    const long nb = (long)R.bn[r][0] * R.bn[r][1] * R.bn[r][2];
                    const long n = ((long)(bi - R.blo[r][0]) * R.bn[r][1] + (bj - R.blo[r][1])) * R.bn[r][2] + (bk - R.blo[r][2]);
                    for (int q = 0; q < kMonWords; ++q) hit[(size_t)(kMonWords * R.off[r] + q * nb + n)] += 1;   // (k_monitor_reduce)
                }
    for (unsigned char h : hit) EXPECT(h == 1);
    EXPECT((P.box_lo[0] + P.box_n[0]) * 16 < nx + 16 && (P.box_lo[1] + P.box_n[1]) * 16 < ny + 16 &&
           (P.box_lo[2] + P.box_n[2]) * 16 < nz + 16);
    std::vector<double> log((size_t)(capacity + 1) * P.row_words, 0.0);
    for (long slot = 0; slot < capacity + 3; ++slot) {
        double *row = log.data() + (slot < capacity ? slot : capacity) * P.row_words;    // (k_monitor_finish)
        for (long w = 0; w < P.row_words; ++w) row[w] += 1.0;
    }
    EXPECT(log.back() == 3.0 && log.front() == 1.0);
}

int main()
{
    walk(23, 19, 37, {0, 23, 0, 19, 0, 37, 3, 20, 2, 17, 5, 31, 17, 20, 17, 19, 33, 36, 0, 3, 0, 3, 0, 3}, {6, 6, 6, 22, 18, 36}, 5);
    walk(560, 48, 48, {0, 560, 0, 48, 0, 48, 505, 540, 3, 47, 1, 48}, {}, 1);
    walk(16, 16, 16, {15, 16, 15, 16, 15, 16}, {15, 15, 15}, 2);
    {
        std::vector<int> eight;
        for (int r = 0; r < 8; ++r) { const int v[6] = {r, 40, 0, 40 - r, r, r + 1}; eight.insert(eight.end(), v, v + 6); }
        std::vector<int> many;
        for (int q = 0; q < 256; ++q) { const int v[3] = {q % 40, (q / 7) % 40, 39 - q % 40}; many.insert(many.end(), v, v + 3); }
        walk(40, 40, 40, eight, many, 3);
    }
    MonPlan P;
    const int reg[6] = {0, 20, 0, 20, 0, 40}, prb[3] = {1, 2, 3};
    EXPECT(monitor_plan(20, 20, 40, 0, 0, reg, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 9, reg, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 257, prb, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, nullptr, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 1, nullptr, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 1, prb, 1000, 0, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 39, 0, 1, reg, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);      // the region leaves the box
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 1, prb, 1000, 4, &P) == ADI_OK);
    const int far[3] = {0, 0, 40}, neg[3] = {-1, 0, 0}, empty[6] = {4, 4, 0, 20, 0, 40}, back[6] = {0, 20, 9, 3, 0, 40};
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 1, far, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, reg, 1, neg, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, empty, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(20, 20, 40, 0, 1, back, 1, prb, 1000, 4, &P) == ADI_ERR_ARG);
    const int line[6] = {0, 1, 0, 1, 0, 16 * 65535 + 1};
    EXPECT(monitor_plan(1, 1, 16 * 65535 + 1, 0, 1, line, 0, nullptr, 1L << 40, 4, &P) == ADI_ERR_ARG);
    EXPECT(monitor_plan(1, 1, 16 * 65535, 0, 1, line, 0, nullptr, 1L << 40, 4, &P) == ADI_ERR_ARG);     // (the region)
    const int line_ok[6] = {0, 1, 0, 1, 0, 16 * 65535};
    EXPECT(monitor_plan(1, 1, 16 * 65535, 0, 1, line_ok, 0, nullptr, 1L << 40, 4, &P) == ADI_OK && P.records == 65535);
    printf(failures ? "monitor_plan_check: %d FAILED\n" : "monitor_plan_check: ok\n", failures);
    return failures ? 1 : 0;
}
