// cyl_monitor_host_check.cpp -- a stand-alone program around the host twin of the cylindrical field monitor
// (adi_cyl_monitor_record_host): the kernels' index arithmetic, per-pair code and order of operations on the CPU, over the
// shapes of tests/cyl_monitor_cases.py, with every array allocated at exactly the size the header promises is touched.
// It is meant for a sanitizer build of the host code, which needs no GPU and makes no HIP call:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         adi_thermal_fields_amd/csrc/adi_cyl_monitor.hip scripts/cyl_monitor_host_check.cpp -o cyl_monitor_host_check
// and stands in for the two functions of the library the translation unit needs (adi::set_err, adi::err_buf).
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../include/adi_hip.h"

namespace adi {
static char g_err[512];
char *err_buf() { return g_err; }
int set_err(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace adi

struct Block {
    double t0, dt;
    long long n, slot, capacity;
};

static int run(int nr, int nphi, int nz, long pad, bool masked, bool with_extra, unsigned seed)
{
    const long sx = (long)nphi * nz + pad;
    const size_t cells = (size_t)(nr - 1) * sx + (size_t)nphi * nz;      // the last plane carries no padding
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> temp(-500.0, 1700.0), coin(0.0, 1.0);
    std::vector<double> T(cells), X(with_extra ? cells : 0);
    std::vector<uint8_t> act(masked ? cells : 0);
    // the whole grid, one cell (the last of all), across the seam, j1 = j0 + nphi, inside pairs, two overlapping boxes
    const int wrap0 = nphi - 1, wrap1 = nphi > 1 ? nphi + 1 : nphi, full0 = nphi > 1 ? 1 : 0;
    const int regions[][6] = {{0, nr, 0, nphi, 0, nz},
                              {nr - 1, nr, nphi - 1, nphi, nz - 1, nz},
                              {0, nr, wrap0, wrap1, 0, nz},
                              {0, nr, full0, full0 + nphi, 2, nz},
                              {0, nr, 0, nphi, 1, 3},
                              {0, nr, 0, nphi / 2 + 1, 0, nz / 2 + 1},
                              {nr / 2, nr, 0, nphi, nz / 4, nz}};
    const int nreg = 7;
    const int probes[][3] = {{0, 0, 0}, {nr - 1, nphi - 1, nz - 1}, {0, nphi - 1, nz % 2 ? nz - 2 : nz - 1}};
    const int nprobe = 3;
    const int capacity = 2, guard = 8;
    const long row_words = nprobe + (long)ADI_CYL_MONITOR_REGION_WORDS * nreg;
    const int64_t guard_word = 0x5a5a5a5a5a5a5a5aLL;
    std::vector<int64_t> store((capacity + 1) * row_words + 2 * guard, guard_word);
    double *log = (double *)(store.data() + guard);
    for (long w = 0; w < (capacity + 1) * row_words; ++w) log[w] = NAN;
    Block blk = {1.5, 0.25, 0, 0, capacity};
    long long seen = 0;
    for (int n = 0; n < 4; ++n) {
        for (size_t p = 0; p < cells; ++p) {
            T[p] = temp(rng);
            if (with_extra) X[p] = coin(rng) < 0.1 ? NAN : coin(rng);
            if (masked && coin(rng) < 0.3) act[p] = 1;                     // births: the active set only grows
        }
        const int rc = adi_cyl_monitor_record_host(&blk, T.data(), with_extra ? X.data() : nullptr,
                                                   masked ? act.data() : nullptr, nr, nphi, nz, sx, 0.03, 1.0e-3, nreg,
                                                   &regions[0][0], nprobe, &probes[0][0], log, capacity);
        if (rc != ADI_OK) {
            fprintf(stderr, "%d x %d x %d: error %d: %s\n", nr, nphi, nz, rc, adi::err_buf());
            return 1;
        }
        int64_t c0;
        memcpy(&c0, log + (blk.slot < capacity ? blk.slot : capacity) * row_words + nprobe, sizeof(c0));
        seen += c0;
        blk.n += 1;
        blk.slot += 1;
    }
    for (int g = 0; g < guard; ++g)
        if (store[g] != guard_word || store[store.size() - 1 - g] != guard_word) {
            fprintf(stderr, "%d x %d x %d: a guard word of the log was written\n", nr, nphi, nz);
            return 1;
        }
    printf("%4d x %3d x %5d  stride +%ld  %s  %s  active cells seen %lld\n", nr, nphi, nz, pad, masked ? "masked" : "all   ",
           with_extra ? "extra" : "     ", seen);
    return 0;
}

int main()
{
    const int shapes[][3] = {{3, 5, 7}, {2, 1, 36}, {1, 4, 130}, {5, 8, 129}, {2, 3, 1030}, {2, 2, 65540}};
    int bad = 0;
    unsigned seed = 1;
    for (const auto &s : shapes)
        for (long pad : {0L, 3L})
            for (bool masked : {false, true}) bad += run(s[0], s[1], s[2], pad, masked, seed % 3u != 0u, seed), ++seed;
    // what the checks refuse comes back as ADI_ERR_ARG without a touch of the arrays
    double x = 0.0, row[ADI_CYL_MONITOR_REGION_WORDS];
    Block blk = {0.0, 0.1, 0, 0, 1};
    const int whole[6] = {0, 1, 0, 1, 0, 1}, past[6] = {0, 1, 1, 2, 0, 1}, far[6] = {0, 1, 0, 3, 0, 1};
    bad += adi_cyl_monitor_record_host(&blk, &x, nullptr, nullptr, 1, 1, 1, 0, 0.0, 1.0, 1, whole, 0, nullptr, row, 1) != ADI_OK;
    bad += adi_cyl_monitor_record_host(&blk, &x, nullptr, nullptr, 1, 1, 1, 0, 0.0, 1.0, 1, past, 0, nullptr, row, 1) != ADI_ERR_ARG;
    bad += adi_cyl_monitor_record_host(&blk, &x, nullptr, nullptr, 1, 1, 1, 0, 0.0, 1.0, 1, far, 0, nullptr, row, 1) != ADI_ERR_ARG;
    bad += adi_cyl_monitor_record_host(&blk, &x, nullptr, nullptr, 1, 1, 1, 0, 0.0, 0.0, 1, whole, 0, nullptr, row, 1) != ADI_ERR_ARG;
    bad += adi_cyl_monitor_record_host(&blk, nullptr, nullptr, nullptr, 1, 1, 1, 0, 0.0, 1.0, 1, whole, 0, nullptr, row, 1) != ADI_ERR_ARG;
    printf(bad ? "FAILED\n" : "cyl_monitor_host_check: all clean\n");
    return bad ? 1 : 0;
}
