// cyl_solid_host_check.cpp -- a stand-alone program around the host twins of the cylindrical step's solidification record
// (adi_cyl_solid_record_host, adi_cyl_solid_hot_seed_host): the kernel's per-cell code, neighbour arithmetic (the periodic seam,
// the box faces, the padded plane stride) and tile loop on the CPU, over the shapes of tests/cyl_solid_cases.py, with every
// array allocated at exactly the size the header promises is touched.  It is meant for a sanitizer build of the host code,
// which needs no GPU and makes no HIP call:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         adi_thermal_fields_amd/csrc/adi_cyl_solid.hip scripts/cyl_solid_host_check.cpp -o cyl_solid_host_check
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

static int run(int nr, int nphi, int nz, long pad, int mode, unsigned seed)   // mode 0: all cells, no words; 1: all cells, hot
{                                                                              // words; 2: a growing active set, no words
    const long sx = (long)nphi * nz + pad;
    const size_t cells = (size_t)(nr - 1) * sx + (size_t)nphi * nz;      // the last plane carries no padding
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> temp(1300.0, 1550.0), step(-150.0, 150.0), coin(0.0, 1.0);
    const double qnan = NAN, T_f = 1425.0;
    std::vector<double> A(cells), B(cells), ts(cells, qnan), cr(cells, qnan), g2(cells, qnan);
    std::vector<uint8_t> act(cells, 0);
    for (size_t p = 0; p < cells; ++p) A[p] = temp(rng);
    const int capacity = 2, guard = 8;
    std::vector<int32_t> store((capacity + 1) * ADI_CYL_HISTORY_LOG_INTS + 2 * guard, 0x5a5a5a5a);
    int32_t *log = store.data() + guard;
    for (int r = 0; r <= capacity; ++r) {
        const int32_t empty[ADI_CYL_HISTORY_LOG_INTS] = {0, INT32_MAX, INT32_MAX, INT32_MAX, -1, -1, -1, 0, 0, 0, 0, 0};
        memcpy(log + r * ADI_CYL_HISTORY_LOG_INTS, empty, sizeof(empty));
    }
    const long ntile = ((long)nphi * nz + ADI_CYL_SOLID_TILE - 1) / ADI_CYL_SOLID_TILE;
    std::vector<int32_t> hot_store((size_t)nr * ntile + 2 * guard, 0x5a5a5a5a);
    int32_t *hot = hot_store.data() + guard;
    Block blk = {1.5, 0.25, 0, 0, capacity};
    long long frozen = 0;
    int rc = ADI_OK;
    if (mode == 1) rc = adi_cyl_solid_hot_seed_host(T_f, A.data(), nullptr, hot, nr, nphi, nz, sx);
    for (int n = 0; n < 6 && rc == ADI_OK; ++n) {
        for (size_t p = 0; p < cells; ++p) {
            if (mode == 2 && coin(rng) < 0.2) act[p] = 1;                  // births: the active set only grows
            B[p] = A[p] + step(rng);
        }
        rc = adi_cyl_solid_record_host(T_f, 0.03, 1.0e-3, 6.283185307179586 / nphi, 1.2e-3, &blk, A.data(), B.data(), ts.data(),
                                       cr.data(), g2.data(), log, mode == 2 ? act.data() : nullptr, mode == 1 ? hot : nullptr,
                                       nr, nphi, nz, sx);
        frozen += log[(blk.slot < capacity ? blk.slot : capacity) * ADI_CYL_HISTORY_LOG_INTS];
        blk.n += 1;
        blk.slot += 1;
        A = B;
    }
    if (rc != ADI_OK) {
        fprintf(stderr, "%d x %d x %d: error %d: %s\n", nr, nphi, nz, rc, adi::err_buf());
        return 1;
    }
    for (int g = 0; g < guard; ++g)
        if (store[g] != 0x5a5a5a5a || store[store.size() - 1 - g] != 0x5a5a5a5a || hot_store[g] != 0x5a5a5a5a ||
            hot_store[hot_store.size() - 1 - g] != 0x5a5a5a5a) {
            fprintf(stderr, "%d x %d x %d: a guard word of the log or of the hot words was written\n", nr, nphi, nz);
            return 1;
        }
    printf("%4d x %3d x %4d  stride +%ld  %s  cells frozen (rows summed) %lld\n", nr, nphi, nz, pad,
           mode == 0 ? "all   " : (mode == 1 ? "hot   " : "masked"), frozen);
    return frozen > 0 ? 0 : 1;
}

int main()
{
    const int shapes[][3] = {{3, 5, 7}, {2, 1, 36}, {1, 4, 130}, {2, 2, 8}, {5, 8, 129}, {2, 3, 1030}};
    int bad = 0;
    unsigned seed = 1;
    for (const auto &s : shapes)
        for (long pad : {0L, 3L})
            for (int mode : {0, 1, 2}) bad += run(s[0], s[1], s[2], pad, mode, seed++);
    // what the checks refuse comes back as ADI_ERR_ARG without a touch of the arrays
    double x = 0.0, y = 0.0, z = 0.0, u = 0.0, v = 0.0;
    int32_t row[ADI_CYL_HISTORY_LOG_INTS] = {0};
    Block blk = {0.0, 0.1, 0, 0, 1};
    bad += adi_cyl_solid_record_host(1425.0, 0.0, 1e-3, 0.1, 1e-3, &blk, &x, &x, &z, &u, &v, row, nullptr, nullptr, 1, 1, 1, 0) !=
           ADI_ERR_ARG;
    bad += adi_cyl_solid_record_host(1425.0, 0.0, 0.0, 0.1, 1e-3, &blk, &x, &y, &z, &u, &v, row, nullptr, nullptr, 1, 1, 1, 0) !=
           ADI_ERR_ARG;
    bad += adi_cyl_solid_hot_seed_host(NAN, &x, nullptr, row, 1, 1, 1, 0) != ADI_ERR_ARG;
    printf(bad ? "FAILED\n" : "cyl_solid_host_check: all clean\n");
    return bad ? 1 : 0;
}
