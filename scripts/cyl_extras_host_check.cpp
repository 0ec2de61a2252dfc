// cyl_extras_host_check.cpp -- a stand-alone program around the host twins of the cylindrical step's latent heat and thermal
// history (adi_cyl_phase_apply_host, adi_cyl_history_record_host): the kernels' per-cell code and index arithmetic on the CPU,
// over the shapes of tests/cyl_extras_cases.py, with every array allocated at exactly the size the header promises is touched.
// It is meant for a sanitizer build of the host code, which needs no GPU and makes no HIP call:
//     hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         adi_thermal_fields_amd/csrc/adi_cyl_extras.hip scripts/cyl_extras_host_check.cpp -o cyl_extras_host_check
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

static int run(int nr, int nphi, int nz, long pad, bool masked, unsigned seed)
{
    const long sx = (long)nphi * nz + pad;
    const size_t cells = (size_t)(nr - 1) * sx + (size_t)nphi * nz;      // the last plane carries no padding
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> temp(300.0, 1700.0), step(-600.0, 600.0), coin(0.0, 1.0);
    const double qnan = NAN;
    std::vector<double> A(cells), B(cells), f(cells, qnan), peak(cells, qnan), thi(cells, qnan), tlo(cells, qnan);
    std::vector<uint8_t> act(cells, 0);
    for (size_t p = 0; p < cells; ++p) A[p] = temp(rng);
    const int capacity = 2, guard = 8;
    std::vector<int32_t> store((capacity + 1) * ADI_CYL_HISTORY_LOG_INTS + 2 * guard, 0x5a5a5a5a);
    int32_t *log = store.data() + guard;
    for (int r = 0; r <= capacity; ++r) {
        int32_t *row = log + r * ADI_CYL_HISTORY_LOG_INTS;
        const int32_t empty[ADI_CYL_HISTORY_LOG_INTS] = {0, INT32_MAX, INT32_MAX, INT32_MAX, -1, -1, -1, 0, 0, 0, 0, 0};
        memcpy(row, empty, sizeof(empty));
    }
    Block blk = {1.5, 0.25, 0, 0, capacity};
    const adi_phase_change law = {2.7e5, 1400.0, 1450.0};
    const adi_history_levels lev = {1073.15, 773.15, 1450.0};
    long long pool = 0;
    for (int n = 0; n < 6; ++n) {
        for (size_t p = 0; p < cells; ++p) {
            if (masked && coin(rng) < 0.2) act[p] = 1;                     // births: the active set only grows
            B[p] = A[p] + step(rng);
        }
        const uint8_t *a = masked ? act.data() : nullptr;
        int rc = adi_cyl_phase_apply_host(&law, 500.0, B.data(), f.data(), A.data(), a, n % 2, (n / 2) % 2, nr, nphi, nz, sx);
        if (rc == ADI_OK)
            rc = adi_cyl_history_record_host(&lev, &blk, A.data(), B.data(), peak.data(), thi.data(), tlo.data(), log, a, nr,
                                             nphi, nz, sx);
        if (rc != ADI_OK) {
            fprintf(stderr, "%d x %d x %d: error %d: %s\n", nr, nphi, nz, rc, adi::err_buf());
            return 1;
        }
        pool += log[(blk.slot < capacity ? blk.slot : capacity) * ADI_CYL_HISTORY_LOG_INTS];
        blk.n += 1;
        blk.slot += 1;
        A = B;
    }
    for (int g = 0; g < guard; ++g)
        if (store[g] != 0x5a5a5a5a || store[store.size() - 1 - g] != 0x5a5a5a5a) {
            fprintf(stderr, "%d x %d x %d: a guard word of the log was written\n", nr, nphi, nz);
            return 1;
        }
    printf("%4d x %3d x %4d  stride +%ld  %s  pool cells seen %lld\n", nr, nphi, nz, pad, masked ? "masked" : "all   ", pool);
    return 0;
}

int main()
{
    const int shapes[][3] = {{3, 5, 7}, {2, 1, 36}, {1, 4, 130}, {5, 8, 129}, {2, 3, 1030}};
    int bad = 0;
    unsigned seed = 1;
    for (const auto &s : shapes)
        for (long pad : {0L, 3L})
            for (bool masked : {false, true}) bad += run(s[0], s[1], s[2], pad, masked, seed++);
    // what the checks refuse comes back as ADI_ERR_ARG without a touch of the arrays
    double x = 0.0;
    const adi_phase_change law = {2.7e5, 1400.0, 1450.0};
    bad += adi_cyl_phase_apply_host(&law, 500.0, &x, &x, nullptr, nullptr, 0, 0, 1, 1, 1, 0) != ADI_ERR_ARG;
    bad += adi_cyl_phase_apply_host(&law, 500.0, &x, nullptr, nullptr, nullptr, 0, 0, 1, 1, 1, 0) != ADI_ERR_ARG;
    printf(bad ? "FAILED\n" : "cyl_extras_host_check: all clean\n");
    return bad ? 1 : 0;
}
