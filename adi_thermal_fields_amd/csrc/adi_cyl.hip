// adi_cyl.hip -- cylindrical (r, phi, z) backward-Euler ADI step for MI355X (gfx950).
//
// Replaces adi3d_cyl_phi_v3.py:332-350 (scheme="be": r-Thomas -> periodic phi solve -> z-Thomas)
// and the void-clamping wrapper adi_step_masked (quick_spiral_deposition_gif_v5.py:31-70).
// Field layout C-order (nr, nphi, nz): r is the slowest axis, z is contiguous.
//
//   r sweep   strided axis 0, lines indexed by the flattened (phi, z) index; the tridiagonal
//             coefficients depend on the radius index only (build_coeff_r, :155-202) and come from a
//             small per-plan table; the source term and the void pre-clamp are fused into the load.
//   phi sweep strided axis 1, periodic.  The reference solves it spectrally (phi_solve_spectral,
//             :302-329), i.e. it inverts the circulant tridiagonal (-f_i, 1+2 f_i, -f_i) exactly; here
//             the same system is solved as an ordinary tridiagonal plus a Sherman-Morrison rank-one
//             correction whose vector z_i = A'^-1 u depends on the radius only and is tabulated at
//             plan creation (valid for any nphi, power of two or not).  f_0 = 0: the axis row is identity.
//   z sweep   contiguous axis 2 (build_coeff_z, :255-298): constant coefficients, the two end rows
//             carry the neumann0 / dirichlet / robin closure; the void post-clamp is fused into the store.
//
// Moving heat source (the *_src / *_tick instantiations): q evaluated in the r sweep's load from a device block, the block's
// step counter advanced by the z sweep; no source field, so no extra traffic.
// Algorithmic HBM traffic: 16 B/cell/sweep (+8 with a source field, +1 per masked pass).
// Cache policy of this translation unit: PLAIN loads and stores (the Cartesian kernels stream their outputs with nt stores).
// The cylindrical sweeps run in place on a field of 134 MB at BASELINE configs[3] -- inside the 256 MB Infinity Cache -- and a
// streaming store evicts exactly the lines the next sweep is about to read: 0.145 -> 0.133 ms per step in the loop, 0.154 ->
// 0.143 ms with the reference's step semantics (scripts/cyl_probe.py, nt against plain).
#define ADI_STORE_AUX 0
#define ADI_LOAD_NT_CONTIG 0
#define ADI_CYL_NT 0
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "adi_cyl_dev.hpp"

using namespace adi;

struct adi_cyl_plan {
    int nr, nphi, nz, device;
    long sx;                     // plane (one radius) stride in elements
    double s_scale;              // dt / (rho cp): what a source in W/m^3 adds to R0
    // r sweep
    double *d_ar, *d_br, *d_cr;  // [nr]
    double r_add_last;
    double *d_rfac;              // [r_nseg][RF_STRIDE] FAST form: the factorisation of every segment (cyl_build_r_fast)
    int r_M, r_nseg;
    // phi sweep
    double *d_fac;               // [nr]
    double *d_zt;                // [nr * nphi]  Sherman-Morrison vector per radius
    double *d_smden;             // [nr]         1 / (1 + v.z)
    void *d_uphi;                // [nr] UniC<phi_M>: constants of the uniform interior block (-f_i, 1+2f_i, -f_i) per radius
    int phi_M;                   // rows per thread of the phi FAST kernel (0: not available for this nphi)
    // z sweep
    CylZ z;
    UniC<16> zU;                 // constants of the uniform block (-f, 1+2f, -f) of the z FAST kernel
    CylGeo geo;                  // geometry (cell centres of the moving source)
};

static void plan_free(adi_cyl_plan *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    void *ptrs[] = {p->d_ar, p->d_br, p->d_cr, p->d_fac, p->d_zt, p->d_smden, p->d_uphi, p->d_rfac};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    delete p;
}

// what adi_cyl_plan_create_annular and adi_cyl_plan_tables both refuse, before anything is built or allocated
static int cyl_plan_check(int nr, int nphi, int nz, double r_in, int kind_bot, int kind_top)
{
    ADI_REQUIRE(r_in >= 0.0, "adi_cyl_plan_create: negative inner radius");
    ADI_REQUIRE(nr > 0 && nphi > 0 && nz > 0, "adi_cyl_plan_create: bad grid");
    ADI_REQUIRE(kind_bot >= 0 && kind_bot <= 2, "unknown zbc.kind_bot");  // ValueError, adi3d_cyl_phi_v3.py:283
    ADI_REQUIRE(kind_top >= 0 && kind_top <= 2, "unknown zbc.kind_top");  // :296
    ADI_REQUIRE(nr <= kMaxFastLine && nphi <= kMaxFastLine && nz <= kMaxFastLine,
                "adi_cyl_plan_create: axis longer than %d cells is not supported", kMaxFastLine);
    return ADI_OK;
}

static bool upload(void **dst, const void *src, size_t bytes)
{
    return hipMalloc(dst, bytes) == hipSuccess && hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}
static bool upload(double **dst, const std::vector<double> &v) { return upload((void **)dst, v.data(), v.size() * sizeof(double)); }

// constants of the uniform phi blocks, one UniC<M> per radius
template <int M>
static bool upload_unic(void **dst, const std::vector<double> &pf)
{
    std::vector<UniC<M>> u;
    for (double f : pf) u.push_back(make_unic<M>(f));
    return upload(dst, u.data(), u.size() * sizeof(UniC<M>));
}

// f(std::integral_constant<int, M>) for the one M of Ms that equals m: a run-time row count picks a kernel instantiation
template <int... Ms, class F>
static void with_rows(int m, F &&f)
{
    (void)(((m == Ms) && (f(std::integral_constant<int, Ms>{}), true)) || ...);
}

static int strided_rows(int n)
{
    return n <= 16 ? 2 : (n <= 32 ? 4 : (n <= 512 ? 8 : 16));
}
static int contig_rows(int n) { return n <= 128 ? 2 : (n <= 256 ? 4 : (n <= 512 ? 8 : 16)); }

// blk != nullptr (MODE 0, the r sweep: n_outer == 1): the moving source of the block (k_cyl_strided_src) instead of S
template <int M, int MODE>
static void launch_cyl_strided(const adi_cyl_plan *pl, const double *in, double *out, int n, long stride, int n_inner,
                               long n_outer, long outer_stride, const double *S, const uint8_t *act, double T_void,
                               hipStream_t st, const CylSrcBlock *blk)
{
    const int Lp = next_pow2((n + M - 1) / M);
    const int min_lines = 16, min_threads = 512;
    // 16 adjacent lines = whole 128-byte pieces per row; 512 threads per tile measured best on 128 x 256 x 512
    // (0.219 -> 0.205 ms per step against 8 lines / 256 threads)
    int lines = min_lines;
    while (lines * Lp < min_threads) lines <<= 1;
    while (lines > 8 && (lines * Lp > (M <= 8 ? 1024 : 512) || 64 * lines * (Lp + 1) > 48 * 1024)) lines >>= 1;
    const int tiles_inner = (n_inner + lines - 1) / lines;
    const long ntiles = (long)tiles_inner * n_outer;
    const size_t lds = (size_t)8 * lines * (Lp + 1) * sizeof(double);
    const dim3 grid((unsigned)ntiles), block(lines * Lp);
    if constexpr (MODE == 0)
        if (blk != nullptr) {
            hipLaunchKernelGGL((k_cyl_strided_src<M>), grid, block, lds, st, in, out, n, stride, n_inner, Lp, lines, tiles_inner,
                               ntiles, pl->d_ar, pl->d_br, pl->d_cr, pl->r_add_last, pl->s_scale, act, T_void, blk, pl->geo);
            return;
        }
    hipLaunchKernelGGL((k_cyl_strided<M, MODE>), grid, block, lds, st, in, out, n, stride, n_inner, outer_stride, Lp, lines,
                       tiles_inner, ntiles, pl->d_ar, pl->d_br, pl->d_cr, pl->r_add_last, S, pl->s_scale, act, T_void,
                       pl->d_fac, pl->d_zt, pl->d_smden);
}

// blk != nullptr: the moving source of the block (k_cyl_r_fast_src / k_cyl_strided_src) instead of d_S
static int cyl_sweep_r(const adi_cyl_plan *pl, const double *in, double *out, const double *d_S, const uint8_t *d_active,
                       double T_void, hipStream_t st, const CylSrcBlock *blk)
{
    const int nr = pl->nr;
    const long plane = (long)pl->nphi * pl->nz;
    if (pl->r_M && plane % 64 == 0 && (long)nr * pl->sx < (1L << 31)) {
        const int Lp = pl->r_nseg;
        const long ntiles = plane / 64;
        const dim3 grid((unsigned)ntiles), block(64 * Lp);
        const size_t lds = (size_t)3 * Lp * 64 * sizeof(double);
        with_rows<8, 16>(pl->r_M, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (blk != nullptr)
                hipLaunchKernelGGL((k_cyl_r_fast_src<M>), grid, block, lds, st, in, out, nr, pl->sx, (int)plane, pl->r_nseg, Lp,
                                   ntiles, pl->d_rfac, pl->r_add_last, pl->s_scale, d_active, T_void, blk, pl->geo);
            else
                hipLaunchKernelGGL((k_cyl_r_fast<M>), grid, block, lds, st, in, out, nr, pl->sx, (int)plane, pl->r_nseg, Lp,
                                   ntiles, pl->d_rfac, pl->r_add_last, d_S, pl->s_scale, d_active, T_void);
        });
    } else {
        with_rows<2, 4, 8, 16>(strided_rows(nr), [&](auto m) {
            launch_cyl_strided<decltype(m)::value, 0>(pl, in, out, nr, pl->sx, (int)plane, 1, 0, d_S, d_active, T_void, st, blk);
        });
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

static int cyl_sweep_phi(const adi_cyl_plan *pl, const double *in, double *out, hipStream_t st)
{
    const int nr = pl->nr, nphi = pl->nphi, nz = pl->nz;
    if (pl->phi_M && nz % 32 == 0) {
        const int Lp = nphi / pl->phi_M;
        int lines = 32;                                   // 256-byte row pieces (64-line tiles, one wave per segment and the
        while (lines * Lp > 1024) lines >>= 1;            // Sherman-Morrison vector by scalar loads: 62.7 us against 55.6)
        const int tiles_inner = nz / lines;
        const long ntiles = (long)tiles_inner * nr;
        const size_t lds = (size_t)7 * lines * (Lp + 1) * sizeof(double);
        with_rows<8, 16>(pl->phi_M, [&](auto m) {
            constexpr int M = decltype(m)::value;
            hipLaunchKernelGGL((k_cyl_phi_fast<M>), dim3((unsigned)ntiles), dim3(lines * Lp), lds, st, in, out, nphi, (long)nz, nz,
                               pl->sx, Lp, lines, tiles_inner, ntiles, (const UniC<M> *)pl->d_uphi, pl->d_fac, pl->d_zt, pl->d_smden);
        });
    } else {
        with_rows<2, 4, 8, 16>(strided_rows(nphi), [&](auto m) {
            launch_cyl_strided<decltype(m)::value, 1>(pl, in, out, nphi, nz, nz, nr, pl->sx, nullptr, nullptr, 0.0, st, nullptr);
        });
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

// kern(args...) on 256-thread blocks or, with a tick, kern_tick(args..., tick): the same sweep, whose first thread also
// advances the source block's counter (k_*_tick)
template <class K, class KT, class... A>
static void launch_z(K kern, KT kern_tick, unsigned grid, hipStream_t st, unsigned long long *tick, A... args)
{
    if (tick != nullptr) hipLaunchKernelGGL(kern_tick, dim3(grid), dim3(256), 0, st, args..., tick);
    else hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, args...);
}

static int cyl_sweep_z(const adi_cyl_plan *pl, const double *in, double *out, const uint8_t *d_active, double T_void,
                       double T_inner, hipStream_t st, unsigned long long *tick)
{
    const int nphi = pl->nphi, nz = pl->nz;
    const CylZ &z = pl->z;
    const long nlines = (long)pl->nr * nphi, lines_per_r0 = nphi;
    const bool aligned = ((((uintptr_t)in | (uintptr_t)out) & 15) == 0) && pl->sx % 2 == 0;
    const int Lpf = nz / 16, lwf = Lpf > 0 ? 64 / Lpf : 0;
    const bool fast = !z.dir0 && !z.dirN && nz >= 128 && nz % 16 == 0 && Lpf <= 64 && (Lpf & (Lpf - 1)) == 0 &&
                      nphi % lwf == 0 && aligned;
    if (fast) {
        const long waves = nlines / lwf;
        launch_z(k_cyl_z_fast<16>, k_cyl_z_fast_tick<16>, (unsigned)((waves + 3) / 4), st, tick, in, out, nlines, nz, Lpf, z,
                 pl->zU, d_active, T_void, T_inner, lines_per_r0, pl->sx);
    } else {
        with_rows<2, 4, 8, 16>(contig_rows(nz), [&](auto m) {
            constexpr int M = decltype(m)::value;
            const int Lp = next_pow2((nz + M - 1) / M);
            const int lw = 64 / Lp;
            const long waves = (nlines + lw - 1) / lw;
            const unsigned grid = (unsigned)((waves + 3) / 4);
            const auto go = [&](auto vec) {
                constexpr bool VEC = decltype(vec)::value;
                launch_z(k_cyl_contig<M, VEC>, k_cyl_contig_tick<M, VEC>, grid, st, tick, in, out, nlines, nz, Lp, z, d_active,
                         T_void, T_inner, lines_per_r0, pl->sx);
            };
            if (aligned && nz % M == 0) go(std::true_type{});
            else go(std::false_type{});
        });
    }
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

// one sweep; blk != nullptr: axis 0 adds the block's source instead of d_S, axis 2 advances its counter
static int cyl_sweep(const adi_cyl_plan *pl, int axis, const double *in, double *out, const double *d_S,
                     const uint8_t *d_active, double T_void, double T_inner, hipStream_t st, CylSrcBlock *blk)
{
    // out == in is allowed: every thread of every sweep kernel of adi_cyl_dev.hpp reads only the rows it later writes (and
    // reads them before the barriers that precede its stores), which is why `in` / `out` carry no __restrict__ there
    if (axis == 0) return cyl_sweep_r(pl, in, out, d_S, d_active, T_void, st, blk);
    if (axis == 2) return cyl_sweep_z(pl, in, out, d_active, T_void, T_inner, st, blk ? &blk->n : nullptr);
    if (pl->nphi > 1) return cyl_sweep_phi(pl, in, out, st);
    const size_t cnt = (size_t)pl->nr * pl->sx;      // the reference returns a copy, adi3d_cyl_phi_v3.py:303-304
    hipLaunchKernelGGL(k_copy, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, in, out, cnt);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

// r sweep: T_in -> T_out (source and void pre-clamp fused); then phi and z IN PLACE on T_out: the working set of the two
// sweeps is one field (134 MB at 128 x 256 x 512, inside the 256 MB Infinity Cache) instead of two.  nphi == 1: the
// reference's phi solve returns a copy (:303-304) -- nothing to do.  z sweep: void post-clamp fused.
static int cyl_step(const adi_cyl_plan *pl, const double *T_in, double *T_out, const double *d_S, const uint8_t *d_active,
                    double T_void, double T_inner, hipStream_t st, CylSrcBlock *blk)
{
    if (int rc = cyl_sweep(pl, 0, T_in, T_out, d_S, d_active, T_void, T_inner, st, blk)) return rc;
    if (pl->nphi > 1)
        if (int rc = cyl_sweep(pl, 1, T_out, T_out, nullptr, nullptr, 0.0, 0.0, st, blk)) return rc;
    return cyl_sweep(pl, 2, T_out, T_out, nullptr, d_active, T_void, T_inner, st, blk);
}

static int check_cyl_source(const adi_cyl_heat_source *h, const char *fn)
{
    ADI_REQUIRE(h != nullptr, "%s: null source", fn);
    const double v[] = {h->power, h->eta, h->a, h->b, h->c_f, h->c_r, h->f_f, h->r_c, h->phi0, h->omega, h->z0, h->v_z};
    for (double x : v) ADI_REQUIRE(std::isfinite(x), "%s: non-finite source parameter", fn);
    ADI_REQUIRE(h->power >= 0.0, "%s: power < 0", fn);
    ADI_REQUIRE(h->eta >= 0.0 && h->eta <= 1.0, "%s: eta outside [0, 1]", fn);
    ADI_REQUIRE(h->a > 0.0 && h->b > 0.0 && h->c_f > 0.0 && h->c_r > 0.0, "%s: non-positive length", fn);
    ADI_REQUIRE(h->f_f > 0.0 && h->f_f < 2.0, "%s: f_f outside (0, 2)", fn);
    ADI_REQUIRE(h->r_c >= 0.0, "%s: r_c < 0", fn);
    ADI_REQUIRE(h->depth == ADI_CYL_DEPTH_Z || h->depth == ADI_CYL_DEPTH_R, "%s: depth must be 'z' (0) or 'r' (1)", fn);
    return ADI_OK;
}

extern "C" {

int adi_cyl_plan_create(int nr, int nphi, int nz, long plane_stride, double dr, double dphi, double dz, double rho,
                        double cp, double k,
                        double dt, double robin_h, double robin_Tinf, int kind_bot, int kind_top, double h_bot,
                        double h_top, double Tinf_bot, double Tinf_top, double T_bot, double T_top,
                        adi_cyl_plan **out)
{
    return adi_cyl_plan_create_annular(nr, nphi, nz, plane_stride, dr, dphi, dz, 0.0, rho, cp, k, dt, robin_h, robin_Tinf, kind_bot,
                                       kind_top, h_bot, h_top, Tinf_bot, Tinf_top, T_bot, T_top, out);
}

int adi_cyl_plan_tables(int nr, int nphi, int nz, double dr, double dphi, double dz, double r_in, double rho, double cp,
                        double k, double dt, double robin_h, double robin_Tinf, int kind_bot, int kind_top, double h_bot,
                        double h_top, double Tinf_bot, double Tinf_top, double T_bot, double T_top, double *a, double *b,
                        double *c, double *r_add_last, double *phi_fac, double *zt, double *smden, double *zclosure, int *fast,
                        double *rfac, long rfac_capacity)
{
    if (int rc = cyl_plan_check(nr, nphi, nz, r_in, kind_bot, kind_top)) return rc;
    CylTables T;
    cyl_build_tables(nr, nphi, dr, dphi, dz, r_in, rho, cp, k, dt, robin_h, robin_Tinf, kind_bot, kind_top, h_bot, h_top,
                     Tinf_bot, Tinf_top, T_bot, T_top, T);
    ADI_REQUIRE(rfac == nullptr || rfac_capacity >= (long)T.rfac.size(), "adi_cyl_plan_tables: rfac_capacity %ld < %ld",
                rfac_capacity, (long)T.rfac.size());
    const auto put = [](double *dst, const std::vector<double> &v) {
        if (dst != nullptr) std::copy(v.begin(), v.end(), dst);
    };
    put(a, T.ar); put(b, T.br); put(c, T.cr);
    if (r_add_last != nullptr) *r_add_last = T.r_add_last;
    put(phi_fac, T.pf); put(zt, T.zt); put(smden, T.smden);
    if (zclosure != nullptr) std::copy(T.z, T.z + ADI_CYL_ZCLOSURE_LEN, zclosure);
    if (fast != nullptr) { fast[0] = T.r_M; fast[1] = T.r_nseg; fast[2] = T.phi_M; }
    put(rfac, T.rfac);
    return ADI_OK;
}

int adi_cyl_plan_create_annular(int nr, int nphi, int nz, long plane_stride, double dr, double dphi, double dz, double r_in,
                                double rho, double cp, double k,
                                double dt, double robin_h, double robin_Tinf, int kind_bot, int kind_top, double h_bot,
                                double h_top, double Tinf_bot, double Tinf_top, double T_bot, double T_top,
                                adi_cyl_plan **out)
{
    ADI_REQUIRE(out, "adi_cyl_plan_create: null output");
    if (int rc = cyl_plan_check(nr, nphi, nz, r_in, kind_bot, kind_top)) return rc;
    const long sx = plane_stride ? plane_stride : (long)nphi * nz;
    ADI_REQUIRE(sx >= (long)nphi * nz, "adi_cyl_plan_create: plane_stride < nphi*nz");
    int device;
    ADI_HIP_TRY(hipGetDevice(&device));
    CylTables T;
    cyl_build_tables(nr, nphi, dr, dphi, dz, r_in, rho, cp, k, dt, robin_h, robin_Tinf, kind_bot, kind_top, h_bot, h_top,
                     Tinf_bot, Tinf_top, T_bot, T_top, T);
    adi_cyl_plan *p = new (std::nothrow) adi_cyl_plan();      // (value-initialised: every pointer null)
    if (!p) return set_err(ADI_ERR_HIP, "out of host memory");
    p->nr = nr; p->nphi = nphi; p->nz = nz; p->device = device; p->sx = sx;
    p->s_scale = dt * (1.0 / (rho * cp));
    p->r_add_last = T.r_add_last; p->r_M = T.r_M; p->r_nseg = T.r_nseg; p->phi_M = T.phi_M;
    p->z = CylZ{T.z[0], T.z[1], T.z[2], T.z[3], T.z[4], T.z[5], T.z[6], T.z[7], T.z[8], (int)T.z[9], (int)T.z[10]};
    p->zU = make_unic<16>(p->z.f);
    p->geo = CylGeo{r_in, dr, dphi, dz, nz};
    const bool ok = upload(&p->d_ar, T.ar) && upload(&p->d_br, T.br) && upload(&p->d_cr, T.cr) && upload(&p->d_fac, T.pf) &&
                    upload(&p->d_zt, T.zt) && upload(&p->d_smden, T.smden) && (!T.r_M || upload(&p->d_rfac, T.rfac)) &&
                    (T.phi_M != 8 || upload_unic<8>(&p->d_uphi, T.pf)) && (T.phi_M != 16 || upload_unic<16>(&p->d_uphi, T.pf));
    if (!ok) {
        plan_free(p);
        return set_err(ADI_ERR_HIP, "adi_cyl_plan_create: device table upload failed");
    }
    *out = p;
    return ADI_OK;
}

int adi_cyl_plan_destroy(adi_cyl_plan *plan)
{
    plan_free(plan);
    return ADI_OK;
}

int adi_cyl_sweep(const adi_cyl_plan *pl, int axis, const double *d_in, double *d_out, const double *d_S,
                  const uint8_t *d_active, double T_void, double T_inner, void *stream)
{
    ADI_REQUIRE(pl && d_in && d_out, "adi_cyl_sweep: bad argument");
    ADI_REQUIRE(axis >= 0 && axis < 3, "adi_cyl_sweep: bad axis %d", axis);
    ADI_REQUIRE((long)pl->nphi * pl->nz <= 0x7fffffffL, "adi_cyl_sweep: (nphi, nz) plane too large");
    return cyl_sweep(pl, axis, d_in, d_out, d_S, d_active, T_void, T_inner, as_stream(stream), nullptr);
}

int adi_cyl_step(const adi_cyl_plan *pl, const double *d_T_in, double *d_T_out, double *d_tmp_a, double *d_tmp_b,
                 const double *d_S, const uint8_t *d_active, double T_void, double T_inner, void *stream)
{
    (void)d_tmp_a; (void)d_tmp_b;     // unused since ABI v13: the phi and z sweeps run in place on d_T_out
    ADI_REQUIRE(pl && d_T_in && d_T_out, "adi_cyl_step: null argument");
    ADI_REQUIRE(d_T_out != d_T_in, "adi_cyl_step: T_out aliases T_in (the step returns a new field, adi3d_cyl_phi_v3.py:350)");
    ADI_REQUIRE((long)pl->nphi * pl->nz <= 0x7fffffffL, "adi_cyl_step: (nphi, nz) plane too large");
    return cyl_step(pl, d_T_in, d_T_out, d_S, d_active, T_void, T_inner, as_stream(stream), nullptr);
}

int adi_cyl_source_set(void *d_block, const adi_cyl_heat_source *h_src, double t0, double dt, long long n, void *stream)
{
    if (int rc = check_cyl_source(h_src, "adi_cyl_source_set")) return rc;
    ADI_REQUIRE(d_block, "adi_cyl_source_set: null block");
    ADI_REQUIRE(std::isfinite(t0) && std::isfinite(dt) && dt > 0.0 && n >= 0, "adi_cyl_source_set: bad t0 / dt / n");
    CylSrcBlock v;
    memset(&v, 0, sizeof(v));
    v.s = *h_src;
    v.t0 = t0; v.dt = dt; v.n = (unsigned long long)n;
    hipLaunchKernelGGL(k_cyl_source_set, dim3(1), dim3(1), 0, as_stream(stream), (CylSrcBlock *)d_block, v);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_source_sample(const adi_cyl_heat_source *h_src, int nr, int nphi, int nz, long plane_stride, double r_in,
                          double dr, double dphi, double dz, double t, const uint8_t *d_active, double *d_out, void *stream)
{
    if (int rc = check_cyl_source(h_src, "adi_cyl_source_sample")) return rc;
    ADI_REQUIRE(d_out, "adi_cyl_source_sample: null output");
    ADI_REQUIRE(nr > 0 && nphi > 0 && nz > 0, "adi_cyl_source_sample: bad grid");
    const double g[] = {r_in, dr, dphi, dz, t};
    for (double x : g) ADI_REQUIRE(std::isfinite(x), "adi_cyl_source_sample: non-finite geometry / t");
    ADI_REQUIRE(r_in >= 0.0 && dr > 0.0 && dphi > 0.0 && dz > 0.0, "adi_cyl_source_sample: bad r_in / dr / dphi / dz");
    const long sx = plane_stride ? plane_stride : (long)nphi * nz;
    ADI_REQUIRE(sx >= (long)nphi * nz, "adi_cyl_source_sample: plane_stride < nphi*nz");
    const long cells = (long)nr * nphi * nz;
    hipLaunchKernelGGL(k_cyl_source_sample, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, as_stream(stream), *h_src,
                       CylGeo{r_in, dr, dphi, dz, nz}, nr, nphi, sx, t, d_active, d_out);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_cyl_sweep_src(const adi_cyl_plan *pl, int axis, void *d_block, const double *d_in, double *d_out,
                      const uint8_t *d_active, double T_void, double T_inner, void *stream)
{
    ADI_REQUIRE(pl && d_block && d_in && d_out, "adi_cyl_sweep_src: bad argument");
    ADI_REQUIRE(axis >= 0 && axis < 3, "adi_cyl_sweep_src: bad axis %d", axis);
    ADI_REQUIRE((long)pl->nphi * pl->nz <= 0x7fffffffL, "adi_cyl_sweep_src: (nphi, nz) plane too large");
    return cyl_sweep(pl, axis, d_in, d_out, nullptr, d_active, T_void, T_inner, as_stream(stream), (CylSrcBlock *)d_block);
}

int adi_cyl_step_src(const adi_cyl_plan *pl, void *d_block, const double *d_T_in, double *d_T_out,
                     const uint8_t *d_active, double T_void, double T_inner, void *stream)
{
    ADI_REQUIRE(pl && d_block && d_T_in && d_T_out, "adi_cyl_step_src: null argument");
    ADI_REQUIRE(d_T_out != d_T_in, "adi_cyl_step_src: T_out aliases T_in");
    ADI_REQUIRE((long)pl->nphi * pl->nz <= 0x7fffffffL, "adi_cyl_step_src: (nphi, nz) plane too large");
    return cyl_step(pl, d_T_in, d_T_out, nullptr, d_active, T_void, T_inner, as_stream(stream), (CylSrcBlock *)d_block);
}

}  // extern "C"
