// adi_matmap_phase.hip -- latent heat of melting and freezing on a grid of several materials (include/adi_hip.h, "Several
// materials: latent heat and surface loss"): the correction of adi_phase.hip with the law of the cell's
// own material, or none for a material that never melts.
//   k_mapphase_apply   every step, T and f in place
//   k_mapphase_seed    f = f_eq(T) of the cell's own law on selected in-mask cells, 0 off the mask and in law-less cells;
//                      rewrites the phase summary and the brick's id set
// One workgroup of 256 threads per 16 x 16 x 16 brick, cell ownership and pair loads of adi_brick_dev.hpp, as adi_phase.hip.  The
// laws travel by value (at most 8 PhaseLaw records and the set of materials that have one).  Per brick the apply kernel reads
// the brick's id set (bits 0-7 of its brick_ids word: the ids among its in-mask cells) first:
//   no material of the set has a law (an empty set included)   return, nothing else is read
//   one material, with a law      the body of k_phase_apply with that law in scalar registers, no id loads
//   several materials             the id bytes of the thread's pairs are loaded and the law is read per cell from a copy of the
//                                 table in LDS (a lane-dependent index into the kernel arguments would land in scratch)
// A cell the law leaves alone -- at rest, Dirichlet, off the mask, of a law-less material -- is never written, and T is not read
// where no cell of a pair has a law.  Contraction off: the operations of MapPhaseField.correct_of.
#include "adi_phase_dev.hpp"
#include "adi_matmap_dev.hpp"

namespace adi {

struct MapPhaseTable {
    PhaseLaw law[kMapMaxMat];
    unsigned on;                // bit m: material m has a law (the records of the others are zeros and never read)
};

constexpr int kLawFields = sizeof(PhaseLaw) / sizeof(double);
static_assert(kLawFields == 8, "PhaseLaw is 8 doubles");
enum { LAW_CP, LAW_L, LAW_TS, LAW_TL, LAW_DT, LAW_HS, LAW_HL, LAW_CM };

// the table into LDS, field-major (sL[field * kMapMaxMat + m]: the ids of a wave's cells fall into adjacent banks)
__device__ __forceinline__ void phase_laws_to_lds(const MapPhaseTable &tab, double *sL)
{
    const double *kl = reinterpret_cast<const double *>(tab.law);
    for (int t = threadIdx.x; t < kLawFields * kMapMaxMat; t += blockDim.x)
        sL[(t % kLawFields) * kMapMaxMat + t / kLawFields] = kl[t];
    __syncthreads();
}

// one law for the whole brick, in scalar registers
struct OneLaw {
    static constexpr bool mixed = false;
    PhaseLaw w;
    __device__ __forceinline__ bool on(unsigned) const { return true; }
    __device__ __forceinline__ double get(int field, unsigned) const
    {
        return field == LAW_CP ? w.cp : field == LAW_L ? w.L : field == LAW_TS ? w.Ts : field == LAW_TL ? w.Tl :
               field == LAW_DT ? w.dT : field == LAW_HS ? w.Hs : field == LAW_HL ? w.Hl : w.cm;
    }
};

// the law of material `id` from the table's copy in LDS
struct LdsLaws {
    static constexpr bool mixed = true;
    const double *t;
    unsigned onmask;
    __device__ __forceinline__ bool on(unsigned id) const { return ((onmask >> id) & 1u) != 0u; }
    __device__ __forceinline__ double get(int field, unsigned id) const { return t[field * kMapMaxMat + id]; }
};

// the body of k_phase_apply (adi_phase.hip) with the law taken from LAWS: uniform (OneLaw) or per cell (LdsLaws)
template <bool VEC, class LAWS>
__device__ __forceinline__ void phase_brick(const LAWS &laws, double *__restrict__ T, double *__restrict__ F,
                                            const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                            const uint8_t *__restrict__ ids, const uint8_t *__restrict__ dir,
                                            unsigned *__restrict__ entry, const Lay &L, int bi, int bj, int bk, unsigned tid)
{
#pragma clang fp contract(off)
    const bool have_f = *entry != 0u;                       // (uniform over the workgroup)
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    PhaseCell c[kPhaseIter];
    double t[kPhaseIter][2], f[kPhaseIter][2];
    unsigned id[kPhaseIter];
    // the loads of the brick, issued together: f (only where some f of the brick is non-zero), flags (only where the flags
    // summary does not say all-solid), ids (several materials: only where a cell of the pair is in the mask), T (only where a
    // cell of the pair is in the mask and its material has a law)
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        c[it] = phase_cell(L, bi, bj, bk, it, tid);
        f[it][0] = 0.0; f[it][1] = 0.0;
        if (have_f && c[it].in) load_pair<VEC>(F, c[it], f[it][0], f[it][1]);
        if (c[it].in) c[it].m = solid ? c[it].in : (load_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        id[it] = 0u;
        if (LAWS::mixed && c[it].m) {
            id[it] = load_id_pair<VEC>(ids, c[it]);
            c[it].m &= (laws.on(id_of(id[it], 0)) ? 1u : 0u) | (laws.on(id_of(id[it], 1)) ? 2u : 0u);
        }
    }
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        t[it][0] = 0.0; t[it][1] = 0.0;
        if (c[it].m) load_pair<VEC>(T, c[it], t[it][0], t[it][1]);
    }
    bool any = false;                                       // a non-zero f in this thread's cells after the pass
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const double fs = f[it][s], ts = t[it][s];
            double fn = fs;
            if ((c[it].m >> s) & 1u) {                      // in the mask, of a material with a law
                const unsigned m = id_of(id[it], s);
                const double Ts = laws.get(LAW_TS, m), Tl = laws.get(LAW_TL, m);
                const bool rest = (fs == 0.0 && ts <= Ts) || (fs == 1.0 && ts >= Tl);
                if (!rest && (dir == nullptr || dir[c[it].p + s] == 0)) {
                    const double cp = laws.get(LAW_CP, m), Lh = laws.get(LAW_L, m);
                    const double Hs = laws.get(LAW_HS, m), Hl = laws.get(LAW_HL, m);
                    const double h1 = cp * ts;
                    const double h2 = Lh * fs;
                    const double H = h1 + h2;
                    double tn;
                    if (H <= Hs) {
                        tn = H / cp;
                        fn = 0.0;
                    } else if (H >= Hl) {
                        const double d = H - Lh;
                        tn = d / cp;
                        fn = 1.0;
                    } else {
                        const double d = H - Hs;
                        const double q = d / laws.get(LAW_CM, m);
                        tn = Ts + q;
                        const double e = tn - Ts;
                        fn = clamp01(e / laws.get(LAW_DT, m));
                    }
                    T[c[it].p + s] = tn;
                    F[c[it].p + s] = fn;
                }
            }
            any = any || fn != 0.0;
        }
    }
    const int nonzero = __syncthreads_or(any ? 1 : 0);
    if (tid == 0 && (have_f || nonzero)) *entry = nonzero ? 1u : 0u;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mapphase_apply(MapPhaseTable tab, double *__restrict__ T, double *__restrict__ F,
                                                            const uint8_t *__restrict__ flags,
                                                            const unsigned *__restrict__ bricks,
                                                            const uint8_t *__restrict__ ids, const uint8_t *__restrict__ dir,
                                                            unsigned *__restrict__ summary,
                                                            const unsigned *__restrict__ brick_ids, Lay L, int nby, int nbz)
{
    __shared__ double sL[kLawFields * kMapMaxMat];
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const long e = ((long)bi * nby + bj) * nbz + bk;
    const unsigned set = brick_ids[e] & 0xffu;              // (uniform over the workgroup)
    if ((set & tab.on) == 0u) return;                       // no in-mask cell, or none whose material has a law
    if ((set & (set - 1u)) == 0u) {
        // one material: its law by selects over constant indices, so the record stays in scalar registers
        const int m = __ffs(set) - 1;
        OneLaw one;
        one.w = tab.law[0];
#pragma unroll
        for (int i = 1; i < kMapMaxMat; ++i)
            if (m == i) one.w = tab.law[i];
        phase_brick<VEC>(one, T, F, flags, bricks, ids, dir, summary + e, L, bi, bj, bk, tid);
    } else {
        phase_laws_to_lds(tab, sL);
        LdsLaws laws;
        laws.t = sL;
        laws.onmask = tab.on;
        phase_brick<VEC>(laws, T, F, flags, bricks, ids, dir, summary + e, L, bi, bj, bk, tid);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mapphase_seed(MapPhaseTable tab, const double *__restrict__ T,
                                                           double *__restrict__ F, const uint8_t *__restrict__ flags,
                                                           const unsigned *__restrict__ bricks,
                                                           const uint8_t *__restrict__ ids, const uint8_t *__restrict__ sel,
                                                           unsigned *__restrict__ summary, unsigned *__restrict__ brick_ids,
                                                           Lay L, int nby, int nbz)
{
#pragma clang fp contract(off)
    __shared__ double sL[kLawFields * kMapMaxMat];
    __shared__ unsigned s_set;
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_set = 0u;
    phase_laws_to_lds(tab, sL);                             // (its barrier also publishes s_set = 0)
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    bool any = false;
    unsigned mine = 0u;                                     // the ids among this thread's in-mask cells
#pragma unroll 2
    for (int it = 0; it < kPhaseIter; ++it) {
        PhaseCell c = phase_cell(L, bi, bj, bk, it, tid);
        if (!c.in) continue;
        c.m = solid ? c.in : (load_mask_pair<VEC>(flags, c) & c.in);
        double t0 = 0.0, t1 = 0.0;
        unsigned idp = 0u;
        if (c.m) {
            idp = load_id_pair<VEC>(ids, c);
            load_pair<VEC>(T, c, t0, t1);
        }
        for (int s = 0; s < 2; ++s) {
            if (!((c.in >> s) & 1u)) continue;
            const long p = c.p + s;
            double fn;
            if (!((c.m >> s) & 1u)) {
                fn = 0.0;
                F[p] = fn;
            } else {
                const unsigned m = id_of(idp, s);
                mine |= 1u << m;
                if (!((tab.on >> m) & 1u)) {
                    fn = 0.0;
                    F[p] = fn;
                } else if (sel == nullptr || sel[p] != 0) {
                    const double e = (s ? t1 : t0) - sL[LAW_TS * kMapMaxMat + m];
                    fn = clamp01(e / sL[LAW_DT * kMapMaxMat + m]);
                    F[p] = fn;
                } else {
                    fn = F[p];
                }
            }
            any = any || fn != 0.0;
        }
    }
    if (mine) atomicOr(&s_set, mine);
    const int nonzero = __syncthreads_or(any ? 1 : 0);      // (a barrier: s_set is complete after it)
    if (tid == 0) {
        const long e = ((long)bi * nby + bj) * nbz + bk;
        summary[e] = nonzero ? 1u : 0u;
        brick_ids[e] = s_set;
    }
}

// ADI_OK and the table as the kernels take it (the constants of each law exactly those of make_phase_law with the material's
// own cp; h_cp null: 1, the seed uses Ts and dT alone), or the first rule of the header the arguments break
static int make_phase_table(const char *who, int nmat, const adi_phase_change *h_laws, const int *h_on, const double *h_cp,
                            MapPhaseTable *t)
{
    ADI_REQUIRE(nmat >= 1 && nmat <= kMapMaxMat, "%s: %d materials (1 to %d)", who, nmat, kMapMaxMat);
    *t = MapPhaseTable{};
    for (int m = 0; m < nmat; ++m) {
        if (!h_on[m]) continue;
        if (int rc = make_phase_law(who, h_laws[m], h_cp ? h_cp[m] : 1.0, &t->law[m])) return rc;
        t->on |= 1u << m;
    }
    return ADI_OK;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_matmap_phase_apply(int nmat, const adi_phase_change *h_laws, const int *h_on, const double *h_cp, double *d_T,
                           double *d_f, const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids,
                           const uint8_t *d_dir_mask, uint32_t *d_summary, const uint32_t *d_brick_ids, int nx, int ny, int nz,
                           long plane_stride, void *stream)
{
    ADI_REQUIRE(h_laws && h_on && h_cp && d_T && d_f && d_flags && d_ids && d_summary && d_brick_ids,
                "adi_matmap_phase_apply: null argument");
    ADI_REQUIRE(d_T != d_f, "adi_matmap_phase_apply: d_f aliases d_T");
    MapPhaseTable tab;
    if (int rc = make_phase_table("adi_matmap_phase_apply", nmat, h_laws, h_on, h_cp, &tab)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_matmap_phase_apply", nx, ny, nz, plane_stride, &g)) return rc;
    if (map_pair_vec(g.L, d_flags, d_ids, d_T, d_f))
        hipLaunchKernelGGL(k_mapphase_apply<true>, g.grid, dim3(256), 0, as_stream(stream), tab, d_T, d_f, d_flags, d_bricks,
                           d_ids, d_dir_mask, (unsigned *)d_summary, (const unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    else
        hipLaunchKernelGGL(k_mapphase_apply<false>, g.grid, dim3(256), 0, as_stream(stream), tab, d_T, d_f, d_flags, d_bricks,
                           d_ids, d_dir_mask, (unsigned *)d_summary, (const unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matmap_phase_seed(int nmat, const adi_phase_change *h_laws, const int *h_on, const double *d_T, double *d_f,
                          const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids, const uint8_t *d_sel,
                          uint32_t *d_summary, uint32_t *d_brick_ids, int nx, int ny, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(h_laws && h_on && d_T && d_f && d_flags && d_ids && d_summary && d_brick_ids,
                "adi_matmap_phase_seed: null argument");
    ADI_REQUIRE(d_T != d_f, "adi_matmap_phase_seed: d_f aliases d_T");
    MapPhaseTable tab;
    if (int rc = make_phase_table("adi_matmap_phase_seed", nmat, h_laws, h_on, nullptr, &tab)) return rc;
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_matmap_phase_seed", nx, ny, nz, plane_stride, &g)) return rc;
    if (map_pair_vec(g.L, d_flags, d_ids, d_T, d_f))
        hipLaunchKernelGGL(k_mapphase_seed<true>, g.grid, dim3(256), 0, as_stream(stream), tab, d_T, d_f, d_flags, d_bricks,
                           d_ids, d_sel, (unsigned *)d_summary, (unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    else
        hipLaunchKernelGGL(k_mapphase_seed<false>, g.grid, dim3(256), 0, as_stream(stream), tab, d_T, d_f, d_flags, d_bricks,
                           d_ids, d_sel, (unsigned *)d_summary, (unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
