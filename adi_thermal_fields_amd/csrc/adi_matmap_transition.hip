// adi_matmap_transition.hip -- a cell's material changes when the cell gets hot enough (include/adi_hip.h, "Several materials:
// transitions"): powder that reaches its liquidus is dense metal from then on.
//   k_maptransition   after the step, on its output: id, the six pack values and (with a liquid fraction) f of every cell
//                         that changes; the brick's id set, phase summary and the count of changed cells
//   k_mapbricksets   the id set of every brick from flags and ids (for a caller without a MapPhaseField, whose seed keeps
//                         those words otherwise)
// One workgroup of 256 threads per 16 x 16 x 16 brick, cell ownership and pair loads of adi_brick_dev.hpp.  The rules travel by
// value (kMapMaxMat targets and thresholds; with a liquid fraction Ts, dT and the set of materials that have a law).  Per brick:
//   the id set holds no material with a rule          return, nothing else is read
//   flags (unless the brick is all solid) and T of the in-mask cells; no cell at or above the smallest threshold among the set's
//   ruled materials                                   return: a cold powder brick costs one read of T
//   otherwise the id bytes, and per cell the decision of MaterialTransitions.apply_reference
//   nothing changed                                   return, nothing was written
// A changed cell is finished by the thread that owns it: the id byte, then the six pack values from map_coeffs_cell_c with the
// new material's C (they depend on the cell's own id and on its neighbours' mask bytes only, so no other cell's values move),
// then f = f_eq(T) of the new material's law or 0 -- the operations of k_mapphase_seed.  The new id set is gathered in LDS with
// integer atomics; thread 0 writes the words and adds the brick's count to the 64-bit counter.  T is never written.  No float
// atomics, contraction off, no scratch (tests/test_transitions_cpu.py reads it from the code object).
#include "adi_phase_dev.hpp"
#include "adi_matmap_dev.hpp"

namespace adi {

// v, field-major (v[field * kMapMaxMat + m]): TR_TAT the threshold of material m (read only where `ruled` has bit m); with a
// liquid fraction TR_TS and TR_DT, solidus and melting range of material m (where `on` has bit m); TR_C, C_m dx^3
enum { TR_TAT, TR_TS, TR_DT, TR_C, TR_FIELDS };

struct MapTransTable {
    double v[TR_FIELDS * kMapMaxMat];
    unsigned to;                // 4 bits per material: the material m turns into
    unsigned ruled;             // bit m: material m has a rule
    unsigned on;                // bit m: material m has a latent-heat law
};

struct MapTransPacks {
    double *c0, *c1, *c2, *q0, *q1, *q2;
};

template <bool VEC, bool PHASE>
__global__ __launch_bounds__(256) void k_maptransition(MapTransTable tab, const double *__restrict__ T, uint8_t *ids,
                                                               const uint8_t *__restrict__ flags,
                                                               const unsigned *__restrict__ bricks,
                                                               const uint8_t *__restrict__ mask, const uint8_t *__restrict__ dir,
                                                               double *F, unsigned *__restrict__ summary,
                                                               unsigned *__restrict__ brick_ids,
                                                               unsigned long long *__restrict__ counter, Lay L, int nby, int nbz,
                                                               double A, MapFaceSpec h, MapFaceSpec q, MapTransPacks pk)
{
#pragma clang fp contract(off)
    __shared__ double sT[TR_FIELDS * kMapMaxMat];
    __shared__ unsigned s_set, s_count;
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    const long e = ((long)bi * nby + bj) * nbz + bk;
    const unsigned set = brick_ids[e] & 0xffu;              // (uniform over the workgroup)
    const unsigned live = set & tab.ruled;
    if (live == 0u) return;                                 // no in-mask cell, or none whose material has a rule
    // the smallest threshold among the set's ruled materials, by selects over constant indices (scalar registers)
    double t_min = 0.0;
    bool first = true;
#pragma unroll
    for (int m = 0; m < kMapMaxMat; ++m)
        if ((live >> m) & 1u) {
            t_min = (first || tab.v[TR_TAT * kMapMaxMat + m] < t_min) ? tab.v[TR_TAT * kMapMaxMat + m] : t_min;
            first = false;
        }
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    PhaseCell c[kPhaseIter];
    double t[kPhaseIter][2];
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        c[it] = phase_cell(L, bi, bj, bk, it, tid);
        if (c[it].in) c[it].m = solid ? c[it].in : (load_mask_pair<VEC>(flags, c[it]) & c[it].in);
    }
    bool hot = false;
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        t[it][0] = 0.0; t[it][1] = 0.0;
        if (c[it].m) load_pair<VEC>(T, c[it], t[it][0], t[it][1]);
        hot = hot || ((c[it].m & 1u) && t[it][0] >= t_min) || ((c[it].m & 2u) && t[it][1] >= t_min);
    }
    if (!__syncthreads_or(hot ? 1 : 0)) return;             // a cold brick: one read of T (a NaN is not hot)

    // the tables into LDS (a lane-dependent index into the kernel arguments would land in scratch)
    {
        const double *kt = tab.v;
        for (int u = tid; u < TR_FIELDS * kMapMaxMat; u += blockDim.x) sT[u] = kt[u];
        if (tid == 0) { s_set = 0u; s_count = 0u; }
        __syncthreads();
    }
    unsigned chg = 0u;                                      // bit 2 it + s: that cell changes
    unsigned mine = 0u;                                     // the ids among this thread's in-mask cells after the pass
#pragma unroll
    for (int it = 0; it < kPhaseIter; ++it) {
        if (!c[it].m) continue;
        const unsigned idp = load_id_pair<VEC>(ids, c[it]);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            if (!((c[it].m >> s) & 1u)) continue;
            unsigned m = id_of(idp, s);
            if (((tab.ruled >> m) & 1u) && t[it][s] >= sT[TR_TAT * kMapMaxMat + m] &&
                (dir == nullptr || dir[c[it].p + s] == 0)) {
                chg |= 1u << (2 * it + s);
                m = (tab.to >> (4 * m)) & (unsigned)(kMapMaxMat - 1);
            }
            mine |= 1u << m;
        }
    }
    if (!__syncthreads_or(chg != 0u ? 1 : 0)) return;       // hot cells, but none that changes: nothing is written

    // the changed cells, one at a time (a vanishing share of all cells: the loop is not unrolled, the cell is found again from
    // its bit and its T read again)
    bool any = false;                                       // a non-zero f among the cells this thread has seen
    const bool have_f = PHASE && summary[e] != 0u;          // (uniform over the workgroup)
    unsigned left = chg;
#pragma unroll 1
    while (left) {
        const int b = __ffs(left) - 1;
        left &= left - 1u;
        const int it = b >> 1, s = b & 1;
        const int row = it * 32 + (int)(tid >> 3);
        const int i = bi * kBrick + (row >> 4), j = bj * kBrick + (row & 15), k = bk * kBrick + 2 * (int)(tid & 7u) + s;
        const long p = (long)i * L.sx + (long)j * L.nz + k;
        const unsigned m = ids[p] & (unsigned)(kMapMaxMat - 1);
        const unsigned n = (tab.to >> (4 * m)) & (unsigned)(kMapMaxMat - 1);
        ids[p] = (uint8_t)n;
        map_coeffs_cell_c(mask, L, A, sT[TR_C * kMapMaxMat + n], h, q, i, j, k, p, pk.c0, pk.c1, pk.c2, pk.q0, pk.q1, pk.q2);
        if (PHASE) {
            double fn = 0.0;
            if ((tab.on >> n) & 1u) {
                const double d = T[p] - sT[TR_TS * kMapMaxMat + n];
                fn = clamp01(d / sT[TR_DT * kMapMaxMat + n]);
            }
            F[p] = fn;
            any = any || fn != 0.0;
        }
    }
    if (PHASE) {
        // the other cells' f, where some f of the brick was non-zero before the pass
        if (have_f) {
#pragma unroll
            for (int it = 0; it < kPhaseIter; ++it) {
                if (!c[it].in) continue;
                double f0, f1;
                load_pair<VEC>(F, c[it], f0, f1);
                any = any || (!((chg >> (2 * it)) & 1u) && f0 != 0.0) || (!((chg >> (2 * it + 1)) & 1u) && f1 != 0.0);
            }
        }
    }
    if (mine) atomicOr(&s_set, mine);
    if (chg) atomicAdd(&s_count, (unsigned)__popc(chg));
    const int nonzero = __syncthreads_or(any ? 1 : 0);      // (a barrier: s_set and s_count are complete after it)
    if (tid == 0) {
        brick_ids[e] = s_set;
        if (PHASE && (have_f || nonzero)) summary[e] = nonzero ? 1u : 0u;
        atomicAdd(counter, (unsigned long long)s_count);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mapbricksets(const uint8_t *__restrict__ flags, const unsigned *__restrict__ bricks,
                                                               const uint8_t *__restrict__ ids, unsigned *__restrict__ brick_ids,
                                                               Lay L, int nby, int nbz)
{
    __shared__ unsigned s_set;
    const int bk = (int)blockIdx.x, bj = (int)blockIdx.y, bi = (int)blockIdx.z;
    const unsigned tid = threadIdx.x;
    if (tid == 0) s_set = 0u;
    __syncthreads();
    const bool solid = brick_all_solid(bricks, L, bi, bj, bk);
    unsigned mine = 0u;
#pragma unroll 2
    for (int it = 0; it < kPhaseIter; ++it) {
        PhaseCell c = phase_cell(L, bi, bj, bk, it, tid);
        if (!c.in) continue;
        c.m = solid ? c.in : (load_mask_pair<VEC>(flags, c) & c.in);
        if (!c.m) continue;
        const unsigned idp = load_id_pair<VEC>(ids, c);
        if (c.m & 1u) mine |= 1u << id_of(idp, 0);
        if (c.m & 2u) mine |= 1u << id_of(idp, 1);
    }
    if (mine) atomicOr(&s_set, mine);
    __syncthreads();
    if (tid == 0) brick_ids[((long)bi * nby + bj) * nbz + bk] = s_set;
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_matmap_transition(int nmat, const int *h_to, const double *h_T_at, const adi_phase_change *h_laws, const int *h_on,
                          const double *d_T, uint8_t *d_ids, const uint8_t *d_flags, const uint32_t *d_bricks,
                          const uint8_t *d_mask, const uint8_t *d_dir_mask, double *d_f, uint32_t *d_summary,
                          uint32_t *d_brick_ids, unsigned long long *d_count, int nx, int ny, int nz, long plane_stride,
                          double dx, const double *h_C, const int *h_mode, const double *h_scalar,
                          const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                          const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, void *stream)
{
#pragma clang fp contract(off)
    const char *who = "adi_matmap_transition";
    ADI_REQUIRE(h_to && h_T_at && d_T && d_ids && d_flags && d_mask && d_brick_ids && d_count && h_C && h_mode && h_scalar &&
                    q_mode && q_scalar && d_coeff && d_qflux,
                "%s: null argument", who);
    const bool phase = h_laws != nullptr;
    ADI_REQUIRE(phase ? (h_on && d_f && d_summary) : (!d_f && !d_summary),
                "%s: the laws, d_f and d_summary go together (all of them, or none)", who);
    ADI_REQUIRE((const void *)d_T != (const void *)d_f, "%s: d_f aliases d_T", who);
    ADI_REQUIRE(isfinite(dx) && dx > 0.0, "%s: dx must be finite and > 0", who);
    if (int rc = check_tables(who, nmat, nullptr, h_C)) return rc;
    MapTransTable tab = {};
    const double V = dx * dx * dx;
    for (int m = 0; m < kMapMaxMat; ++m) tab.v[TR_C * kMapMaxMat + m] = m < nmat ? h_C[m] * V : 1.0;
    for (int m = 0; m < nmat; ++m) {
        if (h_to[m] < 0) continue;
        ADI_REQUIRE(h_to[m] < nmat && h_to[m] != m, "%s: material %d turns into %d (another of the %d materials)", who, m,
                    h_to[m], nmat);
        ADI_REQUIRE(isfinite(h_T_at[m]), "%s: the threshold of material %d is not finite", who, m);
        tab.to |= (unsigned)h_to[m] << (4 * m);
        tab.v[TR_TAT * kMapMaxMat + m] = h_T_at[m];
        tab.ruled |= 1u << m;
    }
    if (phase)
        for (int m = 0; m < nmat; ++m) {
            if (!h_on[m]) continue;
            PhaseLaw w;
            if (int rc = make_phase_law(who, h_laws[m], 1.0, &w)) return rc;   // (Ts and dT alone are used, as the seed's)
            tab.v[TR_TS * kMapMaxMat + m] = w.Ts; tab.v[TR_DT * kMapMaxMat + m] = w.dT;
            tab.on |= 1u << m;
        }
    PhaseLaunch g;
    if (int rc = make_phase_launch(who, nx, ny, nz, plane_stride, &g)) return rc;
    MapFaceSpec h, q;
    if (int rc = make_face_specs(who, h_mode, h_scalar, d_h_field, q_mode, q_scalar, d_q_field, &h, &q)) return rc;
    for (int a = 0; a < 3; ++a) ADI_REQUIRE(d_coeff[a] && d_qflux[a], "%s: null output", who);
    const MapTransPacks pk = {d_coeff[0], d_coeff[1], d_coeff[2], d_qflux[0], d_qflux[1], d_qflux[2]};
    const double A = dx * dx;
    const bool vec = map_pair_vec(g.L, d_flags, d_ids, d_T, d_f);
    by_bool(vec, [&](auto v) {
        by_bool(phase, [&](auto ph) {
            hipLaunchKernelGGL((k_maptransition<v.value, ph.value>), g.grid, dim3(256), 0, as_stream(stream), tab, d_T,
                               d_ids, d_flags, d_bricks, d_mask, d_dir_mask, d_f, (unsigned *)d_summary,
                               (unsigned *)d_brick_ids, d_count, g.L, g.nby, g.nbz, A, h, q, pk);
        });
    });
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_matmap_brick_sets(const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids, uint32_t *d_brick_ids, int nx,
                          int ny, int nz, long plane_stride, void *stream)
{
    ADI_REQUIRE(d_flags && d_ids && d_brick_ids, "adi_matmap_brick_sets: null argument");
    PhaseLaunch g;
    if (int rc = make_phase_launch("adi_matmap_brick_sets", nx, ny, nz, plane_stride, &g)) return rc;
    if (map_pair_vec(g.L, d_flags, d_ids, nullptr, nullptr))
        hipLaunchKernelGGL(k_mapbricksets<true>, g.grid, dim3(256), 0, as_stream(stream), d_flags, d_bricks, d_ids,
                           (unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    else
        hipLaunchKernelGGL(k_mapbricksets<false>, g.grid, dim3(256), 0, as_stream(stream), d_flags, d_bricks, d_ids,
                           (unsigned *)d_brick_ids, g.L, g.nby, g.nbz);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"
