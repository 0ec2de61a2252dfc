// adi_condense.hip -- K5: slab decomposition along memory axis 0 (BASELINE.json: "2/4/8-GPU runs exchange one ghost plane
// per sweep").  Pass A of a sweep whose lines continue on neighbouring GPUs condenses every local line to six numbers:
//   k_condense_strided, k_condense_strided_fast   the tiled kernels (whole segments), GENERAL and FAST
//   k_condense_generic                            one thread per line, any n; also the listed lines of the dot-product form
//   k_classify_lines0, k_dots_finish              pass A from the dot products the marching explicit kernel accumulated
//                                                 (adi_explicit_rhs_dots, adi_explicit.hip)
// The interface kernels solve the reduced system (adi_interface.hip); pass B is the ordinary sweep with the two boundary
// values injected (adi_sweep_strided.hip).  No counterpart in the reference (single process); the per-line algebra is
// thomas_solve's (adi3d_numba_coeff.py:121-130) block elimination.
#include <type_traits>

#include "adi_cart_host.hpp"
#include "adi_strided_dev.hpp"

namespace adi {

// ------------------------------------------------------------------------------------------------
// K5a: slab condensation (pass A of a sweep whose lines continue on neighbouring GPUs).  Same loads and
// per-thread work as K2's phase 1, but every thread condenses ALL its M rows and the Lp blocks of a line
// are merged by an ordered tree reduction; lane 0 writes the six numbers that describe the slab's part of
// the line to its neighbours:  x_first = gF - aF*xl - cF*xr,  x_last = gL - aL*xl - cL*xr.
// Requires n % M == 0 (whole segments).  cond: [6][nlines] dense.
// ------------------------------------------------------------------------------------------------
// lane 0 of every line: ordered merge of the Lp block condensations -> six numbers per line
__device__ __forceinline__ void tile_reduce_store(double *sm, int tid, int kk, int sg, int Lp, int LINES, const Cond &k,
                                                  int nblk, long to, int ti, const LineGeom &g, long nlines,
                                                  double *__restrict__ cond)
{
    const int ld = Lp + 1;
    const int plane = LINES * ld;
    {
        const int w = kk * ld + sg;
        sm[w] = k.gF; sm[plane + w] = k.aF; sm[2 * plane + w] = k.cF;
        sm[3 * plane + w] = k.gL; sm[4 * plane + w] = k.aL; sm[5 * plane + w] = k.cL;
    }
    __syncthreads();
    const int pl = tid >> (__ffs(Lp) - 1), ps = tid & (Lp - 1);   // Lp is a power of two
    const int w = pl * ld + ps;
    Cond q;
    q.gF = sm[w]; q.aF = sm[plane + w]; q.cF = sm[2 * plane + w];
    q.gL = sm[3 * plane + w]; q.aL = sm[4 * plane + w]; q.cL = sm[5 * plane + w];
    q = reduce_cond(q, ps, Lp, nblk);
    const int kc2 = ti * LINES + pl;
    if (ps == 0 && kc2 < g.n_inner) {
        const long id = to * (long)g.n_inner + kc2;
        cond[id] = q.gF; cond[nlines + id] = q.aF; cond[2 * nlines + id] = q.cF;
        cond[3 * nlines + id] = q.gL; cond[4 * nlines + id] = q.aL; cond[5 * nlines + id] = q.cL;
    }
}

template <int M, bool HAS_DIR, bool HAS_Q, bool FUSE = false>
__device__ __forceinline__ void condense_tile_general(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
    const uint8_t *__restrict__ dmask, const double *__restrict__ dval, const double *__restrict__ qf,
    double *__restrict__ cond, long nlines, const LineGeom &g, int Lp, int LINES, int tiles_inner, long tile,
    const SweepScal &s, double *sm, const Fuse &fz, const int tid)
{
    const long to = (long)((unsigned)tile / (unsigned)tiles_inner);   // block-uniform, < 2^31 tiles
    const int ti = (int)(tile - to * tiles_inner);
    const int kk = tid & (LINES - 1), sg = tid >> (__ffs(LINES) - 1);   // LINES is a power of two
    const int kcol = ti * LINES + kk;
    const bool active = kcol < g.n_inner;
    const long base = to * g.outer_stride + kcol;
    const int r0 = sg * M;
    double a[M], b[M], c[M], d[M];
    {
        // same assembly as the solve pass, but the end couplings stay in a[0] / c[n-1] (they are the
        // aF, aL / cF, cL of the slab)
        SegRaw<M> R;
        load_segment_raw<M, HAS_DIR, HAS_Q, FUSE>(in, flags, coeff, dmask, dval, qf, g, base, r0, active, s, R, fz, nullptr, tid);
        if (FUSE && fz.r0_out != nullptr) {
#pragma unroll
            for (int r = 0; r < M; ++r)
                if (active && (r0 + r) < g.n) fz.r0_out[base + (long)(r0 + r) * g.stride] = R.vin[r];
        }
#pragma unroll
        for (int r = 0; r < M; ++r) assemble_one<M, HAS_DIR, HAS_Q>(R, r, g.lbit, s, a[r], b[r], c[r], d[r]);
    }
    Cond k;
    condense_full<M>(a, b, c, d, k);
    tile_reduce_store(sm, tid, kk, sg, Lp, LINES, k, g.n / M, to, ti, g, nlines, cond);
}

template <int M, bool HAS_DIR, bool HAS_Q, bool FUSE = false>
__global__ __launch_bounds__(M <= 8 ? 1024 : 512) void k_condense_strided(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
    const uint8_t *__restrict__ dmask, const double *__restrict__ dval, const double *__restrict__ qf,
    double *__restrict__ cond, long nlines, LineGeom g, int Lp, int LINES, int tiles_inner, long ntiles,
    SweepScal s, const unsigned *__restrict__ queue, int ratio, int tiles_inner_f, Fuse fz)
{
    extern __shared__ __align__(16) double sm[];
    if (queue == nullptr) {
        condense_tile_general<M, HAS_DIR, HAS_Q, FUSE>(in, flags, coeff, dmask, dval, qf, cond, nlines, g, Lp, LINES,
                                                       tiles_inner, xcd_chunk_tile(blockIdx.x, ntiles), s, sm, fz, (int)threadIdx.x);
    } else {
        const long cnt = (long)queue[0] * ratio;
        for (long i = blockIdx.x; i < cnt; i += gridDim.x) {
            const long u = queue[1 + (unsigned)i / (unsigned)ratio];
            const long to = (long)((unsigned)u / (unsigned)tiles_inner_f);
            const long tig = (u - to * tiles_inner_f) * ratio + ((unsigned)i % (unsigned)ratio);
            int tid = (int)threadIdx.x;
            asm volatile("" : "+v"(tid));      // (keeps the per-row offsets out of the loop-carried state, see k_sweep_strided)
            if (tig < tiles_inner)
                condense_tile_general<M, HAS_DIR, HAS_Q, FUSE>(in, flags, coeff, dmask, dval, qf, cond, nlines, g, Lp,
                                                               LINES, tiles_inner, to * tiles_inner + tig, s, sm, fz, tid);
            __syncthreads();
        }
    }
}

// FAST pass A: uniform-interior segments (see k_sweep_strided_fast); the block of a thread = its M-1 uniform
// interior rows merged with its general separator row.
template <int M, bool HAS_DIR, bool HAS_Q, bool FUSE = false>
__global__ __launch_bounds__(512, FUSE ? ADI_FUSE_OCC : 1) void k_condense_strided_fast(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
    const uint8_t *__restrict__ dmask, const double *__restrict__ dval, const double *__restrict__ qf,
    double *__restrict__ cond, long nlines, LineGeom g, int Lp, int LINES, int tiles_inner, long ntiles,
    SweepScal s, unsigned *__restrict__ queue, UniC<M> U, Fuse fz)
{
    extern __shared__ __align__(16) double sm[];
    const int tid = threadIdx.x;
    long tile = xcd_chunk_tile(blockIdx.x, ntiles);
    if (FUSE && fz.kg > 0) tile = tile_jfast(tile, fz);
    const long to = (long)((unsigned)tile / (unsigned)tiles_inner);   // block-uniform, < 2^31 tiles
    const int ti = (int)(tile - to * tiles_inner);
    const int kk = tid & (LINES - 1), sg = tid >> (__ffs(LINES) - 1);   // LINES is a power of two
    const int kcol = ti * LINES + kk;
    const bool active = kcol < g.n_inner;
    const long base = to * g.outer_stride + kcol;
    const int r0 = sg * M;

    double d[M];
    unsigned f0, fS;
    bool dirS;
    // block-uniform tile base (scalar) + one 32-bit per-thread offset for every row of every array
    const long tbase = to * g.outer_stride + (long)ti * LINES;
    const unsigned voff = (unsigned)((long)r0 * g.stride + kk);
    const bool pad = r0 >= g.n;                    // this thread's segment lies beyond the end of the line
    int kind = SEG_NONE, Lm = 0;                   // segment class (classify_mixed) and length of a mixed run
    bool lane_fast;
    if constexpr (FUSE) {
        // whole tiles only (block-uniform): anything else goes to the GENERAL kernel before a single load is issued
        if (LINES != 16 || (ti + 1) * LINES > g.n_inner || g.n % M != 0) {
            if (tid == 0) enqueue_unit(queue, (unsigned)tile);
            return;
        }
        // a padding segment (line with fewer than Lp segments) re-reads segment 0 -- valid addresses, values unused
        const int r0e = pad ? 0 : r0;
        lane_fast = fast_segment_load_fused<M, HAS_DIR>(in, flags + tbase, HAS_DIR ? dmask + tbase : dmask, g,
                                                        pad ? (unsigned)kk : voff, r0e, kk, tbase, fz, d, f0, fS, dirS, kind,
                                                        Lm) || pad;
        if (pad) kind = SEG_PAD;
    } else {
        // whole tiles whose rows fit 31-bit byte offsets take the buffer-addressed loader (block-uniform choice)
        const bool whole = kBufStrided && (ti + 1) * LINES <= g.n_inner && Lp * M == g.n &&
                           (long)g.n * g.stride * 8 < 0x7fffffffL;
        if (whole)
            lane_fast = fast_segment_load_buf<M, HAS_DIR>(in + tbase, flags + tbase, HAS_DIR ? dmask + tbase : dmask, g, voff, d,
                                                          f0, fS, dirS, kind, Lm);
        else
            lane_fast = fast_segment_load<M, HAS_DIR>(in + tbase, flags + tbase, HAS_DIR ? dmask + tbase : dmask, g, voff, r0,
                                                      active, d, f0, fS, dirS, kind, Lm);
    }
    if (pad) { f0 = 0; fS = 0; dirS = false; }       // (the fused loader showed a padding thread segment 0's flags)
    if (!__syncthreads_and(lane_fast)) {
        if (tid == 0) enqueue_unit(queue, (unsigned)tile);
        return;
    }
    if constexpr (FUSE) {
        if (fz.r0_out != nullptr && !pad) {
            const __amdgpu_buffer_rsrc_t rO = __builtin_amdgcn_make_buffer_rsrc((void *)(fz.r0_out + tbase), 0, 0x7fffffff,
                                                                                0x00020000);
#pragma unroll
            for (int r = 0; r < M; ++r) buf_store_f64(rO, voff * 8u, (unsigned)r * (unsigned)(g.stride * 8), d[r], s.nt != 0);
        }
    }
    double a0, b0, aS, bS, cS;
    fast_segment_ends<M, HAS_DIR, HAS_Q>(coeff, dval, qf, g, base, r0, f0, fS, dirS, s, d, a0, b0, aS, bS, cS);
    Cond ki;
    double kappa;
    condense_uniform<M>(U, a0, b0, d, ki, kappa);
    if (pad) {                                     // finite values; tile_reduce_store ignores blocks >= n / M
        ki.gF = ki.aF = ki.cF = ki.gL = ki.aL = ki.cL = 0.0;
        aS = 0.0; bS = 1.0; cS = 0.0; d[M - 1] = 0.0;
    } else if (kind == SEG_OFF) {                  // segment outside the mask: M identity rows
        ki.gF = d[0]; ki.gL = d[M - 2];
        ki.aF = ki.cF = ki.aL = ki.cL = 0.0;
        aS = 0.0; bS = 1.0; cS = 0.0;
    } else if (kind >= SEG_TAIL) {                 // the surface crosses the segment once
        double2 bmod;
        mixed_lane_condense<M, HAS_Q>(kind, Lm, U, s, coeff + base + (long)r0 * g.stride,
                                      HAS_Q ? qf + base + (long)r0 * g.stride : qf, g.stride, a0, b0, d, bmod, ki);
    }
    const double ib = frcp(bS);
    Cond rowc;
    rowc.gF = rowc.gL = d[M - 1] * ib;
    rowc.aF = rowc.aL = aS * ib;
    rowc.cF = rowc.cL = cS * ib;
    const Cond k = merge_cond(ki, rowc);
    tile_reduce_store(sm, tid, kk, sg, Lp, LINES, k, g.n / M, to, ti, g, nlines, cond);
}

// K5b: generic slab condensation, one thread per line, two serial recurrences (any n; reads rows twice).
template <bool HAS_DIR, bool HAS_Q>
__global__ __launch_bounds__(256) void k_condense_generic(
    const double *__restrict__ in, const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
    const uint8_t *__restrict__ dmask, const double *__restrict__ dval, const double *__restrict__ qf,
    double *__restrict__ cond, long nlines, LineGeom g, long inner_stride, SweepScal s,
    const unsigned *__restrict__ list = nullptr, long lb = 0, long nsel = 0)
{
    // list != nullptr: only the listed lines that fall into [lb, lb + nsel), written to a [6][nsel] block
    long lid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long oid = lid, ostr = nlines;
    if (list != nullptr) {
        if (lid >= (long)list[0]) return;
        lid = list[1 + lid];
        if (lid < lb || lid >= lb + nsel) return;
        oid = lid - lb; ostr = nsel;
    }
    if (lid >= nlines) return;
    const long o = lid / g.n_inner, kc = lid - o * g.n_inner;
    const long base = o * g.outer_stride + kc * inner_stride;
    const int n = g.n;
    double a0 = 0.0, cn = 0.0;
    // top-down: last component of B^-1 d, B^-1 e_0 ; 1/pivot_last
    double ip = 0.0, y = 0.0, e = 1.0, cprev = 0.0;
    for (int r = 0; r < n; ++r) {
        const long p = base + (long)r * g.stride;
        const unsigned f = flags[p];
        double a, b, c, d;
        assemble_row<HAS_DIR, HAS_Q>(f & 1u, (f >> g.lbit) & 1u, (f >> (g.lbit + 1)) & 1u, HAS_DIR && dmask[p] != 0,
                                     in[p], coeff[p], HAS_DIR ? dval[p] : 0.0, HAS_Q ? qf[p] : 0.0, s, a, b, c, d);
        if (r == 0) { a0 = a; ip = 1.0 / b; y = d; }
        else { const double w = a * ip; ip = 1.0 / (b - w * cprev); y = d - w * y; e = -w * e; }
        cprev = c;
        if (r == n - 1) cn = c;
    }
    const double gL = y * ip, aL = a0 * (e * ip), cL = cn * ip;
    // bottom-up
    double jp = 0.0, z = 0.0, f2 = 1.0, anext = 0.0;
    for (int r = n - 1; r >= 0; --r) {
        const long p = base + (long)r * g.stride;
        const unsigned f = flags[p];
        double a, b, c, d;
        assemble_row<HAS_DIR, HAS_Q>(f & 1u, (f >> g.lbit) & 1u, (f >> (g.lbit + 1)) & 1u, HAS_DIR && dmask[p] != 0,
                                     in[p], coeff[p], HAS_DIR ? dval[p] : 0.0, HAS_Q ? qf[p] : 0.0, s, a, b, c, d);
        if (r == n - 1) { jp = 1.0 / b; z = d; }
        else { const double w = c * jp; jp = 1.0 / (b - w * anext); z = d - w * z; f2 = -w * f2; }
        anext = a;
    }
    cond[oid] = z * jp; cond[ostr + oid] = a0 * jp; cond[2 * ostr + oid] = cn * (f2 * jp);
    cond[3 * ostr + oid] = gL; cond[4 * ostr + oid] = aL; cond[5 * ostr + oid] = cL;
}

// ---- pass A from the dot products (slab decomposition) -----------------------------------------------------------------
// A line is "uniform" for the axis-0 sweep when its rows 1..n-2 are in the mask with both axis neighbours and are not
// Dirichlet, its end rows are in the mask (not Dirichlet) with their inward neighbour, and at most one end row differs
// from the interior row (line start/end, Robin coefficient).  cls[line] = 1 for those; the others are appended to
// list[1..] (list[0] = count) and condensed by k_condense_generic from the stored R0.
__global__ __launch_bounds__(256) void k_classify_lines0(const uint8_t *__restrict__ flags,
                                                         const uint8_t *__restrict__ dmask, Lay L,
                                                         uint8_t *__restrict__ cls, unsigned *__restrict__ list)
{
    const long nlines = (long)L.ny * L.nz;
    const long lid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lid >= nlines) return;
    const int n = L.nx;
    bool ok = n >= 2;
    unsigned f0 = 0, fn = 0;
    for (int r = 0; r < n; ++r) {
        const long p = (long)r * L.sx + lid;
        const unsigned f = flags[p];
        if (dmask != nullptr && dmask[p] != 0) ok = false;
        if (r == 0) { f0 = f; ok = ok && ((f & 5u) == 5u); }                 // in mask, next row in mask
        else if (r == n - 1) { fn = f; ok = ok && ((f & 3u) == 3u); }        // in mask, previous row in mask
        else ok = ok && ((f & 7u) == 7u);
    }
    // an end row without its outward neighbour is a modified row (b = 1 + tg + dt*coeff): at most one per line
    if (ok && !(f0 & 2u) && !(fn & 4u)) ok = false;
    cls[lid] = ok ? 1 : 0;
    if (!ok) list[1 + atomicAdd(&list[0], 1u)] = (unsigned)lid;
}

// cond[6][nsel] of the lines [lb, le) from the partial dot products (uniform lines only; the others keep what
// k_condense_generic wrote).  Formulas: condense_uniform (adi_core.hpp) applied to the whole line.
template <bool HAS_Q>
__global__ __launch_bounds__(256) void k_dots_finish(const double *__restrict__ part, int nchunk,
                                                     const double *__restrict__ wu, const uint8_t *__restrict__ cls,
                                                     const uint8_t *__restrict__ flags, const double *__restrict__ coeff,
                                                     const double *__restrict__ qf, Lay L, SweepScal s, long lb, long le,
                                                     double *__restrict__ cond)
{
    const long nlines = (long)L.ny * L.nz, nsel = le - lb;
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= nsel) return;
    const long lid = lb + id;
    if (!cls[lid]) return;
    const int n = L.nx;
    double gu = 0.0, gv = 0.0;
    for (int c = 0; c < nchunk; ++c) {                      // fixed order: deterministic
        gu += part[(long)c * 2 * nlines + lid];
        gv += part[((long)c * 2 + 1) * nlines + lid];
    }
    const long pF = lid, pL = (long)(n - 1) * L.sx + lid;
    const unsigned fF = flags[pF], fL = flags[pL];
    const bool loF = (fF & 2u) != 0, hiL = (fL & 4u) != 0;   // the line continues below / above the slab
    const double p0 = wu[0], pn = wu[n - 1];
    const double bu = 1.0 + 2.0 * s.tg;
    // right-hand side terms of the end rows beyond R0 (assemble_row): dt*q + dt*coeff*Tinf on axis-exposed cells
    const double coF = loF ? 0.0 : coeff[pF], coL = hiL ? 0.0 : coeff[pL];
    double xF = s.dt * coF * s.Tinf, xL = s.dt * coL * s.Tinf;
    if (HAS_Q) { if (!loF) xF += s.dt * qf[pF]; if (!hiL) xL += s.dt * qf[pL]; }
    gu += p0 * xF + pn * xL;                                 // (U^-1 d)_0
    gv += pn * xF + p0 * xL;                                 // (U^-1 d)_{n-1}
    const double a0 = loF ? -s.tg : 0.0, cn = hiL ? -s.tg : 0.0;
    double gF, aF, cF, gL, aL, cL;
    if (!loF) {            // row 0 modified: b0 = 1 + tg + dt*coF
        const double delta = (1.0 + s.tg + s.dt * coF) - bu;
        const double kappa = delta / (1.0 + delta * p0);
        const double f1 = 1.0 - kappa * p0, kpl = kappa * pn;
        gF = gu * f1;            gL = gv - kpl * gu;
        aF = 0.0;                aL = 0.0;
        cF = cn * (pn - kpl * p0); cL = cn * (p0 - kpl * pn);
    } else if (!hiL) {     // row n-1 modified
        const double delta = (1.0 + s.tg + s.dt * coL) - bu;
        const double kappa = delta / (1.0 + delta * p0);
        const double f1 = 1.0 - kappa * p0, kpl = kappa * pn;
        gL = gv * f1;            gF = gu - kpl * gv;
        cL = 0.0;                cF = 0.0;
        aL = a0 * (pn - kpl * p0); aF = a0 * (p0 - kpl * pn);
    } else {
        gF = gu; gL = gv;
        aF = a0 * p0; cF = cn * pn; aL = a0 * pn; cL = cn * p0;
    }
    cond[id] = gF; cond[nsel + id] = aF; cond[2 * nsel + id] = cF;
    cond[3 * nsel + id] = gL; cond[4 * nsel + id] = aL; cond[5 * nsel + id] = cL;
}

// ------------------------------------------------------------------------------------------------
// host-side launch logic
// ------------------------------------------------------------------------------------------------
// Pass A hands its kernels null for the arrays their build (by_variant, adi_cart_host.hpp) does not read.
static SweepArgs read_arrays(bool has_dir, bool has_q, SweepArgs a)
{
    if (!has_dir) { a.dmask = nullptr; a.dval = nullptr; }
    if (!has_q) a.qf = nullptr;
    return a;
}

template <int MF, bool HAS_DIR, bool HAS_Q, bool FUSE>
static void launch_condense_fast(const StridedPlan &P, const SweepArgs &a, double *cond, long nlines, const LineGeom &g,
                                 SweepScal s, unsigned *queue, hipStream_t st, const Fuse &fz)
{
    hipLaunchKernelGGL((k_condense_strided_fast<MF, HAS_DIR, HAS_Q, FUSE>), dim3((unsigned)P.ntiles_f),
                       dim3(P.lines_f * P.Lpf), P.lds_f, st, a.in, a.flags, a.coeff, a.dmask, a.dval, a.qf, cond, nlines, g,
                       P.Lpf, P.lines_f, P.tiles_inner_f, P.ntiles_f, s, queue, make_unic<MF>(s.tg), fz);
}

template <int M, bool HAS_DIR, bool HAS_Q, bool FUSE>
static void launch_condense(const StridedPlan &P, const SweepArgs &a, double *cond, long nlines, const LineGeom &g,
                            SweepScal s, unsigned *queue, hipStream_t st, const Fuse &fz)
{
    unsigned ggrid = (unsigned)P.ntiles_g;
    if (queue != nullptr) {
        (void)hipMemsetAsync(queue, 0, sizeof(unsigned), st);
        // (the 32-row wide tiling is not built with the fused loader: the host plans fused passes without it)
        if (P.Mf == 32) launch_condense_fast<32, HAS_DIR, HAS_Q, false>(P, a, cond, nlines, g, s, queue, st, fz);
        else if (P.Mf == 16) launch_condense_fast<16, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz);
        else launch_condense_fast<8, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz);
        ggrid = P.ntiles_g < 1024 ? (unsigned)P.ntiles_g : 1024u;
    }
    hipLaunchKernelGGL((k_condense_strided<M, HAS_DIR, HAS_Q, FUSE>), dim3(ggrid), dim3(P.lines_g * P.Lpg), P.lds_g, st,
                       a.in, a.flags, a.coeff, a.dmask, a.dval, a.qf, cond, nlines, g, P.Lpg, P.lines_g, P.tiles_inner_g,
                       P.ntiles_g, s, queue, P.ratio, P.tiles_inner_f, fz);
}

// the tiled kernels by rows per thread of the GENERAL kernel
template <bool HAS_DIR, bool HAS_Q, bool FUSE>
static void launch_condense_rows(const StridedPlan &P, const SweepArgs &a, double *cond, long nlines, const LineGeom &g,
                                 SweepScal s, unsigned *queue, hipStream_t st, const Fuse &fz)
{
    switch (P.Mg) {
        case 2: launch_condense<2, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz); break;
        case 4: launch_condense<4, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz); break;
        case 8: launch_condense<8, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz); break;
        default: launch_condense<16, HAS_DIR, HAS_Q, FUSE>(P, a, cond, nlines, g, s, queue, st, fz); break;
    }
}

// the serial two-recurrence condensation: of every line (list == nullptr), or of the lines in `list` that fall into
// [lb, lb + nsel) (grid sized for all lines, the kernel returns beyond the list's count)
template <bool HAS_DIR, bool HAS_Q>
static void launch_condense_generic(const SweepArgs &a, double *cond, long nlines, const LineGeom &g, long inner_stride,
                                    SweepScal s, const unsigned *list, long lb, long nsel, hipStream_t st)
{
    hipLaunchKernelGGL((k_condense_generic<HAS_DIR, HAS_Q>), dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, st, a.in,
                       a.flags, a.coeff, a.dmask, a.dval, a.qf, cond, nlines, g, inner_stride, s, list, lb, nsel);
}

template <bool HAS_DIR, bool HAS_Q>
static int condense_dispatch(int axis, const SweepArgs &a, const Lay &L, SweepScal s, double *cond, void *work,
                             size_t work_bytes, hipStream_t st, const Fuse *fzp)
{
    long inner_stride;
    const LineGeom g = line_geom(axis, L, &inner_stride);
    const long nlines = (long)g.n_inner * g.n_outer;
    const int n = g.n;
    bool tiled = false;
    StridedPlan P;
    if (axis != 2 && n <= kMaxFastLine) {
        P = strided_plan(g, s.sparse != 0 && work != nullptr, fzp == nullptr, fzp != nullptr);
        tiled = (n % P.Mg == 0) && (n / P.Mg <= 64);     // the tiled kernels need whole segments
    }
    if (fzp != nullptr && (axis != 0 || !tiled))
        return set_err(ADI_ERR_UNSUPPORTED, "fused explicit + condensation: axis 0, whole segments only (n = %d)", n);
    if (!tiled) {
        launch_condense_generic<HAS_DIR, HAS_Q>(a, cond, nlines, g, inner_stride, s, nullptr, 0, 0, st);
        return ADI_OK;
    }
    unsigned *queue = nullptr;
    if (P.Mf && use_fast(s, work, work_bytes, P.ntiles_f)) queue = (unsigned *)work;
    else if (P.Mf) P = strided_plan(g, false, false);
    if (fzp != nullptr) {
        Fuse fz = *fzp;
        if (queue != nullptr && !fuse_fast_ok(P, L, fz)) { queue = nullptr; P = strided_plan(g, false, false); }
        fuse_tile_order(fz, P, L);
        launch_condense_rows<HAS_DIR, HAS_Q, true>(P, a, cond, nlines, g, s, queue, st, fz);
    } else {
        launch_condense_rows<HAS_DIR, HAS_Q, false>(P, a, cond, nlines, g, s, queue, st, Fuse());
    }
    return ADI_OK;
}

int condense_sweep(bool has_dir, bool has_q, int axis, const SweepArgs &a, const Lay &L, const SweepScal &s, double *cond,
                   void *work, size_t work_bytes, hipStream_t st, const Fuse *fz)
{
    const SweepArgs v = read_arrays(has_dir, has_q, a);
    return by_variant(has_dir, has_q, [&](auto dir, auto q) {
        return condense_dispatch<dir.value, q.value>(axis, v, L, s, cond, work, work_bytes, st, fz);
    });
}

}  // namespace adi

using namespace adi;

extern "C" {

int adi_axis0_classify(const uint8_t *d_flags, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                       uint8_t *d_cls, unsigned *d_list, void *stream)
{
    ADI_REQUIRE(d_flags && d_cls && d_list, "adi_axis0_classify: null argument");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    hipStream_t st = as_stream(stream);
    ADI_HIP_TRY(hipMemsetAsync(d_list, 0, sizeof(unsigned), st));
    const long nlines = (long)ny * nz;
    hipLaunchKernelGGL(k_classify_lines0, dim3((unsigned)((nlines + 255) / 256)), dim3(256), 0, st, d_flags, d_dir_mask, L,
                       d_cls, d_list);
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

int adi_axis0_dots_finish(int variant, const double *d_part, const double *d_weights, const uint8_t *d_cls,
                          const unsigned *d_list, const double *d_R0, const uint8_t *d_flags, const double *d_coeff,
                          const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux, int nx, int ny,
                          int nz, long plane_stride, double theta, double gam, double dt, double Tinf, long line_begin,
                          long line_end, double *d_cond, void *stream)
{
    bool has_dir, has_q;
    if (int rc = variant_flags(variant, &has_dir, &has_q)) return rc;
    ADI_REQUIRE(d_part && d_weights && d_cls && d_list && d_R0 && d_flags && d_coeff && d_cond,
                "adi_axis0_dots_finish: null argument");
    ADI_REQUIRE(!has_dir || (d_dir_mask && d_dir_val), "adi_axis0_dots_finish: variant needs Dirichlet arrays");
    ADI_REQUIRE(!has_q || d_qflux, "adi_axis0_dots_finish: variant needs the flux array");
    Lay L;
    if (int rc = make_lay(nx, ny, nz, plane_stride, &L)) return rc;
    const long nlines = (long)ny * nz;
    ADI_REQUIRE(line_begin >= 0 && line_end <= nlines && line_begin < line_end, "adi_axis0_dots_finish: bad line range");
    SweepScal s;
    s.tg = theta * gam; s.dt = dt; s.Tinf = Tinf; s.sparse = 0; s.box = 0;
    hipStream_t st = as_stream(stream);
    const long nsel = line_end - line_begin;
    const auto finish = has_q ? k_dots_finish<true> : k_dots_finish<false>;
    hipLaunchKernelGGL(finish, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, st, d_part, dots_nchunk(nx), d_weights, d_cls,
                       d_flags, d_coeff, d_qflux, L, s, line_begin, line_end, d_cond);
    // the lines that are not uniform: the serial two-recurrence condensation from the stored R0
    long inner_stride;
    const LineGeom g = line_geom(0, L, &inner_stride);
    const SweepArgs v = read_arrays(has_dir, has_q, {d_R0, d_flags, d_coeff, d_dir_mask, d_dir_val, d_qflux});
    by_variant(has_dir, has_q, [&](auto dir, auto q) {
        launch_condense_generic<dir.value, q.value>(v, d_cond, nlines, g, inner_stride, s, d_list, line_begin, nsel, st);
    });
    ADI_CHECK_LAUNCH();
    return ADI_OK;
}

}  // extern "C"

