// adi_cyl_monitor_dev.hpp -- what the kernels of the cylindrical field monitor (adi_cyl_monitor.hip) and their host twin share
// (include/adi_hip.h, "Field monitor of the cylindrical step"): the regions as they travel by value, the plan of a record --
// every argument rule, the chunks a region can meet, the offsets in the partial buffer, the launch box --, the index and
// per-cell code of a pair, the keys of the extrema, r_i, and the host loop that performs the operations of the three kernels
// in their order.  The plan and the host loop are host arithmetic alone (no HIP call), so a stand-alone program can run them
// under a sanitizer (scripts/cyl_monitor_host_check.cpp).
// A plane of radius i is cut into pairs q = j * per_line + p of the cells (j, 2p), (j, 2p + 1), per_line = ceil(nz / 2), and
// into chunks of 256 consecutive pairs: the order of every sum follows from that and from the region's box alone.
#pragma once
#include <vector>

#include "adi_cyl_extras_dev.hpp"

namespace adi {

constexpr int kCylMonRegions = ADI_MONITOR_MAX_REGIONS;
constexpr int kCylMonWords = ADI_CYL_MONITOR_PARTIAL_WORDS;   // per record: sum_T, sum_extra, key_min, key_max, cells
static_assert(ADI_CYL_MONITOR_REGION_WORDS == 8 && ADI_CYL_MONITOR_PARTIAL_WORDS == 5, "cylindrical monitor row layout");
constexpr long long kCylMonKeyMax = 0x7fffffffffffffffLL;

struct CylMonRegions {
    int n;
    int i0[kCylMonRegions], i1[kCylMonRegions];          // radii, half open
    int j0[kCylMonRegions], nj[kCylMonRegions];          // first phi cell and count: the cells (j0 + d) mod nphi, d < nj
    int k0[kCylMonRegions], k1[kCylMonRegions];          // z cells, half open
    // the chunks a region can meet: those of the pairs of its phi interval [j0, min(j0 + nj, nphi)) -- ca .. cb inclusive -- and,
    // when it wraps, of [0, j0 + nj - nphi) -- wa .. wb (wa > wb: no such interval)
    int ca[kCylMonRegions], cb[kCylMonRegions], wa[kCylMonRegions], wb[kCylMonRegions];
    long off[kCylMonRegions];       // chunk records ahead of the region's: region r holds (i1 - i0) * nchunk of them
    long poff[kCylMonRegions];      // plane records ahead of the region's: region r holds (i1 - i0) of them
};

struct CylMonPlan {
    CylBox g;
    CylMonRegions R;
    unsigned per_line, per_plane, nchunk;
    int ilo, ni, clo, nc;           // the launch box: radii [ilo, ilo + ni), chunks [clo, clo + nc)
    int max_ni;                     // the most radii of one region
    long chunk_records, plane_records;
    long row_words;
};

// the finite doubles in their order, -0.0 below +0.0, as signed 64-bit integers; its own inverse
__host__ __device__ __forceinline__ long long cyl_mon_key(long long bits) { return bits ^ ((bits >> 63) & kCylMonKeyMax); }

// r_i as GridCyl.r computes it: (i + 1/2) exact, one product, one sum
__host__ __device__ __forceinline__ double cyl_mon_r(double r_in, double dr, int i)
{
#pragma clang fp contract(off)
    const double h = (double)i + 0.5;
    const double s = h * dr;
    return r_in + s;
}

__host__ __device__ __forceinline__ bool cyl_mon_meets(const CylMonRegions &R, int r, int c)
{
    return (c >= R.ca[r] && c <= R.cb[r]) || (c >= R.wa[r] && c <= R.wb[r]);
}

// pair q of a plane: its phi cell, its first z cell and which of its two cells exist (bit 0, bit 1)
struct CylMonPair {
    int j, k;
    unsigned in;
};
__host__ __device__ __forceinline__ CylMonPair cyl_mon_pair(unsigned q, unsigned per_line, unsigned per_plane, int nz)
{
    CylMonPair c;
    const bool in = q < per_plane;
    const unsigned j = in ? q / per_line : 0u;
    c.j = (int)j;
    c.k = in ? 2 * (int)(q - j * per_line) : 0;
    c.in = in ? ((c.k + 1 < nz) ? 3u : 1u) : 0u;
    return c;
}

// which cells of the pair (j, k), (j, k + 1) region r holds, out of the cells `m` (bit 0, bit 1) that exist and are active
__host__ __device__ __forceinline__ unsigned cyl_mon_member(const CylMonRegions &R, int r, int nphi, int j, int k, unsigned m)
{
    int d = j - R.j0[r];
    d = d < 0 ? d + nphi : d;
    if (d >= R.nj[r]) return 0u;
    const unsigned s0 = (k >= R.k0[r] && k < R.k1[r]) ? 1u : 0u, s1 = (k + 1 >= R.k0[r] && k + 1 < R.k1[r]) ? 2u : 0u;
    return m & (s0 | s1);
}

// what one thread hands to the reductions for one region: the pair's sum of T and of the extra field (excluded cells and NaN
// of the extra field as +0.0), the keys of its included cells and their number
struct CylMonTerm {
    double sT, sX;
    long long kmin, kmax;
    unsigned cnt;
};
__host__ __device__ __forceinline__ CylMonTerm cyl_mon_term(unsigned inc, double t0, double t1, bool has_x, double x0, double x1)
{
#pragma clang fp contract(off)
    CylMonTerm o;
    const double a0 = (inc & 1u) ? t0 : 0.0, a1 = (inc & 2u) ? t1 : 0.0;
    o.sT = a0 + a1;
    o.sX = 0.0;
    if (has_x) {
        const double b0 = ((inc & 1u) && x0 == x0) ? x0 : 0.0, b1 = ((inc & 2u) && x1 == x1) ? x1 : 0.0;
        o.sX = b0 + b1;
    }
    o.kmin = kCylMonKeyMax;
    o.kmax = -kCylMonKeyMax - 1;
    o.cnt = 0u;
    if (inc & 1u) {
        const long long key = cyl_mon_key(__builtin_bit_cast(long long, t0));
        o.kmin = key; o.kmax = key; o.cnt = 1u;
    }
    if (inc & 2u) {
        const long long key = cyl_mon_key(__builtin_bit_cast(long long, t1));
        o.kmin = key < o.kmin ? key : o.kmin; o.kmax = key > o.kmax ? key : o.kmax; o.cnt += 1u;
    }
    return o;
}

// words of the partial buffer a record of these regions needs (chunk records, then plane records)
inline long cyl_monitor_words(long chunk_records, long plane_records) { return (chunk_records + plane_records) * kCylMonWords; }

// ADI_OK and the plan, or the first rule of the header the arguments break
inline int cyl_monitor_plan(const char *who, int nr, int nphi, int nz, long plane_stride, double r_in, double dr, int nreg,
                            const int *h_regions, int nprobe, const int *h_probes, long capacity, CylMonPlan *P)
{
    ADI_REQUIRE(nreg >= 1 && nreg <= ADI_MONITOR_MAX_REGIONS, "%s: %d regions (1 to %d)", who, nreg, ADI_MONITOR_MAX_REGIONS);
    ADI_REQUIRE(nprobe >= 0 && nprobe <= ADI_MONITOR_MAX_PROBES, "%s: %d probes (0 to %d)", who, nprobe, ADI_MONITOR_MAX_PROBES);
    ADI_REQUIRE(h_regions != nullptr && (nprobe == 0 || h_probes != nullptr), "%s: null argument", who);
    ADI_REQUIRE(capacity >= 1 && capacity < (1L << 31), "%s: capacity %ld is not in [1, 2^31)", who, capacity);
    ADI_REQUIRE(isfinite(r_in) && isfinite(dr) && r_in >= 0.0 && dr > 0.0, "%s: r_in must be >= 0 and dr > 0", who);
    if (int rc = make_cyl_box(who, nr, nphi, nz, plane_stride, &P->g)) return rc;
    P->per_line = (unsigned)((nz + 1) / 2);
    P->per_plane = P->per_line * (unsigned)nphi;
    P->nchunk = (P->per_plane + 255u) / 256u;
    CylMonRegions &R = P->R;
    R.n = nreg;
    long off = 0, poff = 0;
    int ilo = 0x7fffffff, ihi = -1, clo = 0x7fffffff, chi = -1, max_ni = 0;
    for (int r = 0; r < kCylMonRegions; ++r) {
        R.off[r] = off; R.poff[r] = poff;
        R.i0[r] = R.i1[r] = R.j0[r] = R.nj[r] = R.k0[r] = R.k1[r] = 0;
        R.ca[r] = R.wa[r] = 1; R.cb[r] = R.wb[r] = 0;
        if (r >= nreg) continue;
        const int *b = h_regions + 6 * r;
        ADI_REQUIRE(b[0] < b[1] && b[2] < b[3] && b[4] < b[5], "%s: region %d is empty", who, r);
        ADI_REQUIRE(b[0] >= 0 && b[1] <= nr && b[4] >= 0 && b[5] <= nz, "%s: region %d leaves the grid along r or z", who, r);
        ADI_REQUIRE(b[2] >= 0 && b[2] < nphi && (long)b[3] <= (long)b[2] + nphi,
                    "%s: region %d: phi cells [%d, %d) need 0 <= j0 < nphi and j1 <= j0 + nphi", who, r, b[2], b[3]);
        R.i0[r] = b[0]; R.i1[r] = b[1]; R.j0[r] = b[2]; R.nj[r] = b[3] - b[2]; R.k0[r] = b[4]; R.k1[r] = b[5];
        const long first_p = b[4] / 2, last_p = (b[5] - 1) / 2;
        const int ja_end = b[3] < nphi ? b[3] : nphi;                 // [j0, ja_end) and, wrapped, [0, j1 - nphi)
        R.ca[r] = (int)(((long)b[2] * P->per_line + first_p) / 256);
        R.cb[r] = (int)(((long)(ja_end - 1) * P->per_line + last_p) / 256);
        if (b[3] > nphi) {
            R.wa[r] = (int)(first_p / 256);
            R.wb[r] = (int)(((long)(b[3] - nphi - 1) * P->per_line + last_p) / 256);
        }
        const int lo = (b[3] > nphi && R.wa[r] < R.ca[r]) ? R.wa[r] : R.ca[r];
        const int hi = (b[3] > nphi && R.wb[r] > R.cb[r]) ? R.wb[r] : R.cb[r];
        ilo = b[0] < ilo ? b[0] : ilo; ihi = b[1] > ihi ? b[1] : ihi;
        clo = lo < clo ? lo : clo; chi = hi > chi ? hi : chi;
        max_ni = (b[1] - b[0]) > max_ni ? (b[1] - b[0]) : max_ni;
        off += (long)(b[1] - b[0]) * P->nchunk;
        poff += b[1] - b[0];
    }
    for (int q = 0; q < nprobe; ++q) {
        const int n[3] = {nr, nphi, nz};
        for (int a = 0; a < 3; ++a)
            ADI_REQUIRE(h_probes[3 * q + a] >= 0 && h_probes[3 * q + a] < n[a], "%s: probe %d lies outside the grid along axis %d: %d",
                        who, q, a, h_probes[3 * q + a]);
    }
    P->ilo = ilo; P->ni = ihi - ilo; P->clo = clo; P->nc = chi - clo + 1; P->max_ni = max_ni;
    P->chunk_records = off; P->plane_records = poff;
    P->row_words = (long)nprobe + (long)ADI_CYL_MONITOR_REGION_WORDS * nreg;
    return ADI_OK;
}

// ---- the operations of a workgroup on the host: 256 values, the butterfly in each wave, then ((w0 + w1) + w2) + w3 ----------
inline double cyl_mon_waves_host(double *v)
{
#pragma clang fp contract(off)
    double w[4];
    for (int wv = 0; wv < 4; ++wv) {
        double *a = v + 64 * wv, b[64];
        for (int o = 1; o <= 32; o <<= 1) {
            for (int l = 0; l < 64; ++l) b[l] = a[l] + a[l ^ o];
            for (int l = 0; l < 64; ++l) a[l] = b[l];
        }
        w[wv] = a[0];
    }
    const double s01 = w[0] + w[1];
    const double s012 = s01 + w[2];
    return s012 + w[3];
}

// the 8 words of a region's row entry from what the finishing loop gathered
struct CylMonTotal {
    double sT, sR, sX, sRX;
    long long kmin, kmax, cnt, sum_i;
};
__host__ __device__ __forceinline__ void cyl_mon_total_init(CylMonTotal &a)
{
    a.sT = 0.0; a.sR = 0.0; a.sX = 0.0; a.sRX = 0.0;
    a.kmin = kCylMonKeyMax; a.kmax = -kCylMonKeyMax - 1; a.cnt = 0; a.sum_i = 0;
}
// radius i joins: S_T and S_X of its plane, its keys and its count
__host__ __device__ __forceinline__ void cyl_mon_total_add(CylMonTotal &a, double r_in, double dr, int i, double ST, double SX,
                                                           long long kmin, long long kmax, long long cnt)
{
#pragma clang fp contract(off)
    const double ri = cyl_mon_r(r_in, dr, i);
    a.sT = a.sT + ST;
    const double p = ri * ST;
    a.sR = a.sR + p;
    a.sX = a.sX + SX;
    const double px = ri * SX;
    a.sRX = a.sRX + px;
    a.kmin = kmin < a.kmin ? kmin : a.kmin;
    a.kmax = kmax > a.kmax ? kmax : a.kmax;
    a.cnt += cnt;
    a.sum_i += (long long)i * cnt;
}
__host__ __device__ __forceinline__ void cyl_mon_total_store(const CylMonTotal &a, double *o)
{
    o[0] = __builtin_bit_cast(double, a.cnt);
    o[1] = __builtin_bit_cast(double, a.sum_i);
    o[2] = a.cnt ? __builtin_bit_cast(double, cyl_mon_key(a.kmin)) : cyl_nan();
    o[3] = a.cnt ? __builtin_bit_cast(double, cyl_mon_key(a.kmax)) : cyl_nan();
    o[4] = a.sT; o[5] = a.sR; o[6] = a.sX; o[7] = a.sRX;
}

// the record over host arrays into `row`: the three kernels' operations in their order
inline void cyl_monitor_record_host(const CylMonPlan &P, double r_in, double dr, const double *T, const double *X,
                                    const uint8_t *act, int nprobe, const int *probes, double *row)
{
#pragma clang fp contract(off)
    const CylBox &g = P.g;
    const CylMonRegions &R = P.R;
    for (int q = 0; q < nprobe; ++q) {
        const long p = (long)probes[3 * q] * g.sx + (long)probes[3 * q + 1] * g.nz + probes[3 * q + 2];
        row[q] = (act == nullptr || act[p] != 0) ? T[p] : cyl_nan();
    }
    std::vector<double> partT(P.nchunk), partX(P.nchunk);
    double vT[256], vX[256];
    for (int r = 0; r < R.n; ++r) {
        CylMonTotal tot;
        cyl_mon_total_init(tot);
        for (int i = R.i0[r]; i < R.i1[r]; ++i) {
            long long kmin = kCylMonKeyMax, kmax = -kCylMonKeyMax - 1, cnt = 0;
            for (int c = 0; c < (int)P.nchunk; ++c) {
                partT[c] = 0.0; partX[c] = 0.0;
                if (!cyl_mon_meets(R, r, c)) continue;
                for (unsigned t = 0; t < 256u; ++t) {
                    const CylMonPair pr = cyl_mon_pair((unsigned)c * 256u + t, P.per_line, P.per_plane, g.nz);
                    const long p = (long)i * g.sx + (long)pr.j * g.nz + pr.k;
                    unsigned m = pr.in;
                    if (act != nullptr) m &= ((pr.in & 1u) && act[p] ? 1u : 0u) | ((pr.in & 2u) && act[p + 1] ? 2u : 0u);
                    const unsigned inc = cyl_mon_member(R, r, g.nphi, pr.j, pr.k, m);
                    double t0 = 0.0, t1 = 0.0, x0 = 0.0, x1 = 0.0;
                    if (inc & 1u) { t0 = T[p]; if (X) x0 = X[p]; }
                    if (inc & 2u) { t1 = T[p + 1]; if (X) x1 = X[p + 1]; }
                    const CylMonTerm e = cyl_mon_term(inc, t0, t1, X != nullptr, x0, x1);
                    vT[t] = e.sT; vX[t] = e.sX;
                    kmin = e.kmin < kmin ? e.kmin : kmin; kmax = e.kmax > kmax ? e.kmax : kmax; cnt += e.cnt;
                }
                partT[c] = cyl_mon_waves_host(vT);
                if (X) partX[c] = cyl_mon_waves_host(vX);
            }
            for (unsigned t = 0; t < 256u; ++t) {
                double aT = 0.0, aX = 0.0;
                for (unsigned n = t; n < P.nchunk; n += 256u) {
                    if (!cyl_mon_meets(R, r, (int)n)) continue;
                    aT = aT + partT[n];
                    aX = aX + partX[n];
                }
                vT[t] = aT; vX[t] = aX;
            }
            const double ST = cyl_mon_waves_host(vT), SX = X ? cyl_mon_waves_host(vX) : 0.0;
            cyl_mon_total_add(tot, r_in, dr, i, ST, SX, kmin, kmax, cnt);
        }
        cyl_mon_total_store(tot, row + nprobe + ADI_CYL_MONITOR_REGION_WORDS * r);
    }
}

}  // namespace adi
