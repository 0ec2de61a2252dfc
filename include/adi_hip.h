/*
 * include/adi_hip.h -- C ABI of libadi_hip.so, the MI355X (gfx950) ADI heat-equation hot path.
 *
 * The reference (Matemusi/ADI_thermal_fields) has no FFI: its boundary is a Python module
 * namespace (`import adi3d_numba_coeff as adi` / `import adi3d_gpu_coeff as adi`,
 * waam_from_stl_v7_mm.py:321-335).  This header is what a binding for that namespace calls;
 * each entry point cites the reference function it replaces.  adi_thermal_fields_amd/ binds
 * it with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, every call returns int (ADI_OK == 0) and never throws.
 *   - adi_last_error() returns a thread-local, human-readable message for the last failure.
 *   - Fields are C-order (n0, n1, n2) fp64 arrays; masks are 1 byte per cell (0 / non-zero)
 *     (adi3d_numba_coeff.py:14-19, :29-36).  Axis 2 is contiguous.
 *   - "d_" pointers are DEVICE pointers owned by the caller (hipMalloc / torch); "h_" pointers are
 *     host pointers borrowed for the duration of the call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Stateless entry points
 *     only enqueue work; they never synchronise.
 *   - Face order everywhere: 0 'x-', 1 'x+', 2 'y-', 3 'y+', 4 'z-', 5 'z+' (axis = face / 2).
 */
#ifndef ADI_HIP_H
#define ADI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADI_OK              0
#define ADI_ERR_ARG         1   /* bad argument (the Python host maps it to ValueError / AssertionError) */
#define ADI_ERR_HIP         2   /* a HIP runtime call failed */
#define ADI_ERR_UNSUPPORTED 3   /* valid request this build cannot serve */
#define ADI_ERR_STATE       4   /* context used out of order (e.g. step before build_coeffs) */

#define ADI_ABI_VERSION 18

/* per-face BC data mode for adi_build_coeffs */
#define ADI_FACE_NONE   0   /* face carries no data (robin_h is None / face absent from `neumann`) */
#define ADI_FACE_SCALAR 1
#define ADI_FACE_FIELD  2   /* per-voxel fp64 array */

/* z-end boundary kinds of the cylindrical path (adi3d_cyl_phi_v3.py:60-68, :271-296) */
#define ADI_ZBC_NEUMANN0  0
#define ADI_ZBC_DIRICHLET 1
#define ADI_ZBC_ROBIN     2

/* sweep kernel variants (which pack arrays a sweep reads; selects the byte count of the roofline) */
#define ADI_SWEEP_GENERAL   0   /* in, flags, coeff, dir_mask, dir_val, qflux -> out : 42 B/cell */
#define ADI_SWEEP_NO_DIR    1   /* no Dirichlet cells: in, mask, coeff, qflux -> out : 33 B/cell */
#define ADI_SWEEP_NO_Q      2   /* no Neumann flux:    in, mask, coeff, dir_mask, dir_val -> out : 34 B/cell */
#define ADI_SWEEP_LEAN      3   /* neither:            in, mask, coeff -> out : 25 B/cell */

int         adi_abi_version(void);
/* identity of this build: 16 hex digits of the SHA-256 over the library's sources and compile flags (independent of the
 * directory it was built in); profiles/pmc_traffic.json is stamped with it and bench.py quotes measured HBM traffic only
 * for a library that reports the same stamp.  "unstamped" for a library not built by adi_thermal_fields_amd/build.py. */
const char *adi_build_stamp(void);
const char *adi_last_error(void);
int         adi_device_count(int *count);
/* name: caller buffer of >= 256 bytes; cu_count / hbm_bytes / lds_per_cu may be NULL */
int         adi_device_info(int device, char *name, int *cu_count, size_t *hbm_bytes, size_t *lds_per_cu);
/* The constructors of the reference copy their array arguments and the step returns a new array
 * (adi3d_numba_coeff.py:18, :31-36, :135, :302): with HOST arrays at the boundary that is one transfer of every plane
 * in each direction.  nplanes planes of plane_bytes each, src_pitch / dst_pitch bytes apart (the device layout pads its
 * planes, the host array is dense), as ONE 2-D DMA on `stream`; to_device: 1 = host -> device, 0 = device -> host. */
int         adi_copy_planes(void *dst, size_t dst_pitch, const void *src, size_t src_pitch, size_t plane_bytes,
                            size_t nplanes, int to_device, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Stateless device entry points (caller-owned device memory).
 *
 * Device layout of every field and mask: element (i, j, k) at i*plane_stride + j*nz + k, with
 * plane_stride >= ny*nz in ELEMENTS (0 means dense, ny*nz).  A padded plane stride keeps the rows of an
 * axis-0 line off the same HBM channels; adi_recommended_plane_stride() returns the pitch this library
 * wants for a given (ny, nz).  Per-line arrays (d_xlo, d_xhi, d_cond) are dense.
 *
 * Box limit: nx * plane_stride < ADI_MAX_BOX_CELLS (2^32 cells, 32 GiB per fp64 field).  The strided kernels address a
 * row as one 32-bit element offset from a tile base that, along axis 0, can be anywhere in the box; every Cartesian entry
 * point (and adi_ctx_create) refuses a larger box with ADI_ERR_UNSUPPORTED before any HIP call.  Planes are limited to
 * ny * nz < 2^31 cells.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_MAX_BOX_CELLS 4294967296LL
long adi_recommended_plane_stride(int ny, int nz);

/* Physical extents the library recommends for a logical (nx, ny, nz) grid (ABI v16): each >= the logical extent, chosen
 * per axis among the logical length and the next few multiples of 16 so that the lines fill the FAST kernels' workgroups
 * (a 257-row line runs on the GENERAL kernels, a 272-row one on the FAST ones).  The caller allocates fields with the
 * physical extents (plane stride from adi_recommended_plane_stride(*py, *pz)), marks every cell outside the logical box
 * off-mask -- off-mask cells are identity rows and are never read by an in-mask cell, so the results inside the logical box
 * are those of the logical grid (the reference treats the edge of the domain and an off-mask neighbour alike,
 * adi3d_numba_coeff.py:38-55) -- and passes the physical extents to every entry point.  adi3d_hip_coeff.Layout does this. */
int adi_recommended_dims(int nx, int ny, int nz, int *px, int *py, int *pz);

/* exposed_mask(mask, face): adi3d_numba_coeff.py:38-55 / adi3d_gpu_coeff.py:31-48 */
int adi_exposed_mask(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, int face,
                     uint8_t *d_exposed, void *stream);

/* Exposed faces per plane k of axis 2, counted from the neighbour-flags digest (adi_build_nbr_flags): the count loop of
 * quick_compare_layer_birth_robin_v3.py:97-108 (exposed x-/x+/y-/y+ faces of the 2-D section, the digital perimeter
 * divided by dx) for every layer of a 3-D mask at once.  face_bits: bit f set = count face f (0..5 = x-, x+, y-, y+, z-,
 * z+; 15 = the four lateral faces).  d_counts: nz unsigned 64-bit integers (zeroed here). */
int adi_count_exposed_faces(const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride, int face_bits,
                            unsigned long long *d_counts, void *stream);

/* A layer birth in one pass over the planes [k_begin, k_end) of axis 2 (activate_layer, waam_from_stl_v7_mm.py:487-495):
 * newborn = full & ~active; T[newborn] = Ts; active |= full.  *d_newborn (device, 64-bit) receives the number of
 * newborn cells.  The caller then rebuilds the flags and the packs, as the reference's drivers do (:494-495, :534). */
int adi_birth_planes(double *d_T, uint8_t *d_active, const uint8_t *d_full, int nx, int ny, int nz, long plane_stride,
                     int k_begin, int k_end, double Ts, unsigned long long *d_newborn, void *stream);

/*
 * precompute_coeff_packs_unified: adi3d_numba_coeff.py:57-118 / adi3d_gpu_coeff.py:50-110.
 * One pass over the grid writes the three Robin coefficient fields and the three Neumann flux fields:
 *   coeff[axis] += h_f * dx^2 / (rho cp dx^3) on cells exposed on face f ('-' face first, then '+'),
 *   qflux[axis] += q_f * dx^2 / (rho cp dx^3) on exposed cells.
 * h_mode/q_mode[6]: ADI_FACE_*; h_scalar/q_scalar[6]; h_field/q_field[6]: device pointers or NULL.
 * d_coeff[3], d_qflux[3]: device output fields (fully overwritten).
 */
int adi_build_coeffs(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, double dx,
                     double rho, double cp,
                     const int *h_mode, const double *h_scalar, const double *const *d_h_field,
                     const int *q_mode, const double *q_scalar, const double *const *d_q_field,
                     double *const *d_coeff, double *const *d_qflux, void *stream);
/* ... restricted to the planes [k_begin, k_end) of axis 2 (in-place update of packs built earlier: see
 * adi_build_nbr_flags_planes). */
int adi_build_coeffs_planes(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, double dx, double rho,
                            double cp, const int *h_mode, const double *h_scalar, const double *const *d_h_field,
                            const int *q_mode, const double *q_scalar, const double *const *d_q_field,
                            double *const *d_coeff, double *const *d_qflux, int k_begin, int k_end, void *stream);

/*
 * Neighbour flags, the device-side digest of the mask every step kernel reads instead of the raw mask:
 *   bit0 = cell in mask; bit(1+2a) / bit(2+2a) = the minus / plus neighbour along axis a exists and is in
 *   the mask (the `mask[i-1,j,k]` / `mask[i+1,j,k]` tests of adi3d_numba_coeff.py:150-153, :246-251).
 * Rebuild whenever the mask changes (same moment the packs are rebuilt, waam_from_stl_v7_mm.py:494-495, :534).
 * For a slab of a larger grid, build the flags on the slab plus its two halo planes and pass the interior.
 */
int adi_build_nbr_flags(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride,
                        uint8_t *d_flags, void *stream);
/* The same restricted to the planes [k_begin, k_end) of axis 2: after a layer birth only the planes of the layer and
 * the one below / above it change (waam_from_stl_v7_mm.py:487-495 rebuilds everything; the result is the same). */
int adi_build_nbr_flags_planes(const uint8_t *d_mask, int nx, int ny, int nz, long plane_stride, uint8_t *d_flags,
                               int k_begin, int k_end, void *stream);
/* Flags summary: one bit per brick of 16 x 16 x 16 cells of the box (nx, ny, nz), set iff every flags byte of the brick is
 * the one its position implies -- in the mask, and each of the six neighbour bits set iff that neighbour lies inside the
 * box.  The bit of the brick of cell (i, j, k) is bit (i/16) % 32 of word ((j/16) * nbz + k/16) * nwx + i/512, with
 * nbz = ceil(nz/16), nwx = ceil(ceil(nx/16)/32); adi_flag_bricks_words gives the number of 32-bit words (0: bad box).
 * adi_build_flag_bricks compares d_flags with the implied bytes on the device and rewrites the bits of every brick that holds
 * a plane of [k_begin, k_end) of axis 2: call it over the same range whenever the flags change.  A stale summary gives
 * wrong results.  The *_bricks entry points below take it (d_bricks NULL: the plain entry point): their FAST kernels
 * synthesize the flags bytes of segments whose bricks are set instead of loading them; results are bit-identical. */
long adi_flag_bricks_words(int nx, int ny, int nz);
int adi_build_flag_bricks(const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride, uint32_t *d_bricks,
                          int k_begin, int k_end, void *stream);

/* lap1D_x/y/z + R0 = Tn + dt*kappa*(1-theta)*(Lx+Ly+Lz): adi3d_numba_coeff.py:240-288, :298 */
int adi_explicit_rhs(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                     double dx, double dt, double kappa, double theta, double *d_R0, void *stream);
/* the same for planes [i_begin, i_end) of the array only (neighbour planes are still read where they exist): lets a
 * slab compute its interior planes while the halo planes are in flight */
int adi_explicit_rhs_planes(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                            double dx, double dt, double kappa, double theta, double *d_R0,
                            int i_begin, int i_end, void *stream);

/*
 * sweep_axis0/1/2: adi3d_numba_coeff.py:133-237 (full-length identity-row form of
 * adi3d_gpu_coeff.py:154-191).  One independent tridiagonal system per grid line along `axis`.
 * variant: ADI_SWEEP_*; arrays a variant does not read may be NULL.  d_out must not alias d_in.
 * d_xlo / d_xhi (optional, dense, one value per line): value of the unknown just before the first / after
 * the last local row when the line continues on a neighbouring GPU (see adi_interface_solve); the coupling
 * itself is read from the halo bits of d_flags.  NULL for a stand-alone grid.
 * sparse != 0 asserts the invariant of packs built by adi_build_coeffs -- coeff/qflux of this axis are zero
 * except on cells that lack an in-mask neighbour along the axis -- so the kernel loads them only there
 * (and dir_val only where dir_mask is set).  Pass 0 for hand-built packs.  Bit 1 (value 2) is an optional hint: every
 * cell of the box is in the mask (an all-solid box), which lets the strided FAST kernels (fused and unfused) run their leaner build; results do not depend on it.
 * Bit 2 (value 4) is a PROMISE, not a hint: the FAST kernel takes every unit of this sweep, so the queue reset and the
 * GENERAL launch behind it are skipped (units the FAST kernel cannot take would be left unwritten).  Which units are queued
 * depends on the flags, the Dirichlet mask, the variant, `sparse` and the shape only -- never on the field -- so a caller
 * may set the bit after it has seen the queue of an identical call come back empty: after a sweep without the bit the first
 * 32-bit word of d_work is the number of queued units (adi3d_hip_coeff.py does exactly that, once per mask / pack version).
 * That word is written only by a sweep that launched a FAST kernel: not with theta * gam < 1e-9 (a vanishing time step: the
 * GENERAL kernels take the whole sweep), not on axis 2 with d_xlo / d_xhi, not where the line length has no FAST kernel.
 * What it holds after such a sweep says nothing about an identical call at another dt, theta or interface argument.
 * d_work/work_bytes (adi_sweep_workspace_bytes): c'/d' scratch for lines longer than the in-register limit,
 * otherwise the unit queue that lets a sparse sweep run as a FAST kernel (solid interior) followed by the
 * GENERAL kernel on the queued surface units; with NULL/0 the GENERAL kernel processes everything.

 * h_face_consts (ABI v14, optional, HOST pointer to 4 doubles; NULL: read the arrays): packs built from per-face SCALARS
 * (adi_face_constants) -- (c-, c+, q-, q+) = h_f dx^2 / (rho cp dx^3) and q_f dx^2 / (rho cp dx^3) of the minus / plus face
 * of the sweep axis.  The coefficient of a cell exposed along the axis is then (0 + [no minus neighbour] c-) + [no plus
 * neighbour] c+ -- the accumulation order of the reference (:93-99), hence the value stored in the array bit for bit -- and
 * follows from the flags byte alone: the kernels do not load coeff / qflux at all (on a curved solid those loads can only be
 * issued after the flags have arrived).  Honoured only together with `sparse` (stale / hand-built packs are read).
 */
int adi_sweep(int axis, int variant, const double *d_in, const uint8_t *d_flags, const double *d_coeff,
              const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux,
              int nx, int ny, int nz, long plane_stride, int sparse,
              double theta, double gam, double dt, double Tinf,
              double *d_out, const double *d_xlo, const double *d_xhi, const double *h_face_consts,
              void *d_work, size_t work_bytes, void *stream);
/* adi_sweep with the flags summary of d_flags (adi_build_flag_bricks) */
int adi_sweep_bricks(int axis, int variant, const double *d_in, const uint8_t *d_flags, const uint32_t *d_bricks,
                     const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux,
                     int nx, int ny, int nz, long plane_stride, int sparse,
                     double theta, double gam, double dt, double Tinf,
                     double *d_out, const double *d_xlo, const double *d_xhi, const double *h_face_consts,
                     void *d_work, size_t work_bytes, void *stream);
/* (c-, c+, q-, q+) per axis for adi_sweep & co.: h_consts[12] = [axis][4], h_valid[3] = 1 where both faces of the axis carry
 * scalars or nothing (ADI_FACE_SCALAR / ADI_FACE_NONE) for h AND q -- only then may h_consts + 4*axis be passed on.
 * Host arithmetic, the very expressions of adi_build_coeffs. */
int adi_face_constants(double dx, double rho, double cp, const int *h_mode, const double *h_scalar, const int *q_mode,
                       const double *q_scalar, double *h_consts, int *h_valid);
int adi_sweep_workspace_bytes(int axis, int nx, int ny, int nz, long plane_stride, size_t *bytes);

/*
 * Slab decomposition of a sweep (no counterpart in the reference, which is single-process): pass A.
 * For every line, the local rows are condensed to six numbers (d_cond: [6][nlines], dense) such that
 *   x_first = c0 - c1*xl - c2*xr,   x_last = c3 - c4*xl - c5*xr
 * with xl / xr the unknowns adjacent to the slab on the neighbouring GPUs.  Same inputs as adi_sweep.
 */
int adi_sweep_condense(int axis, int variant, const double *d_in, const uint8_t *d_flags,
                       const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val,
                       const double *d_qflux, int nx, int ny, int nz, long plane_stride, int sparse,
                       double theta, double gam, double dt, double Tinf, double *d_cond, const double *h_face_consts,
                       void *d_work, size_t work_bytes, void *stream);
/*
 * Explicit stage folded into the axis-0 sweep (ABI v7): lap1D_x/y/z + R0 (adi3d_numba_coeff.py:240-288, :292-298)
 * are evaluated inside the loads of sweep_axis0 (:133-166, :299), so R0 never travels through HBM -- the first two
 * stages of adi_step_numba_coeff cost one read of T and one write of U.  Same arithmetic in the same order as
 * adi_explicit_rhs followed by adi_sweep(axis 0): the result is bit-identical to running the two stages.
 * d_T: the state (the `Tn` of the step), box (nx, ny, nz) with plane_stride; neighbours outside the box are read
 * where the flags byte says they exist (halo planes of a slab, rows next to a sub-box of lines), so the caller states
 * which element offsets relative to d_T may be read: [valid_lo, valid_hi) must cover the box and lie inside the
 * allocation (whole buffer: valid_lo = -(offset of d_T in it), valid_hi = its length - that offset).
 * adi_explicit_fused_supported(pass): 1 when pass 0 (sweep) / pass 1 (condensation) can run fused on this box
 * (nx <= 1024 planes; pass 1: whole register segments); otherwise run adi_explicit_rhs + adi_sweep.
 * adi_explicit_condense0: d_R0_out (optional, same box layout as d_T) also receives R0, so that pass B can be the plain
 * adi_sweep on it instead of evaluating the explicit stage a second time.
 */
int adi_explicit_fused_supported(int nx, int ny, int nz, long plane_stride, int pass);
int adi_explicit_sweep0(int variant, const double *d_T, long valid_lo, long valid_hi, const uint8_t *d_flags,
                        const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val,
                        const double *d_qflux, int nx, int ny, int nz, long plane_stride, int sparse,
                        double dx, double dt, double kappa, double theta, double Tinf,
                        double *d_out, const double *d_xlo, const double *d_xhi, const double *h_face_consts,
                        void *d_work, size_t work_bytes, void *stream);
/* adi_explicit_sweep0 with the flags summary of d_flags (adi_build_flag_bricks) */
int adi_explicit_sweep0_bricks(int variant, const double *d_T, long valid_lo, long valid_hi, const uint8_t *d_flags,
                               const uint32_t *d_bricks, const double *d_coeff, const uint8_t *d_dir_mask,
                               const double *d_dir_val, const double *d_qflux, int nx, int ny, int nz, long plane_stride,
                               int sparse, double dx, double dt, double kappa, double theta, double Tinf,
                               double *d_out, const double *d_xlo, const double *d_xhi, const double *h_face_consts,
                               void *d_work, size_t work_bytes, void *stream);
int adi_explicit_condense0(int variant, const double *d_T, long valid_lo, long valid_hi, const uint8_t *d_flags,
                           const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val,
                           const double *d_qflux, int nx, int ny, int nz, long plane_stride, int sparse,
                           double dx, double dt, double kappa, double theta, double Tinf,
                           double *d_cond, double *d_R0_out, const double *h_face_consts,
                           void *d_work, size_t work_bytes, void *stream);
/*
 * Pass A folded into the explicit stage (ABI v7): for a line whose rows are uniform along axis 0 (solid interior; at
 * most one end row differs) the six pass-A numbers follow from two dot products of R0 with fixed weights -- the first
 * column u of tridiag(-tg, 1+2tg, -tg)^-1 and its reverse -- which the marching explicit kernel accumulates while it
 * writes R0, so the slab's inputs are read once.  Lines that are not uniform are condensed from the stored R0.
 *   adi_axis0_dots_setup      u for (n, theta, gam) -> d_weights[n]                       (once per dt; synchronises)
 *   adi_axis0_classify        d_cls[ny*nz] (1 = uniform) and d_list (count + ids of the others)   (once per mask)
 *   adi_explicit_rhs_dots     adi_explicit_rhs_planes + partial dot products d_part (adi_axis0_dots_workspace).  The lines
 *                             are planes [i_org, i_org + n_line) of the array; a call may cover part of them in whole
 *                             chunks of adi_axis0_dots_ichunk(n_line) planes (interior first, halo-adjacent planes later)
 *   adi_axis0_dots_finish     -> d_cond [6][line_end - line_begin] of the lines [line_begin, line_end), the format of
 *                             adi_sweep_condense; arrays are those of the box (nx = i_end - i_begin planes)
 */
int adi_axis0_dots_supported(int nx, int ny, int nz, long plane_stride);
int adi_axis0_dots_workspace(int nx, int ny, int nz, size_t *part_bytes, size_t *list_bytes);
int adi_axis0_dots_setup(int n, double theta, double gam, double *d_weights, void *stream);
int adi_axis0_classify(const uint8_t *d_flags, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                       uint8_t *d_cls, unsigned *d_list, void *stream);
int adi_axis0_dots_ichunk(int n_line);   /* planes per chunk of partial sums for lines of n_line rows */
int adi_explicit_rhs_dots(const double *d_T, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                          double dx, double dt, double kappa, double theta, double *d_R0, int i_begin, int i_end,
                          int i_org, int n_line, const double *d_weights, double *d_part, void *stream);
int adi_axis0_dots_finish(int variant, const double *d_part, const double *d_weights, const uint8_t *d_cls,
                          const unsigned *d_list, const double *d_R0, const uint8_t *d_flags, const double *d_coeff,
                          const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux,
                          int nx, int ny, int nz, long plane_stride, double theta, double gam, double dt, double Tinf,
                          long line_begin, long line_end, double *d_cond, void *stream);
/* d_cond_all: [nranks][6][nlines], the all-gathered pass-A output ordered by slab.  Solves the reduced
 * interface system of every line and writes this rank's boundary values for pass B (adi_sweep). */
int adi_interface_solve(const double *d_cond_all, int nranks, int rank, long nlines,
                        double *d_xlo, double *d_xhi, void *stream);
/* Neighbour-only interface solve, for slabs thick enough that the coupling across a boundary window has decayed
 * below rounding (the caller checks |aL| of its last-rows window and |cF| of its first-rows window).
 * d_my_lo / d_my_hi: [6][nlines] pass-A output of this slab's first / last window of planes;
 * d_prev_hi: rows 3..5 (gL, aL, cL) of the last window of the slab below, d_next_lo: rows 0..1 (gF, aF) of the
 * first window of the slab above; NULL where there is no neighbour (boundary value 0, never used). */
int adi_interface_pair(const double *d_my_lo, const double *d_my_hi, const double *d_prev_hi, const double *d_next_lo,
                       long nlines, double *d_xlo, double *d_xhi, void *stream);

/*
 * Deferred form of the slab decomposition (ABI v12; no counterpart in the reference, which is single-process).  For slabs
 * whose sharded-axis lines are all uniform (solid, no Dirichlet cell) the two-pass scheme above is not needed:
 *   1. every rank runs the ordinary single-domain kernel (adi_explicit_sweep0 / adi_sweep along axis 0, d_xlo = d_xhi =
 *      NULL) on its slab: each line solved with zero boundary values -> x0.  Planes 0 and nx-1 of x0 are exactly the
 *      pass-A right-hand sides (gF, gL), so "one ghost plane per sweep" travels to each neighbour and nothing else;
 *   2. adi_interface_deferred: the 2 x 2 system per boundary and line -> the two interface values of every line;
 *   3. by linearity  x = x0 + ulo * w[i] + uhi * w[nx-1-i]  with w the decaying homogeneous solution of the uniform
 *      row (adi_axis0_deferred_setup).  That rank-two update is not applied to x0 in memory: adi_sweep_corrected, the
 *      axis-1 sweep that consumes the field next (sweep_axis1, adi3d_numba_coeff.py:300), adds it to every value it
 *      loads -- two planes re-read from L2 instead of a second pass over the slab.
 * adi_axis0_deferred_setup: w (nx doubles, device) for (theta, gam); entries <= tol are stored as exactly 0 (the kernels
 *   skip them), *h_reach = number of non-zero entries, *h_omega = w[0].  The form is valid when the weights have decayed
 *   across the slab (*h_reach < nx): then neither the far end's closure nor the next-but-one slab matters.  Synchronises.
 * adi_interface_deferred: d_first / d_last = planes 0 / nx-1 of this rank's x0 (dense ny*nz), d_prev_last / d_next_first
 *   = the neighbours' adjacent planes (NULL: no neighbour) -> d_ulo, d_uhi (dense ny*nz; 0 where there is no neighbour).
 * adi_sweep_corrected: adi_sweep(axis = 1, ...) reading  in + w[i] * ulo[j][k] + w[nx-1-i] * uhi[j][k]  (d_ulo or d_uhi
 *   NULL: that term is absent; d_w NULL: plain adi_sweep).
 */
int adi_axis0_deferred_setup(int n, double theta, double gam, double tol, double *d_w, double *h_omega, int *h_reach,
                             void *stream);
int adi_interface_deferred(const double *d_first, const double *d_last, const double *d_prev_last,
                           const double *d_next_first, double omega, long nlines, double *d_ulo, double *d_uhi,
                           void *stream);
/* The weights adi_axis0_dots_setup (kind DOTS: c = 1) and adi_axis0_deferred_setup (kind DEFERRED: c = theta*gam) upload,
 * on the host: h_w[n] = c * first column of tridiag(-tg, 1+2tg, -tg)^-1, entries <= tol stored as exactly 0,
 * *h_reach = number of entries kept (tol = 0 cuts nothing).  The same builder as those entries; host arithmetic only: no
 * HIP call, no device needed.  n < 2, tol < 0, an unknown kind or a NULL pointer is ADI_ERR_ARG. */
#define ADI_AXIS0_WEIGHTS_DOTS     0
#define ADI_AXIS0_WEIGHTS_DEFERRED 1
int adi_axis0_weights_host(int n, double theta, double gam, int kind, double tol, double *h_w, int *h_reach);
/* The deferred form WITHOUT decay (ABI v15: thin slabs / strong scaling, e.g. 512^3 over 8 GPUs = 64 planes at cfl 200).
 * x = x0 + c_lo w[i] + c_hi w[n-1-i] still holds (adi_axis0_deferred_setup with tol = 0: no weight is cut); the interface
 * system now couples all ranks, as in the two-pass `exact` form, but only its right-hand sides change from step to step:
 *   per step   all-gather [2][nlines] = (plane 0, plane nx-1 of x0) -> d_g_all [nranks][2][nlines]   (a third of the payload
 *              of the six-number block), adi_interface_solve_uniform -> (d_xlo, d_xhi), adi_deferred_exact_coef -> the
 *              per-line coefficients (d_clo, d_chi) of w[i] and w[nx-1-i] for adi_sweep_corrected;
 *   per plan   adi_deferred_exact_setup: d_mat [4][nlines] = (aF, cF, aL, cL) of this rank and d_kap [2][nlines], the
 *              Sherman-Morrison factors of a global end row (first / last rank: the line start / end with its Robin
 *              coefficient, read from planes 0 / nx-1 of the axis-0 coefficient array); all-gather d_mat ->
 *              d_mat_all [nranks][4][nlines] (read for ranks 0 and nranks-1 only: a middle rank's entries are the two numbers
 *              (w[0], w[nx-1]) of ITS slab, d_scal_all [nranks][2], gathered likewise -- slabs may differ in thickness).
 * d_flags_first / _last, d_coeff_first / _last: planes 0 and nx-1 (dense ny*nz). */
int adi_deferred_exact_setup(const uint8_t *d_flags_first, const uint8_t *d_flags_last, const double *d_coeff_first,
                             const double *d_coeff_last, double theta, double gam, double dt, double w0, double wn,
                             long nlines, double *d_mat, double *d_kap, void *stream);
int adi_interface_solve_uniform(const double *d_g_all, const double *d_mat_all, const double *d_scal_all, int nranks, int rank,
                                long nlines, double *d_xlo, double *d_xhi, void *stream);
int adi_deferred_exact_coef(const double *d_xlo, const double *d_xhi, const double *d_kap, long nlines, double *d_clo,
                            double *d_chi, void *stream);
/* The deferred form for lines that are NOT uniform (curved solids, voids, Dirichlet cells -- an STL part on slabs; ABI v17,
 * reworked in v18).  The algebra above needs no uniform rows, only the two homogeneous solutions of every line; where they decay
 * across the slab they are non-zero on K < nx planes at each end.  v17 streamed K planes of per-cell weights at each end into
 * the axis-1 sweep (at cfl 200: 399 of 512 planes, more than the field itself).  v18 sorts the lines once per plan, per side,
 * by what their first (last) K rows look like:
 *     uniform  all K rows solid interior rows, no Dirichlet cell: the line's homogeneous solution IS the scalar w[i] of the
 *              uniform deferred form on those rows (up to the decay tolerance) -> adi_sweep_corrected adds it, as for boxes;
 *     off      all K rows outside the mask: identity rows, weight 0;
 *     flagged  everything else (the line crosses a void, the surface or a Dirichlet cell within reach of the interface): its
 *              own K weights, kept compactly as d_wc [K][nflag], and applied IN MEMORY to the zero-boundary solution by
 *              adi_deferred_lines_apply before the axis-1 sweep -- a sparse pass over the flagged lines only.
 *   per plan   two ordinary adi_sweep(axis 0) calls on the slab with a zero field, Tinf = 0, no fluxes, zero Dirichlet values
 *              and d_xlo = 1 (resp. d_xhi = 1): w_lo, w_hi of every line; the caller checks that they are below its tolerance
 *              beyond K planes, sorts the lines, compacts the weights of the flagged ones and exchanges the planes next to the
 *              interfaces (om_* below) with the neighbours;
 *   per step   step 1 as above; adi_interface_deferred_lines: the 2 x 2 systems with per-line weights -> d_ulo, d_uhi (every
 *              line) and d_ulo_uni / d_uhi_uni = the same values on the uniform lines, 0 elsewhere (d_uni_lo / d_uni_hi: one
 *              byte per line, non-zero = uniform; all four NULL: not wanted); adi_deferred_lines_apply for each side;
 *              adi_sweep_corrected with the scalar weights and the *_uni planes.
 * om_lo_own / om_hi_own: plane 0 of w_lo / plane nx-1 of w_hi of this rank; om_hi_prev / om_lo_next: the same planes of the
 * neighbours (dense ny*nz; NULL together with the neighbour's plane where there is none). */
int adi_interface_deferred_lines(const double *d_first, const double *d_last, const double *d_prev_last,
                                 const double *d_next_first, const double *d_om_lo_own, const double *d_om_hi_prev,
                                 const double *d_om_hi_own, const double *d_om_lo_next, long nlines, double *d_ulo,
                                 double *d_uhi, const uint8_t *d_uni_lo, const uint8_t *d_uni_hi, double *d_ulo_uni,
                                 double *d_uhi_uni, void *stream);
/* x[i][cell[q]] += wc[r][q] * u[cell[q]]  for q < nflag, r < K, with plane i = r (from_high_end == 0) or nx-1-r: the rank-one
 * update of the flagged lines of one side.  d_x: the slab field (nx planes, plane_stride elements apart); d_cells: nflag
 * offsets of the flagged lines inside a plane (j*nz + k, ascending); d_wc: [K][nflag]; d_u: a dense (ny*nz) interface plane;
 * d_nrows (may be NULL): per flagged line the number of leading rows that can carry a non-zero weight -- a line's weights are
 * exact zeros beyond its first row outside the mask, and rows >= d_nrows[q] are not even read. */
int adi_deferred_lines_apply(double *d_x, int nx, long plane_stride, long plane_cells, const int *d_cells, long nflag,
                             const double *d_wc, int K, const double *d_u, int from_high_end, const int *d_nrows, void *stream);
int adi_sweep_corrected(int variant, const double *d_in, const uint8_t *d_flags, const double *d_coeff,
                        const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux,
                        int nx, int ny, int nz, long plane_stride, int sparse,
                        double theta, double gam, double dt, double Tinf,
                        double *d_out, const double *d_ulo, const double *d_uhi, const double *d_w,
                        const double *h_face_consts, void *d_work, size_t work_bytes, void *stream);

/*
 * adi_step_numba_coeff / adi_step_gpu_coeff: adi3d_numba_coeff.py:290-302, adi3d_gpu_coeff.py:213-230.
 * d_T_in is not modified; d_T_out receives the new field; d_tmp_a / d_tmp_b are two scratch fields.
 * d_coeff[3], d_qflux[3]: per-axis pack arrays; dir data shared by the three packs (:116-118).
 */
int adi_step(const double *d_T_in, double *d_T_out, double *d_tmp_a, double *d_tmp_b,
             const uint8_t *d_flags, const double *const *d_coeff, const uint8_t *d_dir_mask,
             const double *d_dir_val, const double *const *d_qflux, int variant, int sparse,
             int nx, int ny, int nz, long plane_stride, double dx, double rho, double cp, double k,
             double dt, double theta, double Tinf, const double *h_face_consts /* [3][4] or NULL, see adi_sweep */,
             void *d_work, size_t work_bytes, void *stream);
/* The same step, reporting in h_queued[axis] (three HOST words, valid once the stream is synchronised) how many units the
 * FAST kernel of each sweep handed to the GENERAL kernel.  That number depends on the flags, the Dirichlet mask, the
 * variant, `sparse` and the shape -- not on the field -- so three zeros license bit 2 of `sparse` (the no-fallback promise,
 * see adi_sweep) on every later step of the same configuration.  One exception: a step with theta * k dt / (rho cp dx^2)
 * < 1e-9 runs no FAST kernel at all (a vanishing time step; theta = 0 included) and reports three zeros whatever the mask:
 * zeros from such a step license nothing.  adi_ctx_step learns on the first step at or above that bound after a mask / pack
 * change and passes the bit to such steps only. */
int adi_step_queued(const double *d_T_in, double *d_T_out, double *d_tmp_a, double *d_tmp_b,
             const uint8_t *d_flags, const double *const *d_coeff, const uint8_t *d_dir_mask,
             const double *d_dir_val, const double *const *d_qflux, int variant, int sparse,
             int nx, int ny, int nz, long plane_stride, double dx, double rho, double cp, double k,
             double dt, double theta, double Tinf, const double *h_face_consts,
             void *d_work, size_t work_bytes, void *stream, unsigned *h_queued);
/* adi_step / adi_step_queued with the flags summary of d_flags (adi_build_flag_bricks) */
int adi_step_bricks(const double *d_T_in, double *d_T_out, double *d_tmp_a, double *d_tmp_b,
             const uint8_t *d_flags, const uint32_t *d_bricks, const double *const *d_coeff, const uint8_t *d_dir_mask,
             const double *d_dir_val, const double *const *d_qflux, int variant, int sparse,
             int nx, int ny, int nz, long plane_stride, double dx, double rho, double cp, double k,
             double dt, double theta, double Tinf, const double *h_face_consts,
             void *d_work, size_t work_bytes, void *stream);
int adi_step_queued_bricks(const double *d_T_in, double *d_T_out, double *d_tmp_a, double *d_tmp_b,
             const uint8_t *d_flags, const uint32_t *d_bricks, const double *const *d_coeff, const uint8_t *d_dir_mask,
             const double *d_dir_val, const double *const *d_qflux, int variant, int sparse,
             int nx, int ny, int nz, long plane_stride, double dx, double rho, double cp, double k,
             double dt, double theta, double Tinf, const double *h_face_consts,
             void *d_work, size_t work_bytes, void *stream, unsigned *h_queued);

/*
 * The callers either side of the path.  Masks here are DENSE uint8 (nx, ny, nz), C order.
 * adi_morph6: op 0 = dilate6 (waam_from_stl_v7_mm.py:73-82), op 1 = erode6 (:84-96); d_out must not alias d_in.
 * adi_flood_outside: flood_fill_outside (:106-134) as its comment describes it -- air connected to the outside of the
 *   box through 6-connectivity (the reference pads the solid with True and therefore returns all-False: DESIGN.md D8);
 *   line scans instead of one-cell dilations; d_flag: one int of device scratch; synchronises the stream.
 * adi_pack_frame_f32be: fp64 field in the padded-plane layout -> big-endian float32 in VTK point order (x fastest),
 *   the payload of a legacy-VTK BINARY SCALARS block (the reference writes ASCII: vtk_writer.py:4-30).
 */
int adi_morph6(int op, const uint8_t *d_in, uint8_t *d_out, int nx, int ny, int nz, void *stream);
int adi_flood_outside(const uint8_t *d_solid, uint8_t *d_outside, int nx, int ny, int nz, int *d_flag, int *rounds,
                      void *stream);
int adi_pack_frame_f32be(const double *d_T, int nx, int ny, int nz, long plane_stride, uint32_t *d_out, void *stream);

/*
 * Projection of a triangle mesh onto the faces of a voxel mask: voxel_bc_correction.py:53-167 (STLBoundaryCorrector), the
 * stage that produces the per-voxel robin_h fields of a curved part.  Every sub-triangle of the reference's subdivision is a
 * "slot"; the caller owns the workspaces and does the two pieces of plumbing between the calls (an exclusive scan of the
 * counts, a STABLE sort of the keys).  Masks and fields share one layout: element (i, j, k) at i*stride_x + j*stride_y + k.
 *
 * adi_stlcorr_count: d_tri (ntri, 3, 3) vertices, d_area (ntri); d_count[t] = n*n, the sub-triangles of triangle t
 *   (n = ceil of its largest bounding-box extent in voxels, clamped to [1, max_subdiv]), or 0 when area <= area_epsilon.
 * adi_stlcorr_bin: d_offset (ntri + 1) = exclusive scan of d_count, d_offset[ntri] == nslot.  Slot s of triangle t is
 *   sub-triangle s - d_offset[t] in the order of _subdivide_triangle (i, then j, lower before upper).  Writes d_key[s] = the
 *   element offset of the voxel that holds the sub-triangle's centroid, or ADI_STLCORR_DROPPED when the centroid is outside
 *   the grid or off-mask; d_sub_area[s]; d_slot_tri[s] = t.  The centroid is rounded operation by operation, as NumPy does.
 * adi_stlcorr_accumulate: d_key_sorted / d_order = the keys sorted stably and the slot each sorted entry came from.  One
 *   thread per voxel sums its entries IN SLOT ORDER -- the reference's order of addition -- per face: area * |normal
 *   component| where the component passes 1e-12.  For every face that received a contribution it writes the sum to
 *   h_area[face] (where not NULL) and, where h_robin[face] / h_scale[face] are not NULL, sum / dx^2 to the scale field and
 *   h_base[face] * that to the Robin field.  The three tables are HOST arrays of six device pointers (face order of this
 *   header); untouched cells keep what the caller put there (zeros).  No atomics: two runs give the same bits.
 * adi_stlcorr_fallback: build_corrected_fields(fallback_to_base=True), :155-165 -- in-mask cells whose `face` neighbour is
 *   off-mask or outside the box and whose Robin value is <= 0 get `base` and scale 1.
 * None of the four synchronises.  Counts, offsets, keys and slot numbers are 64-bit.
 */
#define ADI_STLCORR_DROPPED    0x7fffffffffffffffLL
#define ADI_STLCORR_MAX_SUBDIV 4096
int adi_stlcorr_count(const double *d_tri, const double *d_area, long ntri, double dx, int max_subdiv,
                      double area_epsilon, long *d_count, void *stream);
int adi_stlcorr_bin(const double *d_tri, const double *d_area, const long *d_offset, long ntri, long nslot,
                    const uint8_t *d_mask, int nx, int ny, int nz, long stride_x, long stride_y, const double *h_origin,
                    double dx, int max_subdiv, long *d_key, double *d_sub_area, long *d_slot_tri, void *stream);
int adi_stlcorr_accumulate(const long *d_key_sorted, const long *d_order, const double *d_sub_area, const long *d_slot_tri,
                           const double *d_normal, long nslot, double dx, const double *h_base, double *const *h_area,
                           double *const *h_robin, double *const *h_scale, void *stream);
int adi_stlcorr_fallback(const uint8_t *d_mask, int nx, int ny, int nz, long stride_x, long stride_y, int face, double base,
                         double *d_robin, double *d_scale, void *stream);

/*
 * Solid voxelisation of a closed triangle mesh: voxel (i, j, k) of the dense uint8 mask (nx, ny, nz),
 * C order, is 1 exactly when its centre h_origin[m] + (index + 0.5) * dx lies inside the surface.  Rays run along `axis`
 * (0, 1 or 2) through every column of centres; with b = (axis + 1) % 3 and c = (axis + 2) % 3 a triangle covers a column
 * when the three edge functions of its projection onto (b, c) have one strict sign (edges in lexicographic order, a zero
 * broken as if the centre were nudged by (+eps, +eps^2)), its depth there is d0 + (l1 (d1 - d0) + l2 (d2 - d0)), and the
 * crossing toggles every voxel of the column whose centre is >= depth.  Solid = an odd number of toggles.  No operation
 * is contracted to an FMA: the result is the bit-for-bit value of the same arithmetic in IEEE doubles.
 *
 * The toggle grid is caller-owned, adi_voxelize_words() 32-bit words, zeroed by the caller before adi_voxelize_toggle:
 * one bit per voxel along the ray and one more per column for crossings behind the last voxel.
 *
 * adi_voxelize_count: d_tri (ntri, 3, 3) vertices; d_count[t] = the 4 x 4 column tiles of triangle t's bounding box
 *   clipped to the grid, 0 for zero projected area or a triangle outside.
 * adi_voxelize_toggle: d_offset (ntri + 1) = exclusive scan of d_count, d_offset[ntri] == nitem.  Sixteen lanes per tile,
 *   one integer atomic XOR of one bit per crossing: the grid does not depend on the order of arrival.
 * adi_voxelize_scan: prefix XOR along every column (in place: d_words then holds the solid bits), the dense mask written
 *   to d_mask, and the number of columns with an odd number of crossings ("leaks": the surface is not closed there)
 *   ADDED to *d_leaks, a device int the caller zeroed.  d_words and d_mask 16-byte aligned.
 * adi_voxelize_majority: d_out[q] = 1 where at least two of the three masks are non-zero (the three ray axes of a mesh
 *   with small gaps); d_out may be one of the inputs.
 * None of them synchronises.  Counts and offsets are 64-bit.
 */
int adi_voxelize_words(int nx, int ny, int nz, int axis, long *words);
int adi_voxelize_count(const double *d_tri, long ntri, const double *h_origin, double dx, int nx, int ny, int nz, int axis,
                       long *d_count, void *stream);
int adi_voxelize_toggle(const double *d_tri, const long *d_offset, long ntri, long nitem, const double *h_origin, double dx,
                        int nx, int ny, int nz, int axis, uint32_t *d_words, void *stream);
int adi_voxelize_scan(uint32_t *d_words, int nx, int ny, int nz, int axis, uint8_t *d_mask, int *d_leaks, void *stream);
int adi_voxelize_majority(const uint8_t *d_m0, const uint8_t *d_m1, const uint8_t *d_m2, size_t n, uint8_t *d_out, void *stream);

/* T[sel != 0] = value   (layer birth: waam_from_stl_v7_mm.py:487-495 `T[newborn] = Ts`); flat over n elements */
int adi_masked_fill(double *d_T, const uint8_t *d_sel, size_t n, double value, void *stream);
/* dst = a | b  (birth bookkeeping: mask_act |= newborn) */
int adi_mask_or(uint8_t *d_dst, const uint8_t *d_a, const uint8_t *d_b, size_t n, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Cylindrical (r, phi, z) backward-Euler step: adi3d_cyl_phi_v3.py:332-350 (scheme="be").
 * Field layout (nr, nphi, nz) with the same padded-plane convention (plane = one radius).
 * d_S may be NULL (no source).  d_tmp_a/d_tmp_b: scratch fields.
 * d_active (optional, may be NULL): adi_step_masked of quick_spiral_deposition_gif_v5.py:31-70 --
 * void cells are clamped to T_void before and after the step, inactive axis-row cells to T_inner.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_cyl_plan adi_cyl_plan;
/* GridCyl + Material + Params(dt) + RobinR + ZBC (adi3d_cyl_phi_v3.py:33-68) frozen into device tables:
 * the r coefficients of build_coeff_r (:155-202), the per-radius phi factors of phi_solve_spectral
 * (:302-329) and the z closures of build_coeff_z (:255-298).  Created on the current device.
 * ADI_ERR_ARG ("unknown zbc.kind_bot/top") mirrors the reference's ValueError (:283, :296). */
int adi_cyl_plan_create(int nr, int nphi, int nz, long plane_stride, double dr, double dphi, double dz,
                        double rho, double cp, double k, double dt,
                        double robin_h, double robin_Tinf,
                        int kind_bot, int kind_top, double h_bot, double h_top,
                        double Tinf_bot, double Tinf_top, double T_bot, double T_top,
                        adi_cyl_plan **out);
/* The same on an annular grid r_i = r_in + (i + 1/2) dr -- the grid quick_spiral_deposition_gif_v5.py:74-80
 * (build_grid_annular) and tests/test_spiral_vs_analytic.py ask for with GridCyl(..., R_in=R_in); the reference's GridCyl has
 * no such parameter (TypeError at HEAD).  Every formula is the reference's with r shifted: row 0 keeps the
 * zero-flux closure of :177-181 (now the inner wall) and its identity phi row (:315-317). */
int adi_cyl_plan_create_annular(int nr, int nphi, int nz, long plane_stride, double dr, double dphi, double dz,
                                double r_in, double rho, double cp, double k, double dt,
                                double robin_h, double robin_Tinf,
                                int kind_bot, int kind_top, double h_bot, double h_top,
                                double Tinf_bot, double Tinf_top, double T_bot, double T_top,
                                adi_cyl_plan **out);
int adi_cyl_plan_destroy(adi_cyl_plan *plan);
/* The tables a plan holds, on the host: the scalar arguments of adi_cyl_plan_create_annular in the same order (without
 * plane_stride and out), the same validation with the same error texts, the same builders -- what this writes is what plan
 * creation uploads.  Host arithmetic only: no HIP call, no device needed.  Every output is a caller-provided host array and
 * may be NULL (skipped):
 *   a, b, c [nr], r_add_last [1]   the r operator and the Robin increment of the last row's right-hand side
 *   phi_fac [nr], zt [nr*nphi], smden [nr]   f_i; the Sherman-Morrison vector A'^-1 u per radius and 1 / (1 + v.z), with
 *        A' the tridiagonal (-f, b0, -f), b0 = 1 + 2f, whose first / last diagonal is 2 b0 / b0 + f^2/b0: the phi sweep
 *        solves A' y = d and returns x = y - zt (y_0 + (f/b0) y_{n-1}) smden.  nphi <= 2: zt = 0, smden = 1.
 *   zclosure [ADI_CYL_ZCLOSURE_LEN]   f, b0, bN, aN, c0, add0, addN, T0, TN, dir0, dirN: the interior row is (-f, 1+2f, -f),
 *        row 0 (0, b0, c0) with add0 added to its right-hand side, row n-1 (aN, bN, 0) with addN; dir0 / dirN = 1: the
 *        row's right-hand side is T0 / TN instead
 *   fast [3]   r_M, r_nseg, phi_M: rows per thread and segments of the FAST r kernel, rows per thread of the FAST phi
 *        kernel; 0 where the axis length has none
 *   rfac [r_nseg * ADI_CYL_RF_STRIDE]   the tabulated factorisation of the r operator, per segment: four arrays of
 *        ADI_CYL_RF_MAXM - 1 doubles (forward multipliers wf, backward multipliers wb, inverse pivots ip, the c of the
 *        interior rows), ten scalars (ipl jpf aF cF aL cL a0 aS cS bS), then the PCR multipliers pk1[6], pk2[6] and the
 *        inverse diagonal of the reduced separator system.  rfac_capacity: doubles available at rfac; too few is
 *        ADI_ERR_ARG. */
#define ADI_CYL_ZCLOSURE_LEN 11
#define ADI_CYL_RF_MAXM 16
#define ADI_CYL_RF_STRIDE 83
int adi_cyl_plan_tables(int nr, int nphi, int nz, double dr, double dphi, double dz,
                        double r_in, double rho, double cp, double k, double dt,
                        double robin_h, double robin_Tinf,
                        int kind_bot, int kind_top, double h_bot, double h_top,
                        double Tinf_bot, double Tinf_top, double T_bot, double T_top,
                        double *a, double *b, double *c, double *r_add_last,
                        double *phi_fac, double *zt, double *smden, double *zclosure, int *fast,
                        double *rfac, long rfac_capacity);
/* adi_step (BE): T_in is not modified and must differ from T_out.  d_tmp_a / d_tmp_b are unused since ABI v13 (may be
 * NULL): the r sweep writes T_out and the phi and z sweeps run in place on it. */
int adi_cyl_step(const adi_cyl_plan *plan, const double *d_T_in, double *d_T_out,
                 double *d_tmp_a, double *d_tmp_b, const double *d_S,
                 const uint8_t *d_active, double T_void, double T_inner, void *stream);
/* One sweep of the BE step (stage entry point for per-stage parity tests and benchmarks): axis 0 = r
 * (build_coeff_r + thomas_batch, adi3d_cyl_phi_v3.py:155-202, :71-87; d_S / d_active / T_void as in adi_cyl_step),
 * axis 1 = phi (phi_solve_spectral, :302-329), axis 2 = z (build_coeff_z + thomas_batch, :255-298; d_active / T_void /
 * T_inner: the post-clamp of adi_step_masked).  d_out may equal d_in (ABI v13): every sweep kernel reads only the rows it
 * writes, so a sweep can run in place -- which halves the working set of a loop that does not need the previous field. */
int adi_cyl_sweep(const adi_cyl_plan *plan, int axis, const double *d_in, double *d_out, const double *d_S,
                  const uint8_t *d_active, double T_void, double T_inner, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Volumetric heat source of the Cartesian step (no counterpart in the reference's Cartesian path; the cylindrical step's
 * `S` is adi3d_cyl_phi_v3.py:339).  For a step t_n -> t_n + dt with a source q(x, t) in W/m^3:
 *     R0 = Tn + dt*kappa*(1-theta)*(Lx+Ly+Lz) + dt * q(x_c, t_n + dt/2) / (rho*cp)      on in-mask cells
 * and the three sweeps run unchanged.  Cell centres x_c = ((i+1/2)dx, (j+1/2)dx, (k+1/2)dx); off-mask cells (padding of a
 * physical box included) receive nothing, Dirichlet rows keep dir_val.
 *
 * adi_heat_source: Goldak's double ellipsoid (Goldak, Chakravarti & Bibby 1984), axis-aligned.  With xi, y, z the offsets
 * of a point from the centre along travel_axis, the transverse axis (the remaining one) and depth_axis:
 *     q = 6 sqrt(3) f eta P / (a b c pi^1.5) * exp(-3 xi^2/c^2 - 3 y^2/a^2 - 3 z^2/b^2)
 *     (f, c) = (f_f, c_f) where travel_sign*xi >= 0, else (2 - f_f, c_r);  q = 0 exactly where the exponent exceeds
 *     ADI_SOURCE_E_CUT (support: +-sqrt(E_CUT/3) times a, b, c).
 * Over all space q integrates to 2 eta P, over the half-space on one side of the centre plane normal to depth_axis to
 * eta P (Goldak's normalisation for a centre on the surface; the mask cuts the rest, nothing is renormalised).
 * The centre at time t is origin + travel_sign * velocity * t along travel_axis (metres; same origin as the cell centres).
 * Valid: finite values, power >= 0, 0 <= eta <= 1, a, b, c_f, c_r > 0, 0 < f_f < 2, velocity >= 0, axes in 0..2 with
 * travel_axis != depth_axis, travel_sign = +-1.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_heat_source {
    double power;        /* P [W] */
    double eta;          /* efficiency */
    double a, b;         /* transverse half-width, depth [m] */
    double c_f, c_r;     /* front / rear length [m] */
    double f_f;          /* front fraction; f_r = 2 - f_f */
    double origin[3];    /* centre at t = 0 [m] */
    double velocity;     /* travel speed [m/s] */
    int travel_axis, travel_sign, depth_axis, reserved;
} adi_heat_source;

#define ADI_SOURCE_E_CUT 40.0
/* device parameter block of a moving source: the source, t0, dt and a 64-bit step counter n (t_n = t0 + n*dt, computed,
 * never accumulated).  Kernels read it through a pointer, so a captured graph follows the source as the block changes. */
#define ADI_SOURCE_BLOCK_BYTES 128

/* the source sampled at the cell centres at time t into d_out (box layout; 0 on off-mask cells) */
int adi_source_sample(const adi_heat_source *h_src, const uint8_t *d_flags, int nx, int ny, int nz, long plane_stride,
                      double dx, double t, double *d_out, void *stream);
/* writes the parameter block d_block (ADI_SOURCE_BLOCK_BYTES, device) on `stream`: the source, t0, dt and the counter n */
int adi_source_set(void *d_block, const adi_heat_source *h_src, double t0, double dt, long long n, void *stream);
/* n += 1 in the block (one thread; what a captured step ends with) */
int adi_source_tick(void *d_block, void *stream);
/* The moving source of one step by superposition: sweep 0 is linear in its right-hand side, so the source term
 * s = dt*q(t_n + dt/2)/(rho*cp) of R0 adds w = A0^-1 s to its output U.  On the axis-0 lines whose (j, k) can meet the
 * support (placed on the device from the block's current centre) this solves A0 w = s over the whole line -- A0 assembled
 * exactly as adi_sweep(axis 0) assembles it for the same pack: d_coeff, or h_face_consts under `sparse` bit 0, d_dir_mask
 * (NULL: no Dirichlet cells) -- and adds w to d_U in place.  h_src gives the support's extent (the launch grid); its
 * shape (a, b, c_f, c_r, axes, sign) must be the block's.  The block's counter is not advanced.  Lines of up to 1024 rows
 * are solved in registers; longer lines need d_work / work_bytes >= adi_source_workspace_bytes (0 for nx <= 1024). */
int adi_source_workspace_bytes(const adi_heat_source *h_src, int nx, int ny, int nz, double dx, size_t *bytes);
int adi_source_lines0(const void *d_block, const adi_heat_source *h_src, double *d_U, const uint8_t *d_flags,
                      const double *d_coeff, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                      int sparse, double dx, double theta, double gam, double dt, double rho, double cp,
                      const double *h_face_consts, void *d_work, size_t work_bytes, void *stream);
/* The same on one slab of a grid cut along axis 0: the box (nx, ny, nz) is the slab, whose local plane i lies at global plane
 * i_org + i (cell centre (i_org + i + 1/2) dx; i_org = 0 is adi_source_lines0).  Every line is solved over the slab's rows
 * only, with ZERO values beyond its ends: the coupling bits of rows 0 and nx-1 to the halo planes (d_flags of a slab) enter
 * the diagonal as in adi_sweep(axis 0) without d_xlo / d_xhi, and their off-diagonal entries multiply zeros.  That is the
 * local solve of the deferred forms of the sharded-axis sweep, whose interface step then carries w to the other slabs. */
int adi_source_lines0_slab(const void *d_block, const adi_heat_source *h_src, double *d_U, const uint8_t *d_flags,
                           const double *d_coeff, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                           int i_org, int sparse, double dx, double theta, double gam, double dt, double rho, double cp,
                           const double *h_face_consts, void *d_work, size_t work_bytes, void *stream);
/* The source term itself, added to R0: d_R0 += dt*q(t_n + dt/2)/(rho*cp) on the in-mask cells of local planes
 * [i_begin, i_end) of the box that are not Dirichlet cells (d_dir_mask may be NULL), q from the block's centre and the cell
 * centres ((i_org + i + 1/2) dx, (j + 1/2) dx, (k + 1/2) dx).  One thread per cell of the support's launch box, placed on the
 * device from the block; nothing else is touched.  0 <= i_begin <= i_end <= nx, i_org >= 0.  For the slab forms that need the
 * whole right-hand side before the sweep (their condensation reads R0). */
int adi_source_add_r0(const void *d_block, const adi_heat_source *h_src, double *d_R0, const uint8_t *d_flags,
                      const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride, int i_org, int i_begin,
                      int i_end, double dx, double dt, double rho, double cp, void *stream);
/* adi_explicit_rhs with a source FIELD d_S [W/m^3] (box layout): R0 += dt*S/(rho*cp) on in-mask cells */
int adi_explicit_rhs_src(const double *d_T, const double *d_S, const uint8_t *d_flags, int nx, int ny, int nz,
                         long plane_stride, double dx, double dt, double kappa, double theta, double rho, double cp,
                         double *d_R0, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Scan path: Goldak's double ellipsoid driven along straight segments, STEP-AVERAGED.  The source of a step [t, t + dt] is
 *     q_step(x) = sum over the segments k, ascending, of (1/dt) * integral over [t, t + dt] n [t_k, t_{k+1}] of q_k(x, tau) dtau
 * with q_k the double ellipsoid above in the frame of segment k (xi along its in-plane direction d, y across it, z along
 * depth_axis; the other two axes in increasing order are the in-plane axes u, v), its centre at p + d*speed*(tau - t_k).  The
 * integral is closed (four erf per point) where the piece travels at least 1e-3 min(c_f, c_r), Simpson's rule on three
 * instantaneous values below that, and the instantaneous value times the piece's length for a dwell.  The cuts bound xi and
 * (y, z) separately: the exponent of (y, z) at most ADI_SOURCE_E_CUT, xi within sqrt(E_CUT/3) times c_f ahead of the piece's
 * last centre and c_r behind its first.  The host definition is heat_source.ScanPath (q_step); csrc/adi_scan_eval.hpp follows
 * it operation for operation, fp64, no contraction, so the device differs from it by the rounding of erf and exp only.
 *
 * Segment table: K rows of ADI_SCAN_TABLE_COLS doubles { t_begin, p[3] start point [m], d[2] in-plane unit direction,
 * speed [m/s], power [W] }, segment k active on [t_begin[k], t_begin[k+1]), the last one up to t_end.  Valid: finite values,
 * 1 <= K <= ADI_SCAN_MAX_SEGMENTS, t_begin strictly ascending, t_end after the last t_begin, |d| = 1, speed >= 0, power >= 0
 * (0: a jump or an idle dwell, which deposits nothing); the shape as adi_heat_source.  Everything else is ADI_ERR_ARG,
 * checked before any HIP call wherever the table is a host array.  A device table (d_table) is the same rows in device
 * memory; the kernels read it only at rows [0, K), K travelling by value in every launch.
 *
 * The step takes the result as a source FIELD (adi_explicit_rhs_src); a correction of sweep 0 from the path itself, as
 * adi_source_lines0 does for the moving source, is not part of the library.  The step of several materials materialises R0
 * and takes the path itself, added there (adi_matmap_scan_add_r0).
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_scan_shape {
    double eta;          /* efficiency */
    double a, b;         /* half-width across the leg, depth [m] */
    double c_f, c_r;     /* front / rear length [m] */
    double f_f;          /* front fraction; f_r = 2 - f_f */
    int depth_axis, reserved;
} adi_scan_shape;

#define ADI_SCAN_TABLE_COLS 8
#define ADI_SCAN_MAX_SEGMENTS (1 << 24)

/* q_step of the step [t, t + dt] at the cell centres of a dense C-order (nx, ny, nz) HOST array h_out, 0 where h_mask (same
 * shape; NULL: every cell) is 0: the evaluator on the CPU.  No HIP call: it runs on a machine without a GPU. */
int adi_scan_sample_host(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, const uint8_t *h_mask,
                         int nx, int ny, int nz, double dx, double t, double dt, double *h_out);
/* the same on the device into d_out (box layout; 0 on off-mask cells): the twin of adi_source_sample for a window.  d_table:
 * the K rows in device memory. */
int adi_scan_sample(const adi_scan_shape *h_shape, const double *d_table, int K, double t_end, const uint8_t *d_flags, int nx,
                    int ny, int nz, long plane_stride, double dx, double t, double dt, double *d_out, void *stream);
/* The window of the step [t, t + dt] on an (nx, ny, nz) grid, from the host table alone (no HIP call): h_seg_out receives the
 * segment range { k0, k1 } the step can overlap, h_box_out { i0, i1, j0, j1, k0, k1 }, the union of the index boxes of its
 * powered pieces as [lo, hi) per axis, all zeros when there is none.  What adi_matmap_scan_add_r0 launches on. */
int adi_scan_window_box(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, int nx, int ny, int nz,
                        double dx, double t, double dt, int *h_seg_out, int *h_box_out);
/* The path inside the step of a grid of several materials ("Several materials" below), without the field: added to the explicit
 * stage's output,
 *     R0_i = R0_i + (dt q_step(x_i; t, dt)) / C_{id_i}     on the in-mask cells of the window's index box,
 * the operations of adi_matmap_explicit's d_S term, in its order, with q_step evaluated in the kernel at the cell centres
 * ((i + 1/2) dx, ...).  The segment range [k0, k1) of the window and the union of the index boxes of its powered pieces are
 * found ON THE HOST from h_table (the K rows in host memory, checked as adi_scan_sample_host checks them) and travel by value
 * with t and dt in one plain launch, one thread per cell of the box; d_table is the same rows in device memory.  The kernel
 * reads d_table, d_flags, d_ids (one byte per cell, the material id) and R0 and writes R0: 17 bytes per in-mask cell of the box.
 * A cell whose q_step is 0 and an off-mask cell are not written.  h_C: C_m = rho_m cp_m of the nmat (1 to ADI_MATMAP_MAX)
 * materials, finite and > 0.  A window that meets no powered piece launches nothing.  h_box_out (NULL, or six ints): receives
 * { i0, i1, j0, j1, k0, k1 }, the box as [lo, hi) per axis, all zeros when it is empty.  Every argument is checked before any
 * HIP call. */
int adi_matmap_scan_add_r0(const adi_scan_shape *h_shape, const double *h_table, const double *d_table, int K, double t_end,
                           double *d_R0, const uint8_t *d_flags, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                           double dx, double t, double dt, int nmat, const double *h_C, int *h_box_out, void *stream);
/* The same on the CPU over dense C-order (nx, ny, nz) HOST arrays: h_R0 in place, h_mask 0 / 1 bytes (NULL: every cell is in),
 * h_ids the id bytes.  No HIP call: the twin of the kernel, as adi_scan_sample_host is of adi_scan_sample. */
int adi_matmap_scan_add_r0_host(const adi_scan_shape *h_shape, const double *h_table, int K, double t_end, double *h_R0,
                                const uint8_t *h_mask, const uint8_t *h_ids, int nx, int ny, int nz, double dx, double t,
                                double dt, int nmat, const double *h_C, int *h_box_out);

/* ------------------------------------------------------------------------------------------------
 * Bead deposition along a scan path: the cells a path brings to life during a step [t, t + dt].  A segment of the table
 * above DEPOSITS when its power is > 0 and its speed is > 0 (jumps, idle dwells and dwells with power lay nothing).  For the
 * piece (ta, tb) of a depositing segment inside the step (times since the segment's start) and a cell centre x, with da the
 * depth axis and (u, v) the in-plane axes, one fp64 operation each and no contraction:
 *     ou = x_u - p_u;  ov = x_v - p_v;  z = x_da - p_da
 *     xi0 = ou*d0 + ov*d1;  y = ov*d0 - ou*d1
 *     sa = speed*ta;  sb = speed*tb;  xc = min(max(xi0, sa), sb);  e = xi0 - xc
 *     r2 = e*e + y*y;  half = 0.5*width;  h2 = half*half
 *     cap = height (box)  or  height*(1 - r2/h2) (parabola)
 *     inside = r2 <= h2  and  z <= 0  and  -z <= cap
 * the cells within width/2 of the path travelled (round ends, closed corners) and at most `cap` below the path's depth
 * coordinate, which is the TOP of the bead.  The result of a step is
 *     born = (OR of inside over the pieces of the step) and within (where given) and not active, inside the logical box;
 * newborn cells get T = Ts and active = 1, every other cell of T and of the mask keeps its bits.  A cell beside a cut of the
 * step is clamped to e = 0 by one of the two pieces, so the union of born over any partition of an interval into steps is
 * that of one step over the whole interval.  The host definition is deposition.PathDeposit.reference; csrc/adi_bead_eval.hpp
 * follows it operation for operation on the host and on the device.
 *
 * Every argument is checked before any HIP call (ADI_ERR_ARG): the shape (finite width and height > 0, profile 0 or 1,
 * depth_axis 0..2), the host table by the rules above, the grid, finite t, dt > 0, finite Ts, the logical box inside the
 * physical one, an active mask that is not `within`.  The index box of a step reaches width/2 (1 + 1e-9) in the plane around
 * both ends of every piece and [p_da - height (1 + 1e-9), p_da] in depth, converted by floor / ceil(x / dx - 0.5) and clipped
 * to the logical grid; the device entry computes it itself from the HOST table, so no caller can pass a box.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_bead_shape {
    double width, height;    /* [m] */
    int profile;             /* 0 box, 1 parabola */
    int depth_axis;
} adi_bead_shape;

/* host, no HIP call: index box [i0,i1) x [j0,j1) x [k0,k1) of the LOGICAL grid (box = { i0, i1, j0, j1, k0, k1 }) that holds
 * every cell the step can bear; *deposits = 0 and an empty box when no segment deposits in [t, t + dt] */
int adi_bead_index_box(const adi_bead_shape *shape, const double *h_table, int K, double t_end, int nx, int ny, int nz,
                       double dx, double t, double dt, int box[6], int *deposits);
/* the evaluator on the CPU over dense C-order (nx, ny, nz) HOST arrays (h_active, h_within: NULL for "no cell is active" /
 * "every cell may be born"): h_born = 1 on the newborn cells, 0 elsewhere.  No HIP call. */
int adi_bead_deposit_host(const adi_bead_shape *shape, const double *h_table, int K, double t_end, const uint8_t *h_active,
                          const uint8_t *h_within, int nx, int ny, int nz, double dx, double t, double dt, uint8_t *h_born);
/* the births of the step on the device: (lx, ly, lz) the logical box inside the physical (nx, ny, nz, plane_stride) of d_T,
 * d_active and d_within (box layout; d_within NULL: every cell may be born); h_table and d_table the same K rows on the host
 * and in device memory.  *d_newborn is zeroed here and then counted with 64-bit integer atomics, as adi_birth_planes does.  An
 * empty index box launches nothing. */
int adi_bead_deposit(const adi_bead_shape *shape, const double *h_table, const double *d_table, int K, double t_end, double *d_T,
                     uint8_t *d_active, const uint8_t *d_within, int lx, int ly, int lz, int nx, int ny, int nz,
                     long plane_stride, double dx, double t, double dt, double Ts, unsigned long long *d_newborn, void *stream);
/* adi_bead_deposit on a grid of several materials ("Several materials" below): on exactly the newborn cells it also writes
 * d_ids[p] = id (0 <= id < ADI_MATMAP_MAX; d_ids in the box layout, not NULL, no alias of a mask); every other id keeps its
 * bits, and d_T, d_active and *d_newborn are what adi_bead_deposit gives (one kernel serves both). */
int adi_bead_deposit_ids(const adi_bead_shape *shape, const double *h_table, const double *d_table, int K, double t_end,
                         double *d_T, uint8_t *d_active, const uint8_t *d_within, uint8_t *d_ids, int id, int lx, int ly, int lz,
                         int nx, int ny, int nz, long plane_stride, double dx, double t, double dt, double Ts,
                         unsigned long long *d_newborn, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Temperature-dependent surface loss of the Cartesian step (no counterpart in the reference, which freezes robin_h when the
 * packs are built; it accepts per-voxel robin_h, so the lagged law below is a sequence of calls the reference can run).
 * Before a step the Robin coefficient of every exposed cell is rewritten from the cell's own temperature T (degrees, the
 * field's unit) at the START of the step.  For face f, with T in the cell, ambient Tinf and SIGMA = 5.670374419e-8:
 *     Tk  = T + T_offset                      Ta = Tinf + T_offset                      (kelvin)
 *     rad = ((emissivity[f]*SIGMA) * (Tk*Tk + Ta*Ta)) * (Tk + Ta)
 *     tab = knot_h[j] + ((knot_h[j+1]-knot_h[j])/(knot_T[j+1]-knot_T[j])) * (T - knot_T[j])   for knot_T[j] <= T < knot_T[j+1],
 *           knot_h[0] below the first knot, knot_h[n_knots-1] from the last knot on; 0 without a table and on a face whose
 *           h[f] and emissivity[f] are both 0
 *     h_f = (h[f] + tab) + rad
 *     coeff[axis] += (h_f * dx^2 / (rho cp dx^3))    on cells exposed on face f, '-' face first, then '+'
 * every operation IEEE fp64 in this order, no contraction: the arrays are bit-identical to adi_build_coeffs with the six
 * h_f fields.  The radiation's ambient is the step's Tinf, the one the Robin term of the sweeps relaxes to.
 * Valid: finite values, h[f] >= 0, 0 <= emissivity[f] <= 1, n_knots 0 or 2..ADI_SURFACE_LOSS_MAX_KNOTS with strictly
 * increasing knot_T, Tinf + T_offset > 0.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_SURFACE_LOSS_MAX_KNOTS 16
#define ADI_SURFACE_LOSS_SIGMA 5.670374419e-8
typedef struct adi_surface_loss {
    double h[6];            /* convection coefficient per face [W/m^2/K]: x-, x+, y-, y+, z-, z+ */
    double emissivity[6];   /* per face */
    double T_offset;        /* field unit -> kelvin (273.15 for degrees Celsius) */
    int n_knots, reserved;  /* 0: no table */
    double knot_T[ADI_SURFACE_LOSS_MAX_KNOTS];
    double knot_h[ADI_SURFACE_LOSS_MAX_KNOTS];
} adi_surface_loss;

/* Rewrites d_coeff[0..2] (the pack arrays of the three axes, box layout) from d_T on the planes [k_begin, k_end) of axis 2.
 * Exposure comes from d_flags (adi_build_nbr_flags: in mask, and a neighbour bit of the axis clear).
 * full = 0 (every step): writes d_coeff[axis] only at in-mask cells exposed along that axis, reads d_T only at cells with an
 *   exposed face, and with d_bricks (adi_build_flag_bricks for the same flags; NULL: none) skips the bricks that hold no such
 *   cell without reading their flags.  Nothing else is touched.
 * full = 1 (a new pack set, or the planes a birth changed): also writes exact zeros to every other cell of those planes, so
 *   a cell that stopped being exposed keeps no stale coefficient.
 * The law travels by value in the launch: a captured graph keeps the law it was captured with. */
int adi_surface_loss_update(const adi_surface_loss *h_law, double Tinf, const double *d_T, const uint8_t *d_flags,
                            const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, double dx, double rho,
                            double cp, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Latent heat of melting and freezing of the Cartesian step (no counterpart in the reference, whose step has constant cp; the
 * correction below is applied to the field its step returns, so the law is a sequence of calls the reference can run).
 * State per cell: the temperature T and a liquid fraction f in [0, 1] (fp64, box layout, 0 off the mask).  The step runs at
 * constant cp from (T, f); afterwards the enthalpy cp*T + L*f of every in-mask cell that is not a Dirichlet cell is put back
 * on the equilibrium curve f_eq(T) = min(max((T - Ts)/(Tl - Ts), 0), 1) (temperature recovery: lagged, first order in dt).
 * Host constants, one fp64 operation each: dT = Tl - Ts, Hs = cp*Ts, Hl = cp*Tl + L, cm = cp + L/dT.  With T* the step's
 * result:
 *     if (f == 0 and T* <= Ts) or (f == 1 and T* >= Tl):   nothing is written
 *     else  H = cp*T* + L*f
 *           H <= Hs:  T = H/cp;             f = 0
 *           H >= Hl:  T = (H - L)/cp;       f = 1
 *           else:     T = Ts + (H - Hs)/cm; f = min(max((T - Ts)/dT, 0), 1)
 * every operation IEEE fp64 in this order, no contraction.  Off-mask cells and Dirichlet cells keep T and f bit for bit.
 * Valid: finite values, latent_heat > 0, T_solidus < T_liquidus, cp > 0.  Everything else is ADI_ERR_ARG, checked before any
 * HIP call.
 *
 * Phase summary: one 32-bit word per 16 x 16 x 16 brick of the box (the bricks of adi_build_flag_bricks), entry
 * ((i/16) * nby + j/16) * nbz + k/16 with nby = ceil(ny/16), nbz = ceil(nz/16); adi_phase_summary_words gives their number
 * (0: bad box).  An entry is 0 exactly when every f of the brick is 0 in memory.  One workgroup owns a brick, its cells and
 * its entry: a workgroup whose entry is 0 does not load f (it takes f = 0); it loads flags only where d_bricks (the flags
 * summary; NULL: none) does not say all-solid, the Dirichlet byte only of cells that reach the `else` above, and it rewrites
 * its entry when it loaded f or wrote a non-zero f.  Far from the melt pool the pass costs one read of T.
 * The law travels by value in the launch: a captured graph keeps the law it was captured with.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_phase_change {
    double latent_heat;     /* L [J/kg] */
    double T_solidus;       /* Ts, the field's unit */
    double T_liquidus;      /* Tl */
} adi_phase_change;

long adi_phase_summary_words(int nx, int ny, int nz);
/* The correction, d_T and d_f in place.  d_dir_mask (NULL: no Dirichlet cells): box layout, non-zero on Dirichlet cells. */
int adi_phase_apply(const adi_phase_change *h_law, double cp, double *d_T, double *d_f, const uint8_t *d_flags,
                    const uint32_t *d_bricks, const uint8_t *d_dir_mask, uint32_t *d_summary, int nx, int ny, int nz,
                    long plane_stride, void *stream);
/* f = f_eq(T) on the in-mask cells d_sel selects (uint8, box layout; NULL: every in-mask cell), Dirichlet cells included;
 * f = 0 off the mask; in-mask cells not selected keep f.  Every entry of the summary is rewritten. */
int adi_phase_seed(const adi_phase_change *h_law, const double *d_T, double *d_f, const uint8_t *d_flags,
                   const uint32_t *d_bricks, const uint8_t *d_sel, uint32_t *d_summary, int nx, int ny, int nz,
                   long plane_stride, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Temperature-dependent conductivity and heat capacity of the Cartesian step (no counterpart in the reference, whose Material
 * is three scalars; the two passes below run around its step, so the law is a sequence of calls the reference can run).
 * k(T) and cp(T) are piecewise-linear in n_knots knots x[] and held at their end values outside; cp may jump at a knot (latent
 * heat as a boost of cp between two knots).  Two exact changes of variable:
 *     Kirchhoff temperature  Theta(T) = x[0] + (1/k_ref) int_{x[0]}^{T} k dT,   so div(k grad T) = k_ref lap(Theta)
 *     enthalpy               H(T) = int cp dT [J/kg],  H = c_lo*T below the first knot
 * and rho dH/dt = k_ref lap(Theta) + q is stepped as: theta = Theta(T_n) (adi_matlaw_theta); the linear step on theta with
 * the constant material (rho, cp_ref, k_ref), ambient Theta(Tinf), Dirichlet values Theta(value), sources and Neumann fluxes
 * unchanged (they are energy); then per cell H(T_new) = H(T_n) + cp_ref*(theta* - Theta(T_n)) (adi_matlaw_recover).  Lagged,
 * first order in dt, stateless.  Stable exactly when cp_ref <= 2 theta_imp min(cp k_ref / k), theta_imp the step's implicitness.
 * Tables (host constants, each one fp64 operation; piece m is anchored at x[m], the last piece has slope 0):
 *     kq[m] = k(x[m])/k_ref          hks[m] = half the slope of k/k_ref on [x[m], x[m+1])        ks2[m] = twice that slope
 *     c[m]  = cp just right of x[m]  hcs[m], cs2[m] likewise for cp                              c_lo = cp below x[0]
 *     theta[0] = x[0], theta[m+1] = theta[m] + (kq[m] + hks[m]*d)*d with d = x[m+1] - x[m];  H[0] = c_lo*x[0], H[m+1] likewise
 * On the piece that holds t (the last m with t >= x[m]; below x[0]: anchored at x[0] with values kq[0] / c_lo and slope 0):
 *     V(t) = V[m] + (y[m] + hs[m]*e)*e,  e = t - x[m]
 *     inverse (the last m with V >= V[m]):  dV = V - V[m];  t = x[m] + (dV + dV) / (y[m] + sqrt(y[m]*y[m] + s2[m]*dV))
 * every operation IEEE fp64 in this order, no contraction.
 * Valid: 2..ADI_MATLAW_MAX_KNOTS knots, finite values, x, theta and H strictly increasing, kq, c, c_lo, k_ref, cp_ref > 0, zero
 * slopes on the last piece, radicands > 0 on every interval.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * The law travels by value in every launch: a captured graph keeps the law it was captured with.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_MATLAW_MAX_KNOTS 16
typedef struct adi_material_law {
    int n_knots, reserved;
    double k_ref, cp_ref, c_lo;
    double x[ADI_MATLAW_MAX_KNOTS];
    double kq[ADI_MATLAW_MAX_KNOTS], hks[ADI_MATLAW_MAX_KNOTS], ks2[ADI_MATLAW_MAX_KNOTS], theta[ADI_MATLAW_MAX_KNOTS];
    double c[ADI_MATLAW_MAX_KNOTS], hcs[ADI_MATLAW_MAX_KNOTS], cs2[ADI_MATLAW_MAX_KNOTS], H[ADI_MATLAW_MAX_KNOTS];
} adi_material_law;

/* d_theta = Theta(d_T) on in-mask cells, d_T bit for bit on every other cell of the box (the sweeps pass off-mask cells
 * through, so the step's result holds T there).  One workgroup per 16^3 brick; d_bricks (NULL: none) spares the flags of
 * all-solid bricks. */
int adi_matlaw_theta(const adi_material_law *h_law, const double *d_T, double *d_theta, const uint8_t *d_flags,
                     const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream);
/* d_out holds theta* (the linear step's result) and is overwritten with T_new; d_T is T_n.  Off-mask cells are not written.
 * Dirichlet cells (d_dir_mask non-zero; NULL: none): T_new = Theta^-1(theta*).  Every other in-mask cell:
 *     d = theta* - Theta(T_n);   d == 0: T_new = T_n bit for bit;   else T_new = H^-1(H(T_n) + cp_ref*d) */
int adi_matlaw_recover(const adi_material_law *h_law, const double *d_T, double *d_out, const uint8_t *d_flags,
                       const uint32_t *d_bricks, const uint8_t *d_dir_mask, int nx, int ny, int nz, long plane_stride,
                       void *stream);
/* adi_surface_loss_update with every h_f multiplied, ahead of dx^2 / (rho cp dx^3), by
 *     ratio = (T - Tinf) / (Theta(T) - Theta(Tinf)),   1 / (k(Tinf)/k_ref) where the denominator is 0
 * so that the sweeps' sink coeff*(theta - Theta(Tinf)) is the loss h_f (T - Tinf).  cp: cp_ref.  Both modes of `full`. */
int adi_matlaw_loss_update(const adi_material_law *h_mat, const adi_surface_loss *h_law, double Tinf, const double *d_T,
                           const uint8_t *d_flags, const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, double dx,
                           double rho, double cp, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Thermal history of the Cartesian step (no counterpart in the reference; the rules below are applied to the pair of fields
 * around one of its steps, so the recorder is a sequence of calls the reference can run).  State per cell (fp64, box layout,
 * NaN off the mask and where "never happened"): the peak temperature T_peak, and the times t_hi, t_lo of the last downward
 * crossing of the levels T_hi > T_lo (cooling time = t_lo - t_hi, the t8/5 of welding for 800 / 500 degrees C).  For a step
 * A (the field at t_n) -> B (the step's final result at t_n + dt), on in-mask cells only:
 *     1.  B > T_peak:              T_peak = B
 *     2.  A > T_hi and B <= T_hi:  t_hi = t_n + dt*((A - T_hi)/(A - B));  t_lo = NaN   (a new cooling cycle begins)
 *     3.  A > T_lo and B <= T_lo:  t_lo = t_n + dt*((A - T_lo)/(A - B))                (after 2: one step may do both)
 *     4.  melt pool record of the step: the number of cells with B >= T_melt and the smallest / largest (i, j, k) among them
 * every operation IEEE fp64 in this order, no contraction.  Off-mask cells are never written.
 * Precondition: every in-mask A has been recorded, A <= T_peak (the recorder follows every step, and adi_history_seed follows
 * every outside edit of T).  One workgroup owns a 16 x 16 x 16 brick (the bricks of adi_build_flag_bricks): it loads flags
 * only where d_bricks (NULL: none) does not say all-solid, B and T_peak of in-mask cells, and A only when some T_peak of the
 * brick exceeds T_lo -- under the precondition no other brick holds a crossing.  t_hi and t_lo are only ever stored.
 *
 * Clock and log: the block (device, ADI_HISTORY_BLOCK_BYTES) is five 8-byte words { double t0, dt; int64 n, slot, capacity };
 * t_n = t0 + n*dt.  The record kernel reads it through the pointer, so a captured graph follows the clock; adi_history_tick
 * (one thread) does n += 1, slot += 1 after it.  The log is (capacity + 1) rows of ADI_HISTORY_LOG_INTS 32-bit integers
 * { cells, lo[3], hi[3], pad }; a step writes row min(slot, capacity) -- row `capacity` is a spill row -- with integer
 * atomics (add / min / max), so the result does not depend on the order of the workgroups.  An empty row is
 * { 0, INT32_MAX x 3, -1 x 3, 0 }.  slot never saturates: max(0, slot - capacity) steps were dropped.
 * The levels travel by value in the launch: a captured graph keeps the levels it was captured with.
 * Valid: finite levels, T_hi > T_lo (T_melt is independent), capacity >= 1, no state array aliasing a field or another state
 * array.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_HISTORY_BLOCK_BYTES 40
#define ADI_HISTORY_LOG_INTS 8
typedef struct adi_history_levels {
    double T_hi;            /* upper level of the cooling time, the field's unit */
    double T_lo;            /* lower level */
    double T_melt;          /* a cell with T >= T_melt belongs to the melt pool */
} adi_history_levels;

/* rules 1 - 4 for the step d_T_in -> d_T_out at the block's clock, into the block's log row */
int adi_history_record(const adi_history_levels *h_levels, const void *d_block, const double *d_T_in, const double *d_T_out,
                       double *d_peak, double *d_t_hi, double *d_t_lo, int32_t *d_log, const uint8_t *d_flags,
                       const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream);
/* t0 and dt of the block, n = 0; slot and capacity stay */
int adi_history_set_clock(void *d_block, double t0, double dt, void *stream);
/* n += 1, slot += 1 */
int adi_history_tick(void *d_block, void *stream);
/* T_peak = T, t_hi = t_lo = NaN on the in-mask cells d_sel selects (uint8, box layout; NULL: every in-mask cell); all three
 * NaN off the mask; in-mask cells not selected keep their state */
int adi_history_seed(const double *d_T, double *d_peak, double *d_t_hi, double *d_t_lo, const uint8_t *d_flags,
                     const uint32_t *d_bricks, const uint8_t *d_sel, int nx, int ny, int nz, long plane_stride,
                     void *stream);
/* every one of the capacity + 1 rows of d_log empty; the block: slot = 0, n = 0, `capacity`; t0 and dt stay */
int adi_history_reset_log(void *d_block, int32_t *d_log, long capacity, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Solidification record of the Cartesian step (no counterpart in the reference; like the thermal history, rules applied to
 * the pair of fields around one of its steps).  State per cell (fp64, box layout, NaN off the mask and where the cell never
 * froze), taken at the moment the cell last froze: the crossing time t_solid, the cooling rate and the SQUARE of the thermal
 * gradient, g2 = |grad T|^2 -- every stored number comes from + - * / alone; the square root is the caller's.  For a step
 * A (the field at t_n) -> B (the step's final result at t_n + dt), an in-mask cell freezes exactly when
 * A > T_freeze and B <= T_freeze, and then
 *     den = A - B;  num = A - T_freeze;  fr = num / den;  off = dt * fr;  t_solid = t_n + off
 *     cooling_rate = den / dt
 *     per axis a, for F in (A, B), with lo / hi = the minus / plus neighbour along a is in the mask (bits 1 + 2a / 2 + 2a
 *     of the cell's flags byte; a box face counts as absent):
 *         both:     d = F[+1] - F[-1];  g = d / (2.0*dx)          hi only:  d = F[+1] - F[0];  g = d / dx
 *         lo only:  d = F[0] - F[-1];   g = d / dx                neither:  g = 0.0
 *       dg = gB - gA;  sg = fr * dg;  g_a = gA + sg               (the gradient at the crossing time)
 *     xx = gx*gx;  yy = gy*gy;  zz = gz*gz;  s = xx + yy;  g2 = s + zz
 * every operation IEEE fp64 in this order, no contraction; 2.0*dx is formed once on the host.  A cell that does not freeze in
 * the step is not written; a cell that freezes again is overwritten.  Off-mask cells are never written by the record.
 * One workgroup owns a 16 x 16 x 16 brick (the bricks of adi_build_flag_bricks) and its word of d_hot (nbx*nby*nbz 32-bit
 * words, brick (bi, bj, bk) at (bi*nby + bj)*nbz + bk): "some in-mask B of the brick is above T_freeze", rewritten by every
 * record.  A is loaded only in bricks whose word from the previous record is set.  Precondition, under which that skip is
 * exact: this step's A is the previous record's B on the mask (the recorder follows every step, and adi_solid_seed follows
 * every outside edit of T).  The clock is a block of the thermal history's layout (ADI_HISTORY_BLOCK_BYTES), driven by
 * adi_history_set_clock and adi_history_tick; the record reads it through the pointer.  T_freeze and dx travel by value.
 * Valid: finite T_freeze, dx > 0, no state array aliasing a field or another state array.  Everything else is ADI_ERR_ARG,
 * checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
int adi_solid_record(double T_freeze, double dx, const void *d_block, const double *d_T_in, const double *d_T_out,
                     double *d_t_solid, double *d_rate, double *d_g2, uint32_t *d_hot, const uint8_t *d_flags,
                     const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, void *stream);
/* all three fields NaN on the in-mask cells d_sel selects (uint8, box layout; NULL: every in-mask cell) and off the mask;
 * in-mask cells not selected keep their state.  The word of a brick is set where a seeded in-mask cell of it has
 * T > T_freeze; a word that is set stays set (zero d_hot once, before the first seed). */
int adi_solid_seed(double T_freeze, const double *d_T, double *d_t_solid, double *d_rate, double *d_g2, uint32_t *d_hot,
                   const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_sel, int nx, int ny, int nz,
                   long plane_stride, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Field monitor of the Cartesian step (no counterpart in the reference, whose drivers take a probe value on the host after
 * every step): one row of a device log per recorded step, taken from the step's final field T.  Stateless per cell: it reads
 * T, the flags and their summary as they are, so a mask change needs no call.
 *   probes   nprobe <= ADI_MONITOR_MAX_PROBES cells (i, j, k) of the box: T at the cell, NaN where the cell is off the mask.
 *   regions  1 <= nreg <= ADI_MONITOR_MAX_REGIONS half-open index boxes { i0, i1, j0, j1, k0, k1 } (h_regions: 6 ints each),
 *            non-empty, inside the box; they may overlap.  Per region, over its in-mask cells:
 *            cells (int64), T_min, T_max (NaN when cells == 0), sum_T, sum_wT (with d_ids: w[id]*T, the product formed
 *            first, one operation; h_weights: nmat <= ADI_MATMAP_MAX doubles by value), sum_extra (with d_extra, a second
 *            field summed like T).  A quantity that is not asked for is logged as 0.
 *   row      nprobe + ADI_MONITOR_REGION_WORDS * nreg 8-byte words: the probes, then per region
 *            { cells, T_min, T_max, sum_T, sum_wT, sum_extra }.  The log is (capacity + 1) rows; a step writes row
 *            min(slot, capacity) of the block (the thermal history's, ADI_HISTORY_BLOCK_BYTES, driven by
 *            adi_history_set_clock / adi_history_tick; read through the pointer, so a captured graph follows it).
 * The order of every sum is fixed by the decomposition of the box into 16 x 16 x 16 bricks and the region's box alone --
 * not by the scheduling of workgroups, the launch box, the all-solid or the flag-reading path, or the width of the loads.
 * An excluded cell (off the mask or outside the region) contributes +0.0.
 *   brick (k_monitor_reduce, one workgroup of 256 threads per brick of the brick box that meets a region): thread t owns the
 *     pairs of cells local (i, j, k) = (2 g + (t >> 7), (t >> 3) & 15, 2 (t & 7) + {0, 1}) of row groups g = 0 .. 7:
 *     pair_g = v0 + v1;  acc = pair_0;  acc = acc + pair_g (g = 1 .. 7);  the 64 lanes of a wave by xor-butterfly
 *     v = v + v[lane ^ o], o = 1, 2, 4, 8, 16, 32;  the four waves ((w0 + w1) + w2) + w3: one partial per (region, brick) in
 *     d_partial, region r's bricks numbered lexicographically (bi, bj, bk) over its own brick box from offset
 *     sum of the brick counts of the regions before it.
 *   region (k_monitor_finish, one workgroup): thread t, acc = +0.0;  acc = acc + partial[n] for n = t, t + 256, ... in
 *     increasing n;  then the same butterfly and the same wave order.
 * Rounding operations from a cell to the logged sum: d = 17 + ceil(nb / 256) + 9, nb the bricks of the region's brick box
 * (one more for sum_wT, whose product rounds first).  No floating-point atomics.  T_min / T_max are the extrema in the total
 * order of the finite doubles in which -0.0 < +0.0: among zeros the minimum is -0.0 if one is present, the maximum +0.0 if
 * one is present; NaN must not occur on in-mask cells.
 * d_partial: ADI_MONITOR_PARTIAL_WORDS 8-byte words per (region, brick), partial_words of them in all (>= the need).
 * d_probes: the device copy of h_probes (3 ints per probe) the kernel reads; a triple outside the box logs NaN.
 * Valid: non-null block, T, flags, partial, log (d_bricks, d_extra, d_ids, h_weights may be null; d_ids needs h_weights and
 * 1 <= nmat <= ADI_MATMAP_MAX; probes null only with nprobe == 0), 1 <= nreg <= 8, 0 <= nprobe <= 256, every region
 * non-empty and inside the box, every probe inside the box, capacity >= 1, neither the log nor the partials aliasing T or
 * the extra field, a brick box within 65535 bricks per axis.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_MONITOR_MAX_REGIONS 8
#define ADI_MONITOR_MAX_PROBES 256
#define ADI_MONITOR_REGION_WORDS 6
#define ADI_MONITOR_PARTIAL_WORDS 6
/* k_monitor_reduce and k_monitor_finish for the field d_T into row min(slot, capacity) of d_log; the caller ticks the block */
int adi_monitor_record(const void *d_block, const double *d_T, const double *d_extra, const uint8_t *d_ids,
                       const uint8_t *d_flags, const uint32_t *d_bricks, int nx, int ny, int nz, long plane_stride, int nreg,
                       const int *h_regions, int nprobe, const int *h_probes, const int *d_probes, int nmat,
                       const double *h_weights, double *d_partial, long partial_words, double *d_log, long capacity,
                       void *stream);
/* every word of the capacity + 1 rows of d_log NaN; the block: slot = 0, n = 0, `capacity`; t0 and dt stay */
int adi_monitor_reset_log(void *d_block, double *d_log, long capacity, long row_words, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Moving heat source of the cylindrical step.  For a step t_n -> t_n + dt:
 *     R0 = Tn + dt * q(x_c, t_n + dt/2) / (rho*cp)
 * and the three sweeps run unchanged.  Cell centres r_i = r_in + (i+1/2) dr, phi_j = (j+1/2) dphi, z_k = (k+1/2) dz (z from
 * the bottom face).  With `d_active` (the adi_step_masked form) q is added on active cells only; void cells keep the clamps.
 *
 * adi_cyl_heat_source: Goldak's double ellipsoid riding on the wall.  Centre at time t: radius r_c, angle
 * phi_c = phi0 + omega t (omega signed), height z_c = z0 + v_z t (v_z = pitch |omega| / 2 pi: a helix; 0: a ring).  Offsets
 * in the Cartesian frame (tangent, radial, axial) at the centre, with delta = phi - phi_c and s = sign(omega) (+1 for 0):
 *     xi = s r sin(delta),  rho = r cos(delta) - r_c,  zeta = z - z_c
 * depth = ADI_CYL_DEPTH_Z (the arc on top of a wall):      E = 3 xi^2/c^2 + 3 rho^2/a^2 + 3 zeta^2/b^2
 * depth = ADI_CYL_DEPTH_R (cladding on a cylinder face):   E = 3 xi^2/c^2 + 3 zeta^2/a^2 + 3 rho^2/b^2
 *     q = 6 sqrt(3) f eta P / (a b c pi^1.5) exp(-E),  (f, c) = (f_f, c_f) where xi >= 0, else (2 - f_f, c_r);
 *     q = 0 exactly where E > ADI_SOURCE_E_CUT.
 * The ellipsoid is rigid, so Goldak's normalisation holds: 2 eta P over all space, eta P over the half-space on one side of
 * the centre plane normal to the depth axis.  Valid: finite values, power >= 0, 0 <= eta <= 1, a, b, c_f, c_r > 0,
 * 0 < f_f < 2, r_c >= 0, depth 0 or 1.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * The parameter block (ADI_SOURCE_BLOCK_BYTES) holds the source, t0, dt and the step counter n at the offsets of the
 * Cartesian block (adi_source_tick advances either); t_n = t0 + n*dt.  The step kernels read it through the pointer, so a
 * captured graph follows every parameter as the block changes.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_CYL_DEPTH_Z 0
#define ADI_CYL_DEPTH_R 1
typedef struct adi_cyl_heat_source {
    double power;        /* P [W] */
    double eta;          /* efficiency */
    double a, b;         /* transverse half-width, depth [m] */
    double c_f, c_r;     /* front / rear length [m] */
    double f_f;          /* front fraction; f_r = 2 - f_f */
    double r_c;          /* radius of the centre [m] */
    double phi0, omega;  /* angle of the centre at t = 0 [rad], angular velocity [rad/s] */
    double z0, v_z;      /* height of the centre at t = 0 [m], axial velocity [m/s] */
    int depth;           /* ADI_CYL_DEPTH_Z or ADI_CYL_DEPTH_R */
    int reserved;
} adi_cyl_heat_source;

/* writes the parameter block d_block (device, ADI_SOURCE_BLOCK_BYTES) on `stream`: the source, t0, dt and the counter n */
int adi_cyl_source_set(void *d_block, const adi_cyl_heat_source *h_src, double t0, double dt, long long n, void *stream);
/* q [W/m^3] at the cell centres of an (nr, nphi, nz) grid at time t into d_out (plane stride plane_stride, 0: nphi*nz);
 * d_active (optional): 0 on inactive cells */
int adi_cyl_source_sample(const adi_cyl_heat_source *h_src, int nr, int nphi, int nz, long plane_stride, double r_in,
                          double dr, double dphi, double dz, double t, const uint8_t *d_active, double *d_out,
                          void *stream);
/* adi_cyl_step with the source of d_block at t_n + dt/2 (plan's dt) evaluated in the r sweep's load; the z sweep advances
 * the block's counter by one (a loop of these needs no separate tick) */
int adi_cyl_step_src(const adi_cyl_plan *plan, void *d_block, const double *d_T_in, double *d_T_out,
                     const uint8_t *d_active, double T_void, double T_inner, void *stream);
/* adi_cyl_sweep with the block: axis 0 adds the source, axis 1 is the plain phi sweep, axis 2 advances the counter */
int adi_cyl_sweep_src(const adi_cyl_plan *plan, int axis, void *d_block, const double *d_in, double *d_out,
                      const uint8_t *d_active, double T_void, double T_inner, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Several materials in one grid.  Every in-mask cell carries a material id (d_ids: one uint8 per
 * cell in the layout of the fields, < nmat on in-mask cells; an id off the mask is never read).  nmat <= ADI_MATMAP_MAX
 * materials with C_m = rho_m cp_m (h_C: nmat doubles) and the pair table h_G: ADI_MATMAP_MAX x ADI_MATMAP_MAX doubles, row m
 * = the cell's own material,
 *     kf(m, m) = k_m,   kf(m, n) = (2 k_m k_n) / (k_m + k_n)   (two half-cells in series),
 *     G[m][n] = (kf(m, n) dt) / (C_m (dx dx)),
 * computed by the caller in fp64 and carried by value in every launch (entries beyond nmat are not read).
 *   explicit stage, in-mask cells (off the mask R0 = T):
 *     R0_i = T_i + (1 - theta) sum over axis 0 -, 0 +, 1 -, 1 +, 2 -, 2 + where that neighbour n is in the mask of
 *            G[id_i][id_n] (T_n - T_i)   [ + (dt S_i) / C_{id_i} ]
 *   sweep along `axis`, whole grid lines in the full-length identity-row form:
 *     free cell (in the mask, not Dirichlet)   (e + p + q) x_i - p x_{i-1} - q x_{i+1} = d,
 *         e = 1 + dt coeff_i,   d = in_i + dt qflux_i + dt coeff_i Tinf,
 *         p = theta G[id_i][id_{i-1}] where the lower neighbour is in the mask, else 0;  q likewise with the upper one
 *     Dirichlet cell   x = dir_value          off-mask cell   x = in
 *   The rows either side of a material interface differ (each is divided by its own C): not symmetric, strictly row-dominant.
 *   packs: coeff_i = sum over the exposed faces of the axis, '-' then '+', of (h (dx dx)) / (C_{id_i} (dx dx dx)); qflux alike.
 * Every entry point validates its arguments before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_MATMAP_MAX 8
/* adi_build_coeffs with the id field and the C table; the arrays are zero wherever a cell is not exposed along the axis */
int adi_matmap_build_coeffs(const uint8_t *d_mask, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride, double dx,
                            int nmat, const double *h_C, const int *h_mode, const double *h_scalar,
                            const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                            const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, void *stream);
/* The same on the planes [k_begin, k_end) of axis 2 only (0 <= k_begin < k_end <= nz, else ADI_ERR_ARG "bad plane range"): inside
 * the range every cell of the six arrays gets exactly what adi_matmap_build_coeffs writes, zeros where it is not exposed;
 * outside it not one byte is written.  After a birth or a deposit only the planes it touched and one either side change
 * exposure.  Nothing but d_mask, d_ids and the per-voxel fields is read. */
int adi_matmap_build_coeffs_planes(const uint8_t *d_mask, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                                   double dx, int nmat, const double *h_C, const int *h_mode, const double *h_scalar,
                                   const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                                   const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, int k_begin,
                                   int k_end, void *stream);
/* A moving Goldak source on such a grid, added to the explicit stage's output: R0_i = R0_i + (dt q_i(t_n + dt/2)) / C_{id_i} on
 * the in-mask cells the support reaches, q from the parameter block d_block of adi_source_set / adi_source_tick and the cell
 * centres ((i + 1/2) dx, ...) -- the operations of adi_matmap_explicit's d_S term, in its order, with q evaluated in the
 * kernel.  One thread per cell of the support's launch box, placed on the device from the block and clipped to the grid as
 * adi_source_add_r0 places it (h_src: the same source on the host, for the box's extent); off-mask cells and cells the support
 * misses are not written.  Reads flags, id and R0 and writes R0: 17 bytes per in-mask cell of the support. */
int adi_matmap_source_add_r0(const void *d_block, const adi_heat_source *h_src, double *d_R0, const uint8_t *d_flags,
                             const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride, double dx, double dt, int nmat,
                             const double *h_C, void *stream);
/* R0 into d_out (must not alias d_T); d_S (optional): source field in W/m^3 */
int adi_matmap_explicit(const double *d_T, const double *d_S, const uint8_t *d_flags, const uint8_t *d_ids, int nx, int ny,
                        int nz, long plane_stride, int nmat, const double *h_G, const double *h_C, double dt, double theta,
                        double *d_out, void *stream);
/* bytes of workspace adi_matmap_sweep needs along `axis` (0: none).  Lines of at most 1024 rows are solved in registers
 * (segments of a line per thread: tiles of adjacent lines along axes 0 and 1, the lanes of a wave along axis 2); longer lines by
 * one thread per line with one field of doubles in the workspace. */
int adi_matmap_workspace_bytes(int axis, int nx, int ny, int nz, long plane_stride, size_t *bytes);
/* one sweep; `variant` as in adi_sweep (which of dir_mask / dir_val / qflux are read).  coeff / qflux are read only on free
 * cells exposed along the axis (the arrays of adi_matmap_build_coeffs for the mask d_flags describes), dir_val on Dirichlet
 * cells.  d_out must not alias d_in or the workspace. */
int adi_matmap_sweep(int axis, int variant, const double *d_in, const uint8_t *d_flags, const uint8_t *d_ids,
                     const double *d_coeff, const uint8_t *d_dir_mask, const double *d_dir_val, const double *d_qflux, int nx,
                     int ny, int nz, long plane_stride, int nmat, const double *h_G, double dt, double theta, double Tinf,
                     double *d_out, void *d_work, size_t work_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Several materials: latent heat and surface loss.  The two pointwise passes around the step, with
 * the law of the cell's own material: "Latent heat" and "Temperature-dependent surface loss" above, cell by cell, with
 * cp = cp_id and rho cp = C_id of the cell's id (d_ids as in "Several materials": an id off the mask is never used).
 *
 * Latent heat.  h_laws: nmat laws; h_on: nmat ints, 0 = the material never melts (its h_laws entry is not read): its cells
 * keep T and f (= 0) bit for bit.  h_cp: nmat heat capacities; the host constants dT, Hs, Hl, cm are evaluated per material as
 * for adi_phase_apply.  d_summary: the phase summary of "Latent heat", same rule.  d_brick_ids: one more 32-bit word per brick
 * (same indexing, adi_phase_summary_words of them): bits 0-7 are the set of ids among the brick's in-mask cells, 0 where it has
 * none.  adi_matmap_phase_seed rewrites it, adi_matmap_phase_apply reads it FIRST and believes it: a brick whose set holds no
 * material with a law is left at once, nothing else read; a brick of one material runs that law without reading ids; only
 * a brick of several materials reads the id bytes, and T only where a cell has a law.  After the mask or the ids changed the
 * words are stale until the next adi_matmap_phase_seed.
 * ---------------------------------------------------------------------------------------------- */
/* The correction, d_T and d_f in place.  d_dir_mask (NULL: no Dirichlet cells): box layout, non-zero on Dirichlet cells. */
int adi_matmap_phase_apply(int nmat, const adi_phase_change *h_laws, const int *h_on, const double *h_cp, double *d_T,
                           double *d_f, const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids,
                           const uint8_t *d_dir_mask, uint32_t *d_summary, const uint32_t *d_brick_ids, int nx, int ny, int nz,
                           long plane_stride, void *stream);
/* f = f_eq(T) of the cell's own law on the in-mask cells d_sel selects (NULL: every in-mask cell), Dirichlet cells included;
 * f = 0 off the mask and in every cell of a material without a law; other in-mask cells keep f.  Every entry of the summary
 * and of d_brick_ids is rewritten. */
int adi_matmap_phase_seed(int nmat, const adi_phase_change *h_laws, const int *h_on, const double *d_T, double *d_f,
                          const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids, const uint8_t *d_sel,
                          uint32_t *d_summary, uint32_t *d_brick_ids, int nx, int ny, int nz, long plane_stride, void *stream);

/* Surface loss.  The laws of up to ADI_MATMAP_MAX materials are too large to travel by value: they live in a device table of
 * adi_matmap_loss_table_bytes() bytes that the caller owns.  adi_matmap_loss_table fills its HOST image (no HIP call) from
 * nmat laws, h_C (C_m = rho_m cp_m) and dx: per law the products and quotients that do not depend on the cell or on Tinf, and
 * C_m (dx dx dx); the caller copies it to the device once, outside any capture.  adi_matmap_loss_update is
 * adi_surface_loss_update with the law and the heat capacity of the cell's id: Ta = Tinf + T_offset and Ta*Ta are evaluated
 * from Tinf (by value) in the kernel, coeff[axis] += (h_f (dx dx)) / (C_id (dx dx dx)) on cells exposed on face f, '-' then '+':
 * bit-identical to adi_matmap_build_coeffs with the six h_f fields.  min_T_offset: the smallest T_offset among the laws
 * (Tinf + T_offset > 0 is checked with it).  full and the plane range as for adi_surface_loss_update. */
size_t adi_matmap_loss_table_bytes(void);
int adi_matmap_loss_table(int nmat, const adi_surface_loss *h_laws, const double *h_C, double dx, void *h_table, size_t bytes);
int adi_matmap_loss_update(const void *d_table, double Tinf, double min_T_offset, const double *d_T, const uint8_t *d_flags,
                           const uint32_t *d_bricks, const uint8_t *d_ids, int nx, int ny, int nz, long plane_stride,
                           double dx, double *const d_coeff[3], int k_begin, int k_end, int full, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Several materials: transitions.  A cell of material m that has a rule (to_m, T_at_m) turns into
 * material to_m when its temperature is at or above T_at_m: loose powder that reaches its liquidus is dense metal from then
 * on.  h_to: nmat ints, the new material of m (another one of the nmat) or < 0 for no rule; h_T_at: nmat doubles, finite where
 * there is a rule and not read elsewhere.  A cell changes exactly when it is in the mask, is not a Dirichlet cell
 * (d_dir_mask, NULL: none), its material has a rule and T >= T_at (equality changes it, a NaN does not); it changes at most
 * once per call -- the decision is taken on the id the call found.  A changed cell gets
 *     its id byte                  to_m
 *     its six pack values          those of adi_matmap_build_coeffs with the new C (d_mask, the face specs and the six arrays
 *                                  of that build; no other cell's values depend on this cell's id)
 *     with a liquid fraction, f    f_eq(T) of the new material's law as adi_matmap_phase_seed evaluates it, 0 without a law
 * and d_T is never written: the properties switch at constant temperature, so sum C_id V T jumps by (C_to - C_m) V T per cell.
 * h_laws / h_on / d_f / d_summary: all of them (the arguments of adi_matmap_phase_seed) or all NULL.
 * d_brick_ids: the id sets of "Several materials: latent heat" (adi_phase_summary_words of them), read FIRST and believed: a
 * brick whose set holds no material with a rule is left at once; otherwise flags and T of its in-mask cells are read, and the
 * id bytes only where some cell is at or above the smallest threshold among the set's ruled materials.  The words of a brick
 * that changed are rewritten for the new ids; with a liquid fraction so is its summary word, by the rule of adi_phase_apply.
 * d_count: one 64-bit counter on the device, the number of changed cells is added to it (integer atomics, one per brick that
 * changed something).  One launch, capturable.
 * ---------------------------------------------------------------------------------------------- */
int adi_matmap_transition(int nmat, const int *h_to, const double *h_T_at, const adi_phase_change *h_laws, const int *h_on,
                          const double *d_T, uint8_t *d_ids, const uint8_t *d_flags, const uint32_t *d_bricks,
                          const uint8_t *d_mask, const uint8_t *d_dir_mask, double *d_f, uint32_t *d_summary,
                          uint32_t *d_brick_ids, unsigned long long *d_count, int nx, int ny, int nz, long plane_stride,
                          double dx, const double *h_C, const int *h_mode, const double *h_scalar,
                          const double *const *d_h_field, const int *q_mode, const double *q_scalar,
                          const double *const *d_q_field, double *const *d_coeff, double *const *d_qflux, void *stream);
/* every word of d_brick_ids from d_flags and d_ids (d_bricks: the flags summary, optional): what adi_matmap_phase_seed leaves
 * there, for a caller that holds no liquid fraction */
int adi_matmap_brick_sets(const uint8_t *d_flags, const uint32_t *d_bricks, const uint8_t *d_ids, uint32_t *d_brick_ids, int nx,
                          int ny, int nz, long plane_stride, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Latent heat and thermal history of the cylindrical step (no counterpart in the reference; both are rules applied around one
 * of its steps).  The laws are the Cartesian ones ("Latent heat", "Thermal history" above); the conventions are the cylindrical
 * backend's: fields in the (nr, nphi, nz) layout, cell (i, j, k) at i*plane_stride + j*nz + k (plane_stride 0: nphi*nz),
 * d_active an optional byte per cell in the same layout (non-zero: active; NULL: every cell is active), no flags, no bricks
 * and no state to synchronise: a NaN in the state marks a cell that has never been seen active, and the first pass that sees
 * it active seeds it from the step's input d_T_in (a birth needs no call).  Inactive cells are never written.
 *
 * adi_cyl_phase_apply, per active cell, d_T (the step's result T*) and d_f in place, in this order:
 *     on plane k = 0 with skip_k0, or k = nz - 1 with skip_kN (the z sweep's Dirichlet rows):  nothing is written
 *     f is NaN (a newborn):  f = min(max((T_in - Ts)/dT, 0), 1), stored even if the cell is then at rest
 *     then the correction of adi_phase_apply with its rest-state rule
 * every operation IEEE fp64 in that order, no contraction.  d_T_in (NULL: nothing is seeded) is required with d_active and is
 * loaded only by threads that hold a newborn.  A value is stored only where its bits change.  The pass reads 1 + 8 + 8 bytes
 * per cell; there is no summary word and no tile skip.
 *
 * adi_cyl_history_record, per active cell, for the step A = d_T_in (at t_n) -> B = d_T_out (at t_n + dt):
 *     T_peak is NaN (a newborn):  T_peak = A, t_hi = t_lo = NaN
 *     then rules 1 - 3 of adi_history_record
 * A is loaded only where not (T_peak <= T_lo) -- true for NaN -- which is exact under that recorder's precondition A <= T_peak.
 * The clock is a block of the thermal history's layout (ADI_HISTORY_BLOCK_BYTES, adi_history_set_clock, adi_history_tick).
 * The log is (capacity + 1) rows of ADI_CYL_HISTORY_LOG_INTS 32-bit integers { cells, lo[3], hi[3], pad, sum_i (int64 at
 * integers 8 and 9), pad, pad }, 8-byte aligned; a step writes row min(slot, capacity) with integer atomics (add / min / max),
 * so the row does not depend on the order of the workgroups.  cells, lo and hi are over the active cells with B >= T_melt as
 * (i, j, k); sum_i is the sum of their radial index i, which makes dphi*dz*dr*((r_in + dr/2)*cells + dr*sum_i) the exact
 * volume of the pool.  An empty row is { 0, INT32_MAX x 3, -1 x 3, 0, 0, 0, 0, 0 }.
 *
 * The *_host functions are the same loops over HOST arrays in the same layout with the same per-cell code; they make no HIP
 * call and run on a machine without a GPU.  adi_cyl_history_record_host reads the clock from h_block (a host copy of the
 * block), accumulates into the row of h_log that block names and does not tick.
 * Valid: what the Cartesian passes require of the law and the levels; nr <= 65535, nphi*nz < 2^31; no null array, d_f not
 * aliasing d_T, no state array aliasing a field or another state array.  Everything else is ADI_ERR_ARG, checked before any
 * HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_CYL_HISTORY_LOG_INTS 12
int adi_cyl_phase_apply(const adi_phase_change *h_law, double cp, double *d_T, double *d_f, const double *d_T_in,
                        const uint8_t *d_active, int skip_k0, int skip_kN, int nr, int nphi, int nz, long plane_stride,
                        void *stream);
int adi_cyl_phase_apply_host(const adi_phase_change *h_law, double cp, double *h_T, double *h_f, const double *h_T_in,
                             const uint8_t *h_active, int skip_k0, int skip_kN, int nr, int nphi, int nz, long plane_stride);
/* f = f_eq(T) on the active cells d_sel selects (uint8, the same layout; NULL: every active cell), NaN on inactive cells;
 * active cells not selected keep f */
int adi_cyl_phase_seed(const adi_phase_change *h_law, const double *d_T, double *d_f, const uint8_t *d_active,
                       const uint8_t *d_sel, int nr, int nphi, int nz, long plane_stride, void *stream);
int adi_cyl_history_record(const adi_history_levels *h_levels, const void *d_block, const double *d_T_in,
                           const double *d_T_out, double *d_peak, double *d_t_hi, double *d_t_lo, int32_t *d_log,
                           const uint8_t *d_active, int nr, int nphi, int nz, long plane_stride, void *stream);
int adi_cyl_history_record_host(const adi_history_levels *h_levels, const void *h_block, const double *h_T_in,
                                const double *h_T_out, double *h_peak, double *h_t_hi, double *h_t_lo, int32_t *h_log,
                                const uint8_t *h_active, int nr, int nphi, int nz, long plane_stride);
/* T_peak = T, t_hi = t_lo = NaN on the active cells d_sel selects (NULL: every active cell); all three NaN on inactive cells;
 * active cells not selected keep their state */
int adi_cyl_history_seed(const double *d_T, double *d_peak, double *d_t_hi, double *d_t_lo, const uint8_t *d_active,
                         const uint8_t *d_sel, int nr, int nphi, int nz, long plane_stride, void *stream);
/* every one of the capacity + 1 rows of d_log empty; the block: slot = 0, n = 0, `capacity`; t0 and dt stay */
int adi_cyl_history_reset_log(void *d_block, int32_t *d_log, long capacity, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Field monitor of the cylindrical step (no counterpart in the reference): one row of a device log per recorded step, taken
 * from the step's final field T, in the conventions of the cylindrical backend -- fields in the (nr, nphi, nz) layout, cell
 * (i, j, k) at i*plane_stride + j*nz + k (plane_stride 0: nphi*nz), d_active an optional byte per cell (NULL: every cell is
 * active), no flags, no bricks, no per-cell state: a birth needs no call.
 *   probes   nprobe <= ADI_MONITOR_MAX_PROBES cells (i, j, k): T at the cell, NaN where the cell is not active.
 *   regions  1 <= nreg <= ADI_MONITOR_MAX_REGIONS half-open index boxes { i0, i1, j0, j1, k0, k1 } (h_regions: 6 ints each),
 *            non-empty, inside the grid along r and z; phi is periodic: 0 <= j0 < nphi, j0 < j1 <= j0 + nphi, the box holds the
 *            cells j mod nphi.  They may overlap.  Per region, over its active cells, ADI_CYL_MONITOR_REGION_WORDS words:
 *            { cells (int64), sum_i (int64: the sum of the radial index), T_min, T_max (NaN when cells == 0), sum_T, sum_rT,
 *              sum_extra, sum_rextra } -- r_i = r_in + (i + 1/2) dr, so dr dphi dz sum_rT is the volume integral of T; the last
 *            two from d_extra, a second field summed like T with a NaN on an included cell as +0.0; both +0.0 without it.
 *   row      nprobe + ADI_CYL_MONITOR_REGION_WORDS * nreg 8-byte words: the probes, then the regions.  The log is
 *            (capacity + 1) rows; a step writes row min(slot, capacity) of the block (the thermal history's,
 *            ADI_HISTORY_BLOCK_BYTES, adi_history_set_clock / adi_history_tick; read through the pointer).
 * The order of every sum is fixed by the grid's shape, (r_in, dr) and the region's box alone -- not by pointer alignment, the
 * width of the loads, the launch box or the scheduling of workgroups.  An excluded cell (inactive, outside the region, the
 * missing partner of an odd nz) contributes +0.0.
 *   plane of radius i: per_line = ceil(nz / 2); pair q = j*per_line + p holds the cells (j, 2p), (j, 2p + 1): pair = v0 + v1.
 *     Chunk c holds the pairs 256c .. 256c + 255, one per thread (+0.0 past the last pair); the 64 lanes of a wave by
 *     xor-butterfly v = v + v[lane ^ o], o = 1, 2, 4, 8, 16, 32; the four waves ((w0 + w1) + w2) + w3: partial[i][c].  Over
 *     the nchunk = ceil(nphi*per_line / 256) partials: thread t of 256, acc = +0.0; acc = acc + partial[i][n] for
 *     n = t, t + 256, ...; the same butterfly and wave order: S_i.  A chunk that holds no cell of the region has partial +0.0
 *     and may be skipped: acc is never -0.0.
 *   region: sum_T: acc = +0.0; acc = acc + S_i for i = i0 .. i1 - 1.  sum_rT: p = r_i * S_i first (one operation), then
 *     acc = acc + p; r_i = r_in + ((i + 1/2) * dr).  No contraction.  sum_extra and sum_rextra likewise.
 * Rounding operations from a cell to the logged sum: d = 19 + ceil(nchunk / 256) + (i1 - i0), one more for the r-weighted
 * sums.  No floating-point atomics.  T_min / T_max are the extrema in the total order of the finite doubles in which
 * -0.0 < +0.0; NaN must not occur on active cells.
 * d_partial: ADI_CYL_MONITOR_PARTIAL_WORDS 8-byte words per (region, radius, chunk) and per (region, radius):
 * partial_words >= ADI_CYL_MONITOR_PARTIAL_WORDS * sum over the regions of (i1 - i0) * (nchunk + 1).  d_probes: the device
 * copy of h_probes (3 ints per probe).
 * adi_cyl_monitor_record_host is the same code over HOST arrays (block, T, extra, active, log) and returns the same bits; it
 * makes no HIP call, needs no partial buffer and does not tick.  It touches (nr - 1)*plane_stride + nphi*nz elements of a
 * field, ADI_HISTORY_BLOCK_BYTES of the block and one row of the (capacity + 1) rows of the log.
 * Valid: non-null block, T, partial, log (d_active and d_extra may be null; probes null only with nprobe == 0), regions and
 * probes as above, capacity >= 1, finite r_in >= 0 and dr > 0, nr <= 65535, nphi*nz < 2^31, neither the log nor the partials
 * aliasing T or the extra field.  Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_CYL_MONITOR_REGION_WORDS 8
#define ADI_CYL_MONITOR_PARTIAL_WORDS 5
/* the three kernels for the field d_T into row min(slot, capacity) of d_log; the caller ticks the block */
int adi_cyl_monitor_record(const void *d_block, const double *d_T, const double *d_extra, const uint8_t *d_active, int nr,
                           int nphi, int nz, long plane_stride, double r_in, double dr, int nreg, const int *h_regions,
                           int nprobe, const int *h_probes, const int *d_probes, double *d_partial, long partial_words,
                           double *d_log, long capacity, void *stream);
int adi_cyl_monitor_record_host(const void *h_block, const double *h_T, const double *h_extra, const uint8_t *h_active, int nr,
                                int nphi, int nz, long plane_stride, double r_in, double dr, int nreg, const int *h_regions,
                                int nprobe, const int *h_probes, double *h_log, long capacity);
/* every word of the capacity + 1 rows of d_log NaN; the block: slot = 0, n = 0, `capacity`; t0 and dt stay */
int adi_cyl_monitor_reset_log(void *d_block, double *d_log, long capacity, long row_words, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Solidification record of the cylindrical step (no counterpart in the reference): the conditions at the freezing front, in
 * the conventions of the cylindrical backend -- fields in the (nr, nphi, nz) layout, cell (i, j, k) at
 * i*plane_stride + j*nz + k (plane_stride 0: nphi*nz), d_active an optional byte per cell (NULL: every cell is active), no
 * flags, no bricks.  NaN in the state means "never froze", whether or not the cell was ever active: nothing is seeded and a
 * birth needs no call.
 *
 * adi_cyl_solid_record, for the step A = d_T_in (at t_n) -> B = d_T_out (at t_n + dt): an active cell with A > T_freeze and
 * B <= T_freeze freezes in the step and has its three values overwritten; every other cell is never written.
 *     den = A - B, num = A - T_freeze, fr = num/den, off = dt*fr, t_solid = t_n + off, rate = den/dt
 *     per axis, for F in (A, B): d/(2h) central where both neighbours are present, d/h one-sided where one is, 0 where none is;
 *       dg = gB - gA, sg = fr*dg, g = gA + sg
 *     g2 = (g_r*g_r + g_phi*g_phi) + g_z*g_z
 * h = dr along r, dz along z and r_i*dphi along phi with r_i = r_in + ((i + 0.5)*dr).  The neighbours are i -+ 1 and k -+ 1
 * inside the box (a box face counts as absent) and (j -+ 1) mod nphi: none with nphi == 1, the same cell twice with nphi == 2
 * (a central difference of +0.0).  A neighbour is present only where d_active holds it; the values of inactive cells never
 * enter.  Every operation IEEE fp64 in that order, no contraction.  The clock is a block of the thermal history's layout
 * (ADI_HISTORY_BLOCK_BYTES, adi_history_set_clock, adi_history_tick), the log is the cylindrical history's
 * (ADI_CYL_HISTORY_LOG_INTS integers per row, adi_cyl_history_reset_log): row min(slot, capacity) takes { cells, lo[3], hi[3],
 * sum_i } over the cells that froze in the step, with integer atomics.
 *
 * A tile is ADI_CYL_SOLID_TILE consecutive cells p = j*nz + k of one radius' plane; d_hot (optional) holds one 32-bit word per
 * tile, word i*ntile + q with ntile = ceil(nphi*nz / ADI_CYL_SOLID_TILE): set iff some active cell of the tile had
 * T > T_freeze in the field of the last record (its B) or of adi_cyl_solid_hot_seed.  With d_hot a tile whose word is clear
 * reads d_active and B only -- nothing can have frozen there -- and every tile's word is rewritten where it changes.  That is
 * exact under the precondition that on every active cell this record's A is bitwise the previous record's B (or the seeded
 * field) and d_active is unchanged; a birth breaks it, so a caller that activates cells passes NULL.  NULL: every tile runs
 * the full path, with no precondition.
 *
 * The *_host functions are the same loops over HOST arrays with the same per-cell code; they make no HIP call.
 * adi_cyl_solid_record_host reads the clock from h_block, accumulates into the row of h_log that block names and does not tick.
 * Valid: no null array but d_active and d_hot, d_T_in != d_T_out, no state array aliasing a field or another state array,
 * finite T_freeze, finite dr, dphi, dz > 0, finite r_in >= 0, block and log 8-byte aligned, nr <= 65535, nphi*nz < 2^31.
 * Everything else is ADI_ERR_ARG, checked before any HIP call.
 * ---------------------------------------------------------------------------------------------- */
#define ADI_CYL_SOLID_TILE 512
int adi_cyl_solid_record(double T_freeze, double r_in, double dr, double dphi, double dz, const void *d_block,
                         const double *d_T_in, const double *d_T_out, double *d_t_solid, double *d_rate, double *d_g2,
                         int32_t *d_log, const uint8_t *d_active, int32_t *d_hot, int nr, int nphi, int nz, long plane_stride,
                         void *stream);
int adi_cyl_solid_record_host(double T_freeze, double r_in, double dr, double dphi, double dz, const void *h_block,
                              const double *h_T_in, const double *h_T_out, double *h_t_solid, double *h_rate, double *h_g2,
                              int32_t *h_log, const uint8_t *h_active, int32_t *h_hot, int nr, int nphi, int nz,
                              long plane_stride);
/* every word of d_hot from d_T: 1 where an active cell of the tile has T > T_freeze, else 0 */
int adi_cyl_solid_hot_seed(double T_freeze, const double *d_T, const uint8_t *d_active, int32_t *d_hot, int nr, int nphi, int nz,
                           long plane_stride, void *stream);
int adi_cyl_solid_hot_seed_host(double T_freeze, const double *h_T, const uint8_t *h_active, int32_t *h_hot, int nr, int nphi,
                                int nz, long plane_stride);

/* ------------------------------------------------------------------------------------------------
 * Context API: the library owns the device memory; callers hand over HOST arrays.
 * One context per GPU and thread; no hidden global state.
 * ---------------------------------------------------------------------------------------------- */
typedef struct adi_ctx adi_ctx;

/* Grid3D(nx,ny,nz,dx,mask): adi3d_numba_coeff.py:14-19 (mask copied) */
int adi_ctx_create(int nx, int ny, int nz, double dx, int device, adi_ctx **out);
int adi_ctx_destroy(adi_ctx *ctx);
/* grid.mask = ... (drivers rebind the mask between steps: single_track_on_plate.py:159-160) */
int adi_ctx_set_mask(adi_ctx *ctx, const uint8_t *h_mask);
/* precompute_coeff_packs_unified with host-side BC data; h_dir_mask/h_dir_val may be NULL */
int adi_ctx_build_coeffs(adi_ctx *ctx, double rho, double cp,
                         const int *h_mode, const double *h_scalar, const double *const *h_h_field,
                         const int *q_mode, const double *q_scalar, const double *const *h_q_field,
                         const uint8_t *h_dir_mask, const double *h_dir_val);
int adi_ctx_upload_T(adi_ctx *ctx, const double *h_T);
int adi_ctx_download_T(adi_ctx *ctx, double *h_T);
/* read the device-built pack arrays back (axis 0..2); any pointer may be NULL */
int adi_ctx_download_pack(adi_ctx *ctx, int axis, double *h_coeff, double *h_qflux);
/* nsteps calls of adi_step with the same packs and dt (drivers' inner loop,
 * quick_compare_dirichlet_robin.py:169-178); T stays resident on the device */
int adi_ctx_step(adi_ctx *ctx, double rho, double cp, double k, double dt, double theta, double Tinf, int nsteps);
/* wall time in milliseconds of the last adi_ctx_step, measured with HIP events on the context's stream */
int adi_ctx_last_step_ms(adi_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* ADI_HIP_H */
