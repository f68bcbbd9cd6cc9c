/*
 * nbk_hip.h — C ABI of libnbk_hip.so, the hand-written HIP (gfx950)
 * compute core of nbodykit_amd.
 *
 * This is the internal drop-in boundary defined in SURVEY.md §8(b): the
 * reference (bccp/nbodykit) has no C plugin interface — its operator API
 * is the MeshSource/CatalogSource Python duck type — so this ABI carries
 * exactly the pmesh/pfft operations the Python layer replaces:
 *
 *   nbk_paint_f64        <- pmesh ParticleMesh.paint (CIC/TSC/PCS scatter;
 *                           called at nbodykit/source/mesh/catalog.py:287,
 *                           295-296)
 *   nbk_fft_*            <- pfft-python distributed R2C/C2R
 *                           (pmesh RealField.r2c/ComplexField.c2r; called
 *                           via nbodykit/base/mesh.py:301-304), forward
 *                           normalized by 1/Ntotal
 *   nbk_compensate_f64   <- the Fourier-space window compensations
 *                           (nbodykit/source/mesh/catalog.py:419-594)
 *   nbk_interlace_combine_f64
 *                        <- the interlaced-mesh combine
 *                           c = c1/2 + c2/2 exp(i k.H/2)
 *                           (nbodykit/source/mesh/catalog.py:341-347)
 *   nbk_power3d_f64      <- p3d = c1 conj(c2) * V, zero mode cleared
 *                           (nbodykit/algorithms/fftpower.py:114-128)
 *   nbk_bin_power_f64    <- project_to_basis binning sums
 *                           (nbodykit/algorithms/fftpower.py:507-701)
 *   nbk_readout_nnb_f64 / elementwise helpers — support ops.
 *
 * Conventions:
 *   - plain pointers + sizes only; all device pointers are HIP device
 *     memory owned by the caller (torch allocations in practice, but no
 *     torch types cross this boundary);
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *     all launches are asynchronous on that stream;
 *   - return value: 0 on success, a negative NBK_ERR_* code otherwise;
 *     nbk_last_error_string() describes the most recent failure;
 *   - complex double arrays are interleaved (re,im) — C `double _Complex`
 *     layout, i.e. numpy complex128 / torch complex128;
 *   - the mesh is slab-partitioned along axis 0; every kernel taking
 *     `x0/nx_local` operates on the local slab of a global
 *     (n0, n1, n2) mesh.  Single-GPU: x0 = 0, nx_local = n0.
 */
#ifndef NBK_HIP_H
#define NBK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define NBK_OK            0
#define NBK_ERR_HIP      -1   /* HIP runtime error, see last_error_string */
#define NBK_ERR_ARG      -2   /* bad argument (size, window id, ...) */
#define NBK_ERR_UNSUPPORTED -3 /* e.g. non-power-of-two FFT length */

/* window ids (resampler names in the Python layer) */
#define NBK_WINDOW_CIC 0   /* support 2 */
#define NBK_WINDOW_TSC 1   /* support 3 */
#define NBK_WINDOW_PCS 2   /* support 4 */

/* library info ------------------------------------------------------- */
const char* nbk_version(void);
const char* nbk_last_error_string(void);
/* number of HIP devices visible (also a cheap "runtime works" probe) */
int nbk_device_count(void);

/* paint --------------------------------------------------------------
 * Scatter n particles into the local mesh slab with window `window` and
 * half-cell interlacing shift `shift` (0.0 or 0.5, in mesh units;
 * pm.affine.shift(0.5) at source/mesh/catalog.py:292).
 *
 *   pos     : device, SoA layout, 3 contiguous blocks of n doubles
 *             (x[n], y[n], z[n]) — pos + 0, pos + n, pos + 2n
 *   mass    : device, n doubles, or NULL for unit mass
 *   nmesh   : global mesh size (n0, n1, n2)
 *   box     : BoxSize per axis
 *   x0, nx_local : local slab [x0, x0+nx_local) of axis 0; deposits
 *             whose wrapped global x index falls outside are skipped
 *             (ghost copies on the neighbour rank own them)
 *   mesh    : device, local slab, nx_local*n1*n2 doubles, accumulated
 *             into (hold=True semantics)
 */
int nbk_paint_f64(const double* pos, const double* mass, int64_t n,
                  const int64_t nmesh[3], const double box[3],
                  int window, double shift,
                  double* mesh, int64_t x0, int64_t nx_local,
                  void* stream);

/* paint for cell-sorted input: PCS deposits accumulate in an LDS window
 * per contiguous particle run and flush once (CIC and TSC go to
 * nbk_paint_f64, which is faster for them).  Same semantics as
 * nbk_paint_f64; the caller must know the input is cell-ordered (the
 * bucket sort's output is). */
int nbk_paint_sorted_f64(const double* pos, const double* mass, int64_t n,
                         const int64_t nmesh[3], const double box[3],
                         int window, double shift,
                         double* mesh, int64_t x0, int64_t nx_local,
                         void* stream);

/* ownership-gather paint for cell-sorted input: requires the row table
 * produced by nbk_bucket_fine_f64 (rowtab[n0*n1+1]: start of each
 * (ix, iy) row in the sorted SoA arrays, sentinel n at the end).  Each
 * block owns an exclusive LDS mesh tile (P x-planes x RG y-rows x n2;
 * the tile shape is picked per window span — single-plane max-RG for
 * CIC, balanced multi-plane for TSC/PCS — within the 160 KiB LDS
 * budget) and gathers from the source rows whose stencils reach it —
 * deposits
 * are LDS f64 adds and the flush is plain stores, NO global atomics
 * (the global atomic pipe is the ~25 G op/s bound on the scatter
 * kernels above).  accumulate=0 overwrites the slab (fresh mesh, saves
 * the read), accumulate=1 adds (hold semantics for chunked paints).
 * Returns NBK_ERR_UNSUPPORTED when no LDS tile fits (fall back to
 * nbk_paint_f64). */
/* pair_gs >= 0: `rowtab` is the PAIR-BUCKET table of the duplicating
 * sort (nbk_psort_*): [(n0/2)*(n1>>pair_gs)+1] exclusive bases, one
 * contiguous range per (x-plane pair, y-group); the tile geometry is
 * pinned to (1 plane x 1<<pair_gs rows) and the deposit masks drop the
 * duplicated out-of-tile copies.  pair_gs = -1: per-row table from
 * nbk_bucket_fine_f64.  Both table modes serve every window and shift
 * (the sort's [dlo, dhi] must cover the window's rows at that shift),
 * and any n0: on a mesh with fewer x-planes than a tile's source span
 * the plane walk stops after n0 planes, so no source plane and no pair
 * bucket is read twice. */
int nbk_paint_gather_f64(const double* pos, const double* mass, int64_t n,
                         const int64_t nmesh[3], const double box[3],
                         int window, double shift, const int* rowtab,
                         double* mesh, int64_t x0, int64_t nx_local,
                         int accumulate, int pair_gs, void* stream);

/* gather paint with the forward z-axis FFT fused into the tile flush:
 * writes the z half-spectrum ((nx_local, n1, n2/2+1) interleaved c128,
 * every element scaled by `scale`) directly — the real mesh never
 * exists in HBM.  Same source/rowtab semantics as nbk_paint_gather_f64;
 * overwrite-only (single paint per output).  n2 must be a power of two
 * in [8, 4096].  The FFT math is identical to nbk_fft_r2c_z. */
int nbk_paint_gather_fft_f64(const double* pos, const double* mass,
                             int64_t n, const int64_t nmesh[3],
                             const double box[3],
                             int window, double shift, const int* rowtab,
                             double* zspec, int64_t x0, int64_t nx_local,
                             double scale, int pair_gs, void* stream);

/* paint locality sort --------------------------------------------------
 * Two-pass counting sort of particles by coarse mesh cell
 * (bucket = wrapped ix * n1 + iy): count, then (after the caller turns
 * counts into exclusive offsets) scatter into SoA output.  Replaces a
 * general radix sort in the paint driver: the deposit kernel wants
 * bucket-local order, not a total order.  Bucket = cell >> shift
 * (shift 0 = per-cell).  `pos_aos` is the (n,3) row-major input;
 * `offsets` (ncells >> shift, int32) holds the INCLUSIVE bucket cumsum
 * and is consumed (tickets count DOWN to the exclusive base) by the
 * scatter; soa_out selects x/y/z planes (paint layout) vs AoS rows.
 * mass may be NULL.  Requires n < 2^31 (int32 tickets).
 */
int nbk_bucket_count_f64(const double* pos_aos, int64_t n,
                         const int64_t nmesh[3], const double box[3],
                         int shift,
                         int* counts, int* scrambled_flag, void* stream);
int nbk_bucket_scatter_f64(const double* pos_aos, const double* mass,
                           int64_t n, const int64_t nmesh[3],
                           const double box[3], int shift, int soa_out,
                           int* offsets,
                           double* pos_out, double* mass_out,
                           void* stream);

/* Count-matrix sorts (the paint locality passes for big meshes).  The
 * GPU's global-atomic pipe runs at ~25 G ops/s regardless of locality
 * (csrc/count_probe.hip), so the single-level count/scatter above is
 * atomic-bound at 1e9 particles; these pipelines keep every
 * histogram/cursor in LDS.  They share one scheme (csrc/nbk_countsort.h;
 * nbk_pairs_cell_* below is its third key): a *_count step writes one
 * nbuckets-wide histogram row per chunk of `chunk` particles into `mat`
 * (ceil(n/chunk) x nbuckets, int32 row-major), nbk_scan_matrix_i32 scans
 * it, and a *_scatter step re-reads each chunk and places SoA planes
 * from LDS cursors (deterministic bucket ranges, arbitrary order within
 * a bucket).  Every step requires 0 <= n < 2^31, chunk >= 1 (the same
 * chunk in both steps) and 1 <= nbuckets <= 40960 (160 KiB of LDS ints),
 * checks its geometry whatever n is, returns NBK_ERR_ARG before
 * launching anything otherwise, and does nothing for n = 0.
 *
 * nbk_scan_matrix_i32: device scan of `mat` -> per-chunk cursor seeds
 * `bases` (chunk-major) and bucket edges `bucket_bases` (nbuckets+1,
 * exclusive; [nbuckets] = the number of placed particles).  colsum_tmp
 * is 9 * nbuckets ints of scratch (8 segment partials + column sums). */
int nbk_scan_matrix_i32(const int* mat, int64_t nblocks, int64_t nbuck,
                        int* colsum_tmp, int* bases, int* bucket_bases,
                        void* stream);

/* Two-level cell sort: coarse key = ix * (n1>>ys) + (iy>>ys), ys chosen
 * so that BOTH nbuckets = n0*(n1>>ys) and the fine window (1<<ys)*n2 fit
 * the LDS.  nbk_xsort_count_f64 (pass A) also detects cell-ordered input
 * into scrambled_flag (may be NULL); nbk_xsort_scatter_f64 (pass C)
 * writes x[n] y[n] z[n] into pos_out (mass may be NULL);
 * nbk_bucket_fine_f64 runs one block per coarse bucket over that SoA
 * output: it counts the bucket's cells in an LDS window, block-scans it,
 * and emits the exact cell-sorted SoA output — no global atomics.
 * Requires power-friendly dims (n1 divisible by 1<<ys, window
 * divisible by 1024). */
int nbk_xsort_count_f64(const double* pos_aos, int64_t n, int chunk,
                        const int64_t nmesh[3], const double box[3],
                        int ys, int* mat, int* scrambled_flag,
                        void* stream);
int nbk_xsort_scatter_f64(const double* pos_aos, const double* mass,
                          int64_t n, int chunk, const int64_t nmesh[3],
                          const double box[3], int ys, const int* bases,
                          double* pos_out, double* mass_out,
                          void* stream);
int nbk_bucket_fine_f64(const double* pos_soa, const double* mass,
                        int64_t n, const int64_t nmesh[3],
                        const double box[3], int ys,
                        const int* bucket_bases,
                        double* soa_out, double* mass_out,
                        int* rowtab, int rows_only, void* stream);

/* PAIR-BUCKET duplicating sort (see nbk_paint_gather_f64 pair_gs):
 * key = (x-plane pair, y row-group) with each particle duplicated into
 * every y-group rows [iy+dlo, iy+dhi] of its deposit stencil touch
 * (<= 2 copies).  Both steps require n0 even, n1 divisible by 1<<ys and
 * dhi-dlo < 1<<ys; n_out = bucket_bases[nbuck] after
 * nbk_scan_matrix_i32, and the output planes are x[n_out] y[n_out]
 * z[n_out]. */
int nbk_psort_count_f64(const double* pos_aos, int64_t n, int chunk,
                        const int64_t nmesh[3], const double box[3],
                        int ys, int dlo, int dhi, int* mat, void* stream);
int nbk_psort_scatter_f64(const double* pos_aos, const double* mass,
                          int64_t n, int chunk, const int64_t nmesh[3],
                          const double box[3], int ys, int dlo, int dhi,
                          const int* bases, int64_t n_out,
                          double* pos_out, double* mass_out,
                          void* stream);

/* readout (gather dual of paint; window 0/1/2 = cic/tsc/pcs, 3 = nnb).
 * Serves FFTRecon's displacement solve (fftrecon.py:246-249) and the
 * LogNormal generator's nnb reads (mockmaker.py:317-319).  Cells outside
 * the local slab contribute 0 — ghost owners add their partials via the
 * host-side exchange. */
int nbk_readout_f64(const double* pos, int64_t n,
                    const int64_t nmesh[3], const double box[3],
                    int window,
                    const double* mesh, int64_t x0, int64_t nx_local,
                    double* out, void* stream);

/* FFTRecon displacement solve (fftrecon.py:222-238):
 * out = i k_axis/k^2 exp(-k^2 R^2/2) / (bias (1 + (f/bias) mu^2)) in */
int nbk_recon_displacement_f64(double* out, const double* in,
                               const int64_t nmesh[3], const double box[3],
                               const int64_t dims[3], const int64_t off[3],
                               int axis, double R, double bias, double f,
                               const double los[3], void* stream);

/* FFT ----------------------------------------------------------------
 * Power-of-two lengths only (8 <= N <= 4096).  The 3D transform is
 * composed by the Python layer from these batched passes (plus the RCCL
 * alltoall pencil transpose between ranks):
 *
 *   z pass  : real <-> half-complex along the contiguous last axis
 *   strided : in-place complex pass along a strided axis (y or x)
 *
 * Layouts: nbk_fft_r2c_z treats `real` as nlines contiguous lines of nz
 * doubles, writing nlines * (nz/2+1) complex outputs; `scale` multiplies
 * every output (the Python layer passes 1/(n0*n1*n2) here so the forward
 * 3D transform matches pmesh's normalization).  nbk_fft_c2r_z is the
 * unnormalized inverse.  nbk_fft_c_strided transforms n_lines lines of
 * length nfft; element j of line (o, i) lives at
 * cplx[o*outer_stride + j*stride + i] with i < n_inner contiguous.
 * sign: -1 forward, +1 inverse (unnormalized).
 */
int nbk_fft_r2c_z(const double* real, double* cplx,
                  int64_t nlines, int64_t nz, double scale, void* stream);
int nbk_fft_c2r_z(const double* cplx, double* real,
                  int64_t nlines, int64_t nz, void* stream);
int nbk_fft_c_strided(double* cplx, int64_t nfft, int64_t stride,
                      int64_t n_outer, int64_t outer_stride,
                      int64_t n_inner, int sign, void* stream);

/* k-space elementwise ------------------------------------------------
 * All of these address a local complex slab of logical global shape
 * (n0, n1, n2h); `axis_map` gives, for each local axis, which global
 * axis it carries (identity (0,1,2) untransposed; (1,0,2) for the
 * post-alltoall transposed layout), and `off` the global start of the
 * local block along each LOCAL axis.  dims = local shape.
 */
int nbk_compensate_f64(double* cplx, const int64_t nmesh[3],
                       const int64_t dims[3], const int64_t off[3],
                       const int axis_map[3],
                       int window, int interlaced, void* stream);

int nbk_interlace_combine_f64(double* c1, const double* c2,
                              const int64_t nmesh[3], const double box[3],
                              const int64_t dims[3], const int64_t off[3],
                              const int axis_map[3], void* stream);

int nbk_power3d_f64(double* out, const double* c1, const double* c2,
                    double volume,
                    const int64_t dims[3], const int64_t off[3],
                    int clear_zero_mode, void* stream);

/* binning ------------------------------------------------------------
 * project_to_basis sums (fftpower.py:595-666) over the local slab:
 *   xsum, musum            : (Nx+2)*(Nmu+2) doubles
 *   Nsum                   : (Nx+2)*(Nmu+2) doubles (integral values)
 *   ysum                   : nell * (Nx+2)*(Nmu+2) complex doubles
 * kedges (device, nx_edges doubles) are digitized by binary search on
 * k^2; muedges (device, nmu_edges doubles) likewise on mu; Hermitian
 * double-count weights along global axis 2 (weight 2 where kz > 0,
 * meshtools.py:188-215).  `ells` lists the multipole orders (first
 * entry must be 0, mirroring fftpower.py:585).  los is the
 * line-of-sight unit vector.  Outputs are accumulated (caller zeroes).
 * kedges must hold SQUARED bin edges (the digitize runs on |k|^2 / r^2,
 * fftpower.py:578,615).  real_field = 1 bins a configuration-space
 * RealField instead (FFTCorr): relative-position coordinates, all axes
 * full length, no Hermitian double-count (fftcorr.py:150-176).
 */
int nbk_bin_power_f64(const double* cplx, const int64_t nmesh[3],
                      const double box[3],
                      const int64_t dims[3], const int64_t off[3],
                      const int axis_map[3],
                      const double* kedges, int64_t nx_edges,
                      const double* muedges, int64_t nmu_edges,
                      const double los[3],
                      const int* ells, int nell,
                      int real_field,
                      double* xsum, double* musum, double* Nsum,
                      double* ysum, void* stream);

/* fused compensate + cross-power + binning: one streaming pass
 * computing comp1(c1) * conj(comp2(c2)) * volume per element (zero mode
 * cleared but still binned, fftpower.py:114-128) and accumulating the
 * project_to_basis sums — replaces the nbk_compensate_f64 (x2) +
 * nbk_power3d_f64 + nbk_bin_power_f64 sequence without materializing
 * p3d.  window1/window2: NBK_WINDOW_* or -1 for no compensation; c2 may
 * equal c1 (auto power) or be NULL (alias of c1).  The compensation
 * factors are bit-identical to nbk_compensate_f64's. */
int nbk_power_bin_f64(const double* c1, const double* c2, double volume,
                      int window1, int interlaced1,
                      int window2, int interlaced2,
                      int clear_zero_mode,
                      const int64_t nmesh[3], const double box[3],
                      const int64_t dims[3], const int64_t off[3],
                      const int axis_map[3],
                      const double* kedges, int64_t nx_edges,
                      const double* muedges, int64_t nmu_edges,
                      const double los[3],
                      const int* ells, int nell,
                      double* xsum, double* musum, double* Nsum,
                      double* ysum, void* stream);

/* fused x-pass FFT + compensate + auto-power + binning: consumes the
 * PRE-x-pass complex field (z and y axes already transformed, pencil
 * transpose already applied when distributed: element (j, c) of the
 * x-line through flattened local (y, zh) column c lives at
 * data[j * n_inner + c]), runs the final strided x FFT per line in LDS
 * and feeds the results straight into the project_to_basis sums — the
 * finished complex field is never written to HBM and columns wholly
 * beyond the last k-edge are skipped before their loads.  Equivalent to
 * nbk_fft_c_strided(axis 0) + nbk_power_bin_f64(c1 == c2) with
 * clear_zero semantics; bin assignment is bit-identical, the x-FFT
 * element values are bit-identical to the unfused pass.  kedges are
 * SQUARED k edges (as in nbk_bin_power_f64); out_sums is the contiguous
 * [xsum|musum|Nsum|ysum] block of (nx_edges+1)*(nmu_edges+1) doubles
 * each (ysum: nell planar re/im pairs).  nmesh[0] must be a power of
 * two, at least 8 and at most 2048 (1024 with data2, which doubles the
 * tile): the narrowest FFT tile (32 B per x point and field) and the
 * n0-entry tables of a longer line cannot fit the 160 KiB LDS beside any
 * histogram, so larger sizes return NBK_ERR_UNSUPPORTED.  So does any
 * size whose histograms + edges + tables + narrowest tile exceed the
 * 160 KiB less the 4 KiB reserved for the kernel's static arrays; nothing
 * is launched and out_sums is left untouched (callers fall back to the
 * unfused sequence).  At most 8 multipoles (NBK_ERR_ARG beyond). */
/* data2: NULL for a plain auto power; for an INTERLACED mesh the
 * half-cell-shifted paint's pre-x-pass field — both tiles are FFT'd
 * and combined as c = a/2 + b/2 exp(i k.H/2) before compensation and
 * binning.  In that mode the self-conjugate z planes (iz = 0 and, for
 * even n2, the Nyquist plane) are SKIPPED — their Hermitian projection
 * couples columns, so the caller handles those two planes with the
 * standalone kernels and the same out_sums buffer (all the binning
 * entry points accumulate). */
/* dig_hints = {k_lo, k_invd, mu_lo, mu_invd}: the uniform edge-grid
 * parameters (kedges = arange(k_lo, ., 1/k_invd), muedges =
 * linspace(mu_lo, ., 1/mu_invd)) used only as digitize STARTING
 * GUESSES — assignment is corrected against the exact edge arrays, so
 * it stays bit-identical to numpy.digitize. */
int nbk_fft_x_bin_f64(const double* data, const double* data2,
                      const int64_t nmesh[3],
                      int64_t n_inner, int64_t y_off,
                      const double box[3],
                      int window1, int interlaced1,
                      int clear_zero, double volume,
                      const double* kedges, int64_t nx_edges,
                      const double* muedges, int64_t nmu_edges,
                      const double dig_hints[4],
                      const double los[3],
                      const int* ells, int nell,
                      double* out_sums, void* stream);

/* pair counting --------------------------------------------------------
 * Replaces Corrfunc.theory.DD / DDsmu / DDrppi as called from
 * nbodykit/algorithms/pair_counters/corrfunc/theory.py (the compute core
 * of SimulationBoxPairCount): a cell-list pair counter in f64 with no
 * global atomics.
 *
 * Cell grid: cell (cx, cy, cz) of a particle is
 * clamp(floor((p - origin) * inv_cell), 0, ncell - 1) per axis, flattened
 * as (cx * ncell[1] + cy) * ncell[2] + cz; the caller picks a cell side
 * >= the largest 3-D separation counted, and at most
 * ncell[0]*ncell[1]*ncell[2] <= 40960 cells (one LDS histogram).
 *
 * Cell sort (the count-matrix scheme of nbk_xsort_*, with its n / chunk
 * requirements): with nchunks = ceil(n / chunk),
 *   - nbk_pairs_cell_count_f64 writes one ncells-wide histogram row per
 *     chunk into `mat` (nchunks x ncells, int32);
 *   - nbk_scan_matrix_i32(mat, nchunks, ncells, ...) turns it into the
 *     cursor seeds `bases` and the cell-start table bucket_bases
 *     (ncells + 1, [ncells] = n);
 *   - nbk_pairs_cell_scatter_f64 places the (n, 3) row-major positions
 *     and the weights into SoA pos_out = x[n] y[n] z[n] and w_out[n],
 *     ordered by cell (order within a cell is arbitrary).
 */
int nbk_pairs_cell_count_f64(const double* pos_aos, int64_t n, int chunk,
                             const double origin[3],
                             const double inv_cell[3], const int ncell[3],
                             int* mat, void* stream);
int nbk_pairs_cell_scatter_f64(const double* pos_aos, const double* weight,
                               int64_t n, int chunk, const double origin[3],
                               const double inv_cell[3], const int ncell[3],
                               const int* bases, double* pos_out,
                               double* w_out, void* stream);

/* single-pass bin capacity of nbk_pairs_count_f64: nb0 * (j1 - j0) may
 * not exceed it (three 8-byte LDS histograms per bin, 96 KiB) */
#define NBK_PAIRS_MAX_BINS 4096
int nbk_pairs_max_bins(void);

/* Count the ordered pairs (i in catalogue 1, j in catalogue 2) of two
 * cell-sorted SoA catalogues on the same cell grid.
 *   mode 0 (DD):     bins of r;        q = (dx^2 + dy^2) + dz^2
 *   mode 1 (DDsmu):  bins of (r, mu);  mu = |dz| / sqrt(q)
 *   mode 2 (DDrppi): bins of (rp, pi); q = dx^2 + dy^2, pi = |dz|
 * with d = (p1 - p2) - s * box per axis, s the periodic image (-1, 0, 1)
 * of the neighbour cell; periodic = 0 visits in-range neighbours only.
 * First-dimension bin k holds edges0_sq[k] <= q < edges0_sq[k+1]
 * (edges0_sq: device, nb0 + 1 SQUARED edges); second-dimension bin j
 * holds edges1[j] <= v < edges1[j+1] (device, nb1 + 1 edges; nb1 = 1 and
 * edges1 ignored in mode 0), the last mu bin closed at its upper edge.
 * A pair at zero separation (q = 0, reachable when edges0_sq[0] = 0) has
 * no mu and is dropped in mode 1, whatever the slice; modes 0 and 2 count
 * it (pi = 0).
 * Only second-dimension bins j0 <= j < j1 are counted by this call —
 * requests above NBK_PAIRS_MAX_BINS run as several calls over disjoint
 * slices.  autocorr = 1 (both sides the SAME arrays) skips the pairs
 * whose two sorted indices are equal; both orderings are counted.
 * The grid is `nblocks` persistent blocks striding over the cells;
 * `partials` is scratch of 3 * nblocks * nb0 * (j1 - j0) 8-byte words
 * (per-block histograms, plain stores), summed in block order into
 *   npairs[nb0 * nb1] (int64), wsum (sum of w1 * w2), xsum (sum of r or
 *   rp) at columns [j0, j1) — the other columns are left untouched.
 * Integer counts are bitwise reproducible; the float sums are
 * reproducible up to summation order. */
int nbk_pairs_count_f64(const double* pos1, const double* w1,
                        const int* start1, int64_t n1,
                        const double* pos2, const double* w2,
                        const int* start2, int64_t n2,
                        int autocorr, const int ncell[3],
                        const double box[3], int periodic,
                        int mode, const double* edges0_sq, int nb0,
                        const double* edges1, int nb1, int j0, int j1,
                        int nblocks, void* partials,
                        int64_t* npairs, double* wsum, double* xsum,
                        void* stream);

/* The same count for a sky catalogue seen from the origin (the compute
 * core of SurveyDataPairCount): the line of sight of a pair is its
 * midpoint direction.  The grid is never periodic.  With d = p1 - p2,
 * l = p1 + p2, s2 = (dx^2 + dy^2) + dz^2, l2 = (lx^2 + ly^2) + lz^2 and
 * dl = (dx lx + dy ly) + dz lz:
 *   mode 3: bins of (s, mu);   q = s2, mu = |dl| / sqrt(l2 * s2); the last
 *           mu bin takes every mu >= edges1[nb1] (rounding can give
 *           1 + 1 ulp); a NaN mu (l2 = 0 or s2 = 0) is dropped
 *   mode 4: bins of (rp, pi);  pi = sqrt((dl * dl) / l2), q = s2 - pi^2;
 *           pi >= edges1[nb1], l2 = 0 and q < edges0_sq[0] are dropped
 *   mode 5: bins of the angle between unit vectors; q = s2 (the squared
 *           chord, edges0_sq = (2 sin(theta / 2))^2), nb1 = 1, and xsum
 *           sums 2 asin(min(1, sqrt(q) / 2)) * (180 / pi), in degrees
 * Every other argument, the slices, `partials` and the outputs are those
 * of nbk_pairs_count_f64, whose modes 0-2 this entry point rejects (and
 * which rejects 3-5). */
int nbk_pairs_count_sky_f64(const double* pos1, const double* w1,
                            const int* start1, int64_t n1,
                            const double* pos2, const double* w2,
                            const int* start2, int64_t n2,
                            int autocorr, const int ncell[3],
                            int mode, const double* edges0_sq, int nb0,
                            const double* edges1, int nb1, int j0, int j1,
                            int nblocks, void* partials,
                            int64_t* npairs, double* wsum, double* xsum,
                            void* stream);

/* ---- three-point correlation function ------------------------------
 * Multipoles zeta_l(r1, r2) of the isotropic 3PCF of ONE cell-sorted
 * catalogue with itself (the compute core of SimulationBox3PCF and
 * SurveyData3PCF; reference nbodykit/algorithms/threeptcf.py): for every
 * primary i and radial bin b
 *   a_lm(b) = sum_j w_j Y_lm(d_ij / r_ij),  edges[b] < r_ij <= edges[b+1],
 *   zeta_l(b1, b2) = 1 / (4 pi) sum_i w_i sum_{m=0..l} c_m
 *                    Re[a_lm(b1) conj(a_lm(b2))],  c_0 = 1, c_m = 2,
 * with orthonormal Y_lm, d = (p_j - p_i) + s * box per axis (s the periodic
 * image of the neighbour cell, as in nbk_pairs_count_f64; `box` is not
 * read when periodic = 0) and r^2 = (dx^2 + dy^2) + dz^2 compared with
 * edges_sq (device, nbins + 1 SQUARED edges): bins are OPEN below and
 * CLOSED above, the opposite of the pair counter, and a pair at r = 0 (the
 * point itself, a duplicate) is in no bin.  pos / w / start / ncell are the
 * output and grid of nbk_pairs_cell_*, the cell side >= the largest edge.
 *
 * Capacity: lmax <= nbk_3pcf_max_ell() = 15 and nbins <=
 * nbk_3pcf_max_bins(lmax) (64 * nbins * (lmax + 1)(lmax + 2) / 2 bytes of
 * LDS per wave; 0 for an lmax out of range); anything larger returns
 * NBK_ERR_ARG before any launch.  The grid is `nblocks` persistent blocks;
 * `partials` is scratch of nblocks * (lmax + 1) * nbins * (nbins + 1) / 2
 * doubles (per-block sums, plain stores) that a second kernel adds in block
 * order into zeta[(lmax + 1) * nbins * nbins], index (l * nbins + b1) *
 * nbins + b2, all l <= lmax.  No atomics: the same sorted input and the
 * same nblocks give the same bits. */
int nbk_3pcf_max_ell(void);
int nbk_3pcf_max_bins(int lmax);
int nbk_3pcf_zeta_f64(const double* pos, const double* w, const int* start,
                      int64_t n, const int ncell[3], const double box[3],
                      int periodic, const double* edges_sq, int nbins,
                      int lmax, int nblocks, double* partials, double* zeta,
                      void* stream);

/* friends-of-friends -------------------------------------------------
 * The replacement for kdcount.cluster.fof under
 * nbodykit/algorithms/fof.py: two particles are friends iff
 *   r2 = (dx*dx + dy*dy) + dz*dz <= ll_sq,  d = (p_i - p_j) - s * box
 * per axis (s the periodic image of the neighbour cell, as in
 * nbk_pairs_count_f64; zero separation links), and a group is a connected
 * component of that relation.  f64 throughout.
 *
 * Cell grid, two levels: ncell[a] = ncoarse[a] * fine[a] cells per axis
 * with ncoarse[0]*ncoarse[1]*ncoarse[2] <= 40960 and
 * fine[0]*fine[1]*fine[2] <= 40960 (one LDS histogram each) and fewer
 * than 2^31 cells in all.  The fine cell of a particle is
 * c[a] = clamp(floor((p - origin) * inv_cell), 0, ncell - 1) per axis; its
 * coarse cell is the integer c[a] / fine[a] and its sub-cell c[a] % fine[a]
 * (never a second floor).  Cells are numbered BLOCK-MAJOR:
 *   cell = coarse_id * nfine + sub_id,  nfine = fine[0]*fine[1]*fine[2],
 *   coarse_id = ((c[0]/fine[0]) * ncoarse[1] + c[1]/fine[1]) * ncoarse[2]
 *               + c[2]/fine[2],
 *   sub_id = ((c[0]%fine[0]) * fine[1] + c[1]%fine[1]) * fine[2]
 *            + c[2]%fine[2].
 * The caller picks a cell side >= the linking length.
 *
 * Coarse sort (the count-matrix scheme of nbk_xsort_*, with its n / chunk
 * requirements, keyed by coarse_id): nbk_fof_cell_count_f64 ->
 * nbk_scan_matrix_i32(mat, nchunks, ncoarse_all, ...) ->
 * nbk_fof_cell_scatter_f64, which places the (n, 3) row-major positions
 * and the f64 column `index` (the original particle index, exact in a
 * double) into SoA pos_out = x[n] y[n] z[n] and index_out[n]; the scan's
 * bucket_bases (ncoarse_all + 1) is the coarse start table. */
int nbk_fof_cell_count_f64(const double* pos_aos, int64_t n, int chunk,
                           const double origin[3], const double inv_cell[3],
                           const int ncoarse[3], const int fine[3],
                           int* mat, void* stream);
int nbk_fof_cell_scatter_f64(const double* pos_aos, const double* index,
                             int64_t n, int chunk, const double origin[3],
                             const double inv_cell[3], const int ncoarse[3],
                             const int fine[3], const int* bases,
                             double* pos_out, double* index_out,
                             void* stream);
/* Fine pass: one block per coarse cell over the coarse-sorted SoA planes
 * and coarse_start.  Writes the cell-sorted SoA pos_out, the int32
 * original index index_out[n] and the fine start table
 * fine_start[ncells + 1] (exclusive, [ncells] = n), all in block-major cell
 * order; order inside a cell is arbitrary.  No global atomics; correct
 * for a coarse cell of any occupancy from 0 to n.  n = 0 only zeroes
 * fine_start. */
int nbk_fof_fine_sort_f64(const double* pos_soa, const double* index,
                          int64_t n, const double origin[3],
                          const double inv_cell[3], const int ncoarse[3],
                          const int fine[3], const int* coarse_start,
                          double* pos_out, int* index_out, int* fine_start,
                          void* stream);
/* Link: unites every pair of friends in `parent` (n int32, the identity
 * on entry; on return a forest with parent[k] <= k whose trees are the
 * groups).  One thread per sorted particle tests the lower sorted indices
 * of its <= 27 neighbour (cell, shift)s, so each unordered pair is tested
 * once per image; with fewer than 3 cells on a periodic axis a pair may
 * be in range under two shifts, and the second union is a no-op.  Unions
 * hook the larger root under the smaller with an agent-scope 32-bit
 * compare-and-swap; all other accesses to `parent` are agent-scope relaxed
 * atomics.  No fences, no grid barrier, no waiting: every loop is bounded
 * by n even on a corrupt array.  *err (device int, zeroed by the caller)
 * is set when a parent is not below its child; box is not read when
 * periodic = 0. */
int nbk_fof_link_f64(const double* pos_soa, const int* fine_start, int64_t n,
                     const int ncoarse[3], const int fine[3],
                     const double box[3], int periodic, double ll_sq,
                     int* parent, int* err, void* stream);
/* Flatten (a separate launch): root[i] = the root of i in `parent`, into
 * a separate array, with the same bounded walk and the same *err word.
 * Waits for the stream, reads *err back and returns NBK_ERR_ARG when it
 * is set (by this pass or by the link before it); root[i] = -1 where the
 * walk gave up. */
int nbk_fof_flatten_i32(const int* parent, int64_t n, int* root, int* err,
                        void* stream);

/* k-th nearest neighbour ------------------------------------------------
 * The replacement for cKDTree.query under nbodykit/algorithms/kdtree.py
 * (KDDensity).  nbk_knn_max_k() is the largest k, 16.
 *
 * Input: the output of nbk_fof_fine_sort_f64, unchanged: the cell-sorted SoA
 * planes pos_soa[3n], sindex[n] (the input index of every sorted slot) and
 * fine_start[ncells + 1], in the block-major cell order of the grid
 * (origin, inv_cell, ncoarse, fine) above.  inv_cell[a] = 0 is a flat axis
 * (every particle in cell 0 of it).
 *
 * Output, in INPUT order: for the particle in sorted slot i,
 * r2_out[sindex[i]] is the squared distance to its k-th nearest OTHER
 * particle (every sorted slot j != i; coincident points are neighbours at
 * distance 0) and index_out[sindex[i]] that particle's input index.  With
 * fewer than k other particles: +inf and -1.  A slot whose sindex[i] lies
 * outside [0, n) is skipped, never stored through.
 *
 * Distance: per axis d = x_i - x_j and d2 = d*d, or, periodic, the smallest
 * of d*d, (d - L)*(d - L), (d + L)*(d + L) (positions wrapped into [0, L)
 * by the caller; box is not read when periodic = 0);
 * r2 = (dx2 + dy2) + dz2, every operation rounded separately.  Candidates
 * are ordered by the pair (r2, input index), so both outputs are bitwise
 * reproducible whatever the order inside a cell, ties included.
 *
 * Search: one thread per sorted particle visits the cells around its own
 * ring by ring.  Ring s covers, per axis of n_a cells around cell c, the
 * offsets [-min(s, (n_a-1)/2), min(s, n_a/2)] when periodic and
 * [max(-s, -c), min(s, n_a-1-c)] otherwise, less the box of ring s - 1:
 * no cell is visited twice.  It stops when every axis is covered, or when
 * the k-th best r2 <= b*b, b the smallest distance from the particle to a
 * face of the visited box on an axis not yet covered (faces on the edge of a
 * non-periodic domain excluded), less 1e-9 cell sides, clamped at 0.  A
 * cell of a ring whose nearest point, with the same guard, lies beyond the
 * k-th best so far is not read.  Every
 * loop bound is a function of (s, n_a, c); cell ranges are clamped to
 * [0, n); no atomics, no waiting.  At most max n_a rings, so a thread reads
 * at most ncells start-table entries.
 *
 * 1 <= k <= 16, 0 <= n < 2^31, a grid as above, finite origin and
 * inv_cell >= 0, and box > 0 when periodic: anything else returns
 * NBK_ERR_ARG with the outputs untouched.  n = 0 launches nothing. */
int nbk_knn_max_k(void);
int nbk_knn_f64(const double* pos_soa, const int* fine_start,
                const int* sindex, int64_t n, const double origin[3],
                const double inv_cell[3], const int ncoarse[3],
                const int fine[3], const double box[3], int periodic, int k,
                double* r2_out, int* index_out, void* stream);

/* cylindrical groups ----------------------------------------------------
 * The replacement for the pair enumeration and the pandas groupby under
 * nbodykit/algorithms/cgm.py (CylindricalGroups).
 *
 * Input: the output of nbk_fof_fine_sort_f64, unchanged (pos_soa[3n] and
 * fine_start[ncells + 1] on the grid (ncoarse, fine) of the friends-of-
 * friends block above, with its limits), and prio[n], the priority of every
 * sorted slot: a permutation of 0..n-1, a higher value is a higher
 * priority.  The caller guarantees distinct values; they are not checked.
 * Everything written is in sorted-slot order.
 *
 * Neighbours: slots i and j are neighbours iff, with d = p_i - p_j per axis
 * and, periodic, `if (d > box/2) d -= box; if (d <= -box/2) d += box;`
 * (positions wrapped into [0, box) by the caller; box is not read when
 * periodic = 0),
 *   los_mode 0: rlos = (dx*los[0] + dy*los[1]) + dz*los[2],
 *               rlos2 = rlos*rlos
 *   los_mode 1 (observer at the origin; los is not read):
 *               c = 0.5*(p_i + p_j), dot = (dx*cx + dy*cy) + dz*cz,
 *               rlos2 = (dot*dot) / ((cx*cx + cy*cy) + cz*cz)
 *   rsky2 = |((dx*dx + dy*dy) + dz*dz) - rlos2|
 *   rsky2 <= rperp2 && rlos2 <= rpar2,
 * every operation rounded separately; 0/0 is NaN and compares false (two
 * objects placed symmetrically about the observer are not neighbours).
 * The pair is tested from p_i - p_j under this wrap, never under a per-cell
 * image shift.  The caller picks cells whose side on every axis covers the
 * cylinder, so that a neighbour lies at most one cell away.
 *
 * Walk, common to the three calls: one thread per sorted slot visits every
 * neighbour cell once: per axis of n_a cells the offsets
 * [-min(1, (n_a-1)/2), min(1, n_a/2)] when periodic, [-1, 1] clamped to the
 * grid otherwise.  Loop bounds are functions of the start table, clamped to
 * [0, n]; no global read-modify-write, no waiting.
 *
 * nbk_cgm_resolve_f64: one sweep of the greedy selection over state[n]
 * (zeroed by the caller; 0 undecided, 1 central, 2 satellite).  An
 * undecided slot becomes a satellite if a neighbour of higher priority is a
 * central, else a central if no neighbour of higher priority is undecided,
 * else it stays.  `state` is read and written with agent-scope relaxed
 * atomic loads and stores; a stale "undecided" only delays a decision, so
 * the fixpoint, reached after at most n sweeps, is the sequential
 * highest-priority-first selection whatever the thread order.  flags[2]
 * (device ints, zeroed by the caller): flags[0] = 1 when the sweep decided
 * something, flags[1] = 1 when a slot is still undecided after it, both
 * plain stores.  A decided slot costs one load; a sweep over a final state
 * writes nothing.
 *
 * nbk_cgm_host_f64 (state final): host[i] = i for a central, the slot of
 * the highest-priority central among its neighbours for a satellite.
 *
 * nbk_cgm_count_f64: nsat[i] = the number of slots j != i in the neighbour
 * cells of a central i with host[j] == i (no geometry, no atomics); 0 for a
 * satellite.
 *
 * rperp2, rpar2 finite and >= 0, los_mode 0 or 1, los finite in mode 0,
 * box > 0 and finite when periodic, 0 <= n < 2^31 and a grid within the
 * limits above: anything else returns NBK_ERR_ARG with the outputs
 * untouched.  n = 0 launches nothing. */
int nbk_cgm_resolve_f64(const double* pos_soa, const int* fine_start,
                        const int* prio, int64_t n, const int ncoarse[3],
                        const int fine[3], const double box[3], int periodic,
                        int los_mode, const double los[3], double rperp2,
                        double rpar2, int* state, int* flags, void* stream);
int nbk_cgm_host_f64(const double* pos_soa, const int* fine_start,
                     const int* prio, int64_t n, const int ncoarse[3],
                     const int fine[3], const double box[3], int periodic,
                     int los_mode, const double los[3], double rperp2,
                     double rpar2, const int* state, int* host,
                     void* stream);
int nbk_cgm_count_f64(const double* pos_soa, const int* fine_start,
                      const int* prio, int64_t n, const int ncoarse[3],
                      const int fine[3], const double box[3], int periodic,
                      int los_mode, const double los[3], double rperp2,
                      double rpar2, const int* state, const int* host,
                      int* nsat, void* stream);

/* fibre assignment -------------------------------------------------------
 * The replacement for the loop over collision groups under
 * nbodykit/algorithms/fibercollisions.py (FiberCollisions).
 * nbk_fibers_max_group() is the largest group, 1024 members.
 *
 * Input: pos_aos[3n] (n rows of x, y, z), read only through midx;
 * midx[nmember], the input indices of the members of every group, group
 * after group and ascending inside a group; gstart[ngroup + 1], the start
 * table into midx.  collided[nmember] and neighbor[nmember] are written in
 * member order.  nbig is the caller's promise that no group at index >= nbig
 * has more than 64 members.
 *
 * Members a and b collide iff, with d = p_a - p_b per axis,
 * (dx*dx + dy*dy) + dz*dz <= r2, every operation rounded separately (the
 * predicate of nbk_fof_link_f64).  Inside one group all members start
 * active; per round, among the active members, n_coll[j] counts those
 * colliding with j and n_other[j] sums n_coll over them.  When every n_coll
 * is 0 the round loop ends.  Otherwise one member is marked collided and
 * deactivated: largest n_coll, then smallest n_other, then smallest key,
 * then smallest position inside the group, with, modulo 2^64 and i the
 * input index,
 *   z = seed + (i + 1) * 0x9E3779B97F4A7C15
 *   z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *   z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *   key = z ^ (z >> 31).
 * collided is 1 for a marked member and 0 otherwise.  neighbor is, for a
 * marked member, the input index of the unmarked member of its group with the
 * smallest squared distance (ties to the earlier member), -1 otherwise.  A
 * group is not assumed connected; one without a collision, and a group of
 * one member, come out all 0 and -1.
 *
 * Two launches: one block per group [0, nbig) for the groups of more than 64
 * members there, and one wave per group, four per block, for every group of
 * up to 64 members.  No global atomics, nothing shared between blocks; start
 * table entries are clamped to [0, nmember] and every loop is bounded by the
 * clamped size.  *err (device int, zeroed by the caller) is set, and the
 * group's outputs are left untouched, for a group above the cap, a group at
 * or beyond nbig with more than 64 members, and a member index outside
 * [0, n).
 *
 * r2 finite and >= 0, 0 <= n, nmember, ngroup < 2^31, 0 <= nbig <= ngroup and
 * no null pointer with a non-zero count: anything else returns NBK_ERR_ARG
 * with nothing written.  ngroup = 0 launches nothing. */
int nbk_fibers_max_group(void);
int nbk_fibers_assign_f64(const double* pos_aos, int64_t n, const int* midx,
                          int64_t nmember, const int* gstart, int64_t ngroup,
                          int64_t nbig, double r2, uint64_t seed,
                          int* collided, int* neighbor, int* err,
                          void* stream);

/* small helpers ------------------------------------------------------ */
/* out[i] += a[i]  (f64, n elements) */
int nbk_axpy_f64(double* out, const double* a, double alpha, int64_t n,
                 void* stream);
/* mesh *= alpha  or mesh[:] = alpha when set_value != 0 */
int nbk_scale_f64(double* mesh, double alpha, int set_value, int64_t n,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NBK_HIP_H */
