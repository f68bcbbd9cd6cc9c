// Cell-list pair counting (SimulationBoxPairCount): the replacement for
// Corrfunc.theory.DD / DDsmu / DDrppi, f64 throughout.
//
// Pipeline (all launches on the caller's stream, NO global atomics):
//  1. nbk_pairs_cell_count_f64 / nbk_scan_matrix_i32 /
//     nbk_pairs_cell_scatter_f64: the count-matrix sort of
//     nbk_countsort.h with the cell id as its key, into SoA
//     x[n] y[n] z[n] + w[n]; the scan's bucket_bases[ncells + 1] is the
//     cell-start table.
//  2. nbk_pairs_count_f64: a persistent grid strides over
//     (first-catalogue cell, split) work items.  A block keeps up to
//     blockDim first-catalogue particles in registers, walks the <= 27
//     neighbour cells of the second catalogue, stages 256-particle tiles
//     in LDS and bins every candidate into per-block LDS histograms
//     (64-bit count, sum w1 w2, sum r) — then stores its partials with
//     plain vector stores; a second kernel sums the partial rows in
//     block order.
//
// Neighbour walk: per axis the offsets -1, 0, +1 map to
// (cell, shift) = (c + d - s n, s) with s = floor((c + d) / n) for a
// periodic axis, and are dropped when out of range otherwise.  The three
// (cell, shift) pairs of an axis are distinct for EVERY n >= 1: with
// n = 2 the offsets -1 and +1 alias the same cell but carry different
// shifts (0 and -+1), with n = 1 all three alias cell 0 with shifts
// -1, 0, +1.  A pair can be in range (|d - s L| < rmax <= L/2) under at
// most one shift, so nothing is counted twice and nothing is missed.
// The shift is applied as (x1 - x2) - s L, which for in-range pairs is
// the same two roundings as the minimum-image expression
// d = x1 - x2; d -= L if d > L/2; d += L if d < -L/2.
//
// Binning is on squared separations against squared first-dimension
// edges (lower closed, upper open) and on mu = |dz| / r or pi = |dz|
// against the published second-dimension edges; -ffp-contract=off keeps
// every operation separately rounded, like numpy.  A pair at r = 0
// (reachable when edges[0] = 0) has no mu and is dropped in mode 1; modes
// 0 and 2 count it (q = 0, pi = 0).
#include "nbk_countsort.h"
#include "nbk_cells.h"

namespace {

// tile of second-catalogue particles staged in LDS
constexpr int PAIRS_TILE = 256;
constexpr int PAIRS_THREADS = 256;

// the cell sort's key: the clamped cell id
struct PairsCellKey {
    typedef int index_t;
    static constexpr bool two_keys = false;
    double origin[3];
    double inv_cell[3];
    int ncell[3];

    __device__ __forceinline__ int operator()(double x, double y,
                                              double z) const {
        const int cx = cell_axis(x, origin[0], inv_cell[0], ncell[0]);
        const int cy = cell_axis(y, origin[1], inv_cell[1], ncell[1]);
        const int cz = cell_axis(z, origin[2], inv_cell[2], ncell[2]);
        return (cx * ncell[1] + cy) * ncell[2] + cz;
    }
};

// ---- pair count --------------------------------------------------------

// index k of the bin with e[k] <= v < e[k + 1] over n + 1 ascending
// edges; the caller has already checked e[0] <= v < e[n]
__device__ __forceinline__ int bin_search(const double* e, int n, double v) {
    int lo = 0, hi = n;             // invariant: e[lo] <= v < e[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v >= e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

struct PairsArgs {
    const double* p1;  const double* w1;  const int* start1;  int64_t n1;
    const double* p2;  const double* w2;  const int* start2;  int64_t n2;
    int ncell[3];
    int periodic;
    double box[3];
    int autocorr;
    int nb0;            // first-dimension bins
    int nb1;            // second-dimension bins (1 in 1d mode)
    int j0, j1;         // slice [j0, j1) of the second dimension
    int ncopy;          // histogram copies per block (waves share mod)
    int split;          // work items per first-catalogue cell
    const double* e0sq; // nb0 + 1 squared first-dimension edges
    const double* e1;   // nb1 + 1 second-dimension edges (modes 1-4)
                        // — only the slice [j0, j1] is staged in LDS
    unsigned long long* part_n;   // [gridDim.x * nb] partials
    double* part_w;
    double* part_x;
};

// modes without a second dimension
__host__ __device__ constexpr bool mode_is_1d(int mode) {
    return mode == 0 || mode == 5;
}

// MODE 0: 1d (r), 1: 2d (r, mu), 2: projected (rp, pi) along the last
// axis; 3: (s, mu), 4: (rp, pi) along the pair's midpoint direction,
// 5: angle between unit vectors (sky modes, never periodic)
template <int MODE>
__global__ __launch_bounds__(PAIRS_THREADS)
void kpairs_count(PairsArgs a)
{
    extern __shared__ __align__(16) double lds_f64[];
    const int ns = a.j1 - a.j0;         // second-dimension bins this pass
    const int nb = a.nb0 * ns;          // bins this pass
    // layout: tile (xy, zw) | e0sq | e1 slice | count | wsum | xsum
    double2* txy = reinterpret_cast<double2*>(lds_f64);
    double2* tzw = txy + PAIRS_TILE;
    double* e0sq = reinterpret_cast<double*>(tzw + PAIRS_TILE);
    double* e1 = e0sq + (a.nb0 + 1);
    unsigned long long* hn = reinterpret_cast<unsigned long long*>(
        e1 + (mode_is_1d(MODE) ? 0 : ns + 1));
    double* hw = reinterpret_cast<double*>(hn + (size_t)a.ncopy * nb);
    double* hx = hw + (size_t)a.ncopy * nb;

    const int tid = threadIdx.x;
    for (int k = tid; k <= a.nb0; k += blockDim.x) e0sq[k] = a.e0sq[k];
    if (!mode_is_1d(MODE))
        for (int k = tid; k <= ns; k += blockDim.x) e1[k] = a.e1[a.j0 + k];
    for (int k = tid; k < a.ncopy * nb; k += blockDim.x) {
        hn[k] = 0ull;
        hw[k] = 0.0;
        hx[k] = 0.0;
    }
    __syncthreads();

    const double q_lo = e0sq[0], q_hi = e0sq[a.nb0];
    // this pass's slice [v_lo, v_hi) of the second dimension; the last
    // mu bin is closed above (mu <= 1 along an axis; a midpoint mu that
    // rounding pushes past 1 belongs to it too)
    const double v_lo = mode_is_1d(MODE) ? 0.0 : e1[0];
    const double v_hi = mode_is_1d(MODE) ? 0.0 : e1[ns];
    const bool closed = (MODE == 1 || MODE == 3) && a.j1 == a.nb1;
    // mode 4 rejects on s^2 before it knows pi: rp^2 = fl(s^2 - pi^2)
    // >= q_lo needs s^2 >= q_lo (pi^2 >= 0 and s^2 is a double), and
    // rp^2 < q_hi with pi < pimax needs s^2 < q_hi + pimax^2 up to a
    // few roundings, which the factor 1 + 2^-40 covers many times over
    double s_hi = q_hi;
    if (MODE == 4) {
        const double pimax = a.e1[a.nb1];
        s_hi = (q_hi + pimax * pimax) * (1.0 + 0x1p-40);
    }
    const int copy = ((tid >> 6) % a.ncopy) * nb;
    const int ncy = a.ncell[1], ncz = a.ncell[2];
    const int ncells = a.ncell[0] * ncy * ncz;
    const int64_t nitems = (int64_t)ncells * a.split;

    const double* x1 = a.p1;
    const double* y1 = a.p1 + a.n1;
    const double* z1 = a.p1 + 2 * a.n1;
    const double* x2 = a.p2;
    const double* y2 = a.p2 + a.n2;
    const double* z2 = a.p2 + 2 * a.n2;

    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c1 = (int)(item / a.split);
        const int sp = (int)(item - (int64_t)c1 * a.split);
        const int b1 = a.start1[c1], e1c = a.start1[c1 + 1];
        const int cz = c1 % ncz;
        const int cy = (c1 / ncz) % ncy;
        const int cx = c1 / (ncz * ncy);

        // every loop bound below is block-uniform: all threads reach
        // every barrier, lanes without a particle only skip the binning
        for (int ib = b1 + sp * PAIRS_THREADS; ib < e1c;
             ib += a.split * PAIRS_THREADS) {
            const int i = ib + tid;
            const bool have = i < e1c;
            const double xi = have ? x1[i] : 0.0;
            const double yi = have ? y1[i] : 0.0;
            const double zi = have ? z1[i] : 0.0;
            const double wi = have ? a.w1[i] : 0.0;

            for (int dxc = -1; dxc <= 1; dxc++) {
                int nx;  double sx;
                if (!neighbour_axis(cx, dxc, a.ncell[0], a.periodic,
                                    a.box[0], &nx, &sx)) continue;
                for (int dyc = -1; dyc <= 1; dyc++) {
                    int ny;  double sy;
                    if (!neighbour_axis(cy, dyc, ncy, a.periodic,
                                        a.box[1], &ny, &sy)) continue;
                    for (int dzc = -1; dzc <= 1; dzc++) {
                        int nz;  double sz;
                        if (!neighbour_axis(cz, dzc, ncz, a.periodic,
                                            a.box[2], &nz, &sz)) continue;
                        const int c2 = (nx * ncy + ny) * ncz + nz;
                        const int b2 = a.start2[c2];
                        const int e2 = a.start2[c2 + 1];

                        for (int t0 = b2; t0 < e2; t0 += PAIRS_TILE) {
                            const int nt = (e2 - t0 < PAIRS_TILE)
                                         ? e2 - t0 : PAIRS_TILE;
                            __syncthreads();    // previous tile consumed
                            for (int t = tid; t < nt; t += blockDim.x) {
                                txy[t] = make_double2(x2[t0 + t],
                                                      y2[t0 + t]);
                                tzw[t] = make_double2(z2[t0 + t],
                                                      a.w2[t0 + t]);
                            }
                            __syncthreads();
                            if (!have) continue;
                            for (int t = 0; t < nt; t++) {
                                const double2 pxy = txy[t];
                                const double2 pzw = tzw[t];
                                const double dx = (MODE >= 3)
                                    ? xi - pxy.x : (xi - pxy.x) - sx;
                                const double dy = (MODE >= 3)
                                    ? yi - pxy.y : (yi - pxy.y) - sy;
                                const double dz = (MODE >= 3)
                                    ? zi - pzw.x : (zi - pzw.x) - sz;
                                const double rp2 = dx * dx + dy * dy;
                                double q = (MODE == 2)
                                         ? rp2 : rp2 + dz * dz;
                                if (!(q >= q_lo && q < s_hi)) continue;
                                if (a.autocorr && t0 + t == i) continue;
                                double v = 0.0;
                                if (MODE == 3 || MODE == 4) {
                                    const double lx = xi + pxy.x;
                                    const double ly = yi + pxy.y;
                                    const double lz = zi + pzw.x;
                                    const double l2 = (lx * lx + ly * ly)
                                                    + lz * lz;
                                    const double dl = (dx * lx + dy * ly)
                                                    + dz * lz;
                                    if (MODE == 3) {
                                        v = fabs(dl) / sqrt(l2 * q);
                                    } else {
                                        // (NaN for l = 0: dropped here)
                                        const double pi2 = (dl * dl) / l2;
                                        v = sqrt(pi2);
                                        q = q - pi2;
                                        if (!(q >= q_lo && q < q_hi))
                                            continue;
                                    }
                                }
                                const double r = sqrt(q);
                                if (MODE == 1) v = fabs(dz) / r;
                                if (MODE == 2) v = fabs(dz);
                                int j = 0;
                                if (!mode_is_1d(MODE)) {
                                    // (also false for a NaN mu = 0/0: a
                                    // pair at r = 0, or p2 = -p1 in mode
                                    // 3, has no mu bin, in any pass)
                                    if (!(v >= v_lo)) continue;
                                    if (v < v_hi)
                                        j = bin_search(e1, ns, v);
                                    else if (closed)
                                        j = ns - 1;
                                    else
                                        continue;
                                }
                                // the accumulated first variable: r, rp
                                // or the angle of the chord in degrees
                                const double x = (MODE == 5)
                                    ? (2.0 * asin(fmin(1.0, 0.5 * r)))
                                      * (180.0 / M_PI)
                                    : r;
                                const int k = bin_search(e0sq, a.nb0, q);
                                const int h = copy + k * ns + j;
                                atomicAdd(&hn[h], 1ull);
                                atomicAdd(&hw[h], wi * pzw.y);
                                atomicAdd(&hx[h], x);
                            }
                        }
                    }
                }
            }
        }
    }

    __syncthreads();
    // fold the copies in a fixed order and store this block's partials
    for (int k = tid; k < nb; k += blockDim.x) {
        unsigned long long cn = 0ull;
        double cw = 0.0, cx_ = 0.0;
        for (int c = 0; c < a.ncopy; c++) {
            cn += hn[c * nb + k];
            cw += hw[c * nb + k];
            cx_ += hx[c * nb + k];
        }
        const size_t o = (size_t)blockIdx.x * nb + k;
        a.part_n[o] = cn;
        a.part_w[o] = cw;
        a.part_x[o] = cx_;
    }
}

// sums the [nblocks x nb] partial rows in block order into the
// (nb0, nb1) outputs at second-dimension offset j0
__global__ void kpairs_reduce(const unsigned long long* __restrict__ part_n,
                              const double* __restrict__ part_w,
                              const double* __restrict__ part_x,
                              int nblocks, int nb0, int nb1, int j0, int j1,
                              unsigned long long* __restrict__ out_n,
                              double* __restrict__ out_w,
                              double* __restrict__ out_x)
{
    const int ns = j1 - j0;
    const int nb = nb0 * ns;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    unsigned long long cn = 0ull;
    double cw = 0.0, cx = 0.0;
    for (int b = 0; b < nblocks; b++) {
        cn += part_n[(size_t)b * nb + k];
        cw += part_w[(size_t)b * nb + k];
        cx += part_x[(size_t)b * nb + k];
    }
    const int o = (k / ns) * nb1 + j0 + (k % ns);
    out_n[o] = cn;
    out_w[o] = cw;
    out_x[o] = cx;
}

// grid checks + key of nbk_pairs_cell_*; `who` names the entry point
int make_grid(const char* who, const double origin[3],
              const double inv_cell[3], const int ncell[3],
              PairsCellKey* g, int64_t* ncells)
{
    *ncells = 1;
    for (int i = 0; i < 3; i++) {
        if (ncell[i] < 1) {
            NBK_SET_ERR("%s: ncell[%d] = %d", who, i, ncell[i]);
            return NBK_ERR_ARG;
        }
        g->origin[i] = origin[i];
        g->inv_cell[i] = inv_cell[i];
        g->ncell[i] = ncell[i];
        *ncells *= ncell[i];
        if (*ncells > NBK_SORT_LDS_INTS) {
            NBK_SET_ERR("%s: more than %lld cells, the LDS histogram",
                        who, (long long)NBK_SORT_LDS_INTS);
            return NBK_ERR_ARG;
        }
    }
    return NBK_OK;
}

size_t count_lds_bytes(int mode, int nb0, int ns, int ncopy) {
    return (size_t)PAIRS_TILE * 2 * sizeof(double2)
         + (size_t)(nb0 + 1) * sizeof(double)
         + (mode_is_1d(mode) ? 0 : (size_t)(ns + 1) * sizeof(double))
         + (size_t)ncopy * nb0 * ns * 24;
}

template <int MODE>
void launch_count(const PairsArgs& a, int nblocks, size_t lds,
                  hipStream_t s) {
    raise_lds(reinterpret_cast<const void*>(&kpairs_count<MODE>), lds);
    hipLaunchKernelGGL(kpairs_count<MODE>, dim3((uint32_t)nblocks),
                       dim3(PAIRS_THREADS), lds, s, a);
}

// validation, LDS sizing, histogram copies, work split, count and reduce
// of both count entry points; `who` accepts modes [mode_lo, mode_hi]
int count_pairs(const char* who, int mode_lo, int mode_hi,
                const double* pos1, const double* w1, const int* start1,
                int64_t n1, const double* pos2, const double* w2,
                const int* start2, int64_t n2, int autocorr,
                const int ncell[3], const double box[3], int periodic,
                int mode, const double* edges0_sq, int nb0,
                const double* edges1, int nb1, int j0, int j1, int nblocks,
                void* partials, int64_t* npairs, double* wsum, double* xsum,
                void* stream)
{
    if (mode < mode_lo || mode > mode_hi || nb0 < 1 || nb1 < 1
        || (mode_is_1d(mode) && nb1 != 1) || j0 < 0 || j1 > nb1
        || j0 >= j1) {
        NBK_SET_ERR("%s: bad mode/bins (mode=%d nb0=%d nb1=%d slice "
                    "[%d, %d))", who, mode, nb0, nb1, j0, j1);
        return NBK_ERR_ARG;
    }
    if (edges0_sq == nullptr
        || (!mode_is_1d(mode) && edges1 == nullptr)) {
        NBK_SET_ERR("%s: mode %d without its bin edges", who, mode);
        return NBK_ERR_ARG;
    }
    const int64_t nb = (int64_t)nb0 * (j1 - j0);
    if (nb > NBK_PAIRS_MAX_BINS) {
        NBK_SET_ERR("%s: %lld bins in one pass exceed the capacity %d",
                    who, (long long)nb, NBK_PAIRS_MAX_BINS);
        return NBK_ERR_ARG;
    }
    if (n1 < 0 || n2 < 0 || n1 >= ((int64_t)1 << 31)
        || n2 >= ((int64_t)1 << 31) || nblocks < 1) {
        NBK_SET_ERR("%s: n1=%lld n2=%lld nblocks=%d", who, (long long)n1,
                    (long long)n2, nblocks);
        return NBK_ERR_ARG;
    }
    int64_t ncells = 1;
    for (int i = 0; i < 3; i++) {
        if (ncell[i] < 1) {
            NBK_SET_ERR("%s: ncell[%d] = %d", who, i, ncell[i]);
            return NBK_ERR_ARG;
        }
        ncells *= ncell[i];
    }
    if (ncells > NBK_SORT_LDS_INTS) {
        NBK_SET_ERR("%s: too many cells (%lld)", who, (long long)ncells);
        return NBK_ERR_ARG;
    }
    if (autocorr && (pos1 != pos2 || n1 != n2 || start1 != start2)) {
        NBK_SET_ERR("%s: autocorr needs identical sorted inputs", who);
        return NBK_ERR_ARG;
    }

    PairsArgs a;
    a.p1 = pos1;  a.w1 = w1;  a.start1 = start1;  a.n1 = n1;
    a.p2 = pos2;  a.w2 = w2;  a.start2 = start2;  a.n2 = n2;
    for (int i = 0; i < 3; i++) {
        a.ncell[i] = ncell[i];
        a.box[i] = box[i];
    }
    a.periodic = periodic;
    a.autocorr = autocorr;
    a.nb0 = nb0;
    a.nb1 = nb1;
    a.j0 = j0;
    a.j1 = j1;
    // one histogram copy per wave while the copies stay within 48 KiB
    // (so that two blocks stay resident per CU), fewer for more bins
    a.ncopy = (nb * 24 * 4 <= 48 * 1024) ? 4
            : (nb * 24 * 2 <= 48 * 1024) ? 2 : 1;
    // enough work items for the grid when there are few cells
    int64_t split = (4 * (int64_t)nblocks + ncells - 1) / ncells;
    a.split = (int)(split < 1 ? 1 : (split > 64 ? 64 : split));
    a.e0sq = edges0_sq;
    a.e1 = edges1;
    a.part_n = reinterpret_cast<unsigned long long*>(partials);
    a.part_w = reinterpret_cast<double*>(partials) + (size_t)nblocks * nb;
    a.part_x = a.part_w + (size_t)nblocks * nb;

    hipStream_t s = (hipStream_t)stream;
    const size_t lds = count_lds_bytes(mode, nb0, j1 - j0, a.ncopy);
    switch (mode) {
    case 0: launch_count<0>(a, nblocks, lds, s); break;
    case 1: launch_count<1>(a, nblocks, lds, s); break;
    case 2: launch_count<2>(a, nblocks, lds, s); break;
    case 3: launch_count<3>(a, nblocks, lds, s); break;
    case 4: launch_count<4>(a, nblocks, lds, s); break;
    default: launch_count<5>(a, nblocks, lds, s); break;
    }
    NBK_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(kpairs_reduce, dim3((uint32_t)((nb + 255) / 256)),
                       dim3(256), 0, s, a.part_n, a.part_w, a.part_x,
                       nblocks, nb0, nb1, j0, j1,
                       reinterpret_cast<unsigned long long*>(npairs),
                       wsum, xsum);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

}  // namespace

extern "C" int nbk_pairs_cell_count_f64(const double* pos_aos, int64_t n,
                                        int chunk, const double origin[3],
                                        const double inv_cell[3],
                                        const int ncell[3], int* mat,
                                        void* stream)
{
    const char* who = "nbk_pairs_cell_count_f64";
    PairsCellKey g;
    int64_t ncells;
    const int rc = make_grid(who, origin, inv_cell, ncell, &g, &ncells);
    if (rc != NBK_OK) return rc;
    return countsort_count<PairsCellKey, false>(who, pos_aos, n, chunk, g,
                                                ncells, mat, nullptr,
                                                stream);
}

extern "C" int nbk_pairs_cell_scatter_f64(const double* pos_aos,
                                          const double* weight, int64_t n,
                                          int chunk, const double origin[3],
                                          const double inv_cell[3],
                                          const int ncell[3],
                                          const int* bases,
                                          double* pos_out, double* w_out,
                                          void* stream)
{
    const char* who = "nbk_pairs_cell_scatter_f64";
    PairsCellKey g;
    int64_t ncells;
    const int rc = make_grid(who, origin, inv_cell, ncell, &g, &ncells);
    if (rc != NBK_OK) return rc;
    return countsort_scatter(who, pos_aos, weight, n, chunk, g, ncells,
                             bases, n, pos_out, w_out, stream);
}

extern "C" int nbk_pairs_max_bins(void) { return NBK_PAIRS_MAX_BINS; }

extern "C" int nbk_pairs_count_f64(const double* pos1, const double* w1,
                                   const int* start1, int64_t n1,
                                   const double* pos2, const double* w2,
                                   const int* start2, int64_t n2,
                                   int autocorr, const int ncell[3],
                                   const double box[3], int periodic,
                                   int mode, const double* edges0_sq,
                                   int nb0, const double* edges1, int nb1,
                                   int j0, int j1, int nblocks,
                                   void* partials, int64_t* npairs,
                                   double* wsum, double* xsum,
                                   void* stream)
{
    return count_pairs("nbk_pairs_count_f64", 0, 2, pos1, w1, start1, n1,
                       pos2, w2, start2, n2, autocorr, ncell, box,
                       periodic, mode, edges0_sq, nb0, edges1, nb1, j0, j1,
                       nblocks, partials, npairs, wsum, xsum, stream);
}

extern "C" int nbk_pairs_count_sky_f64(const double* pos1, const double* w1,
                                       const int* start1, int64_t n1,
                                       const double* pos2, const double* w2,
                                       const int* start2, int64_t n2,
                                       int autocorr, const int ncell[3],
                                       int mode, const double* edges0_sq,
                                       int nb0, const double* edges1,
                                       int nb1, int j0, int j1, int nblocks,
                                       void* partials, int64_t* npairs,
                                       double* wsum, double* xsum,
                                       void* stream)
{
    const double box[3] = {0.0, 0.0, 0.0};
    return count_pairs("nbk_pairs_count_sky_f64", 3, 5, pos1, w1, start1,
                       n1, pos2, w2, start2, n2, autocorr, ncell, box, 0,
                       mode, edges0_sq, nb0, edges1, nb1, j0, j1, nblocks,
                       partials, npairs, wsum, xsum, stream);
}
