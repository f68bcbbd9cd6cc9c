// k-th nearest neighbour on the two-level cell list of nbk_fof.hip: the
// replacement for scipy's cKDTree.query under the reference's
// nbodykit/algorithms/kdtree.py (KDDensity), f64 throughout.
//
// Input: the output of nbk_fof_fine_sort_f64, unchanged (nbk_twolevel.h:
// block-major cells, SoA positions, the input index of every sorted slot
// and the fine start table).
//
// nbk_knn_f64: one thread per sorted particle i.  It finds its cell by
// the binary search of kfof_link and visits the cells around it ring by
// ring: ring s is the offset box [lo_a(s), hi_a(s)] per axis without the
// box of ring s - 1, so every cell is visited at most once and, once
// every axis is covered, exactly once.  The k best candidates, ordered by
// the pair (r2, input index), live in registers; the search stops after
// the ring that covered every axis, or as soon as the k-th best r2 is
// within b * b, b the smallest distance from the particle to a face of
// the visited box (less a guard of 1e-9 cell sides for the rounding of
// cell_axis): every particle not yet seen lies beyond such a face.  Inside
// a ring, a cell whose nearest point (its nearer image when periodic, less
// the same guard) is already beyond the k-th best is passed over.
//
// Every loop bound is a function of (s, n_a, c) alone and every cell
// range is clamped to [0, n): no loop on data, no waiting, no atomics.
// Apart from read-only loads the only traffic is the two scatter stores
// of the result, in INPUT order.
//
// Distance: per axis d = x_i - x_j, d2 = d * d, and for a periodic run
// the smallest of d * d, (d - L) * (d - L), (d + L) * (d + L);
// r2 = (dx2 + dy2) + dz2, every operation rounded separately
// (-ffp-contract=off).  Positions of a periodic run lie in [0, L), so
// the smallest of the three images is the minimum image whichever cell
// the neighbour was found in.
#include "nbk_twolevel.h"

#include <climits>

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_MAX_K = 16;
// the guard of the stopping rule, in cell sides: cell_axis places a
// coordinate with an error of a few ulps of the coordinate, below 3e-13
// of a side at 1156 cells per axis
constexpr double KNN_FACE_GUARD = 1e-9;

struct KnnArgs {
    const double* pos;
    const int* start;
    const int* sindex;
    int n;
    double origin[3];
    double inv_cell[3];
    int ncoarse[3];
    int fine[3];
    double box[3];
    int periodic;
    int k;
    double* r2_out;
    int* index_out;
};

// offsets [lo, hi] of ring s on an axis of n cells around cell c
__device__ __forceinline__ void ring_axis(int s, int n, int c, int periodic,
                                          int* lo, int* hi) {
    if (periodic) {
        const int below = (n - 1) / 2, above = n / 2;
        *lo = -(s < below ? s : below);
        *hi = s < above ? s : above;
    } else {
        *lo = -(s < c ? s : c);
        *hi = s < n - 1 - c ? s : n - 1 - c;
    }
}

// the smaller of `b` and the guarded distances from coordinate u (from
// the origin; cell c) to the two faces of the offset range [lo, hi] of an
// axis that is not covered; a face on the edge of a non-periodic domain
// has nothing beyond it.  side = 0 stands for a flat axis.
__device__ __forceinline__ double face_bound(double b, double u, double side,
                                             int n, int c, int lo, int hi,
                                             int periodic) {
    if (hi - lo + 1 >= n || side == 0.0) return b;
    const double guard = KNN_FACE_GUARD * side;
    if (periodic || c + lo > 0) {
        const double d = (u - (double)(c + lo) * side) - guard;
        b = d < b ? d : b;
    }
    if (periodic || c + hi + 1 < n) {
        const double d = ((double)(c + hi + 1) * side - u) - guard;
        b = d < b ? d : b;
    }
    return b;
}

// the distance along one axis from coordinate u (cell c) to the cell at
// offset d, to the nearer of its two images when periodic, less the
// guard, clamped at 0: no particle of that cell is nearer on this axis
__device__ __forceinline__ double cell_gap(double u, double side, int n,
                                           int c, int d, int periodic) {
    if (d == 0 || side == 0.0) return 0.0;
    double g = d > 0 ? (double)(c + d) * side - u
                     : u - (double)(c + d + 1) * side;
    if (periodic) {
        // the image on the other side
        const int e = d > 0 ? d - n : d + n;
        const double g2 = e > 0 ? (double)(c + e) * side - u
                                : u - (double)(c + e + 1) * side;
        g = g2 < g ? g2 : g;
    }
    g -= KNN_FACE_GUARD * side;
    return g > 0.0 ? g : 0.0;
}

// a cell index at most one period outside [0, n), wrapped
__device__ __forceinline__ int wrap_cell(int c, int n) {
    return c < 0 ? c + n : (c >= n ? c - n : c);
}

__device__ __forceinline__ double axis_d2(double a, double b, double L,
                                          int periodic) {
    const double d = a - b;
    double d2 = d * d;
    if (periodic) {
        const double dm = d - L, dp = d + L;
        d2 = fmin(d2, fmin(dm * dm, dp * dp));
    }
    return d2;
}

// One thread per sorted particle.  Scratch: none — the K best live in
// registers, every index into them is a constant after unrolling.
template <int K>
__global__ __launch_bounds__(KNN_THREADS)
void kknn(KnnArgs a)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n) return;
    const int i = (int)gi;
    const int n = a.n;
    const int own = a.sindex[i];
    if (own < 0 || own >= n) return;        // never stored through
    const int periodic = a.periodic;
    const int k = a.k;
    const int f0 = a.fine[0], f1 = a.fine[1], f2 = a.fine[2];
    const int nc1 = a.ncoarse[1], nc2 = a.ncoarse[2];
    const int n0 = a.ncoarse[0] * f0, n1 = nc1 * f1, n2 = nc2 * f2;
    const int nfine = f0 * f1 * f2;
    const int ncells = a.ncoarse[0] * nc1 * nc2 * nfine;

    // own cell: the last c with start[c] <= i (log2(ncells) steps)
    int lo = 0, hi = ncells;        // invariant: answer in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.start[mid] <= i) lo = mid; else hi = mid;
    }
    const int coarse = lo / nfine, sub = lo - coarse * nfine;
    const int cx = (coarse / (nc2 * nc1)) * f0 + sub / (f2 * f1);
    const int cy = ((coarse / nc2) % nc1) * f1 + (sub / f2) % f1;
    const int cz = (coarse % nc2) * f2 + sub % f2;

    const double* x = a.pos;
    const double* y = a.pos + n;
    const double* z = a.pos + 2 * (int64_t)n;
    const double xi = x[i], yi = y[i], zi = z[i];
    const double Lx = a.box[0], Ly = a.box[1], Lz = a.box[2];
    // coordinates from the origin and cell sides (0: a flat axis)
    const double ux = xi - a.origin[0], uy = yi - a.origin[1];
    const double uz = zi - a.origin[2];
    const double sx = a.inv_cell[0] > 0.0 ? 1.0 / a.inv_cell[0] : 0.0;
    const double sy = a.inv_cell[1] > 0.0 ? 1.0 / a.inv_cell[1] : 0.0;
    const double sz = a.inv_cell[2] > 0.0 ? 1.0 / a.inv_cell[2] : 0.0;

    // ascending in (r2, input index); the sentinel sorts last
    double br[K];
    int bi[K];
    #pragma unroll
    for (int m = 0; m < K; m++) {
        br[m] = INFINITY;
        bi[m] = INT_MAX;
    }
    double kth = INFINITY;          // br[k - 1]

    int nmax = n0 > n1 ? n0 : n1;
    nmax = nmax > n2 ? nmax : n2;
    // the box of the ring before: empty
    int px0 = 1, px1 = 0, py0 = 1, py1 = 0, pz0 = 1, pz1 = 0;
    for (int s = 0; s < nmax; s++) {
        int x0, x1, y0, y1, z0, z1;
        ring_axis(s, n0, cx, periodic, &x0, &x1);
        ring_axis(s, n1, cy, periodic, &y0, &y1);
        ring_axis(s, n2, cz, periodic, &z0, &z1);
        for (int dx = x0; dx <= x1; dx++) {
            const int gx = periodic ? wrap_cell(cx + dx, n0) : cx + dx;
            const int idx = (gx / f0) * (nc1 * nc2 * nfine)
                            + (gx % f0) * (f1 * f2);
            const bool inx = dx >= px0 && dx <= px1;
            const double wx = cell_gap(ux, sx, n0, cx, dx, periodic);
            const double wx2 = wx * wx;
            for (int dy = y0; dy <= y1; dy++) {
                const int gy = periodic ? wrap_cell(cy + dy, n1) : cy + dy;
                const int idxy = idx + (gy / f1) * (nc2 * nfine)
                                 + (gy % f1) * f2;
                const bool inxy = inx && dy >= py0 && dy <= py1;
                const double wy = cell_gap(uy, sy, n1, cy, dy, periodic);
                const double wxy2 = wx2 + wy * wy;
                for (int dz = z0; dz <= z1; dz++) {
                    if (inxy && dz >= pz0 && dz <= pz1) {
                        dz = pz1;   // seen by an earlier ring: on to pz1 + 1
                        continue;
                    }
                    // a cell wholly beyond the k-th best holds nothing
                    const double wz = cell_gap(uz, sz, n2, cz, dz, periodic);
                    if (wxy2 + wz * wz > kth) continue;
                    const int gz = periodic ? wrap_cell(cz + dz, n2)
                                            : cz + dz;
                    const int c2 = idxy + (gz / f2) * nfine + gz % f2;
                    int b2 = a.start[c2], e2 = a.start[c2 + 1];
                    b2 = b2 < 0 ? 0 : b2;
                    e2 = e2 > n ? n : e2;
                    for (int j = b2; j < e2; j++) {
                        if (j == i) continue;
                        const double r2 =
                            (axis_d2(xi, x[j], Lx, periodic)
                             + axis_d2(yi, y[j], Ly, periodic))
                            + axis_d2(zi, z[j], Lz, periodic);
                        if (r2 > kth) continue;
                        const int id = a.sindex[j];
                        // predicated shift, from the far end down so that
                        // br[m - 1] is still the old entry
                        #pragma unroll
                        for (int m = K - 1; m >= 0; m--) {
                            const bool here = r2 < br[m]
                                || (r2 == br[m] && id < bi[m]);
                            bool prev = false;
                            if (m > 0)
                                prev = r2 < br[m - 1]
                                    || (r2 == br[m - 1] && id < bi[m - 1]);
                            if (here) {
                                br[m] = prev ? br[m > 0 ? m - 1 : 0] : r2;
                                bi[m] = prev ? bi[m > 0 ? m - 1 : 0] : id;
                            }
                        }
                        #pragma unroll
                        for (int m = 0; m < K; m++)
                            kth = (m == k - 1) ? br[m] : kth;
                    }
                }
            }
        }
        px0 = x0; px1 = x1; py0 = y0; py1 = y1; pz0 = z0; pz1 = z1;
        // every axis covered: every cell has been visited
        if (x1 - x0 + 1 >= n0 && y1 - y0 + 1 >= n1 && z1 - z0 + 1 >= n2)
            break;
        double b = INFINITY;
        b = face_bound(b, ux, sx, n0, cx, x0, x1, periodic);
        b = face_bound(b, uy, sy, n1, cy, y0, y1, periodic);
        b = face_bound(b, uz, sz, n2, cz, z0, z1, periodic);
        b = b > 0.0 ? b : 0.0;
        if (kth <= b * b) break;
    }

    int kid = INT_MAX;
    #pragma unroll
    for (int m = 0; m < K; m++) kid = (m == k - 1) ? bi[m] : kid;
    a.r2_out[own] = kth;
    a.index_out[own] = kid == INT_MAX ? -1 : kid;
}

template <int K>
void knn_launch(const KnnArgs& a, hipStream_t s) {
    const int64_t nblocks = ((int64_t)a.n + KNN_THREADS - 1) / KNN_THREADS;
    hipLaunchKernelGGL(kknn<K>, dim3((uint32_t)nblocks), dim3(KNN_THREADS),
                       0, s, a);
}

}  // namespace

extern "C" int nbk_knn_max_k(void) { return KNN_MAX_K; }

extern "C" int nbk_knn_f64(const double* pos_soa, const int* fine_start,
                           const int* sindex, int64_t n,
                           const double origin[3], const double inv_cell[3],
                           const int ncoarse[3], const int fine[3],
                           const double box[3], int periodic, int k,
                           double* r2_out, int* index_out, void* stream)
{
    const char* who = "nbk_knn_f64";
    int64_t ncoarse_all, nfine;
    int rc = fof_grid(who, ncoarse, fine, &ncoarse_all, &nfine);
    if (rc != NBK_OK) return rc;
    rc = fof_check_n(who, n);
    if (rc != NBK_OK) return rc;
    if (k < 1 || k > KNN_MAX_K) {
        NBK_SET_ERR("%s: k = %d (needs 1 <= k <= %d)", who, k, KNN_MAX_K);
        return NBK_ERR_ARG;
    }
    for (int i = 0; i < 3; i++) {
        if (!std::isfinite(origin[i]) || !std::isfinite(inv_cell[i])
            || inv_cell[i] < 0.0) {
            NBK_SET_ERR("%s: origin[%d] = %g, inv_cell[%d] = %g", who, i,
                        origin[i], i, inv_cell[i]);
            return NBK_ERR_ARG;
        }
        if (periodic && (!(box[i] > 0.0) || !std::isfinite(box[i]))) {
            NBK_SET_ERR("%s: periodic box[%d] = %g", who, i, box[i]);
            return NBK_ERR_ARG;
        }
    }
    if (n == 0) return NBK_OK;
    KnnArgs a;
    a.pos = pos_soa;
    a.start = fine_start;
    a.sindex = sindex;
    a.n = (int)n;
    for (int i = 0; i < 3; i++) {
        a.origin[i] = origin[i];
        a.inv_cell[i] = inv_cell[i];
        a.ncoarse[i] = ncoarse[i];
        a.fine[i] = fine[i];
        a.box[i] = periodic ? box[i] : 0.0;
    }
    a.periodic = periodic ? 1 : 0;
    a.k = k;
    a.r2_out = r2_out;
    a.index_out = index_out;
    hipStream_t s = (hipStream_t)stream;
    // k rounded up to the next instantiation
    if (k <= 1) knn_launch<1>(a, s);
    else if (k <= 2) knn_launch<2>(a, s);
    else if (k <= 4) knn_launch<4>(a, s);
    else if (k <= 8) knn_launch<8>(a, s);
    else knn_launch<16>(a, s);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}
