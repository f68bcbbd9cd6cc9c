// Friends-of-friends (FOF) on a two-level cell list with a lock-free
// union-find: the replacement for kdcount.cluster.fof under the
// reference's nbodykit/algorithms/fof.py, f64 throughout.
//
// Cell grid (nbk_twolevel.h, shared with nbk_knn.hip):
// ncell[a] = ncoarse[a] * fine[a] cells per axis.  The fine
// cell of a particle is cell_axis() (nbk_cells.h); its coarse cell is
// that INTEGER divided by fine[a] — never a second floor with a coarse
// inv_cell, whose rounding could disagree with the first at a cell face.
// Cells are numbered block-major: coarse_id * nfine + sub_id, both
// row-major, so the fine cells of one coarse cell are contiguous.
//
// Pipeline (all launches on the caller's stream):
//  1. nbk_fof_cell_count_f64 / nbk_scan_matrix_i32 /
//     nbk_fof_cell_scatter_f64: the count-matrix sort of nbk_countsort.h
//     keyed by the coarse cell; the f64 payload column carries the
//     original particle index (exact below 2^53).
//  2. nbk_fof_fine_sort_f64: one block per coarse cell histograms its
//     particles over the nfine sub-cells in LDS, block-scans, writes its
//     slice of the fine start table and places positions + int32 index
//     from LDS cursors.  No global atomics.
//  3. nbk_fof_link_f64: one thread per sorted particle i walks the <= 27
//     (cell, shift) neighbours and tests every j < i.  Cell order is
//     sorted-index order, so a neighbour cell above the own cell is
//     skipped whole and the own cell stops at i: every unordered pair is
//     tested once per periodic image.  In-range pairs are united by
//     hooking the larger root under the smaller with a 32-bit CAS.
//  4. nbk_fof_flatten_i32: root[i] = find(i), a separate launch into a
//     separate array.
//
// Union-find invariants.  parent[k] <= k always, and a value stored into
// parent[k] is always an ancestor of k that is smaller than k: the CAS
// hooks a root under a smaller index, path compression replaces the
// parent of a NON-root by the root just found.  So chains strictly
// decrease, `find` ends after at most k + 1 steps, and a find that meets
// parent[k] > k (corrupt input) sets *err and leaves.  A failed CAS
// returns the fresh parent of the would-be root, which is smaller; the
// union continues from it, and the larger of its two indices strictly
// decreases from one attempt to the next.  No thread ever waits for
// another one: no fences, no barriers across blocks, no spinning.
//
// Visibility.  The per-XCD L2s are not coherent for plain accesses, so
// every access to `parent` inside the link kernel is an agent-scope
// relaxed atomic (loads and stores bypass L1, the CAS executes at the
// memory side).  A stale load is harmless: an old parent is still an
// ancestor, a stale "root" fails its CAS and returns the fresh value, and
// two finds that meet in one node prove the particles connected already.
#include "nbk_twolevel.h"

namespace {

constexpr int FOF_LINK_THREADS = 256;

// the coarse sort's key
struct FofCoarseKey {
    typedef int index_t;
    static constexpr bool two_keys = false;
    FofGrid g;

    __device__ __forceinline__ int operator()(double x, double y,
                                              double z) const {
        int coarse, sub;
        g.locate(x, y, z, &coarse, &sub);
        return coarse;
    }
};

// ---- fine pass ---------------------------------------------------------

// one block per coarse cell; every loop bound is block-uniform
__global__ void kfof_fine(const double* __restrict__ pos,
                          const double* __restrict__ idx, int n, FofGrid g,
                          int nfine, const int* __restrict__ cstart,
                          double* __restrict__ out,
                          int* __restrict__ idx_out,
                          int* __restrict__ fstart)
{
    extern __shared__ int hist[];   // nfine counts, then cursors
    const int tid = threadIdx.x;
    const int cb = blockIdx.x;
    // (clamped: a bad table must not send a read out of bounds)
    int b = cstart[cb], e = cstart[cb + 1];
    b = b < 0 ? 0 : (b > n ? n : b);
    e = e < b ? b : (e > n ? n : e);
    const double* x = pos;
    const double* y = pos + n;
    const double* z = pos + 2 * (int64_t)n;

    for (int k = tid; k < nfine; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    for (int i = b + tid; i < e; i += blockDim.x) {
        int coarse, sub;
        g.locate(x[i], y[i], z[i], &coarse, &sub);
        atomicAdd(&hist[sub], 1);
    }
    __syncthreads();

    // exclusive scan: a contiguous run of sub-cells per thread
    const int per = (nfine + (int)blockDim.x - 1) / (int)blockDim.x;
    const int k0 = tid * per < nfine ? tid * per : nfine;
    const int k1 = k0 + per < nfine ? k0 + per : nfine;
    int acc = 0;
    for (int k = k0; k < k1; k++) acc += hist[k];
    int run = b + nbk_block_exclusive_scan(acc);
    for (int k = k0; k < k1; k++) {
        const int c = hist[k];
        hist[k] = run;
        fstart[(int64_t)cb * nfine + k] = run;
        run += c;
    }
    if (cb == 0 && tid == 0) fstart[(int64_t)gridDim.x * nfine] = n;
    __syncthreads();

    double* ox = out;
    double* oy = out + n;
    double* oz = out + 2 * (int64_t)n;
    for (int i = b + tid; i < e; i += blockDim.x) {
        const double xi = x[i], yi = y[i], zi = z[i];
        int coarse, sub;
        g.locate(xi, yi, zi, &coarse, &sub);
        const int t = atomicAdd(&hist[sub], 1);
        ox[t] = xi;
        oy[t] = yi;
        oz[t] = zi;
        idx_out[t] = (int)idx[i];
    }
}

// ---- union-find --------------------------------------------------------

__device__ __forceinline__ int parent_load(const int* parent, int k) {
    return __hip_atomic_load(parent + k, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void flag_error(int* err) {
    __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of k, or -1 with *err set when a parent is not below its
// child: every step goes to a strictly smaller index, so at most k + 1
// steps whatever the array holds
__device__ __forceinline__ int fof_find(const int* parent, int k, int* err) {
    for (;;) {
        const int p = parent_load(parent, k);
        if (p == k) return k;
        if (p > k || p < 0) {
            flag_error(err);
            return -1;
        }
        k = p;
    }
}

// find with the parent of the (non-root) start replaced by the root
__device__ __forceinline__ int fof_find_compress(int* parent, int k,
                                                 int* err) {
    const int p = parent_load(parent, k);
    if (p == k) return k;
    if (p > k || p < 0) {
        flag_error(err);
        return -1;
    }
    const int r = fof_find(parent, p, err);
    if (r >= 0 && r != p)
        __hip_atomic_store(parent + k, r, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    return r;
}

// unite the sets of roots-or-descendants a and b; returns the smaller
// root (the caller's next starting point), or -1 on corrupt data.  max(a,
// b) strictly decreases from one round to the next.
__device__ __forceinline__ int fof_unite(int* parent, int a, int b,
                                         int* err) {
    int ra = fof_find(parent, a, err);
    int rb = fof_find_compress(parent, b, err);
    for (;;) {
        if (ra < 0 || rb < 0) return -1;
        if (ra == rb) return ra;
        const int hi = ra > rb ? ra : rb;
        const int lo = ra > rb ? rb : ra;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(
                parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        // hi is a root no longer; `seen` is its fresh parent
        if (seen >= hi || seen < 0) {
            flag_error(err);
            return -1;
        }
        ra = fof_find(parent, seen, err);
        rb = lo;
    }
}

struct LinkArgs {
    const double* pos;
    const int* start;
    int n;
    int ncoarse[3];
    int fine[3];
    double box[3];
    int periodic;
    double ll_sq;
    int* parent;
    int* err;
};

// One thread per sorted particle.  Scratch: none (no indexed arrays).
__global__ __launch_bounds__(FOF_LINK_THREADS)
void kfof_link(LinkArgs a)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n) return;
    const int i = (int)gi;
    const int n = a.n;
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
    const int c1 = lo;
    const int coarse = c1 / nfine, sub = c1 - coarse * nfine;
    const int cx = (coarse / (nc2 * nc1)) * f0 + sub / (f2 * f1);
    const int cy = ((coarse / nc2) % nc1) * f1 + (sub / f2) % f1;
    const int cz = (coarse % nc2) * f2 + sub % f2;

    const double* x = a.pos;
    const double* y = a.pos + n;
    const double* z = a.pos + 2 * (int64_t)n;
    const double xi = x[i], yi = y[i], zi = z[i];
    int ri = i;                     // a root-or-descendant of i's set

    for (int dxc = -1; dxc <= 1; dxc++) {
        int nx;  double sx;
        if (!neighbour_axis(cx, dxc, n0, a.periodic, a.box[0], &nx, &sx))
            continue;
        for (int dyc = -1; dyc <= 1; dyc++) {
            int ny;  double sy;
            if (!neighbour_axis(cy, dyc, n1, a.periodic, a.box[1], &ny,
                                &sy)) continue;
            for (int dzc = -1; dzc <= 1; dzc++) {
                int nz;  double sz;
                if (!neighbour_axis(cz, dzc, n2, a.periodic, a.box[2], &nz,
                                    &sz)) continue;
                const int c2 =
                    (((nx / f0) * nc1 + ny / f1) * nc2 + nz / f2) * nfine
                    + ((nx % f0) * f1 + ny % f1) * f2 + nz % f2;
                if (c2 > c1) continue;      // all of it above i
                int b2 = a.start[c2], e2 = a.start[c2 + 1];
                b2 = b2 < 0 ? 0 : b2;
                e2 = e2 > i ? i : e2;       // only j < i, and in bounds
                for (int j = b2; j < e2; j++) {
                    const double dx = (xi - x[j]) - sx;
                    const double dy = (yi - y[j]) - sy;
                    const double dz = (zi - z[j]) - sz;
                    const double r2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(r2 <= a.ll_sq)) continue;
                    ri = fof_unite(a.parent, ri, j, a.err);
                    if (ri < 0) return;
                }
            }
        }
    }
}

__global__ void kfof_flatten(const int* __restrict__ parent, int n,
                             int* __restrict__ root, int* err)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    root[i] = fof_find(parent, (int)i, err);
}

}  // namespace

extern "C" int nbk_fof_cell_count_f64(const double* pos_aos, int64_t n,
                                      int chunk, const double origin[3],
                                      const double inv_cell[3],
                                      const int ncoarse[3],
                                      const int fine[3], int* mat,
                                      void* stream)
{
    const char* who = "nbk_fof_cell_count_f64";
    FofCoarseKey key;
    int64_t ncoarse_all, nfine;
    const int rc = fof_key(who, origin, inv_cell, ncoarse, fine, &key.g,
                           &ncoarse_all, &nfine);
    if (rc != NBK_OK) return rc;
    return countsort_count<FofCoarseKey, false>(who, pos_aos, n, chunk, key,
                                                ncoarse_all, mat, nullptr,
                                                stream);
}

extern "C" int nbk_fof_cell_scatter_f64(const double* pos_aos,
                                        const double* index, int64_t n,
                                        int chunk, const double origin[3],
                                        const double inv_cell[3],
                                        const int ncoarse[3],
                                        const int fine[3], const int* bases,
                                        double* pos_out, double* index_out,
                                        void* stream)
{
    const char* who = "nbk_fof_cell_scatter_f64";
    FofCoarseKey key;
    int64_t ncoarse_all, nfine;
    const int rc = fof_key(who, origin, inv_cell, ncoarse, fine, &key.g,
                           &ncoarse_all, &nfine);
    if (rc != NBK_OK) return rc;
    return countsort_scatter(who, pos_aos, index, n, chunk, key,
                             ncoarse_all, bases, n, pos_out, index_out,
                             stream);
}

extern "C" int nbk_fof_fine_sort_f64(const double* pos_soa,
                                     const double* index, int64_t n,
                                     const double origin[3],
                                     const double inv_cell[3],
                                     const int ncoarse[3], const int fine[3],
                                     const int* coarse_start,
                                     double* pos_out, int* index_out,
                                     int* fine_start, void* stream)
{
    const char* who = "nbk_fof_fine_sort_f64";
    FofGrid g;
    int64_t ncoarse_all, nfine;
    int rc = fof_key(who, origin, inv_cell, ncoarse, fine, &g, &ncoarse_all,
                     &nfine);
    if (rc != NBK_OK) return rc;
    rc = fof_check_n(who, n);
    if (rc != NBK_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        // an all-empty table; the coarse table is not read
        NBK_CHECK_HIP(hipMemsetAsync(
            fine_start, 0, (size_t)(ncoarse_all * nfine + 1) * sizeof(int),
            s));
        return NBK_OK;
    }
    // (a histogram beyond a few thousand sub-cells leaves room for one
    // block per CU anyway: give its zeroing and its scan 1024 threads)
    const int threads = nfine > 4096 ? 1024 : 256;
    const size_t lds = (size_t)nfine * sizeof(int);
    raise_lds(reinterpret_cast<const void*>(&kfof_fine), lds);
    hipLaunchKernelGGL(kfof_fine, dim3((uint32_t)ncoarse_all), dim3(threads),
                       lds, s, pos_soa, index, (int)n, g, (int)nfine,
                       coarse_start, pos_out, index_out, fine_start);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_fof_link_f64(const double* pos_soa, const int* fine_start,
                                int64_t n, const int ncoarse[3],
                                const int fine[3], const double box[3],
                                int periodic, double ll_sq, int* parent,
                                int* err, void* stream)
{
    const char* who = "nbk_fof_link_f64";
    int64_t ncoarse_all, nfine;
    int rc = fof_grid(who, ncoarse, fine, &ncoarse_all, &nfine);
    if (rc != NBK_OK) return rc;
    rc = fof_check_n(who, n);
    if (rc != NBK_OK) return rc;
    if (!(ll_sq >= 0.0) || !std::isfinite(ll_sq)) {
        NBK_SET_ERR("%s: ll_sq = %g", who, ll_sq);
        return NBK_ERR_ARG;
    }
    if (n == 0) return NBK_OK;
    LinkArgs a;
    a.pos = pos_soa;
    a.start = fine_start;
    a.n = (int)n;
    for (int i = 0; i < 3; i++) {
        a.ncoarse[i] = ncoarse[i];
        a.fine[i] = fine[i];
        a.box[i] = box[i];
    }
    a.periodic = periodic;
    a.ll_sq = ll_sq;
    a.parent = parent;
    a.err = err;
    const int64_t nblocks = (n + FOF_LINK_THREADS - 1) / FOF_LINK_THREADS;
    hipLaunchKernelGGL(kfof_link, dim3((uint32_t)nblocks),
                       dim3(FOF_LINK_THREADS), 0, (hipStream_t)stream, a);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_fof_flatten_i32(const int* parent, int64_t n, int* root,
                                   int* err, void* stream)
{
    const char* who = "nbk_fof_flatten_i32";
    const int rc = fof_check_n(who, n);
    if (rc != NBK_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        hipLaunchKernelGGL(kfof_flatten, dim3((uint32_t)((n + 255) / 256)),
                           dim3(256), 0, s, parent, (int)n, root, err);
        NBK_CHECK_HIP(hipGetLastError());
    }
    int flagged = 0;
    NBK_CHECK_HIP(hipMemcpyAsync(&flagged, err, sizeof(int),
                                 hipMemcpyDeviceToHost, s));
    NBK_CHECK_HIP(hipStreamSynchronize(s));
    if (flagged) {
        NBK_SET_ERR("%s: a parent that is not below its child (the link "
                    "or this pass met a corrupt union-find array)", who);
        return NBK_ERR_ARG;
    }
    return NBK_OK;
}
