// Cylindrical groups on the two-level cell list of nbk_fof.hip: the
// replacement for the kd-tree pair enumeration, the dataframe of all pairs
// and the Python groupby under the reference's nbodykit/algorithms/cgm.py,
// f64 throughout.
//
// Input: the output of nbk_fof_fine_sort_f64, unchanged (nbk_twolevel.h:
// block-major cells, SoA positions and the fine start table), and prio[n],
// the priority of every sorted slot: a permutation of 0..n-1, a higher
// value is a higher priority.  Everything written is in sorted-slot order.
//
// Neighbours.  Objects i and j are neighbours iff, with d = r_i - r_j per
// axis and, periodic, `if (d > L/2) d -= L; if (d <= -L/2) d += L;`
// (the reference's wrap, in its order),
//   rlos  = (dx*lx + dy*ly) + dz*lz,  rlos2 = rlos * rlos      (los_mode 0)
//   c = 0.5 * (r_i + r_j),  dot = (dx*cx + dy*cy) + dz*cz,
//   rlos2 = (dot * dot) / ((cx*cx + cy*cy) + cz*cz)             (los_mode 1)
//   rsky2 = |((dx*dx + dy*dy) + dz*dz) - rlos2|
//   rsky2 <= rperp2 && rlos2 <= rpar2,
// every operation rounded separately (-ffp-contract=off).  0 / 0 is NaN
// and compares false.  The test reads r_i - r_j under the wrap rule, never
// a per-cell image shift, so a pair is tested once under one rounding
// whichever cell it was found in.
//
// One walk, three visitors.  cgm_walk: one thread per sorted particle i
// finds its cell by the binary search of kfof_link and visits every
// neighbour cell ONCE: per axis of n_a cells the offsets
// [-min(1, (n_a-1)/2), min(1, n_a/2)] when periodic (1 cell: itself; 2
// cells: itself and the other, once), [-1, 1] clamped to the grid
// otherwise.  Every loop bound is a function of the start table, clamped to
// [0, n]: no loop on data, no waiting, no global read-modify-write.
//
//  - kcgm_resolve: one sweep of the greedy selection over state[n]
//    (0 undecided, 1 central, 2 satellite).  An undecided i becomes a
//    satellite if a higher-priority neighbour is a central, else a central
//    if no higher-priority neighbour is undecided, else stays.  Both
//    transitions rest on FINAL information (a decided state never changes),
//    so a stale "undecided" read only delays a decision: the fixpoint is
//    the sequential highest-priority-first result whatever the thread
//    order.  The highest-priority undecided object always decides, so n
//    sweeps suffice.
//  - kcgm_host: host[i] = i for a central, the slot of the highest-priority
//    central in the cylinder for a satellite (state is final: plain loads).
//  - kcgm_count: nsat[i] = the number of slots j != i of the neighbour
//    cells with host[j] == i for a central, an integer compare without
//    geometry (the relation is symmetric, so j's central lies in j's
//    neighbour cells iff j lies in the central's); 0 for a satellite.
//
// Visibility.  The per-XCD L2s are not coherent for plain accesses, so
// inside the resolve kernel `state` is read and written with agent-scope
// relaxed atomic loads and stores only, as kfof_link does with `parent`.
// The two flag words are plain stores of the constant 1, read by the host
// after the stream has drained.
#include "nbk_twolevel.h"

namespace {

constexpr int CGM_THREADS = 256;

struct CgmArgs {
    const double* pos;
    const int* start;
    const int* prio;
    int n;
    int ncoarse[3];
    int fine[3];
    double box[3];
    int periodic;
    int los_mode;
    double los[3];
    double rperp2;
    double rpar2;
};

// the reference's wrap of one separation, in its order
__device__ __forceinline__ double cgm_wrap(double d, double L) {
    const double half = L * 0.5;
    if (d > half) d -= L;
    if (d <= -half) d += L;
    return d;
}

// the cylinder predicate of the pair (r1 = i, r2 = j)
__device__ __forceinline__ bool cgm_inside(const CgmArgs& a, double xi,
                                           double yi, double zi, double xj,
                                           double yj, double zj) {
    double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    if (a.periodic) {
        dx = cgm_wrap(dx, a.box[0]);
        dy = cgm_wrap(dy, a.box[1]);
        dz = cgm_wrap(dz, a.box[2]);
    }
    double rlos2;
    if (a.los_mode == 0) {
        const double rlos = (dx * a.los[0] + dy * a.los[1]) + dz * a.los[2];
        rlos2 = rlos * rlos;
    } else {
        const double cx = 0.5 * (xi + xj), cy = 0.5 * (yi + yj);
        const double cz = 0.5 * (zi + zj);
        const double dot = (dx * cx + dy * cy) + dz * cz;
        const double c2 = (cx * cx + cy * cy) + cz * cz;
        rlos2 = (dot * dot) / c2;
    }
    const double dr2 = (dx * dx + dy * dy) + dz * dz;
    const double rsky2 = fabs(dr2 - rlos2);
    return rsky2 <= a.rperp2 && rlos2 <= a.rpar2;
}

// offsets [lo, hi] of the neighbour cells on an axis of n cells around c
__device__ __forceinline__ void cgm_axis(int n, int c, int periodic, int* lo,
                                         int* hi) {
    if (periodic) {
        *lo = -((n - 1) / 2 < 1 ? (n - 1) / 2 : 1);
        *hi = n / 2 < 1 ? n / 2 : 1;
    } else {
        *lo = c > 0 ? -1 : 0;
        *hi = c < n - 1 ? 1 : 0;
    }
}

// a cell index at most one period outside [0, n), wrapped
__device__ __forceinline__ int cgm_wrap_cell(int c, int n) {
    return c < 0 ? c + n : (c >= n ? c - n : c);
}

// The walk of sorted particle i.  For every slot j of the neighbour cells:
// v.candidate(j) (the cheap integer test), then, where V::geometry, the
// cylinder predicate, then v.accept(j), which returns false to end the
// walk.  Scratch: none (no indexed arrays).
template <class V>
__device__ __forceinline__ void cgm_walk(const CgmArgs& a, int i, V& v)
{
    const int n = a.n;
    const int periodic = a.periodic;
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
    // (the own position only where the visitor tests the cylinder)
    double xi = 0.0, yi = 0.0, zi = 0.0;
    if (V::geometry) {
        xi = x[i];
        yi = y[i];
        zi = z[i];
    }

    int x0, x1, y0, y1, z0, z1;
    cgm_axis(n0, cx, periodic, &x0, &x1);
    cgm_axis(n1, cy, periodic, &y0, &y1);
    cgm_axis(n2, cz, periodic, &z0, &z1);
    for (int dxc = x0; dxc <= x1; dxc++) {
        const int gx = periodic ? cgm_wrap_cell(cx + dxc, n0) : cx + dxc;
        for (int dyc = y0; dyc <= y1; dyc++) {
            const int gy = periodic ? cgm_wrap_cell(cy + dyc, n1) : cy + dyc;
            for (int dzc = z0; dzc <= z1; dzc++) {
                const int gz = periodic ? cgm_wrap_cell(cz + dzc, n2)
                                        : cz + dzc;
                const int c2 =
                    (((gx / f0) * nc1 + gy / f1) * nc2 + gz / f2) * nfine
                    + ((gx % f0) * f1 + gy % f1) * f2 + gz % f2;
                int b2 = a.start[c2], e2 = a.start[c2 + 1];
                b2 = b2 < 0 ? 0 : b2;
                e2 = e2 > n ? n : e2;
                for (int j = b2; j < e2; j++) {
                    if (!v.candidate(j)) continue;
                    if (V::geometry
                        && !cgm_inside(a, xi, yi, zi, x[j], y[j], z[j]))
                        continue;
                    if (!v.accept(j)) return;
                }
            }
        }
    }
}

__device__ __forceinline__ int state_load(const int* state, int k) {
    return __hip_atomic_load(state + k, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void state_store(int* state, int k, int v) {
    __hip_atomic_store(state + k, v, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

// ---- resolve -------------------------------------------------------------

struct ResolveVisitor {
    static constexpr bool geometry = true;
    const int* prio;
    const int* state;
    int pi;
    bool blocked;       // a higher-priority neighbour is undecided
    bool satellite;     // a higher-priority neighbour is a central

    __device__ __forceinline__ bool candidate(int j) const {
        return prio[j] > pi;        // (never i itself)
    }
    __device__ __forceinline__ bool accept(int j) {
        const int sj = state_load(state, j);
        if (sj == 1) {
            satellite = true;
            return false;           // final: nothing more to learn
        }
        if (sj == 0) blocked = true;
        return true;
    }
};

__global__ __launch_bounds__(CGM_THREADS)
void kcgm_resolve(CgmArgs a, int* state, int* flags)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n) return;
    const int i = (int)gi;
    if (state_load(state, i) != 0) return;
    ResolveVisitor v;
    v.prio = a.prio;
    v.state = state;
    v.pi = a.prio[i];
    v.blocked = false;
    v.satellite = false;
    cgm_walk(a, i, v);
    if (v.satellite) {
        state_store(state, i, 2);
        flags[0] = 1;
    } else if (!v.blocked) {
        state_store(state, i, 1);
        flags[0] = 1;
    } else {
        flags[1] = 1;
    }
}

// ---- host ----------------------------------------------------------------

struct HostVisitor {
    static constexpr bool geometry = true;
    const int* prio;
    const int* state;
    int best_prio;      // the own priority until a central is found
    int best;

    __device__ __forceinline__ bool candidate(int j) const {
        return prio[j] > best_prio && state[j] == 1;
    }
    __device__ __forceinline__ bool accept(int j) {
        best_prio = prio[j];
        best = j;
        return true;
    }
};

__global__ __launch_bounds__(CGM_THREADS)
void kcgm_host(CgmArgs a, const int* __restrict__ state,
               int* __restrict__ host)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n) return;
    const int i = (int)gi;
    if (state[i] != 2) {
        host[i] = i;
        return;
    }
    HostVisitor v;
    v.prio = a.prio;
    v.state = state;
    v.best_prio = a.prio[i];
    v.best = i;
    cgm_walk(a, i, v);
    host[i] = v.best;
}

// ---- count ---------------------------------------------------------------

struct CountVisitor {
    static constexpr bool geometry = false;
    const int* host;
    int i;
    int count;

    __device__ __forceinline__ bool candidate(int j) const {
        return host[j] == i && j != i;
    }
    __device__ __forceinline__ bool accept(int) {
        count++;
        return true;
    }
};

__global__ __launch_bounds__(CGM_THREADS)
void kcgm_count(CgmArgs a, const int* __restrict__ state,
                const int* __restrict__ host, int* __restrict__ nsat)
{
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n) return;
    const int i = (int)gi;
    if (state[i] != 1) {
        nsat[i] = 0;
        return;
    }
    CountVisitor v;
    v.host = host;
    v.i = i;
    v.count = 0;
    cgm_walk(a, i, v);
    nsat[i] = v.count;
}

// the checks and the argument block common to the three entry points
int cgm_args(const char* who, const double* pos_soa, const int* fine_start,
             const int* prio, int64_t n, const int ncoarse[3],
             const int fine[3], const double box[3], int periodic,
             int los_mode, const double los[3], double rperp2, double rpar2,
             CgmArgs* a)
{
    int64_t ncoarse_all, nfine;
    int rc = fof_grid(who, ncoarse, fine, &ncoarse_all, &nfine);
    if (rc != NBK_OK) return rc;
    rc = fof_check_n(who, n);
    if (rc != NBK_OK) return rc;
    if (!(rperp2 >= 0.0) || !std::isfinite(rperp2) || !(rpar2 >= 0.0)
        || !std::isfinite(rpar2)) {
        NBK_SET_ERR("%s: rperp2 = %g, rpar2 = %g", who, rperp2, rpar2);
        return NBK_ERR_ARG;
    }
    if (los_mode != 0 && los_mode != 1) {
        NBK_SET_ERR("%s: los_mode = %d (0: fixed, 1: observer)", who,
                    los_mode);
        return NBK_ERR_ARG;
    }
    for (int i = 0; i < 3; i++) {
        if (los_mode == 0 && !std::isfinite(los[i])) {
            NBK_SET_ERR("%s: los[%d] = %g", who, i, los[i]);
            return NBK_ERR_ARG;
        }
        if (periodic && (!(box[i] > 0.0) || !std::isfinite(box[i]))) {
            NBK_SET_ERR("%s: periodic box[%d] = %g", who, i, box[i]);
            return NBK_ERR_ARG;
        }
    }
    a->pos = pos_soa;
    a->start = fine_start;
    a->prio = prio;
    a->n = (int)n;
    for (int i = 0; i < 3; i++) {
        a->ncoarse[i] = ncoarse[i];
        a->fine[i] = fine[i];
        a->box[i] = periodic ? box[i] : 0.0;
        a->los[i] = los_mode == 0 ? los[i] : 0.0;
    }
    a->periodic = periodic ? 1 : 0;
    a->los_mode = los_mode;
    a->rperp2 = rperp2;
    a->rpar2 = rpar2;
    return NBK_OK;
}

inline dim3 cgm_blocks(int64_t n) {
    return dim3((uint32_t)((n + CGM_THREADS - 1) / CGM_THREADS));
}

}  // namespace

extern "C" int nbk_cgm_resolve_f64(const double* pos_soa,
                                   const int* fine_start, const int* prio,
                                   int64_t n, const int ncoarse[3],
                                   const int fine[3], const double box[3],
                                   int periodic, int los_mode,
                                   const double los[3], double rperp2,
                                   double rpar2, int* state, int* flags,
                                   void* stream)
{
    CgmArgs a;
    const int rc = cgm_args("nbk_cgm_resolve_f64", pos_soa, fine_start, prio,
                            n, ncoarse, fine, box, periodic, los_mode, los,
                            rperp2, rpar2, &a);
    if (rc != NBK_OK) return rc;
    if (n == 0) return NBK_OK;
    hipLaunchKernelGGL(kcgm_resolve, cgm_blocks(n), dim3(CGM_THREADS), 0,
                       (hipStream_t)stream, a, state, flags);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_cgm_host_f64(const double* pos_soa, const int* fine_start,
                                const int* prio, int64_t n,
                                const int ncoarse[3], const int fine[3],
                                const double box[3], int periodic,
                                int los_mode, const double los[3],
                                double rperp2, double rpar2,
                                const int* state, int* host, void* stream)
{
    CgmArgs a;
    const int rc = cgm_args("nbk_cgm_host_f64", pos_soa, fine_start, prio, n,
                            ncoarse, fine, box, periodic, los_mode, los,
                            rperp2, rpar2, &a);
    if (rc != NBK_OK) return rc;
    if (n == 0) return NBK_OK;
    hipLaunchKernelGGL(kcgm_host, cgm_blocks(n), dim3(CGM_THREADS), 0,
                       (hipStream_t)stream, a, state, host);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_cgm_count_f64(const double* pos_soa, const int* fine_start,
                                 const int* prio, int64_t n,
                                 const int ncoarse[3], const int fine[3],
                                 const double box[3], int periodic,
                                 int los_mode, const double los[3],
                                 double rperp2, double rpar2,
                                 const int* state, const int* host,
                                 int* nsat, void* stream)
{
    CgmArgs a;
    const int rc = cgm_args("nbk_cgm_count_f64", pos_soa, fine_start, prio,
                            n, ncoarse, fine, box, periodic, los_mode, los,
                            rperp2, rpar2, &a);
    if (rc != NBK_OK) return rc;
    if (n == 0) return NBK_OK;
    hipLaunchKernelGGL(kcgm_count, cgm_blocks(n), dim3(CGM_THREADS), 0,
                       (hipStream_t)stream, a, state, host, nsat);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}
