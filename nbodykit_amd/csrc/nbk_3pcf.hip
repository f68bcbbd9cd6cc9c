// Isotropic three-point correlation function multipoles zeta_l(r1, r2)
// (SimulationBox3PCF / SurveyData3PCF): the a_lm algorithm of Slepian &
// Eisenstein (2015) on the cell list of nbk_pairs.hip, f64 throughout,
// NO global atomics, every launch on the caller's stream.
//
// For every primary i the kernel forms, per radial bin b,
//   a_lm(b) = sum_{j in b} w_j Y_lm(d_ij / r_ij),   0 <= m <= l <= lmax,
// and adds w_i / (4 pi) sum_m c_m Re[a_lm(b1) conj(a_lm(b2))] (c_0 = 1,
// c_m = 2) into zeta_l(b1, b2).  d = p_j - p_i is the minimum image
// under the (cell, shift) rule of nbk_cells.h, r^2 = (dx^2 + dy^2) + dz^2
// is binned against squared edges, OPEN below and CLOSED above
// (edges[b] < r <= edges[b + 1]); a pair at r = 0 is in no bin.
//
// Y_lm without trigonometry: Y_lm = N_lm Pt_l^m(z) (x + i y)^m with the
// polynomial Pt_l^m = P_l^m / (1 - z^2)^(m/2) (no Condon-Shortley phase,
// it cancels in a a*):
//   Pt_m^m = (2m - 1)!!,
//   (l - m) Pt_l^m = (2l - 1) z Pt_(l-1)^m - (l + m - 1) Pt_(l-2)^m.
// N_lm^2 = (2l + 1) / (4 pi) (l - m)! / (l + m)! is applied once per
// primary at the zeta step.
//
// Mapping: a persistent grid strides over (cell, split) work items.  A
// block of W waves takes W primaries of the cell at a time, ONE WAVE PER
// PRIMARY, and stages 256-particle tiles of the <= 27 neighbour cells in
// LDS.  A wave tests 64 candidates of the tile at a time, one per lane,
// and deals the hits (the ballot's set bits, in tile order) to its 16
// m-lanes x 4 slices: lane (m, s) takes hit s, s + 4, ... , runs the
// recurrence upwards in l for its m and adds w_j Pt_l^m (x + i y)^m
// into its own LDS row a[s][bin][l, m].  No two lanes share an address:
// no atomics, no same-address serialisation, a fixed summation order.
// After the walk the four slices are summed in order, and the threads of
// the block, each owning fixed (l, b1 <= b2) entries, add the W primaries
// in wave order into the block's zeta accumulator.  Blocks store their
// partials with plain stores; a reduce kernel sums them in block order
// and mirrors b1 <-> b2.  Same sorted input + same nblocks => bitwise
// the same result.
#include "nbk_countsort.h"
#include "nbk_cells.h"

namespace {

constexpr int ZETA_TILE = 256;
constexpr int ZETA_MAX_WAVES = 4;
constexpr int ZETA_MAX_ELL = 15;            // 16 m-lanes
constexpr size_t ZETA_LDS_BYTES = 160 * 1024;

__host__ __device__ constexpr int n_lm(int lmax) {
    return (lmax + 1) * (lmax + 2) / 2;
}

__host__ __device__ constexpr int n_pair(int nbins) {
    return nbins * (nbins + 1) / 2;
}

// index of (b1 <= b2) in the row-major upper triangle
__host__ __device__ constexpr int pair_index(int b1, int b2, int nbins) {
    return b1 * nbins - b1 * (b1 - 1) / 2 + (b2 - b1);
}

// LDS carve, every section a multiple of 16 bytes:
// tile xy | tile zw | a[W][4][nbins][n_lm] | zeta[nent] | esq | kz |
// wprim | pairs
struct ZetaLayout {
    size_t alm, zacc, esq, kz, wprim, pairs, total;
};

__host__ __device__ inline size_t up16(size_t b) {
    return (b + 15) & ~(size_t)15;
}

__host__ __device__ inline ZetaLayout zeta_layout(int nbins, int lmax,
                                                  int nwaves) {
    const size_t nlm = n_lm(lmax);
    ZetaLayout L;
    L.alm = (size_t)ZETA_TILE * 2 * sizeof(double2);
    L.zacc = L.alm + (size_t)nwaves * 4 * nbins * nlm * sizeof(double2);
    L.esq = L.zacc + up16((size_t)(lmax + 1) * n_pair(nbins) * 8);
    L.kz = L.esq + up16((size_t)(nbins + 1) * 8);
    L.wprim = L.kz + up16(nlm * 8);
    L.pairs = L.wprim + up16((size_t)ZETA_MAX_WAVES * 8);
    L.total = L.pairs + up16((size_t)n_pair(nbins) * sizeof(ushort2));
    return L;
}

struct ZetaArgs {
    const double* pos;  const double* w;  const int* start;  int64_t n;
    int ncell[3];
    int periodic;
    double box[3];
    int nbins;
    int lmax;
    int split;              // work items per cell
    const double* esq;      // nbins + 1 squared edges
    double* partials;       // [gridDim.x * (lmax + 1) * n_pair(nbins)]
};

// index b of the bin with e[b] < v <= e[b + 1]; the caller has already
// checked e[0] < v <= e[n]
__device__ __forceinline__ int bin_search_closed_above(const double* e,
                                                       int n, double v) {
    int lo = 0, hi = n;             // invariant: e[lo] < v <= e[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (v > e[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

// lane (m, *) adds w_j Pt_l^m(z) (x + i y)^m, l = m..lmax, into its row.
// The loop over l is unrolled U >= lmax + 1 times with every row entry
// loaded first (unconditionally, from an in-range address: the loads of
// one secondary overlap instead of each waiting for the store before
// it), then the recurrence, then the stores of the lane's own entries.
// ca / cb are the lane's recurrence coefficients, 0 for l <= m, so that
// Pt stays 0 below l = m without a branch.  d / r, the power and the
// recurrence may contract (nothing here is bit-compared with the host;
// the binning is not touched).
template <int U>
__device__ __forceinline__ void add_ylm(double2* row, const double (&ca)[U],
                                        const double (&cb)[U], int m,
                                        int lmax, double pmm, double dx,
                                        double dy, double dz, double q,
                                        double wj)
{
    #pragma clang fp contract(fast)
    double2 acc[U];
    #pragma unroll
    for (int l = 0; l < U; l++) {
        const int lc = l < lmax ? l : lmax;
        acc[l] = row[lc * (lc + 1) / 2 + (m < lc ? m : lc)];
    }
    const double inv = 1.0 / sqrt(q);
    const double x = dx * inv, y = dy * inv, z = dz * inv;
    // (x + i y)^m by squaring, m < 16
    double cr = wj * pmm, ci = 0.0, br = x, bi = y;
    #pragma unroll
    for (int bit = 0; bit < 4; bit++) {
        if ((m >> bit) & 1) {
            const double tr = cr * br - ci * bi;
            ci = cr * bi + ci * br;
            cr = tr;
        }
        const double sr = br * br - bi * bi;
        bi = 2.0 * br * bi;
        br = sr;
    }
    double p1 = 0.0, p2 = 0.0;      // Pt_(l-1)^m, Pt_(l-2)^m over Pt_m^m
    #pragma unroll
    for (int l = 0; l < U; l++) {
        const double p = (l == m) ? 1.0 : ca[l] * z * p1 - cb[l] * p2;
        if (l >= m && l <= lmax) {
            acc[l].x += p * cr;
            acc[l].y += p * ci;
            row[l * (l + 1) / 2 + m] = acc[l];
        }
        p2 = p1;
        p1 = p;
    }
}

// U: the unroll count of the loop over l, >= lmax + 1
template <int U>
__global__ __launch_bounds__(64 * ZETA_MAX_WAVES)
void kzeta_alm(ZetaArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int nwaves = blockDim.x >> 6;
    const int nbins = a.nbins, lmax = a.lmax;
    const int nlm = n_lm(lmax);
    const int npair = n_pair(nbins);
    const int nent = (lmax + 1) * npair;
    const ZetaLayout L = zeta_layout(nbins, lmax, nwaves);
    double2* txy = reinterpret_cast<double2*>(lds_raw);
    double2* tzw = txy + ZETA_TILE;
    double2* alm = reinterpret_cast<double2*>(lds_raw + L.alm);
    double* zacc = reinterpret_cast<double*>(lds_raw + L.zacc);
    double* esq = reinterpret_cast<double*>(lds_raw + L.esq);
    double* kz = reinterpret_cast<double*>(lds_raw + L.kz);
    double* wprim = reinterpret_cast<double*>(lds_raw + L.wprim);
    ushort2* pairs = reinterpret_cast<ushort2*>(lds_raw + L.pairs);

    const int tid = threadIdx.x;
    const int wave = tid >> 6;
    const int lane = tid & 63;
    const int m = lane & 15;        // this lane's order
    const int s = lane >> 4;        // this lane's tile slice
    const int wave_rows = 4 * nbins * nlm;      // double2 per wave
    double2* awave = alm + (size_t)wave * wave_rows;

    // tables: edges, zeta weights, bin pairs
    for (int k = tid; k <= nbins; k += blockDim.x) esq[k] = a.esq[k];
    for (int k = tid; k < nlm; k += blockDim.x) {
        int l = 0;
        while ((l + 1) * (l + 2) / 2 <= k) l++;
        const int mm = k - l * (l + 1) / 2;
        // c_m N_lm^2 / (4 pi)
        double f = 1.0;             // (l + m)! / (l - m)!
        for (int j = l - mm + 1; j <= l + mm; j++) f *= (double)j;
        kz[k] = (mm == 0 ? 1.0 : 2.0) * (double)(2 * l + 1)
              / ((4.0 * M_PI) * (4.0 * M_PI) * f);
    }
    for (int b1 = tid; b1 < nbins; b1 += blockDim.x)
        for (int b2 = b1; b2 < nbins; b2++)
            pairs[pair_index(b1, b2, nbins)] =
                make_ushort2((unsigned short)b1, (unsigned short)b2);
    for (int k = tid; k < nent; k += blockDim.x) zacc[k] = 0.0;
    double pmm = 1.0;               // (2m - 1)!!
    for (int j = 1; j <= m; j++) pmm *= (double)(2 * j - 1);
    // this lane's recurrence: Pt_l = ca[l] z Pt_(l-1) - cb[l] Pt_(l-2)
    double ca[U], cb[U];
    #pragma unroll
    for (int l = 0; l < U; l++) {
        ca[l] = (l > m) ? (double)(2 * l - 1) / (double)(l - m) : 0.0;
        cb[l] = (l > m) ? (double)(l + m - 1) / (double)(l - m) : 0.0;
    }
    __syncthreads();

    const double q_lo = esq[0], q_hi = esq[nbins];
    const int ncy = a.ncell[1], ncz = a.ncell[2];
    const int ncells = a.ncell[0] * ncy * ncz;
    const int64_t nitems = (int64_t)ncells * a.split;
    const double* xs = a.pos;
    const double* ys = a.pos + a.n;
    const double* zs = a.pos + 2 * a.n;

    for (int64_t item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int c1 = (int)(item / a.split);
        const int sp = (int)(item - (int64_t)c1 * a.split);
        const int b1c = a.start[c1], e1c = a.start[c1 + 1];
        const int cz = c1 % ncz;
        const int cy = (c1 / ncz) % ncy;
        const int cx = c1 / (ncz * ncy);

        // every loop bound below is block-uniform: all threads reach
        // every barrier, waves without a primary only skip the adds
        for (int ib = b1c + sp * nwaves; ib < e1c;
             ib += a.split * nwaves) {
            const int nprim = (e1c - ib < nwaves) ? e1c - ib : nwaves;
            const int i = ib + wave;
            const bool have = wave < nprim;
            const double xi = have ? xs[i] : 0.0;
            const double yi = have ? ys[i] : 0.0;
            const double zi = have ? zs[i] : 0.0;
            if (lane == 0) wprim[wave] = have ? a.w[i] : 0.0;
            for (int k = lane; k < wave_rows; k += 64)
                awave[k] = make_double2(0.0, 0.0);

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
                        const int b2c = a.start[c2];
                        const int e2c = a.start[c2 + 1];

                        for (int t0 = b2c; t0 < e2c; t0 += ZETA_TILE) {
                            const int nt = (e2c - t0 < ZETA_TILE)
                                         ? e2c - t0 : ZETA_TILE;
                            __syncthreads();    // previous tile consumed
                            for (int t = tid; t < nt; t += blockDim.x) {
                                txy[t] = make_double2(xs[t0 + t],
                                                      ys[t0 + t]);
                                tzw[t] = make_double2(zs[t0 + t],
                                                      a.w[t0 + t]);
                            }
                            __syncthreads();
                            if (!have) continue;
                            // 64 candidates at a time, one per lane;
                            // their hits go to the slices four at a
                            // time, in tile order: slice s takes hit
                            // s, s + 4, ... of the tile's hits
                            for (int base = 0; base < nt; base += 64) {
                                bool hit = false;
                                if (base + lane < nt) {
                                    const double2 pxy = txy[base + lane];
                                    const double hx = (pxy.x - xi) + sx;
                                    const double hy = (pxy.y - yi) + sy;
                                    const double hz =
                                        (tzw[base + lane].x - zi) + sz;
                                    const double hq = (hx * hx + hy * hy)
                                                    + hz * hz;
                                    hit = hq > q_lo && hq <= q_hi;
                                }
                                unsigned long long mask = __ballot(hit);
                                while (mask) {
                                    int src = -1;
                                    #pragma unroll
                                    for (int j = 0; j < 4; j++) {
                                        if (mask) {
                                            if (s == j)
                                                src = __ffsll(mask) - 1;
                                            mask &= mask - 1;
                                        }
                                    }
                                    if (src < 0 || m > lmax) continue;
                                    const double2 pxy = txy[base + src];
                                    const double2 pzw = tzw[base + src];
                                    // d = p_j - p_i: the negative of
                                    // nbk_pairs.hip's (p1 - p2) - shift,
                                    // the same two roundings
                                    const double dx = (pxy.x - xi) + sx;
                                    const double dy = (pxy.y - yi) + sy;
                                    const double dz = (pzw.x - zi) + sz;
                                    const double q = (dx * dx + dy * dy)
                                                   + dz * dz;
                                    const int b = bin_search_closed_above(
                                        esq, nbins, q);
                                    add_ylm<U>(
                                        awave + (size_t)(s * nbins + b)
                                              * nlm,
                                        ca, cb, m, lmax, pmm, dx, dy, dz, q,
                                        pzw.y);
                                }
                            }
                        }
                    }
                }
            }

            __syncthreads();
            // the four slices in order, into slice 0
            for (int k = lane; k < nbins * nlm; k += 64) {
                double2 v = awave[k];
                #pragma unroll
                for (int c = 1; c < 4; c++) {
                    const double2 u = awave[c * nbins * nlm + k];
                    v.x += u.x;
                    v.y += u.y;
                }
                awave[k] = v;
            }
            __syncthreads();
            // zeta: every entry (l, b1 <= b2) has one owner thread, the
            // primaries of this trip are added in wave order
            for (int e = tid; e < nent; e += blockDim.x) {
                const int l = e / npair;
                const ushort2 bb = pairs[e - l * npair];
                const int k0 = l * (l + 1) / 2;
                double acc = zacc[e];
                for (int wv = 0; wv < nprim; wv++) {
                    const double2* r1 = alm + (size_t)wv * wave_rows
                                      + (size_t)bb.x * nlm + k0;
                    const double2* r2 = alm + (size_t)wv * wave_rows
                                      + (size_t)bb.y * nlm + k0;
                    double sum = 0.0;
                    for (int mm = 0; mm <= l; mm++) {
                        const double2 u = r1[mm], v = r2[mm];
                        sum += kz[k0 + mm] * (u.x * v.x + u.y * v.y);
                    }
                    acc += wprim[wv] * sum;
                }
                zacc[e] = acc;
            }
            __syncthreads();
        }
    }

    __syncthreads();
    for (int e = tid; e < nent; e += blockDim.x)
        a.partials[(size_t)blockIdx.x * nent + e] = zacc[e];
}

// sums the [nblocks x nent] partial rows in block order into
// zeta[lmax + 1][nbins][nbins], both triangles
__global__ void kzeta_reduce(const double* __restrict__ partials,
                             int nblocks, int nbins, int lmax,
                             double* __restrict__ zeta)
{
    const int npair = n_pair(nbins);
    const int nent = (lmax + 1) * npair;
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= (lmax + 1) * nbins * nbins) return;
    const int l = o / (nbins * nbins);
    const int b1 = (o / nbins) % nbins;
    const int b2 = o % nbins;
    const int e = l * npair + (b1 <= b2 ? pair_index(b1, b2, nbins)
                                        : pair_index(b2, b1, nbins));
    double sum = 0.0;
    for (int b = 0; b < nblocks; b++)
        sum += partials[(size_t)b * nent + e];
    zeta[o] = sum;
}

template <int U>
void launch_alm(const ZetaArgs& a, int nblocks, int nwaves, size_t lds,
                hipStream_t s) {
    raise_lds(reinterpret_cast<const void*>(&kzeta_alm<U>), lds);
    hipLaunchKernelGGL(kzeta_alm<U>, dim3((uint32_t)nblocks),
                       dim3(64 * nwaves), lds, s, a);
}

// waves per block: as many (<= 4) as fit the LDS, 0 when one does not
int zeta_waves(int nbins, int lmax) {
    for (int w = ZETA_MAX_WAVES; w >= 1; w--)
        if (zeta_layout(nbins, lmax, w).total <= ZETA_LDS_BYTES) return w;
    return 0;
}

}  // namespace

extern "C" int nbk_3pcf_max_ell(void) { return ZETA_MAX_ELL; }

extern "C" int nbk_3pcf_max_bins(int lmax)
{
    if (lmax < 0 || lmax > ZETA_MAX_ELL) return 0;
    int nbins = 0;
    // (bin pairs are stored as 16-bit indices)
    while (nbins < 65535 && zeta_waves(nbins + 1, lmax) > 0) nbins++;
    return nbins;
}

extern "C" int nbk_3pcf_zeta_f64(const double* pos, const double* w,
                                 const int* start, int64_t n,
                                 const int ncell[3], const double box[3],
                                 int periodic, const double* edges_sq,
                                 int nbins, int lmax, int nblocks,
                                 double* partials, double* zeta,
                                 void* stream)
{
    const char* who = "nbk_3pcf_zeta_f64";
    if (lmax < 0 || lmax > ZETA_MAX_ELL) {
        NBK_SET_ERR("%s: lmax = %d, the kernel holds 0 to %d", who, lmax,
                    ZETA_MAX_ELL);
        return NBK_ERR_ARG;
    }
    if (nbins < 1 || nbins > nbk_3pcf_max_bins(lmax)) {
        NBK_SET_ERR("%s: %d bins at lmax = %d, the LDS holds 1 to %d",
                    who, nbins, lmax, nbk_3pcf_max_bins(lmax));
        return NBK_ERR_ARG;
    }
    if (edges_sq == nullptr || partials == nullptr || zeta == nullptr
        || start == nullptr) {
        NBK_SET_ERR("%s: null edges, start, partials or zeta", who);
        return NBK_ERR_ARG;
    }
    if (n < 0 || n >= ((int64_t)1 << 31) || nblocks < 1
        || (n > 0 && (pos == nullptr || w == nullptr))) {
        NBK_SET_ERR("%s: n=%lld nblocks=%d", who, (long long)n, nblocks);
        return NBK_ERR_ARG;
    }
    int64_t ncells = 1;
    for (int i = 0; i < 3; i++) {
        if (ncell[i] < 1) {
            NBK_SET_ERR("%s: ncell[%d] = %d", who, i, ncell[i]);
            return NBK_ERR_ARG;
        }
        ncells *= ncell[i];
        if (ncells > NBK_SORT_LDS_INTS) {
            NBK_SET_ERR("%s: too many cells (%lld)", who,
                        (long long)ncells);
            return NBK_ERR_ARG;
        }
    }

    ZetaArgs a;
    a.pos = pos;  a.w = w;  a.start = start;  a.n = n;
    for (int i = 0; i < 3; i++) {
        a.ncell[i] = ncell[i];
        a.box[i] = periodic ? box[i] : 0.0;
    }
    a.periodic = periodic;
    a.nbins = nbins;
    a.lmax = lmax;
    // enough work items for the grid when there are few cells
    int64_t split = (4 * (int64_t)nblocks + ncells - 1) / ncells;
    a.split = (int)(split < 1 ? 1 : (split > 64 ? 64 : split));
    a.esq = edges_sq;
    a.partials = partials;

    hipStream_t s = (hipStream_t)stream;
    const int nwaves = zeta_waves(nbins, lmax);
    const size_t lds = zeta_layout(nbins, lmax, nwaves).total;
    if (lmax < 4)
        launch_alm<4>(a, nblocks, nwaves, lds, s);
    else if (lmax < 8)
        launch_alm<8>(a, nblocks, nwaves, lds, s);
    else if (lmax < 12)
        launch_alm<12>(a, nblocks, nwaves, lds, s);
    else
        launch_alm<16>(a, nblocks, nwaves, lds, s);
    NBK_CHECK_HIP(hipGetLastError());
    const int nout = (lmax + 1) * nbins * nbins;
    hipLaunchKernelGGL(kzeta_reduce, dim3((uint32_t)((nout + 255) / 256)),
                       dim3(256), 0, s, partials, nblocks, nbins, lmax,
                       zeta);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}
