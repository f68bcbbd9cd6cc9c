// Particle locality sorts for the paint kernels.
//
// Two count-matrix sorts (the atomic-free scheme of nbk_countsort.h) and
// one ticket sort:
// - nbk_xsort_count/scatter + nbk_bucket_fine (big meshes, the two-level
//   sort): the coarse key is (ix, iy-group); the fine pass then runs
//   count + block scan + placement entirely in LDS, one block per coarse
//   bucket.  Row-only fine mode serves the ownership-gather paint (which
//   needs row grouping, not full cell order) and emits the row table it
//   reads.
// - nbk_psort_count/scatter (big meshes, CIC): the key is (x-plane pair,
//   iy-group) with stencil-boundary particles duplicated into both
//   groups, so the gather paint reads bucket ranges and no fine pass
//   runs.
// - nbk_bucket_count/scatter (small inputs): the single-level counting
//   sort by full cell id with int32 countdown tickets (global atomics),
//   paired with the wave-merged scatter paint.
// nbk_scan_matrix_i32, the scan between count and scatter, lives here
// too and also serves the third key of the scheme, the pair counter's
// cell id (nbk_pairs.hip).
//
// All are non-stable within a bucket/cell (fine: deposits commute) and
// emit SoA (x[n] y[n] z[n]) — the layout the paint kernels read.
#include "nbk_countsort.h"

namespace {

__device__ __forceinline__ int64_t bucket_of(double x, double y, double z,
                                             double invH0, double invH1,
                                             double invH2, int64_t n0,
                                             int64_t n1, int64_t n2,
                                             int shift) {
    const int64_t ix = wrap_idx((int64_t)floor(x * invH0), n0);
    const int64_t iy = wrap_idx((int64_t)floor(y * invH1), n1);
    const int64_t iz = wrap_idx((int64_t)floor(z * invH2), n2);
    return ((ix * n1 + iy) * n2 + iz) >> shift;
}

// also detects (heuristically, lane-adjacent pairs) whether the input
// is already cell-ordered: scrambled -> *scrambled_flag = 1.  The caller
// skips the scatter pass for ordered input.
__global__ void kbucket_count(const double* __restrict__ pos, int64_t n,
                              int64_t n0, int64_t n1, int64_t n2,
                              double invH0, double invH1, double invH2,
                              int shift,
                              int* __restrict__ counts,
                              int* __restrict__ scrambled_flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int out_of_order = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        const int64_t b = bucket_of(pos[3 * i], pos[3 * i + 1],
                                    pos[3 * i + 2], invH0, invH1, invH2,
                                    n0, n1, n2, shift);
        atomicAdd(&counts[b], 1);
        const int64_t b_up = __shfl_up((long long)b, 1, 64);
        if (lane > 0 && b_up > b) out_of_order = 1;
    }
    if (out_of_order) atomicOr(scrambled_flag, 1);
}

// SOA=1: write x/y/z planes (the paint layout); SOA=0: AoS rows (the
// intermediate layout of the two-level sort's coarse pass)
template <int SOA>
__global__ void kbucket_scatter(const double* __restrict__ pos,
                                const double* __restrict__ mass, int64_t n,
                                int64_t n0, int64_t n1, int64_t n2,
                                double invH0, double invH1, double invH2,
                                int shift,
                                int* __restrict__ offsets,
                                double* __restrict__ ox,
                                double* __restrict__ oy,
                                double* __restrict__ oz,
                                double* __restrict__ om)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        const double x = pos[3 * i], y = pos[3 * i + 1], z = pos[3 * i + 2];
        const int64_t b = bucket_of(x, y, z, invH0, invH1, invH2,
                                    n0, n1, n2, shift);
        // offsets holds the INCLUSIVE bucket cumsum; tickets count DOWN
        // to the exclusive base (saves the host-side shift/int64 cast —
        // within-bucket order is arbitrary either way)
        const int64_t t = (int64_t)(atomicSub(&offsets[b], 1) - 1);
        if (SOA) {
            ox[t] = x;
            oy[t] = y;
            oz[t] = z;
        } else {
            ox[3 * t] = x;
            ox[3 * t + 1] = y;
            ox[3 * t + 2] = z;
        }
        if (mass) om[t] = mass[i];
    }
}

// ---- coarse key of the two-level sort ---------------------------------
// Running the fine cell sort on the coarse-sorted output keeps each
// block's cells inside one LDS window instead of thrashing the whole
// multi-GB array.

// coarse key: ix * (n1 >> ys) + (iy >> ys) — ys chosen by the host so
// that BOTH the coarse histogram (nbuckets ints) and the fine pass's
// per-bucket cell window ((1 << ys) * n2 ints) fit in LDS.  The scatter
// emits SoA planes so the fine pass's counting loop can read the
// 8 B/particle y plane instead of 24 B AoS rows — 16 GB less traffic at
// C4 (fine reads y twice: count + scatter).
struct XsortKey {
    typedef int64_t index_t;
    static constexpr bool two_keys = false;
    int64_t n0, n1, n2;
    double invH0, invH1, invH2;
    int ys;

    __device__ __forceinline__ int64_t operator()(double x, double y,
                                                  double) const {
        const int64_t ix = wrap_idx((int64_t)floor(x * invH0), n0);
        const int64_t iy = wrap_idx((int64_t)floor(y * invH1), n1);
        return ix * (n1 >> ys) + (iy >> ys);
    }
    // full cell id: the order the two-level sort produces
    __device__ __forceinline__ int64_t order_key(double x, double y,
                                                 double z) const {
        return bucket_of(x, y, z, invH0, invH1, invH2, n0, n1, n2, 0);
    }
};

// ---- count-matrix scan (replaces the torch transpose/cumsum glue) ----
// mat is [nblocks x nbuck] chunk-major.  Produces bases[c][b] =
// (sum of all buckets < b over every chunk) + (sum of bucket b over
// chunks < c) — the cursor seeds kxsort_scatter reads — and
// bucket_bases[0..nbuck] = exclusive bucket totals (the fine pass's
// block ranges).  One coalesced read for the column sums, one
// read+write for the bases: ~1.5 passes over mat vs the ~8 of the
// transpose+cumsum+sub+transpose torch chain it replaces.

// segmented column sums: with only nbuck (~32K) threads the serial
// per-bucket chunk walks ran at 2 waves/CU and cost ~3 ms/step at C4;
// splitting each column into NSEG segments gives NSEG x the threads
// (full occupancy) at ~1.5 extra matrix passes of traffic.
#define NBK_SCAN_SEG 8

__global__ void kscan_partial(const int* __restrict__ mat,
                              int64_t nblocks, int64_t nbuck,
                              int64_t cs /* chunks per segment */,
                              int* __restrict__ partial /* NSEG*nbuck */)
{
    const int64_t flat = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (flat >= nbuck * NBK_SCAN_SEG) return;
    const int64_t s = flat / nbuck;
    const int64_t b = flat - s * nbuck;
    const int64_t c0 = s * cs;
    const int64_t c1 = (c0 + cs < nblocks) ? c0 + cs : nblocks;
    int acc = 0;
    for (int64_t c = c0; c < c1; c++)
        acc += mat[c * nbuck + b];
    partial[s * nbuck + b] = acc;
}

__global__ void kscan_fold(const int* __restrict__ partial,
                           int64_t nbuck, int* __restrict__ colsum)
{
    const int64_t b = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (b >= nbuck) return;
    int s = 0;
    #pragma unroll
    for (int j = 0; j < NBK_SCAN_SEG; j++)
        s += partial[(int64_t)j * nbuck + b];
    colsum[b] = s;
}

// single-block exclusive scan of colsum (nbuck <= NBK_SORT_LDS_INTS):
// writes the exclusive base back into colsum and the inclusive edges
// into bucket_bases[1..nbuck] (bucket_bases[0] = 0)
__global__ void kscan_exclusive(int* __restrict__ colsum, int64_t nbuck,
                                int* __restrict__ bucket_bases)
{
    const int T = blockDim.x;
    const int t = threadIdx.x;
    const int S = (int)((nbuck + T - 1) / T);
    int acc = 0;
    for (int j = 0; j < S; j++) {
        const int64_t idx = (int64_t)t * S + j;
        if (idx < nbuck) acc += colsum[idx];
    }
    int run = nbk_block_exclusive_scan(acc);
    for (int j = 0; j < S; j++) {
        const int64_t idx = (int64_t)t * S + j;
        if (idx < nbuck) {
            const int c = colsum[idx];
            colsum[idx] = run;
            run += c;
            bucket_bases[idx + 1] = run;
        }
    }
    if (t == 0) bucket_bases[0] = 0;
}

__global__ void kscan_bases(const int* __restrict__ mat, int64_t nblocks,
                            int64_t nbuck, int64_t cs,
                            const int* __restrict__ partial,
                            const int* __restrict__ excl,
                            int* __restrict__ bases)
{
    const int64_t flat = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (flat >= nbuck * NBK_SCAN_SEG) return;
    const int64_t s = flat / nbuck;
    const int64_t b = flat - s * nbuck;
    int run = excl[b];
    for (int64_t j = 0; j < s; j++)
        run += partial[j * nbuck + b];
    const int64_t c0 = s * cs;
    const int64_t c1 = (c0 + cs < nblocks) ? c0 + cs : nblocks;
    for (int64_t c = c0; c < c1; c++) {
        bases[c * nbuck + b] = run;
        run += mat[c * nbuck + b];
    }
}

// fused fine pass: one block per coarse bucket.  The bucket's particles
// are contiguous (coarse sort) and its cells span a window of
// (1 << ys) * n2 entries, so count + exclusive scan + placement all run
// in LDS — ZERO global atomics.  (The count probe measured the global
// atomic pipe at ~25 G ops/s regardless of locality, which bounded the
// old single-level sort; LDS histograms run at the read bandwidth.)
// Output order = exact cell order, identical to the single-level sort.
__global__ void kbucket_fine(const double* __restrict__ px,
                             const double* __restrict__ py,
                             const double* __restrict__ pz,
                             const double* __restrict__ mass,
                             int64_t n1, int64_t n2,
                             double invH1, double invH2,
                             int ys,
                             const int* __restrict__ bbase, /* nbuck+1 */
                             double* __restrict__ ox,
                             double* __restrict__ oy,
                             double* __restrict__ oz,
                             double* __restrict__ om,
                             int* __restrict__ rowtab /* n0*n1, or NULL:
                                 start index of each (ix, iy) row in the
                                 sorted output — consumed by the gather
                                 paint kernel */)
{
    extern __shared__ int lds[];            // win ints (counts->cursors)
    const int64_t win = ((int64_t)1 << ys) * n2;
    const int64_t ymask = ((int64_t)1 << ys) - 1;
    const int T = blockDim.x;
    const int t = threadIdx.x;

    for (int64_t w = t; w < win; w += T) lds[w] = 0;
    __syncthreads();

    const int64_t beg = bbase[blockIdx.x];
    const int64_t end = bbase[blockIdx.x + 1];

    for (int64_t i = beg + t; i < end; i += T) {
        const int64_t iy = wrap_idx((int64_t)floor(py[i] * invH1), n1);
        const int64_t iz = wrap_idx((int64_t)floor(pz[i] * invH2), n2);
        atomicAdd(&lds[(iy & ymask) * n2 + iz], 1);
    }
    __syncthreads();

    // block-wide exclusive scan of lds[0..win), seeded with beg
    const int S = (int)(win / T);           // win % T == 0 (host guard)
    int acc = 0;
    for (int j = 0; j < S; j++) acc += lds[t * S + j];
    int run = (int)beg + nbk_block_exclusive_scan(acc);
    for (int j = 0; j < S; j++) {
        const int c = lds[t * S + j];
        lds[t * S + j] = run;
        run += c;
    }
    __syncthreads();

    if (rowtab) {
        // row r of this bucket starts where its first cell's cursor
        // points (post-scan, pre-scatter)
        const int64_t nyb = n1 >> ys;
        const int64_t ix = blockIdx.x / nyb;
        const int64_t yb = blockIdx.x % nyb;
        for (int r = t; r < (1 << ys); r += T)
            rowtab[ix * n1 + yb * ((int64_t)1 << ys) + r] =
                lds[(int64_t)r * n2];
        __syncthreads();
    }

    for (int64_t i = beg + t; i < end; i += T) {
        const double x = px[i], y = py[i], z = pz[i];
        const int64_t iy = wrap_idx((int64_t)floor(y * invH1), n1);
        const int64_t iz = wrap_idx((int64_t)floor(z * invH2), n2);
        const int slot = atomicAdd(&lds[(iy & ymask) * n2 + iz], 1);
        ox[slot] = x;
        oy[slot] = y;
        oz[slot] = z;
        if (mass) om[slot] = mass[i];
    }
}

// row-only fine pass: when the ownership-gather paint consumes the
// output, full cell order is unnecessary — the gather reads particles
// through ROW intervals (rowtab) and z order within a row is
// irrelevant (unsorted z even reduces its LDS same-address conflicts).
// The window shrinks from (1<<ys)*n2 cells to (1<<ys) rows, so this
// kernel runs at full occupancy with a trivial serial scan.
__global__ void kbucket_fine_rows(const double* __restrict__ px,
                                  const double* __restrict__ py,
                                  const double* __restrict__ pz,
                                  const double* __restrict__ mass,
                                  int64_t n1,
                                  double invH1,
                                  int ys,
                                  const int* __restrict__ bbase,
                                  double* __restrict__ ox,
                                  double* __restrict__ oy,
                                  double* __restrict__ oz,
                                  double* __restrict__ om,
                                  int* __restrict__ rowtab)
{
    extern __shared__ int cur[];            // (1 << ys) cursors
    const int nr = 1 << ys;
    const int64_t ymask = nr - 1;
    const int T = blockDim.x;
    const int t = threadIdx.x;

    for (int r = t; r < nr; r += T) cur[r] = 0;
    __syncthreads();

    const int64_t beg = bbase[blockIdx.x];
    const int64_t end = bbase[blockIdx.x + 1];

    for (int64_t i = beg + t; i < end; i += T) {
        const int64_t iy = wrap_idx((int64_t)floor(py[i] * invH1), n1);
        atomicAdd(&cur[iy & ymask], 1);
    }
    __syncthreads();

    if (t == 0) {
        int run = (int)beg;
        for (int r = 0; r < nr; r++) {
            const int c = cur[r];
            cur[r] = run;
            run += c;
        }
    }
    __syncthreads();

    if (rowtab) {
        const int64_t nyb = n1 >> ys;
        const int64_t ix = blockIdx.x / nyb;
        const int64_t yb = blockIdx.x % nyb;
        for (int r = t; r < nr; r += T)
            rowtab[ix * n1 + yb * (int64_t)nr + r] = cur[r];
        __syncthreads();
    }

    for (int64_t i = beg + t; i < end; i += T) {
        const double x = px[i], y = py[i], z = pz[i];
        const int64_t iy = wrap_idx((int64_t)floor(y * invH1), n1);
        const int slot = atomicAdd(&cur[iy & ymask], 1);
        ox[slot] = x;
        oy[slot] = y;
        oz[slot] = z;
        if (mass) om[slot] = mass[i];
    }
}


// ---- PAIR-BUCKET key (the fine-pass eliminator) -----------------------
// Key = (x-plane PAIR, y row-GROUP) with nbuck = (n0/2) * (n1 >> ys)
// i32 LDS histogram entries, and particles DUPLICATED into every
// y-group their deposit stencil touches (rows [iy+dlo, iy+dhi]; the
// stencil spans <= 5 rows << the group size, so <= 2 copies).  The
// ownership-gather paint then reads each (pair, group) bucket range
// directly — its deposit masks drop the out-of-tile copies — and the
// whole per-row fine pass (56 GB of moves at C4) disappears.  The cost
// moves into the paint's source reads: a pair bucket holds ~3 planes
// of particles, read by each of the pair's 2 tiles.
struct PsortKey {
    typedef int64_t index_t;
    static constexpr bool two_keys = true;
    int64_t n0, n1;
    double invH0, invH1;
    int ys, dlo, dhi;

    __device__ __forceinline__ int64_t operator()(double x, double y,
                                                  double,
                                                  int64_t* k2) const {
        const int64_t ix = wrap_idx((int64_t)floor(x * invH0), n0);
        const int64_t iy = (int64_t)floor(y * invH1);
        const int64_t ng = n1 >> ys;
        const int64_t g1 = wrap_idx(iy + dlo, n1) >> ys;
        const int64_t g2 = wrap_idx(iy + dhi, n1) >> ys;
        const int64_t base = (ix >> 1) * ng;
        *k2 = (g2 == g1) ? -1 : base + g2;
        return base + g1;
    }
};

int sgrid(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 1048576) g = 1048576;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int nbk_bucket_count_f64(const double* pos_aos, int64_t n,
                                    const int64_t nmesh[3],
                                    const double box[3], int shift,
                                    int* counts, int* scrambled_flag,
                                    void* stream)
{
    if (n == 0) return NBK_OK;
    hipLaunchKernelGGL(kbucket_count, dim3(sgrid(n)), dim3(256), 0,
                       (hipStream_t)stream, pos_aos, n,
                       nmesh[0], nmesh[1], nmesh[2],
                       nmesh[0] / box[0], nmesh[1] / box[1],
                       nmesh[2] / box[2], shift, counts, scrambled_flag);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_bucket_scatter_f64(const double* pos_aos,
                                      const double* mass, int64_t n,
                                      const int64_t nmesh[3],
                                      const double box[3], int shift,
                                      int soa_out,
                                      int* offsets,
                                      double* pos_out,
                                      double* mass_out, void* stream)
{
    if (n == 0) return NBK_OK;
    hipStream_t s = (hipStream_t)stream;
    if (soa_out)
        hipLaunchKernelGGL(kbucket_scatter<1>, dim3(sgrid(n)), dim3(256),
                           0, s, pos_aos, mass, n,
                           nmesh[0], nmesh[1], nmesh[2],
                           nmesh[0] / box[0], nmesh[1] / box[1],
                           nmesh[2] / box[2], shift, offsets,
                           pos_out, pos_out + n, pos_out + 2 * n,
                           mass_out);
    else
        hipLaunchKernelGGL(kbucket_scatter<0>, dim3(sgrid(n)), dim3(256),
                           0, s, pos_aos, mass, n,
                           nmesh[0], nmesh[1], nmesh[2],
                           nmesh[0] / box[0], nmesh[1] / box[1],
                           nmesh[2] / box[2], shift, offsets,
                           pos_out, nullptr, nullptr, mass_out);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

namespace {

// geometry checks + key of nbk_xsort_*; `who` names the entry point
int xsort_key(const char* who, const int64_t nmesh[3], const double box[3],
              int ys, XsortKey* key, int64_t* nbuck)
{
    if (ys < 0 || ys > 30 || (nmesh[1] % ((int64_t)1 << ys))) {
        NBK_SET_ERR("%s: bad ys=%d for mesh", who, ys);
        return NBK_ERR_ARG;
    }
    *key = {nmesh[0], nmesh[1], nmesh[2], nmesh[0] / box[0],
            nmesh[1] / box[1], nmesh[2] / box[2], ys};
    *nbuck = nmesh[0] * (nmesh[1] >> ys);
    return NBK_OK;
}

// geometry checks + key of nbk_psort_*
int psort_key(const char* who, const int64_t nmesh[3], const double box[3],
              int ys, int dlo, int dhi, PsortKey* key, int64_t* nbuck)
{
    if (ys < 0 || ys > 30 || (nmesh[0] & 1)
        || (nmesh[1] % ((int64_t)1 << ys))
        || (dhi - dlo) >= ((int64_t)1 << ys)) {
        NBK_SET_ERR("%s: bad geometry ys=%d dlo=%d dhi=%d", who, ys, dlo,
                    dhi);
        return NBK_ERR_ARG;
    }
    *key = {nmesh[0], nmesh[1], nmesh[0] / box[0], nmesh[1] / box[1], ys,
            dlo, dhi};
    *nbuck = (nmesh[0] >> 1) * (nmesh[1] >> ys);
    return NBK_OK;
}

}  // namespace

extern "C" int nbk_xsort_count_f64(const double* pos_aos, int64_t n,
                                   int chunk, const int64_t nmesh[3],
                                   const double box[3], int ys, int* mat,
                                   int* scrambled_flag, void* stream)
{
    const char* who = "nbk_xsort_count_f64";
    XsortKey key;
    int64_t nbuck;
    const int rc = xsort_key(who, nmesh, box, ys, &key, &nbuck);
    if (rc != NBK_OK) return rc;
    return countsort_count<XsortKey, true>(who, pos_aos, n, chunk, key,
                                           nbuck, mat, scrambled_flag,
                                           stream);
}

extern "C" int nbk_xsort_scatter_f64(const double* pos_aos,
                                     const double* mass, int64_t n,
                                     int chunk, const int64_t nmesh[3],
                                     const double box[3], int ys,
                                     const int* bases,
                                     double* pos_out, double* mass_out,
                                     void* stream)
{
    const char* who = "nbk_xsort_scatter_f64";
    XsortKey key;
    int64_t nbuck;
    const int rc = xsort_key(who, nmesh, box, ys, &key, &nbuck);
    if (rc != NBK_OK) return rc;
    return countsort_scatter(who, pos_aos, mass, n, chunk, key, nbuck,
                             bases, n, pos_out, mass_out, stream);
}

/* colsum_tmp must hold (NBK_SCAN_SEG + 1) * nbuck ints: segment
 * partials first, the column-sum/exclusive-base vector last. */
extern "C" int nbk_scan_matrix_i32(const int* mat, int64_t nblocks,
                                   int64_t nbuck, int* colsum_tmp,
                                   int* bases, int* bucket_bases,
                                   void* stream)
{
    if (nblocks == 0 || nbuck == 0) return NBK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int T = 256;
    int* partial = colsum_tmp;
    int* colsum = colsum_tmp + NBK_SCAN_SEG * nbuck;
    const int64_t cs = (nblocks + NBK_SCAN_SEG - 1) / NBK_SCAN_SEG;
    const uint32_t gs_ = (uint32_t)((nbuck * NBK_SCAN_SEG + T - 1) / T);
    const uint32_t g = (uint32_t)((nbuck + T - 1) / T);
    hipLaunchKernelGGL(kscan_partial, dim3(gs_), dim3(T), 0, s,
                       mat, nblocks, nbuck, cs, partial);
    hipLaunchKernelGGL(kscan_fold, dim3(g), dim3(T), 0, s,
                       partial, nbuck, colsum);
    hipLaunchKernelGGL(kscan_exclusive, dim3(1), dim3(1024), 0, s,
                       colsum, nbuck, bucket_bases);
    hipLaunchKernelGGL(kscan_bases, dim3(gs_), dim3(T), 0, s,
                       mat, nblocks, nbuck, cs, partial, colsum, bases);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_bucket_fine_f64(const double* pos_soa,
                                   const double* mass, int64_t n,
                                   const int64_t nmesh[3],
                                   const double box[3], int ys,
                                   const int* bucket_bases,
                                   double* soa_out, double* mass_out,
                                   int* rowtab, int rows_only,
                                   void* stream)
{
    if (n == 0) return NBK_OK;
    const int64_t nbuck = nmesh[0] * (nmesh[1] >> ys);
    if (rows_only) {
        if (nmesh[1] % ((int64_t)1 << ys)) {
            NBK_SET_ERR("nbk_bucket_fine_f64: bad ys=%d", ys);
            return NBK_ERR_ARG;
        }
        const size_t lds = ((size_t)1 << ys) * sizeof(int);
        hipLaunchKernelGGL(kbucket_fine_rows, dim3((uint32_t)nbuck),
                           dim3(1024), lds, (hipStream_t)stream,
                           pos_soa, pos_soa + n, pos_soa + 2 * n,
                           mass, nmesh[1], nmesh[1] / box[1], ys,
                           bucket_bases, soa_out, soa_out + n,
                           soa_out + 2 * n, mass_out, rowtab);
        NBK_CHECK_HIP(hipGetLastError());
        return NBK_OK;
    }
    const int64_t win = ((int64_t)1 << ys) * nmesh[2];
    if (win > NBK_SORT_LDS_INTS || (win % 1024)
        || (nmesh[1] % ((int64_t)1 << ys))) {
        NBK_SET_ERR("nbk_bucket_fine_f64: bad ys=%d for mesh", ys);
        return NBK_ERR_ARG;
    }
    const size_t lds = (size_t)win * sizeof(int);
    raise_lds(reinterpret_cast<const void*>(&kbucket_fine), lds);
    hipLaunchKernelGGL(kbucket_fine, dim3((uint32_t)nbuck), dim3(1024),
                       lds, (hipStream_t)stream,
                       pos_soa, pos_soa + n, pos_soa + 2 * n, mass,
                       nmesh[1], nmesh[2],
                       nmesh[1] / box[1], nmesh[2] / box[2], ys,
                       bucket_bases, soa_out, soa_out + n,
                       soa_out + 2 * n, mass_out, rowtab);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_psort_count_f64(const double* pos_aos, int64_t n,
                                   int chunk, const int64_t nmesh[3],
                                   const double box[3], int ys,
                                   int dlo, int dhi, int* mat,
                                   void* stream)
{
    const char* who = "nbk_psort_count_f64";
    PsortKey key;
    int64_t nbuck;
    const int rc = psort_key(who, nmesh, box, ys, dlo, dhi, &key, &nbuck);
    if (rc != NBK_OK) return rc;
    return countsort_count<PsortKey, false>(who, pos_aos, n, chunk, key,
                                            nbuck, mat, nullptr, stream);
}

extern "C" int nbk_psort_scatter_f64(const double* pos_aos,
                                     const double* mass, int64_t n,
                                     int chunk, const int64_t nmesh[3],
                                     const double box[3], int ys,
                                     int dlo, int dhi,
                                     const int* bases, int64_t n_out,
                                     double* pos_out, double* mass_out,
                                     void* stream)
{
    const char* who = "nbk_psort_scatter_f64";
    PsortKey key;
    int64_t nbuck;
    const int rc = psort_key(who, nmesh, box, ys, dlo, dhi, &key, &nbuck);
    if (rc != NBK_OK) return rc;
    return countsort_scatter(who, pos_aos, mass, n, chunk, key, nbuck,
                             bases, n_out, pos_out, mass_out, stream);
}
