// The chunked count-matrix counting sort, shared by the mesh locality
// sorts (nbk_sort.hip) and the pair counter's cell sort (nbk_pairs.hip).
//
// Three steps, NO global atomics (the global atomic pipe runs at
// ~25 G op/s regardless of locality, csrc/count_probe.hip):
//   count:   one block per chunk of `chunk` particles histograms its
//            keys in LDS and writes one row of the [chunks x buckets]
//            count matrix;
//   scan:    nbk_scan_matrix_i32 (nbk_sort.hip) turns the matrix into
//            per-chunk cursor seeds `bases` and the bucket edges;
//   scatter: each block re-reads its chunk and places the particles
//            from LDS cursors seeded with its row of `bases`, as SoA
//            planes x[] y[] z[] (+ mass[]).
// Order within a bucket is arbitrary.
//
// A sort is one KEY functor, passed by value as a kernel argument:
//   typedef ... index_t;                (the integer type of a bucket)
//   static constexpr bool two_keys;
//   index_t operator()(x, y, z) const;                (!two_keys)
//   index_t operator()(x, y, z, index_t* k2) const;   (two_keys: *k2 is
//       negative, or the bucket of the particle's second copy)
//   int64_t order_key(x, y, z) const;   (only for countsort_count's
//       DETECT: a total order whose inversions between neighbouring
//       lanes flag the input as scrambled)
// The extern "C" entry points validate their geometry, build the key
// and call countsort_count / countsort_scatter below.
#pragma once
#include "nbk_common.h"

// LDS ceiling of every sort histogram / cursor array / fine window, in
// int entries (160 KiB on gfx950)
constexpr int64_t NBK_SORT_LDS_INTS = 40960;

static inline void raise_lds(const void* fn, size_t bytes) {
    if (bytes > 64 * 1024)
        (void)hipFuncSetAttribute(fn,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// Block-wide exclusive scan of one int per thread: wave shfl scan, then
// a serial scan of the (<= 16) wave totals.  Returns the sum of `acc`
// over all lower threads.  blockDim.x must be a multiple of 64, at most
// 1024; every thread must call it, once per kernel (the wave totals
// live in one static LDS array that is read after the last barrier).
__device__ __forceinline__ int nbk_block_exclusive_scan(int acc) {
    __shared__ int wsum[16];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const int wave = t >> 6;
    int v = acc;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int w = 0; w < ((int)blockDim.x >> 6); w++) {
            const int x = wsum[w];
            wsum[w] = run;
            run += x;
        }
    }
    __syncthreads();
    return wsum[wave] + (v - acc);
}

// DETECT also flags (heuristically, lane-adjacent pairs) input that is
// not already in order_key order: scrambled -> *scrambled_flag = 1 (the
// caller skips the scatter for ordered input); the flag may be NULL.
template <class Key, bool DETECT>
__global__ void kcountsort_count(const double* __restrict__ pos, int64_t n,
                                 int chunk, Key key, int nbuck,
                                 int* __restrict__ mat,
                                 int* __restrict__ scrambled_flag)
{
    extern __shared__ int hist[];   // nbuck ints
    for (int b = threadIdx.x; b < nbuck; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    const int64_t beg = (int64_t)blockIdx.x * chunk;
    const int64_t end = (beg + chunk < n) ? beg + chunk : n;
    [[maybe_unused]] const int lane = threadIdx.x & 63;
    [[maybe_unused]] int out_of_order = 0;
    for (int64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
        const double x = pos[3 * i], y = pos[3 * i + 1],
                     z = pos[3 * i + 2];
        if constexpr (Key::two_keys) {
            typename Key::index_t k2;
            atomicAdd(&hist[key(x, y, z, &k2)], 1);
            if (k2 >= 0) atomicAdd(&hist[k2], 1);
        } else {
            atomicAdd(&hist[key(x, y, z)], 1);
        }
        if constexpr (DETECT) {
            if (scrambled_flag) {
                const int64_t b = key.order_key(x, y, z);
                const int64_t b_up = __shfl_up((long long)b, 1, 64);
                if (lane > 0 && b_up > b) out_of_order = 1;
            }
        }
    }
    if constexpr (DETECT) {
        if (out_of_order) atomicOr(scrambled_flag, 1);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < nbuck; b += blockDim.x)
        mat[(int64_t)blockIdx.x * nbuck + b] = hist[b];
}

// mass (and then om) may be NULL
template <class Key>
__global__ void kcountsort_scatter(const double* __restrict__ pos,
                                   const double* __restrict__ mass,
                                   int64_t n, int chunk, Key key, int nbuck,
                                   const int* __restrict__ bases,
                                   double* __restrict__ ox,
                                   double* __restrict__ oy,
                                   double* __restrict__ oz,
                                   double* __restrict__ om)
{
    extern __shared__ int cur[];    // nbuck running cursors
    for (int b = threadIdx.x; b < nbuck; b += blockDim.x)
        cur[b] = bases[(int64_t)blockIdx.x * nbuck + b];
    __syncthreads();
    const int64_t beg = (int64_t)blockIdx.x * chunk;
    const int64_t end = (beg + chunk < n) ? beg + chunk : n;
    for (int64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
        const double x = pos[3 * i], y = pos[3 * i + 1],
                     z = pos[3 * i + 2];
        typename Key::index_t k1, k2 = -1;
        if constexpr (Key::two_keys) k1 = key(x, y, z, &k2);
        else k1 = key(x, y, z);
        // (read after the key: a conditional load in front of it makes
        // the key wait for z and the mass as well, vmcnt(0))
        const double m = mass ? mass[i] : 0.0;
        const auto place = [&](typename Key::index_t k) {
            const int64_t t = (int64_t)atomicAdd(&cur[k], 1);
            ox[t] = x;
            oy[t] = y;
            oz[t] = z;
            if (mass) om[t] = m;
        };
        place(k1);
        if constexpr (Key::two_keys) {
            if (k2 >= 0) place(k2);
        }
    }
}

// ---- host side ---------------------------------------------------------

// the requirements every count-matrix step shares; `who` names the
// extern "C" entry point in the error string
static inline int countsort_check(const char* who, int64_t n, int chunk,
                                  int64_t nbuck)
{
    if (n < 0 || n >= ((int64_t)1 << 31) || chunk < 1) {
        NBK_SET_ERR("%s: n=%lld chunk=%d (needs 0 <= n < 2^31, "
                    "chunk >= 1)", who, (long long)n, chunk);
        return NBK_ERR_ARG;
    }
    if (nbuck < 1 || nbuck > NBK_SORT_LDS_INTS) {
        NBK_SET_ERR("%s: %lld buckets, the LDS histogram holds 1 to %lld",
                    who, (long long)nbuck, (long long)NBK_SORT_LDS_INTS);
        return NBK_ERR_ARG;
    }
    return NBK_OK;
}

template <class Key, bool DETECT>
int countsort_count(const char* who, const double* pos_aos, int64_t n,
                    int chunk, const Key& key, int64_t nbuck, int* mat,
                    int* scrambled_flag, void* stream)
{
    const int rc = countsort_check(who, n, chunk, nbuck);
    if (rc != NBK_OK || n == 0) return rc;
    const int64_t nblocks = (n + chunk - 1) / chunk;
    const size_t lds = (size_t)nbuck * sizeof(int);
    raise_lds(reinterpret_cast<const void*>(&kcountsort_count<Key, DETECT>),
              lds);
    hipLaunchKernelGGL((kcountsort_count<Key, DETECT>),
                       dim3((uint32_t)nblocks), dim3(1024), lds,
                       (hipStream_t)stream, pos_aos, n, chunk, key,
                       (int)nbuck, mat, scrambled_flag);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

// the output planes are n_out apart (n_out > n when keys duplicate)
template <class Key>
int countsort_scatter(const char* who, const double* pos_aos,
                      const double* mass, int64_t n, int chunk,
                      const Key& key, int64_t nbuck, const int* bases,
                      int64_t n_out, double* pos_out, double* mass_out,
                      void* stream)
{
    const int rc = countsort_check(who, n, chunk, nbuck);
    if (rc != NBK_OK || n == 0) return rc;
    const int64_t nblocks = (n + chunk - 1) / chunk;
    const size_t lds = (size_t)nbuck * sizeof(int);
    raise_lds(reinterpret_cast<const void*>(&kcountsort_scatter<Key>), lds);
    hipLaunchKernelGGL(kcountsort_scatter<Key>, dim3((uint32_t)nblocks),
                       dim3(1024), lds, (hipStream_t)stream, pos_aos, mass,
                       n, chunk, key, (int)nbuck, bases, pos_out,
                       pos_out + n_out, pos_out + 2 * n_out, mass_out);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}
