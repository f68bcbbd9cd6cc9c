// Window-deposit ("paint") kernels — the #1 op of the path (replaces
// pmesh's Cython scatter called at
// nbodykit/source/mesh/catalog.py:287,295-296).  Two strategies:
//
// 1. kpaint_gather (+optional fused z-FFT): the BIG-MESH path, fed by
//    the atomic-free two-level locality sort (nbk_sort.hip).  Each
//    block owns an exclusive LDS mesh tile (RG y-rows x full z of one
//    x-plane), gathers the source rows whose stencils can reach it via
//    the sort's row table, deposits with LDS ds_add_f64 and flushes
//    with plain stores — ZERO global atomics (the global atomic pipe
//    measures ~25 G op/s regardless of locality, csrc/count_probe.hip,
//    which bounded the scatter kernel below at 47 ms for 1e9 CIC).
//    The DOFFT variant runs the forward z-FFT on the tile's rows
//    before flushing, so the real mesh never exists in HBM
//    (CatalogMesh.to_complex_field).
//
// 2. kpaint: the scatter fallback for small chunks/meshes.  One thread
//    per particle in wave-contiguous order; deposits use hardware f64
//    global atomics (-munsafe-fp-atomics => global_atomic_add_f64)
//    with a wave-level segmented merge: adjacent lanes holding the
//    same target address combine via a shfl prefix-sum and only the
//    run tail issues the atomic (probe: clumpy 167 -> 45 ms).
//
// Window shapes are the B-splines fixed in-tree by their Fourier duals
// (source/mesh/catalog.py:453-594; Jing 2005 eq. 18, p = 2/3/4);
// a particle exactly on a grid point deposits its full mass there.
#include "nbk_common.h"
#include <type_traits>

namespace {

// one deposit with wave-segmented address merge; addr < 0 = inactive
// lane (tail of the grid or ghost-owned cell) — must still participate
// in the shuffles.
__device__ __forceinline__ void merged_deposit(double* __restrict__ mesh,
                                               long long addr, double val,
                                               int lane) {
    // segment = maximal CONTIGUOUS run of equal addresses.  A plain
    // "same addr at distance d" guard would also fold non-adjacent
    // duplicates ([A A B A] merging the stray A into the first run);
    // the head-bounded Hillis-Steele scan below only sums within the
    // lane's own run.
    const long long a_up1 = __shfl_up(addr, 1, 64);
    const bool head = (lane == 0) || (a_up1 != addr);
    const unsigned long long heads = __ballot(head);
    const unsigned long long below = heads
        & (~0ULL >> (63 - lane));          // head bits at lanes <= lane
    const int myhead = 63 - __clzll(below);
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double v_up = __shfl_up(val, d, 64);
        if (lane - d >= myhead) val += v_up;
    }
    const bool next_head = ((lane < 63)
                            && ((heads >> (lane + 1)) & 1ULL));
    if (addr >= 0 && (lane == 63 || next_head))
        atomicAdd(&mesh[addr], val);
}

// readout-only id of the nearest-grid-point "window" (no weights, not a
// paint window; follows NBK_WINDOW_PCS)
constexpr int WINDOW_NNB = 3;

// cells per axis a window's stencil covers
template <int WINDOW>
constexpr int window_support() {
    return (WINDOW == NBK_WINDOW_CIC) ? 2
         : (WINDOW == NBK_WINDOW_TSC) ? 3 : 4;
}

// unwrapped base cell (first cell of the stencil) of mesh coordinate u:
// TSC is centred on the nearest grid point, CIC and PCS on the cell
template <int WINDOW>
__device__ __forceinline__ int64_t base_cell(double u) {
    const double f = floor(WINDOW == NBK_WINDOW_TSC ? u + 0.5 : u);
    return (int64_t)f - (WINDOW == NBK_WINDOW_CIC ? 0 : 1);
}

// per-axis window weights + unwrapped base cell: the one definition of
// the three window shapes, shared by every paint kernel and the readout
// (their adjointness rests on it).  The three axes are interleaved on
// purpose — the gather kernel's instruction schedule was tuned on it.
template <int WINDOW, int SUP>
__device__ __forceinline__ void paint_weights(double u0, double u1,
                                              double u2,
                                              double (&w0)[SUP],
                                              double (&w1)[SUP],
                                              double (&w2)[SUP],
                                              int64_t& b0, int64_t& b1,
                                              int64_t& b2) {
    if (WINDOW == NBK_WINDOW_CIC) {
        const double f0 = floor(u0), f1 = floor(u1), f2 = floor(u2);
        b0 = base_cell<WINDOW>(u0); b1 = base_cell<WINDOW>(u1);
        b2 = base_cell<WINDOW>(u2);
        w0[SUP - 1] = u0 - f0; w0[0] = 1.0 - (u0 - f0);
        w1[SUP - 1] = u1 - f1; w1[0] = 1.0 - (u1 - f1);
        w2[SUP - 1] = u2 - f2; w2[0] = 1.0 - (u2 - f2);
    } else if (WINDOW == NBK_WINDOW_TSC) {
        const double f0 = floor(u0 + 0.5), f1 = floor(u1 + 0.5),
                     f2 = floor(u2 + 0.5);
        b0 = base_cell<WINDOW>(u0); b1 = base_cell<WINDOW>(u1);
        b2 = base_cell<WINDOW>(u2);
        #pragma unroll
        for (int d = 0; d < 3; d++) {
            const double s0 = u0 - (f0 + d - 1);
            const double s1 = u1 - (f1 + d - 1);
            const double s2 = u2 - (f2 + d - 1);
            const double a0 = fabs(s0), a1 = fabs(s1), a2 = fabs(s2);
            w0[d] = a0 < 0.5 ? 0.75 - s0 * s0
                             : 0.5 * (1.5 - a0) * (1.5 - a0);
            w1[d] = a1 < 0.5 ? 0.75 - s1 * s1
                             : 0.5 * (1.5 - a1) * (1.5 - a1);
            w2[d] = a2 < 0.5 ? 0.75 - s2 * s2
                             : 0.5 * (1.5 - a2) * (1.5 - a2);
        }
    } else {   // PCS
        const double f0 = floor(u0), f1 = floor(u1), f2 = floor(u2);
        b0 = base_cell<WINDOW>(u0); b1 = base_cell<WINDOW>(u1);
        b2 = base_cell<WINDOW>(u2);
        #pragma unroll
        for (int d = 0; d < 4; d++) {
            const double s0 = fabs(u0 - (f0 + d - 1));
            const double s1 = fabs(u1 - (f1 + d - 1));
            const double s2 = fabs(u2 - (f2 + d - 1));
            w0[d] = s0 < 1.0
                ? (4.0 - 6.0 * s0 * s0 + 3.0 * s0 * s0 * s0) / 6.0
                : (2.0 - s0) * (2.0 - s0) * (2.0 - s0) / 6.0;
            w1[d] = s1 < 1.0
                ? (4.0 - 6.0 * s1 * s1 + 3.0 * s1 * s1 * s1) / 6.0
                : (2.0 - s1) * (2.0 - s1) * (2.0 - s1) / 6.0;
            w2[d] = s2 < 1.0
                ? (4.0 - 6.0 * s2 * s2 + 3.0 * s2 * s2 * s2) / 6.0
                : (2.0 - s2) * (2.0 - s2) * (2.0 - s2) / 6.0;
        }
    }
}

template <int WINDOW>
__global__ void kpaint(const double* __restrict__ px,
                       const double* __restrict__ py,
                       const double* __restrict__ pz,
                       const double* __restrict__ mass, int64_t n,
                       int64_t n0, int64_t n1, int64_t n2,
                       double invH0, double invH1, double invH2,
                       double shift,
                       double* __restrict__ mesh,
                       int64_t x0, int64_t nx_local)
{
    constexpr int SUP = window_support<WINDOW>();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    // iterate whole waves so the shuffle stays collective at the tail
    const int64_t wbase0 = blockIdx.x * (int64_t)blockDim.x
        + (threadIdx.x & ~63);
    for (int64_t wb = wbase0; wb < n; wb += stride) {
        const int64_t i = wb + lane;
        const bool valid = i < n;

        const double u0 = valid ? px[i] * invH0 + shift : 0.0;
        const double u1 = valid ? py[i] * invH1 + shift : 0.0;
        const double u2 = valid ? pz[i] * invH2 + shift : 0.0;
        const double m = valid ? (mass ? mass[i] : 1.0) : 0.0;

        double w0[SUP], w1[SUP], w2[SUP];
        int64_t b0, b1, b2;   // base cell per axis
        paint_weights<WINDOW, SUP>(u0, u1, u2, w0, w1, w2, b0, b1, b2);

        #pragma unroll
        for (int dx = 0; dx < SUP; dx++) {
            const int64_t gx = wrap_idx(b0 + dx, n0);
            // ghost-owned cells: keep the lane in the wave ops with a
            // unique negative sentinel so it never merges or deposits
            const bool in_slab = valid && gx >= x0 && gx < x0 + nx_local;
            const int64_t lx = gx - x0;
            #pragma unroll
            for (int dy = 0; dy < SUP; dy++) {
                const int64_t gy = wrap_idx(b1 + dy, n1);
                const double wxy = w0[dx] * w1[dy] * m;
                #pragma unroll
                for (int dz = 0; dz < SUP; dz++) {
                    const int64_t gz = wrap_idx(b2 + dz, n2);
                    const long long addr = in_slab
                        ? (long long)((lx * n1 + gy) * n2 + gz)
                        : (long long)(-1 - lane);
                    merged_deposit(mesh, addr, wxy * w2[dz], lane);
                }
            }
        }
    }
}

// LDS-windowed paint for CELL-SORTED input (instantiated for PCS only,
// see nbk_paint_sorted_f64) — each block owns a contiguous particle
// run, accumulates all support^3 deposits into an LDS window covering
// the run's (x, y) line span x the full z axis (native ds_add_f64),
// then flushes the window once with a sequential stream of global
// atomics.  Cuts global atomics from 64 per PCS particle to ~window/run
// and makes them address-sequential — the direct kernel is
// atomic-issue-bound there (41 vs 127 Gatomic/s for CIC's
// lane-sequential pattern).  Blocks whose particles span a
// window larger than the LDS budget (scrambled input must never reach
// this kernel) fall back to direct per-particle atomics.
#define NBK_TILE_PPB 1024          /* particles per block */
#define NBK_TILE_MAX_CELLS 8192    /* 64 KiB of f64 LDS   */

template <int WINDOW>
__global__ void kpaint_tiled(const double* __restrict__ px,
                             const double* __restrict__ py,
                             const double* __restrict__ pz,
                             const double* __restrict__ mass, int64_t n,
                             int64_t n0, int64_t n1, int64_t n2,
                             double invH0, double invH1, double invH2,
                             double shift,
                             double* __restrict__ mesh,
                             int64_t x0, int64_t nx_local)
{
    constexpr int SUP = window_support<WINDOW>();
    __shared__ double buf[NBK_TILE_MAX_CELLS];
    __shared__ int s_min0, s_max0, s_min1, s_max1;

    const int64_t ibeg = (int64_t)blockIdx.x * NBK_TILE_PPB;
    const int64_t iend = min(ibeg + NBK_TILE_PPB, n);

    if (threadIdx.x == 0) {
        s_min0 = INT_MAX; s_max0 = INT_MIN;
        s_min1 = INT_MAX; s_max1 = INT_MIN;
    }
    __syncthreads();

    // pass 1: the block's unwrapped base-cell bounding box in (x, y)
    int mn0 = INT_MAX, mx0 = INT_MIN, mn1 = INT_MAX, mx1 = INT_MIN;
    for (int64_t i = ibeg + threadIdx.x; i < iend; i += blockDim.x) {
        const double u0 = px[i] * invH0 + shift;
        const double u1 = py[i] * invH1 + shift;
        const int b0 = (int)base_cell<WINDOW>(u0);
        const int b1 = (int)base_cell<WINDOW>(u1);
        mn0 = min(mn0, b0); mx0 = max(mx0, b0);
        mn1 = min(mn1, b1); mx1 = max(mx1, b1);
    }
    atomicMin(&s_min0, mn0); atomicMax(&s_max0, mx0);
    atomicMin(&s_min1, mn1); atomicMax(&s_max1, mx1);
    __syncthreads();

    const int wx = s_max0 - s_min0 + SUP;
    const int wy = s_max1 - s_min1 + SUP;
    const int64_t cells = (int64_t)wx * wy * n2;
    const bool use_lds = (ibeg < iend) && cells > 0
        && cells <= NBK_TILE_MAX_CELLS;

    if (!use_lds) {
        // fallback: direct per-particle atomics (rare for sorted input)
        for (int64_t i = ibeg + threadIdx.x; i < iend; i += blockDim.x) {
            const double u0 = px[i] * invH0 + shift;
            const double u1 = py[i] * invH1 + shift;
            const double u2 = pz[i] * invH2 + shift;
            const double m = mass ? mass[i] : 1.0;
            double w0[SUP], w1[SUP], w2[SUP];
            int64_t b0, b1, b2;
            paint_weights<WINDOW, SUP>(u0, u1, u2, w0, w1, w2, b0, b1, b2);
            for (int dx = 0; dx < SUP; dx++) {
                const int64_t gx = wrap_idx(b0 + dx, n0);
                if (gx < x0 || gx >= x0 + nx_local) continue;
                for (int dy = 0; dy < SUP; dy++) {
                    const int64_t gy = wrap_idx(b1 + dy, n1);
                    const double wxy = w0[dx] * w1[dy] * m;
                    for (int dz = 0; dz < SUP; dz++) {
                        const int64_t gz = wrap_idx(b2 + dz, n2);
                        atomicAdd(&mesh[((gx - x0) * n1 + gy) * n2 + gz],
                                  wxy * w2[dz]);
                    }
                }
            }
        }
        return;
    }

    for (int64_t w = threadIdx.x; w < cells; w += blockDim.x)
        buf[w] = 0.0;
    __syncthreads();

    // pass 2: deposit into the LDS window
    for (int64_t i = ibeg + threadIdx.x; i < iend; i += blockDim.x) {
        const double u0 = px[i] * invH0 + shift;
        const double u1 = py[i] * invH1 + shift;
        const double u2 = pz[i] * invH2 + shift;
        const double m = mass ? mass[i] : 1.0;
        double w0[SUP], w1[SUP], w2[SUP];
        int64_t b0, b1, b2;
        paint_weights<WINDOW, SUP>(u0, u1, u2, w0, w1, w2, b0, b1, b2);
        const int lx = (int)(b0 - s_min0);
        const int ly = (int)(b1 - s_min1);
        for (int dx = 0; dx < SUP; dx++) {
            for (int dy = 0; dy < SUP; dy++) {
                const double wxy = w0[dx] * w1[dy] * m;
                const int64_t base =
                    ((int64_t)(lx + dx) * wy + (ly + dy)) * n2;
                for (int dz = 0; dz < SUP; dz++) {
                    const int64_t gz = wrap_idx(b2 + dz, n2);
                    unsafeAtomicAdd(&buf[base + gz], wxy * w2[dz]);
                }
            }
        }
    }
    __syncthreads();

    // pass 3: flush (sequential global atomics; skip empty cells)
    for (int64_t w = threadIdx.x; w < cells; w += blockDim.x) {
        const double v = buf[w];
        if (v == 0.0) continue;
        const int64_t gz = w % n2;
        const int64_t wyidx = (w / n2) % wy;
        const int64_t wxidx = w / ((int64_t)n2 * wy);
        const int64_t gx = wrap_idx(s_min0 + wxidx, n0);
        if (gx < x0 || gx >= x0 + nx_local) continue;
        const int64_t gy = wrap_idx(s_min1 + wyidx, n1);
        atomicAdd(&mesh[((gx - x0) * n1 + gy) * n2 + gz], v);
    }
}

// ---- register-resident z-FFT of one tile row (kpaint_gather, DOFFT) ----
//
// One wave transforms one row of m = 64 R packed complex points
// (R = 1, 2, 4, 8: n2 = 128 ... 1024) in place in the row's LDS, holding
// the points in registers, max(R, 8) per lane, between the passes:
//
//   m = R * 8 * 8.  Input index n = lane + 64 j, output index
//   k = 8R c + R d + k1   (j, k1 < R;  lane = 8a + b;  a, b, c, d < 8)
//
//   pass 1  lane            reads z[lane + 64 j] (natural order: no
//                           bit-reversal pass), R-point DFT over j -> k1,
//                           times W_m^(lane k1)
//   pass 2  lane' = 8k1 + b 8-point DFT over a -> d, times W_64^(b d)
//   pass 3  lane" = Rd + k1 8-point DFT over b -> c, written to
//                           z[lane" + 8R c] = z[k]: natural order
//
// Passes 2 and 3 run on the first 8R lanes (all 64 at n2 = 1024).  The
// butterflies are straight-line register code whose only constants are
// +-sqrt(1/2); the inter-pass twiddles depend on the lane alone and are
// loaded once per block (zfft_load_twiddles).  A row makes 4 LDS round
// trips: read, two exchanges, natural-order write (+ the split's reads).
//
// Exchange slots (16-byte units, relative to the row), all within
// [0, m) — the exchanges are in place:
//   exchange 1: slot(k1, l) = 64 k1 + (l ^ 8 (k1>>1 & 1)),   l = 8a + b
//   exchange 2: slot(b, q)  = 8R b + (q ^ b),                q = Rd + k1
// LDS banking on gfx950: a 16-byte read is served in four groups of 16
// lanes ({0-3,12-15,20-27}, {4-11,16-19,28-31}, the same + 32) over 16
// slots; a 16-byte write in eight groups of 8 consecutive lanes over 8
// slots.  Writes of exchange 1 (fixed k1), reads of exchange 2 (fixed b)
// and the final writes (fixed c) put consecutive lanes on consecutive
// slots, XORed with a constant below 16: conflict-free.  Reads of
// exchange 1 (fixed a, lane' = 8k1 + b): slot mod 16 is
// b + 8 (a ^ (k1>>1)), and each read group holds b = 0..3 and b = 4..7
// once for an even and once for an odd k1>>1 — 16 distinct slots.
// Writes of exchange 2 (fixed d, lane' = 8k1 + b): within a group k1 is
// fixed and slot mod 8 = (const ^ b), b = 0..7 — 8 distinct slots.
// Every exchange is conflict-free (1-way) for R = 1, 2, 4, 8, counted by
// enumeration of the groups above.
//
// A wave owns its row: the lanes run in lockstep and LDS operations
// complete in program order, so the passes need no block barrier; the
// wave_barrier pins the compiler's schedule across the cross-lane
// dependences, as in the LDS radix-4 network this replaces.
typedef double nbk_f64x2 __attribute__((ext_vector_type(2)));

// 16-byte LDS access of one complex point (the rows are 16-byte aligned)
__device__ __forceinline__ cdouble zfft_ld(const cdouble* z, int i) {
    const nbk_f64x2 v = *reinterpret_cast<const nbk_f64x2*>(z + i);
    return {v.x, v.y};
}
__device__ __forceinline__ void zfft_st(cdouble* z, int i, cdouble a) {
    const nbk_f64x2 v = {a.re, a.im};
    *reinterpret_cast<nbk_f64x2*>(z + i) = v;
}

// forward R-point DFT in registers, natural order in and out
template <int R>
__device__ __forceinline__ void zfft_butterfly(cdouble (&v)[R]) {
    static_assert(R == 1 || R == 2 || R == 4 || R == 8, "radix");
    if constexpr (R == 2) {
        const cdouble a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 4) {
        const cdouble s0 = cadd(v[0], v[2]), s1 = csub(v[0], v[2]);
        const cdouble s2 = cadd(v[1], v[3]), s3 = csub(v[1], v[3]);
        const cdouble is3 = {s3.im, -s3.re};              // -i * s3
        v[0] = cadd(s0, s2);
        v[1] = cadd(s1, is3);
        v[2] = csub(s0, s2);
        v[3] = csub(s1, is3);
    } else if constexpr (R == 8) {
        cdouble e[4] = {v[0], v[2], v[4], v[6]};
        cdouble o[4] = {v[1], v[3], v[5], v[7]};
        zfft_butterfly<4>(e);
        zfft_butterfly<4>(o);
        constexpr double h = 0.70710678118654752440;       // sqrt(1/2)
        // o[k] *= W_8^k
        o[1] = {(o[1].re + o[1].im) * h, (o[1].im - o[1].re) * h};
        o[2] = {o[2].im, -o[2].re};
        o[3] = {(o[3].im - o[3].re) * h, -(o[3].re + o[3].im) * h};
        #pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = cadd(e[k], o[k]);
            v[k + 4] = csub(e[k], o[k]);
        }
    }
}

// the inter-pass twiddles of one lane; they depend on the lane and n2
// only and serve every row the wave transforms.  Only the powers 1, 2
// and 4 of each pass's base twiddle are kept (24 VGPRs, not 56: the
// n2 = 1024 instance has to fit 128 with its 8 points and the
// butterfly's temporaries); zfft_twiddle forms the other powers as
// products where it uses them.
struct zfft_twiddles {
    cdouble w1[3];    // W_m^(lane k1), k1 = 1, 2, 4 (those below R)
    cdouble w2[3];    // W_64^(b d), b = lane & 7, d = 1, 2, 4
};

// v[k] *= w^k, k = 1..N-1, from p = (w, w^2, w^4)
template <int N>
__device__ __forceinline__ void zfft_twiddle(cdouble (&v)[N],
                                             const cdouble (&p)[3]) {
    v[1] = cmul(v[1], p[0]);
    if constexpr (N > 2) {
        const cdouble p3 = cmul(p[0], p[1]);
        v[2] = cmul(v[2], p[1]);
        v[3] = cmul(v[3], p3);
        if constexpr (N > 4) {
            v[4] = cmul(v[4], p[2]);
            v[5] = cmul(v[5], cmul(p[0], p[2]));
            v[6] = cmul(v[6], cmul(p[1], p[2]));
            v[7] = cmul(v[7], cmul(p3, p[2]));
        }
    }
}

template <int LOGM>
__device__ __forceinline__ void zfft_load_twiddles(
    zfft_twiddles& tw, const cdouble* __restrict__ table /* W_n2,
        entries 0..m */, int lane)
{
    constexpr int R = 1 << (LOGM - 6), m = 64 * R;
    // W_n2^e for 0 <= e < n2 from the half table: W^(e) = -W^(e - m)
    auto W = [&](int e) -> cdouble {
        const cdouble w = table[e > m ? e - m : e];
        return e > m ? cdouble{-w.re, -w.im} : w;
    };
    #pragma unroll
    for (int i = 0; i < 3; i++) {
        if ((1 << i) < R) tw.w1[i] = W(2 * lane << i);
        tw.w2[i] = W(2 * R * (lane & 7) << i);
    }
}

// forward complex FFT of the m points z[0..m), natural order in and out
template <int LOGM>
__device__ __forceinline__ void zfft_row(cdouble* z, int lane,
                                         zfft_twiddles tw)
{
    constexpr int R = 1 << (LOGM - 6), L2 = 8 * R;
    // The lane and the kept twiddle powers pass through an empty asm
    // once per row: what is derived from them (the exchange slots, the
    // twiddle products) is then computed where it is used instead of
    // being hoisted out of the caller's row loop into some 50 more
    // registers, which the n2 = 1024 instance does not have.
    asm volatile("" : "+v"(lane));
    #pragma unroll
    for (int i = 0; i < 3; i++) {
        if ((1 << i) < R)
            asm volatile("" : "+v"(tw.w1[i].re), "+v"(tw.w1[i].im));
        asm volatile("" : "+v"(tw.w2[i].re), "+v"(tw.w2[i].im));
    }
    if constexpr (R > 1) {
        // pass 1 (at R = 1 it and its exchange are the identity)
        cdouble v[R];
        #pragma unroll
        for (int j = 0; j < R; j++) v[j] = zfft_ld(z, lane + 64 * j);
        zfft_butterfly<R>(v);
        zfft_twiddle<R>(v, tw.w1);
        __builtin_amdgcn_wave_barrier();
        #pragma unroll
        for (int k1 = 0; k1 < R; k1++)
            zfft_st(z, 64 * k1 + (lane ^ (8 * ((k1 >> 1) & 1))), v[k1]);
        __builtin_amdgcn_wave_barrier();
    }
    const bool active = (L2 == 64) || lane < L2;
    if (active) {
        // pass 2
        const int k1 = lane >> 3, b = lane & 7;
        const int base = 64 * k1 + (b ^ (8 * ((k1 >> 1) & 1)));
        cdouble u[8];
        #pragma unroll
        for (int a = 0; a < 8; a++) u[a] = zfft_ld(z, base ^ (8 * a));
        zfft_butterfly<8>(u);
        zfft_twiddle<8>(u, tw.w2);
        #pragma unroll
        for (int d = 0; d < 8; d++)
            zfft_st(z, L2 * b + ((R * d + k1) ^ b), u[d]);
    }
    __builtin_amdgcn_wave_barrier();
    if (active) {
        // pass 3
        cdouble s[8];
        #pragma unroll
        for (int b = 0; b < 8; b++) s[b] = zfft_ld(z, L2 * b + (lane ^ b));
        zfft_butterfly<8>(s);
        #pragma unroll
        for (int c = 0; c < 8; c++) zfft_st(z, lane + L2 * c, s[c]);
    }
    __builtin_amdgcn_wave_barrier();
}

// OWNERSHIP-GATHER paint for cell-sorted input with a row table
// (nbk_bucket_fine_f64's rowtab): each block owns an exclusive mesh
// tile of RG y-rows x full z of ONE x-plane, accumulates every deposit
// that lands in its tile from the (few) source rows whose stencils can
// reach it, and flushes with PLAIN stores — zero global atomics.  The
// global atomic pipe measures ~25 G ops/s (csrc/count_probe.hip), which
// bounds the scatter kernels above at ~8 atomics/particle; here the
// deposits are LDS ds_add_f64 and the HBM traffic is ~2.1x the particle
// reads plus one mesh write.
// DOFFT: after the deposits the tile's rows (full z-lines) are
// transformed in place (packed-real complex FFT + untwiddle split as
// kfft_r2c_z; zfft_row above for n2 = 128 ... 1024, the LDS radix-4
// network otherwise) and the z half-spectrum is written directly — the real
// mesh never touches HBM.  The row stride is padded (+4 doubles) so the
// butterflies of different rows land in different LDS banks.
// PT: compile-time plane count when > 0 (PT=1 restores the
// single-plane kernel's indexing with zero multi-plane overhead — the
// CIC path is VALU+read balanced and pays for every extra op);
// PT=0 = runtime P.
// ZF (DOFFT only): log2(n2/2) when the row transform is the
// register-resident zfft_row (n2 = 128 ... 1024), 0 = the LDS radix-4
// network (every other length).
template <int WINDOW, bool DOFFT, int PT, int ZF>
__global__ void kpaint_gather(const double* __restrict__ px,
                              const double* __restrict__ py,
                              const double* __restrict__ pz,
                              const double* __restrict__ mass, int64_t n,
                              int64_t n0, int64_t n1, int64_t n2,
                              double invH0, double invH1, double invH2,
                              double shift,
                              const int* __restrict__ rowtab,
                              double* __restrict__ mesh, /* or z-spectrum
                                  (nx_local, n1, n2/2+1) cdouble when
                                  DOFFT */
                              int64_t x0, int64_t nx_local,
                              int RG, int P, int xlo, int xhi,
                              int accumulate,
                              const cdouble* __restrict__ table /* W_n2 */,
                              double scale,
                              int gs, /* >= 0: rowtab is the PAIR-BUCKET
                                  table [(n0/2)*(n1>>gs)+1] of the
                                  duplicating sort (1<<gs == RG); the
                                  tile reads whole (pair, group) ranges
                                  and the deposit masks drop the
                                  out-of-tile copies.  -1: per-row
                                  table (nbk_bucket_fine_f64) */
                              int phases /* perf decomposition only
                                  (NBK_PAINT_PHASES): bit1 deposits,
                                  bit2 FFT+flush; 3 = real kernel */)
{
    constexpr int SUP = window_support<WINDOW>();
    if (PT > 0) P = PT;                  // compile-time plane count
    // P * RG * (n2 [+4]) doubles; rows start on 16 bytes
    extern __shared__ __attribute__((aligned(16))) double tile[];
    const int64_t sp = DOFFT ? n2 + 4 : n2;   // padded row stride
    const int64_t tiles_per_plane = n1 / RG;
    // block owns P consecutive x-planes x RG y-rows: a source plane
    // feeding several owned planes is READ ONCE for all of them, so the
    // per-particle read factor drops from (1 + span) planes to
    // (P + span)/P — the host picks P ~ RG to balance the two halo
    // factors within the 160 KiB LDS budget
    const int64_t px0 = x0 + (blockIdx.x / tiles_per_plane) * P;
    const int64_t r0 = (blockIdx.x % tiles_per_plane) * RG;
    const int T = blockDim.x;
    const int t = threadIdx.x;
    const int64_t win = (int64_t)P * RG * sp;

    for (int64_t w = t; w < win; w += T) tile[w] = 0.0;
    __syncthreads();

    // The particle loop is software-pipelined through registers: each
    // thread stages a batch of U particles (3-4 loads each, issued back
    // to back) and the loads of batch k+1 are issued BEFORE batch k's
    // weights, masks and ds_add_f64, so the HBM read stream and the LDS
    // atomic pipe work at the same time — one block per CU is resident
    // (the tile fills the LDS), so no other block would cover the wait.
    // The two batches ping-pong (no register copies) and the pipeline
    // runs across the tile's ranges: it fills once per tile, not once
    // per range.  A batch never spans two ranges; every load is
    // predicated on its own range's end.
    constexpr int U = (WINDOW == NBK_WINDOW_CIC) ? 4 : 2;
    struct Batch {
        double x[U], y[U], z[U], m[U];   // m only with a mass array
        uint32_t cnt;                 // slot u of thread t holds a
                                      // particle iff u*T + t < cnt
    };

    // row intervals (wrapped) whose particles can deposit into the tile
    const int64_t rspan = (int64_t)RG + (xhi - xlo);
    // row-table mode: the reachable rows [ra, rb] (the same for every
    // source plane); ra > rb = the interval wraps and is read as
    // [ra, n1) then [0, rb]
    const int64_t ra = wrap_idx(r0 + xlo, n1);
    const int64_t rb = wrap_idx(r0 + RG - 1 + xhi, n1);
    int64_t prev_pair = -1;
    // The walk covers P + (xhi - xlo) consecutive source planes.  On a
    // mesh thinner than that it would wrap past its own start and
    // deposit the revisited planes twice: stop after n0 planes (every
    // plane once) — the x analogue of the rspan >= n1 case below.
    // Wave-uniform; a no-op whenever n0 >= P + span.
    const int dp_hi = ((int64_t)P + (xhi - xlo) > n0)
        ? (int)(xlo + n0 - 1) : P - 1 + xhi;
    const int64_t npairs = n0 >> 1;       // pair mode: distinct buckets
    int64_t pairs_read = 0;
    int dp = xlo;
    int64_t tail_p = -1;      // plane whose wrapped second interval waits
    // the next range [i0, i1) of sorted particles this tile reads;
    // wave-uniform (scalar table loads), false when the walk is over
    auto next_range = [&](uint32_t& i0, uint32_t& i1) -> bool {
        if (tail_p >= 0) {
            i0 = rowtab[tail_p * n1];
            i1 = rowtab[tail_p * n1 + rb + 1];
            tail_p = -1;
            return true;
        }
        while (dp <= dp_hi) {
            const int64_t p = wrap_idx(px0 + dp, n0);
            dp++;
            if (gs >= 0) {
                // PAIR-BUCKET mode: the duplicating sort already placed
                // a copy of every stencil-relevant particle in this
                // tile's own (pair, group) bucket — one contiguous
                // range, no halo-row lookups.  Consecutive source
                // planes share a pair: read each pair once.  (prev_pair
                // only catches neighbours: a walk over all n0 planes
                // that starts on an odd plane ends in its first pair
                // again — the count of distinct pairs stops it there.)
                const int64_t q = p >> 1;
                if (q == prev_pair) continue;
                if (pairs_read == npairs) { dp = dp_hi + 1; break; }
                prev_pair = q;
                pairs_read++;
                const int64_t bidx = q * (n1 >> gs) + (r0 >> gs);
                i0 = rowtab[bidx];
                i1 = rowtab[bidx + 1];
            } else if (rspan >= n1) {
                i0 = rowtab[p * n1];
                i1 = rowtab[p * n1 + n1];
            } else if (ra <= rb) {
                i0 = rowtab[p * n1 + ra];
                i1 = rowtab[p * n1 + rb + 1];
            } else {
                i0 = rowtab[p * n1 + ra];
                i1 = rowtab[p * n1 + n1];
                tail_p = p;
            }
            return true;
        }
        return false;
    };

    // unread part [ri, re) of the current range.  The tables are int32
    // (so is every index), and 32-bit scalars keep the walk on the
    // scalar unit: a 64-bit scalar compare is done in vector registers,
    // and a vector temporary that lands on the destination of a load
    // in flight makes the compiler wait for it, vmcnt(0).
    uint32_t ri = 0, re = 0;
    bool more = true;         // ranges left in the walk
    // issue the loads of the next non-empty batch; false = no particles
    // left.  Slot u of thread t holds particle i0 + u*T + t (coalesced
    // per slot, as the unpipelined loop read them).
    auto issue = [&](Batch& b, auto mass_tag) -> bool {
        while (more && ri >= re) more = next_range(ri, re);
        // After the last batch the same loads are still issued, through
        // empty descriptors (every lane dropped, no memory traffic): a
        // path that issued none would make the compiler's count of
        // loads in flight at the consumer collapse to the minimum over
        // paths, i.e. wait for the prefetched batch too.
        if (!more) ri = re = 0;
        // descriptors over the batch's part of the range only: a slot
        // at or past the range's end is dropped by the bounds check —
        // nothing is read beyond `re`, the array may end there
        const uint32_t left = re - ri, full = (uint32_t)(U * T);
        b.cnt = left < full ? left : full;
        const uint32_t bytes = b.cnt * 8u;
        const __amdgpu_buffer_rsrc_t rx = nbk_buffer_rsrc(px + ri, bytes);
        const __amdgpu_buffer_rsrc_t ry = nbk_buffer_rsrc(py + ri, bytes);
        const __amdgpu_buffer_rsrc_t rz = nbk_buffer_rsrc(pz + ri, bytes);
        #pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t off = (uint32_t)(u * T + t) * 8u;
            b.x[u] = nbk_buffer_load_f64(rx, off);
            b.y[u] = nbk_buffer_load_f64(ry, off);
            b.z[u] = nbk_buffer_load_f64(rz, off);
        }
        if constexpr (decltype(mass_tag)::value) {
            const __amdgpu_buffer_rsrc_t rm =
                nbk_buffer_rsrc(mass + ri, bytes);
            #pragma unroll
            for (int u = 0; u < U; u++)
                b.m[u] = nbk_buffer_load_f64(
                    rm, (uint32_t)(u * T + t) * 8u);
        }
        ri += full;
        return more;
    };

    // The power-of-two test of the index wrap is taken once, around two
    // instances of the loop (wrap_idx re-tests n on each of its up to
    // 14 calls per particle); non-power-of-two meshes keep the generic
    // 64-bit modulo.  So is the test for a mass array: with a uniform
    // branch between a batch's loads, the two paths issue different
    // numbers of loads and the counted waits fall to the smaller.
    const uint32_t um0 = (uint32_t)n0 - 1, um1 = (uint32_t)n1 - 1,
                   um2 = (uint32_t)n2 - 1, upx0 = (uint32_t)px0,
                   ur0 = (uint32_t)r0;
    auto particle_loop = [&](auto pot_tag, auto mass_tag) {
        constexpr bool POT = decltype(pot_tag)::value;
        constexpr bool MASS = decltype(mass_tag)::value;
        // weights, tile masks and LDS deposits of one staged batch
        auto consume = [&](const Batch& b) {
            #pragma unroll
            for (int u = 0; u < U; u++) {
                if ((uint32_t)(u * T + t) >= b.cnt) continue;
                const double u0 = b.x[u] * invH0 + shift;
                const double u1 = b.y[u] * invH1 + shift;
                const double u2 = b.z[u] * invH2 + shift;
                const double m = MASS ? b.m[u] : 1.0;
                if (!(phases & 1)) {
                    // reads-only decomposition mode: keep the loads
                    // observable, skip the deposit work
                    if (u0 + u1 + u2 + m == 1e308) tile[0] += 1.0;
                    continue;
                }
                double w0[SUP], w1[SUP], w2[SUP];
                int64_t b0, b1, b2;
                paint_weights<WINDOW, SUP>(u0, u1, u2, w0, w1, w2,
                                           b0, b1, b2);
                // tile plane / row / z cell reached at stencil offset d
                // (plane and row relative to the tile; >= P or >= RG:
                // outside it).  Power-of-two instance: every n <= 2^31,
                // the wrap is an AND and only the low 32 bits of the
                // (exactly converted) base cell matter — unsigned 32-bit
                // modular arithmetic gives the same cells as the 64-bit
                // modulo at half the VALU work.
                using idx_t = std::conditional_t<POT, uint32_t, int64_t>;
                const uint32_t c0 = (uint32_t)b0, c1 = (uint32_t)b1,
                               c2 = (uint32_t)b2;
                auto plane = [&](int d) -> idx_t {
                    if constexpr (POT) return (c0 + d - upx0) & um0;
                    else {
                        const int64_t pl = wrap_generic(b0 + d, n0) - px0;
                        return pl < 0 ? pl + n0 : pl;
                    }
                };
                auto row = [&](int d) -> idx_t {
                    if constexpr (POT) return (c1 + d - ur0) & um1;
                    else {
                        const int64_t ly = wrap_generic(b1 + d, n1) - r0;
                        return ly < 0 ? ly + n1 : ly;
                    }
                };
                auto zcell = [&](int d) -> idx_t {
                    if constexpr (POT) return (c2 + d) & um2;
                    else return wrap_generic(b2 + d, n2);
                };
                // the SUP x SUP deposits of x-weight wx into tile plane pl
                auto deposit_plane = [&](idx_t pl, double wx) {
                    #pragma unroll
                    for (int dy = 0; dy < SUP; dy++) {
                        const idx_t ly = row(dy);
                        if (ly >= (idx_t)RG) continue;
                        const double wxy = wx * w1[dy] * m;
                        #pragma unroll
                        for (int dz = 0; dz < SUP; dz++)
                            unsafeAtomicAdd(
                                &tile[(pl * (idx_t)RG + ly) * (idx_t)sp
                                      + zcell(dz)],
                                wxy * w2[dz]);
                    }
                };
                if (PT == 1) {
                    // single-plane tile: every x offset that hits it
                    // deposits into the same cells, so their weights
                    // are summed first and the y-z stencil is issued
                    // once, not once per x offset (each copy would run
                    // with most lanes masked off: a wave's particles
                    // mix the pair's planes).  On a mesh of at least
                    // SUP planes at most one offset hits and wx is that
                    // offset's weight itself.
                    double wx = 0.0;
                    bool hit = false;
                    #pragma unroll
                    for (int dx = 0; dx < SUP; dx++)
                        if (plane(dx) == 0) { wx += w0[dx]; hit = true; }
                    if (hit) deposit_plane(0, wx);
                } else {
                    #pragma unroll
                    for (int dx = 0; dx < SUP; dx++) {
                        const idx_t pl = plane(dx);
                        if (pl < (idx_t)P) deposit_plane(pl, w0[dx]);
                    }
                }
            }
        };
        Batch A, B;
        bool moreA = issue(A, mass_tag);
        while (moreA) {
            const bool moreB = issue(B, mass_tag);   // in flight during A
            consume(A);
            if (!moreB) break;
            moreA = issue(A, mass_tag);              // in flight during B
            consume(B);
        }
    };
    if (((n0 & (n0 - 1)) | (n1 & (n1 - 1)) | (n2 & (n2 - 1))) == 0
        && (n0 | n1 | n2) <= ((int64_t)1 << 31)) {
        if (mass) particle_loop(std::true_type{}, std::true_type{});
        else particle_loop(std::true_type{}, std::false_type{});
    } else {
        if (mass) particle_loop(std::false_type{}, std::true_type{});
        else particle_loop(std::false_type{}, std::false_type{});
    }
    __syncthreads();

    if (!(phases & 2)) return;       // decomposition mode: no flush/FFT

    if (!DOFFT) {
        // flush the exclusively-owned tile with plain stores
        if (accumulate) {
            for (int64_t w = t; w < win; w += T) {
                const int64_t pl = (PT == 1) ? 0
                    : w / ((int64_t)RG * sp);
                const int64_t rem = (PT == 1) ? w : w - pl * RG * sp;
                const int64_t r = rem / sp, z = rem - r * sp;
                if (z < n2 && tile[w] != 0.0)
                    mesh[((px0 - x0 + pl) * n1 + r0 + r) * n2 + z]
                        += tile[w];
            }
        } else {
            for (int64_t w = t; w < win; w += T) {
                const int64_t pl = (PT == 1) ? 0
                    : w / ((int64_t)RG * sp);
                const int64_t rem = (PT == 1) ? w : w - pl * RG * sp;
                const int64_t r = rem / sp, z = rem - r * sp;
                if (z < n2)
                    mesh[((px0 - x0 + pl) * n1 + r0 + r) * n2 + z]
                        = tile[w];
            }
        }
        return;
    }

    // ---- fused forward z-FFT, one WAVE per tile row (packed-real
    // complex FFT of m = n2/2 points + untwiddle split, as kfft_r2c_z).
    // A wave owns a whole row, so the stage ordering needs no block
    // syncs — CDNA wave64 executes in lockstep and LDS ops complete in
    // program order; the wave_barrier only pins the compiler's
    // scheduling across the cross-lane dependences.  ZF > 0: the
    // complex FFT is zfft_row, its twiddles loaded here once for all
    // the rows of the wave. ----
    const int m = (int)(n2 >> 1);
    const int bits = 31 - __clz((unsigned)m);
    const int lane = t & 63;
    const int wave = t >> 6;
    const int nw = T >> 6;
    zfft_twiddles ztw;
    if constexpr (ZF > 0) zfft_load_twiddles<ZF>(ztw, table, lane);

    for (int r = wave; r < P * RG; r += nw) {
        const int64_t pl = (PT == 1) ? 0 : r / RG;
        const int64_t rr = (PT == 1) ? r : r - pl * RG;
        cdouble* out = (cdouble*)mesh
            + ((px0 - x0 + pl) * n1 + r0 + rr) * (m + 1);
        cdouble* z = (cdouble*)&tile[(int64_t)r * sp];

        if constexpr (ZF > 0) {
            zfft_row<ZF>(z, lane, ztw);
        } else {
        for (int j = lane; j < m; j += 64) {
            const int jr = nbk_bitrev(j, bits);
            if (j < jr) {
                const cdouble a = z[j];
                z[j] = z[jr];
                z[jr] = a;
            }
        }
        __builtin_amdgcn_wave_barrier();

        // fused radix-4 stages (same bit-reversed order; pairs of
        // radix-2 stages become one 4-point butterfly — half the LDS
        // round trips; algebra as lds_fft4 in nbk_fft.hip, validated
        // element-exact against numpy).  Odd log2(m): one multiply-free
        // radix-2 stage first.
        {
            int len = 2;
            if (bits & 1) {
                for (int q = lane; q < (m >> 1); q += 64) {
                    const int i0 = 2 * q;
                    const cdouble u = z[i0];
                    const cdouble v = z[i0 + 1];
                    z[i0] = cadd(u, v);
                    z[i0 + 1] = csub(u, v);
                }
                __builtin_amdgcn_wave_barrier();
                len = 4;
            }
            for (; 2 * len <= m; len <<= 2) {
                const int h = len >> 1;
                const int tw = m / len;
                for (int q = lane; q < (m >> 2); q += 64) {
                    const int grp = q / h;
                    const int pos = q - grp * h;
                    const int base = grp * (len << 1) + pos;
                    const cdouble w1 = table[pos * tw];
                    const cdouble w2 = table[2 * pos * tw];
                    const cdouble w3 = cmul(w1, w2);
                    const cdouble x0 = z[base];
                    const cdouble x1 = z[base + h];
                    const cdouble x2 = z[base + 2 * h];
                    const cdouble x3 = z[base + 3 * h];
                    const cdouble b1 = cmul(x2, w1);
                    const cdouble b2 = cmul(x1, w2);
                    const cdouble b3 = cmul(x3, w3);
                    const cdouble e0 = cadd(x0, b2);
                    const cdouble e1 = csub(x0, b2);
                    const cdouble o0 = cadd(b1, b3);
                    const cdouble o1 = csub(b1, b3);
                    z[base] = cadd(e0, o0);
                    z[base + 2 * h] = csub(e0, o0);
                    const cdouble io1 = {o1.im, -o1.re};   // -i*o1
                    z[base + h] = cadd(e1, io1);
                    z[base + 3 * h] = csub(e1, io1);
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        }   // ZF == 0

        // untwiddle split: X[k] = E[k] + W_n2^k O[k], k = 0..m, written
        // straight to the z half-spectrum
        for (int k = lane; k <= m; k += 64) {
            const cdouble Zk = z[k == m ? 0 : k];
            const cdouble Zm = z[(m - k) % m];
            const cdouble E = cscale(cadd(Zk, cconj(Zm)), 0.5);
            const cdouble D = csub(Zk, cconj(Zm));
            const cdouble O = {0.5 * D.im, -0.5 * D.re};  // D * (-i/2)
            const cdouble X = cadd(E, cmul(table[k], O));
            out[k] = cscale(X, scale);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// windowed gather — the dual of kpaint (pmesh readout, used by
// FFTRecon's displacement solve, fftrecon.py:246-249, and the nnb
// variant by the LogNormal generator, mockmaker.py:317-319).  Each lane
// sums W * mesh over its particle's neighbourhood; cells outside the
// local slab contribute 0 (the ghost owner adds its partial — the host
// exchanges and sums partials across ranks).
template <int WINDOW>
__global__ void kreadout(const double* __restrict__ px,
                         const double* __restrict__ py,
                         const double* __restrict__ pz, int64_t n,
                         int64_t n0, int64_t n1, int64_t n2,
                         double invH0, double invH1, double invH2,
                         const double* __restrict__ mesh,
                         int64_t x0, int64_t nx_local,
                         double* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         i < n; i += stride) {
        const double u0 = px[i] * invH0, u1 = py[i] * invH1,
                     u2 = pz[i] * invH2;

        if (WINDOW == WINDOW_NNB) {
            const int64_t gx = wrap_idx((int64_t)floor(u0 + 0.5), n0);
            const int64_t gy = wrap_idx((int64_t)floor(u1 + 0.5), n1);
            const int64_t gz = wrap_idx((int64_t)floor(u2 + 0.5), n2);
            out[i] = (gx >= x0 && gx < x0 + nx_local)
                ? mesh[((gx - x0) * n1 + gy) * n2 + gz] : 0.0;
            continue;
        }

        constexpr int SUP = window_support<WINDOW>();
        double w0[SUP], w1[SUP], w2[SUP];
        int64_t b0, b1, b2;
        paint_weights<WINDOW, SUP>(u0, u1, u2, w0, w1, w2, b0, b1, b2);

        double acc = 0.0;
        #pragma unroll
        for (int dx = 0; dx < SUP; dx++) {
            const int64_t gx = wrap_idx(b0 + dx, n0);
            if (gx < x0 || gx >= x0 + nx_local) continue;
            const int64_t lx = gx - x0;
            #pragma unroll
            for (int dy = 0; dy < SUP; dy++) {
                const int64_t gy = wrap_idx(b1 + dy, n1);
                const double wxy = w0[dx] * w1[dy];
                #pragma unroll
                for (int dz = 0; dz < SUP; dz++) {
                    const int64_t gz = wrap_idx(b2 + dz, n2);
                    acc += wxy * w2[dz]
                        * mesh[(lx * n1 + gy) * n2 + gz];
                }
            }
        }
        out[i] = acc;
    }
}

int grid_for(int64_t n, int block) {
    int64_t g = (n + block - 1) / block;
    // >> 256 CUs x 8 XCDs want >>2048 workgroups; cap to keep index math sane
    if (g > 1048576) g = 1048576;
    if (g < 1) g = 1;
    return (int)g;
}

// The one place a runtime window id becomes a template argument:
// calls f(std::integral_constant<int, W>{}) for the three paint
// windows; false = unknown id, f not called.
template <class F>
bool with_window(int window, F&& f) {
    switch (window) {
    case NBK_WINDOW_CIC:
        f(std::integral_constant<int, NBK_WINDOW_CIC>{}); return true;
    case NBK_WINDOW_TSC:
        f(std::integral_constant<int, NBK_WINDOW_TSC>{}); return true;
    case NBK_WINDOW_PCS:
        f(std::integral_constant<int, NBK_WINDOW_PCS>{}); return true;
    }
    return false;
}

// The one place the fused z-FFT's length becomes a template argument:
// calls f(std::integral_constant<int, ZF>{}) with ZF = log2(n2/2) for
// the lengths zfft_row holds in registers (m/64 <= 8 points per lane,
// m >= 64), ZF = 0 (the LDS radix-4 network) for every other n2.
template <class F>
void with_zfft(int64_t n2, F&& f) {
    switch (n2) {
    case 128:  f(std::integral_constant<int, 6>{}); return;
    case 256:  f(std::integral_constant<int, 7>{}); return;
    case 512:  f(std::integral_constant<int, 8>{}); return;
    case 1024: f(std::integral_constant<int, 9>{}); return;
    }
    f(std::integral_constant<int, 0>{});
}

}  // namespace

extern "C" int nbk_paint_f64(const double* pos, const double* mass, int64_t n,
                             const int64_t nmesh[3], const double box[3],
                             int window, double shift,
                             double* mesh, int64_t x0, int64_t nx_local,
                             void* stream)
{
    if (n < 0 || !mesh || (!pos && n > 0)) {
        NBK_SET_ERR("nbk_paint_f64: bad pointer/size");
        return NBK_ERR_ARG;
    }
    if (n == 0) return NBK_OK;
    const double invH0 = nmesh[0] / box[0];
    const double invH1 = nmesh[1] / box[1];
    const double invH2 = nmesh[2] / box[2];
    const int block = 256;
    const int grid = grid_for(n, block);
    hipStream_t s = (hipStream_t)stream;
    const double *px = pos, *py = pos + n, *pz = pos + 2 * n;

    if (!with_window(window, [&](auto w) {
            hipLaunchKernelGGL(kpaint<decltype(w)::value>, dim3(grid),
                               dim3(block), 0, s, px, py, pz, mass, n,
                               nmesh[0], nmesh[1], nmesh[2],
                               invH0, invH1, invH2, shift, mesh, x0,
                               nx_local);
        })) {
        NBK_SET_ERR("nbk_paint_f64: unknown window id %d", window);
        return NBK_ERR_ARG;
    }
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_paint_sorted_f64(const double* pos, const double* mass,
                                    int64_t n, const int64_t nmesh[3],
                                    const double box[3], int window,
                                    double shift, double* mesh, int64_t x0,
                                    int64_t nx_local, void* stream)
{
    // Measured on the C3 input (1e8 TSC, bucket-sorted): the LDS-window
    // path is 76 vs 45 ms against the wave-merged direct kernel — PMC
    // shows all TSC variants 71-88% instruction-ISSUE-stalled, so
    // rerouting deposits through LDS buys nothing there.  Only PCS
    // (64 deposits, flush ~3x cheaper than direct) takes the tiled
    // path; CIC and TSC keep the direct kernel, which also rejects an
    // unknown id.
    if (window != NBK_WINDOW_PCS || n == 0)
        return nbk_paint_f64(pos, mass, n, nmesh, box, window, shift,
                             mesh, x0, nx_local, stream);
    const double invH0 = nmesh[0] / box[0];
    const double invH1 = nmesh[1] / box[1];
    const double invH2 = nmesh[2] / box[2];
    const int64_t grid = (n + NBK_TILE_PPB - 1) / NBK_TILE_PPB;
    if (grid > 0x7fffffff) {
        NBK_SET_ERR("nbk_paint_sorted_f64: grid too large");
        return NBK_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const double *px = pos, *py = pos + n, *pz = pos + 2 * n;
    hipLaunchKernelGGL(kpaint_tiled<NBK_WINDOW_PCS>,
                       dim3((uint32_t)grid), dim3(256), 0, s,
                       px, py, pz, mass, n, nmesh[0], nmesh[1],
                       nmesh[2], invH0, invH1, invH2, shift, mesh,
                       x0, nx_local);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_readout_f64(const double* pos, int64_t n,
                               const int64_t nmesh[3], const double box[3],
                               int window,
                               const double* mesh, int64_t x0,
                               int64_t nx_local,
                               double* out, void* stream)
{
    if (n == 0) return NBK_OK;
    const int block = 256;
    const int grid = grid_for(n, block);
    hipStream_t s = (hipStream_t)stream;
    const double iH0 = nmesh[0] / box[0];
    const double iH1 = nmesh[1] / box[1];
    const double iH2 = nmesh[2] / box[2];
    auto launch = [&](auto w) {
        hipLaunchKernelGGL(kreadout<decltype(w)::value>, dim3(grid),
                           dim3(block), 0, s, pos, pos + n, pos + 2 * n, n,
                           nmesh[0], nmesh[1], nmesh[2], iH0, iH1, iH2,
                           mesh, x0, nx_local, out);
    };
    if (window == WINDOW_NNB) {
        launch(std::integral_constant<int, WINDOW_NNB>{});
    } else if (!with_window(window, launch)) {
        NBK_SET_ERR("nbk_readout_f64: unknown window id %d", window);
        return NBK_ERR_ARG;
    }
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}


// pick the gather tile shape (P x-planes x RG y-rows): minimize the
// particle re-read factor (P+sx)/P * (RG+sy)/RG (sx/sy = source span
// beyond the tile from the window support and interlace shift) within
// the 160 KiB LDS budget; powers of two dividing the local dims
// NBK_PAINT_PHASES: perf decomposition only (1 = reads+deposits,
// 0 = reads only, 2 = flush/FFT on an empty tile); default 3
static int nbk_paint_phases(void) {
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("NBK_PAINT_PHASES");
        v = e ? atoi(e) : 3;
        if (v < 0 || v > 3) v = 3;
    }
    return v;
}

static void nbk_pick_tile(int64_t nx_local, int64_t n1, int64_t n2,
                          int64_t pad, int sx, int sy,
                          int* P_out, int* RG_out)
{
    const int64_t budget = 20480 / (n2 + pad);
    // NBK_PAINT_P forces the plane count (tuning); RG fills the budget
    static int forceP = -1;
    if (forceP < 0) {
        const char* e = getenv("NBK_PAINT_P");
        forceP = e ? atoi(e) : 0;
        if (forceP < 0 || forceP > 16) forceP = 0;
    }
    double best = 1e30;
    int bP = 1, bRG = 1;
    // Measured policy (r02 A/B at C4/C3): narrow-span windows (CIC)
    // run fastest single-plane (the PT=1 specialized kernel: pure
    // paint 13.8 vs 15.7 ms, fused 19.9 vs 20.4 at C4) — the extra
    // source-plane read is cheaper than the multi-plane bookkeeping;
    // wide-span windows (TSC/PCS, 4 source planes single-plane) win
    // with the balanced multi-plane tile (C3 fused 4.8 vs 5.1 ms).
    const int prefer_single = (sx <= 1) && !forceP;
    for (int64_t P = 1; P <= nx_local && P <= budget; P <<= 1) {
        if (nx_local % P) break;
        if (forceP && P != forceP) continue;
        if (prefer_single && P > 1) break;
        for (int64_t RG = 1; RG <= n1 && P * RG <= budget; RG <<= 1) {
            if (n1 % RG) break;
            double cost = (double)(P + sx) / (double)P
                        * (double)(RG + sy) / (double)RG;
            if (forceP || prefer_single)
                cost = 1.0 / (double)RG;           // max RG at this P
            if (cost < best - 1e-12) { best = cost; bP = (int)P; bRG = (int)RG; }
        }
    }
    *P_out = bP;
    *RG_out = bRG;
}

// The launch behind nbk_paint_gather_f64 (DOFFT = false: `out` is the
// real slab, written or accumulated into) and nbk_paint_gather_fft_f64
// (DOFFT = true: `out` is the z half-spectrum, rows padded by 4 doubles
// in LDS, `table`/`scale` feed the fused FFT).  `who` names the entry
// point in the error texts; the callers have validated n2.
template <bool DOFFT>
static int paint_gather_launch(const char* who, const double* pos,
                               const double* mass, int64_t n,
                               const int64_t nmesh[3], const double box[3],
                               int window, double shift, const int* rowtab,
                               double* out, int64_t x0, int64_t nx_local,
                               int accumulate, const cdouble* table,
                               double scale, int pair_gs, void* stream)
{
    const int64_t n0 = nmesh[0], n1 = nmesh[1], n2 = nmesh[2];
    const int64_t pad = DOFFT ? 4 : 0;    // the kernel's row stride - n2
    // delta = b0 - ixc range per window/shift: source
    // planes/rows = [xlo, xhi] around the owner
    const bool sh = shift != 0.0;
    int sup, dmin, dmax;
    if (window == NBK_WINDOW_CIC) {
        sup = 2; dmin = 0; dmax = sh ? 1 : 0;
    } else if (window == NBK_WINDOW_TSC) {
        sup = 3; dmin = sh ? 0 : -1; dmax = 0;
    } else if (window == NBK_WINDOW_PCS) {
        sup = 4; dmin = -1; dmax = sh ? 0 : -1;
    } else {
        NBK_SET_ERR("%s: bad window %d", who, window);
        return NBK_ERR_ARG;
    }
    const int xlo = -sup + 1 - dmax;
    const int xhi = -dmin;
    const int span = xhi - xlo;

    int P, RG;
    if (pair_gs >= 0) {
        // pair-bucket mode: tile geometry is pinned by the sort's
        // group size (one plane x one y-group)
        P = 1;
        RG = 1 << pair_gs;
        if ((int64_t)RG * (n2 + pad) * 8 > 160 * 1024 || n1 % RG) {
            NBK_SET_ERR("%s: bad pair_gs=%d", who, pair_gs);
            return NBK_ERR_ARG;
        }
    } else {
        nbk_pick_tile(nx_local, n1, n2, pad, span, span, &P, &RG);
    }
    const int64_t grid = (nx_local / P) * (n1 / RG);
    const size_t lds = (size_t)P * RG * (n2 + pad) * sizeof(double);
    hipStream_t s = (hipStream_t)stream;
    // PT: the kernel's compile-time plane count (1, or 0 = runtime P);
    // ZF: the fused z-FFT's row transform (with_zfft)
    auto launch = [&](auto w, auto pt, auto zf) {
        auto* kernel = &kpaint_gather<decltype(w)::value, DOFFT,
                                      decltype(pt)::value,
                                      decltype(zf)::value>;
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(
                reinterpret_cast<const void*>(kernel),
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(1024), lds,
                           s, pos, pos + n, pos + 2 * n, mass, n,
                           n0, n1, n2,
                           n0 / box[0], n1 / box[1], n2 / box[2], shift,
                           rowtab, out, x0, nx_local, RG, P, xlo, xhi,
                           accumulate, table, scale, pair_gs,
                           nbk_paint_phases());
    };
    with_window(window, [&](auto w) {
        auto go = [&](auto zf) {
            if (P == 1) launch(w, std::integral_constant<int, 1>{}, zf);
            else launch(w, std::integral_constant<int, 0>{}, zf);
        };
        if constexpr (DOFFT) with_zfft(n2, go);
        else go(std::integral_constant<int, 0>{});
    });
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}

extern "C" int nbk_paint_gather_f64(const double* pos, const double* mass,
                                    int64_t n, const int64_t nmesh[3],
                                    const double box[3],
                                    int window, double shift,
                                    const int* rowtab,
                                    double* mesh, int64_t x0,
                                    int64_t nx_local, int accumulate,
                                    int pair_gs, void* stream)
{
    if (nmesh[2] > 20480) {
        NBK_SET_ERR("nbk_paint_gather_f64: no LDS tile for n1=%lld "
                    "n2=%lld", (long long)nmesh[1], (long long)nmesh[2]);
        return NBK_ERR_UNSUPPORTED;
    }
    return paint_gather_launch<false>(
        "nbk_paint_gather_f64", pos, mass, n, nmesh, box, window, shift,
        rowtab, mesh, x0, nx_local, accumulate, nullptr, 1.0, pair_gs,
        stream);
}

extern "C" int nbk_paint_gather_fft_f64(const double* pos,
                                        const double* mass, int64_t n,
                                        const int64_t nmesh[3],
                                        const double box[3],
                                        int window, double shift,
                                        const int* rowtab,
                                        double* zspec, int64_t x0,
                                        int64_t nx_local, double scale,
                                        int pair_gs, void* stream)
{
    const int64_t n1 = nmesh[1], n2 = nmesh[2];
    if (n2 < 8 || n2 > 4096 || (n2 & (n2 - 1))) {
        NBK_SET_ERR("nbk_paint_gather_fft_f64: n2=%lld not a supported "
                    "FFT length", (long long)n2);
        return NBK_ERR_UNSUPPORTED;
    }
    if (n2 + 4 > 20480) {
        NBK_SET_ERR("nbk_paint_gather_fft_f64: no LDS tile for n1=%lld "
                    "n2=%lld", (long long)n1, (long long)n2);
        return NBK_ERR_UNSUPPORTED;
    }
    const double* table = nbk_internal_twiddles(n2);
    if (!table) {
        NBK_SET_ERR("twiddle alloc failed");
        return NBK_ERR_HIP;
    }
    return paint_gather_launch<true>(
        "nbk_paint_gather_fft_f64", pos, mass, n, nmesh, box, window,
        shift, rowtab, zspec, x0, nx_local, 0, (const cdouble*)table,
        scale, pair_gs, stream);
}
