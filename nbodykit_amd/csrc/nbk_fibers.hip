// Fibre assignment inside collision groups: the replacement for the Python
// loop over groups, with a scipy pdist per round, under the reference's
// nbodykit/algorithms/fibercollisions.py (_assign_fibers and
// _assign_multiplets), f64 throughout.
//
// Input: pos_aos[3n], the positions the angular FOF ran on; midx[nmember],
// the input indices of the members of every collision group, group after
// group and ascending inside a group; gstart[ngroup + 1], the start table
// into midx.  Everything written is in member order.  pos_aos is read only
// through midx.
//
// Collision.  Members a and b collide iff, with d = p_a - p_b per axis,
//   (dx*dx + dy*dy) + dz*dz <= r2,
// every operation rounded separately (-ffp-contract=off): the predicate of
// kfof_link, so the collision graph and the FOF groups cannot disagree.
//
// The greedy of one group.  All members start active.  Per round, among the
// active members, n_coll[j] is the number of active members colliding with j
// and n_other[j] the sum of n_coll over them.  If every n_coll is 0 the
// group is done and what is left is clean.  Otherwise ONE member is marked
// collided and deactivated: the one with the largest n_coll, then the
// smallest n_other, then the smallest key, then the smallest slot (slots
// ascend with the input index).  key is the splitmix64 finaliser of
// seed + (input index + 1) * 0x9E3779B97F4A7C15, a fixed priority per object
// where the reference draws from a sequential stream.  A group need not be
// connected: one without a collision comes out all clean.
//
// Neighbour.  A collided member gets the input index of the member of its
// group that is not collided and has the smallest squared distance (the
// expression above), ties to the smaller slot; every other member gets -1.
// The last active member of a group is never collided, so one exists.
//
// Two tiers, one launch each, no communication between blocks, no global
// atomics:
//  - kfib_wave: one wave per group of up to 64 members, four waves per
//    block.  lane = member; positions are staged in LDS once; the adjacency
//    of a member is one 64-bit mask in a register and the active set a
//    wave-uniform 64-bit mask.  n_other reads the n_coll of the active lanes
//    with one cross-lane read each; the choice is a butterfly reduction of
//    (n_coll, n_other, key, slot).
//  - kfib_block: one block of 1024 threads per group [0, nbig) with more than
//    64 members, thread = member.  Positions, the bit matrix (word-major:
//    word w of row t at adj[w * m + t], so a wave's reads are contiguous),
//    n_coll and the active and collided masks live in LDS; the choice is the
//    same reduction, then one pass over the 16 wave results.  Three block
//    barriers per round, all in block-uniform control flow.
// The cap on the group size, FIB_CAP = 1024, is what the 160 KiB of LDS
// give: 128 KiB of bit matrix, 24 KiB of positions, 4 KiB of n_coll and
// under 1 KiB of static arrays.
//
// Bounds.  A start table entry is clamped to [0, nmember] and every loop is
// bounded by the group's size after the clamp.  A member index outside
// [0, n), a group above the cap, and a group at or beyond nbig with more
// than 64 members set err[0] (a plain store of 1) and leave the group's
// outputs untouched.
#include "nbk_countsort.h"

namespace {

constexpr int FIB_WAVE = 64;
constexpr int FIB_WAVES_PER_BLOCK = 4;
constexpr int FIB_CAP = 1024;
constexpr int FIB_BLOCK_THREADS = 1024;
constexpr int FIB_BLOCK_WAVES = FIB_BLOCK_THREADS / FIB_WAVE;
static_assert(FIB_CAP <= FIB_BLOCK_THREADS, "one thread per member");
// dynamic LDS of the block tier: bit matrix, positions, n_coll
constexpr size_t FIB_BLOCK_LDS =
    (size_t)FIB_CAP * (FIB_CAP / 64) * sizeof(unsigned long long)
    + (size_t)3 * FIB_CAP * sizeof(double) + (size_t)FIB_CAP * sizeof(int);
static_assert(FIB_BLOCK_LDS + 1024 <= 160 * 1024, "LDS budget");

struct FibArgs {
    const double* pos;
    const int* midx;
    const int* gstart;
    int n;
    int nmember;
    int ngroup;
    int nbig;
    double r2;
    unsigned long long seed;
    int* collided;
    int* neighbor;
    int* err;
};

// the candidate of a round; n_coll = -1 marks a member that is not active
struct FibPick {
    int ncoll;
    int nother;
    unsigned long long key;
    int slot;
};

__device__ __forceinline__ bool fib_before(const FibPick& a,
                                           const FibPick& b) {
    if (a.ncoll != b.ncoll) return a.ncoll > b.ncoll;
    if (a.nother != b.nother) return a.nother < b.nother;
    if (a.key != b.key) return a.key < b.key;
    return a.slot < b.slot;
}

// the first candidate of the wave, in every lane
__device__ __forceinline__ FibPick fib_wave_first(FibPick p) {
    #pragma unroll
    for (int off = FIB_WAVE / 2; off > 0; off >>= 1) {
        FibPick q;
        q.ncoll = __shfl_xor(p.ncoll, off);
        q.nother = __shfl_xor(p.nother, off);
        q.key = __shfl_xor(p.key, off);
        q.slot = __shfl_xor(p.slot, off);
        if (fib_before(q, p)) p = q;
    }
    return p;
}

__device__ __forceinline__ unsigned long long fib_key(unsigned long long seed,
                                                      int index) {
    unsigned long long z =
        seed + ((unsigned long long)index + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double fib_dist2(const double* x, const double* y,
                                            const double* z, int a, int b) {
    const double dx = x[a] - x[b], dy = y[a] - y[b], dz = z[a] - z[b];
    return (dx * dx + dy * dy) + dz * dz;
}

// the members [b, b + m) of group g, from the clamped start table
__device__ __forceinline__ void fib_range(const FibArgs& a, int g, int* b,
                                          int* m) {
    int lo = a.gstart[g], hi = a.gstart[g + 1];
    lo = lo < 0 ? 0 : (lo > a.nmember ? a.nmember : lo);
    hi = hi < lo ? lo : (hi > a.nmember ? a.nmember : hi);
    *b = lo;
    *m = hi - lo;
}

// ---- the wave tier --------------------------------------------------------

__global__ __launch_bounds__(FIB_WAVE * FIB_WAVES_PER_BLOCK)
void kfib_wave(FibArgs a)
{
    __shared__ double sx[FIB_WAVES_PER_BLOCK][FIB_WAVE];
    __shared__ double sy[FIB_WAVES_PER_BLOCK][FIB_WAVE];
    __shared__ double sz[FIB_WAVES_PER_BLOCK][FIB_WAVE];
    const int wave = threadIdx.x / FIB_WAVE;
    const int lane = threadIdx.x % FIB_WAVE;
    const int64_t g = (int64_t)blockIdx.x * FIB_WAVES_PER_BLOCK + wave;

    // (no wave leaves before the one block barrier)
    bool live = g < a.ngroup;
    int b = 0, m = 0;
    if (live) {
        fib_range(a, (int)g, &b, &m);
        if (m > FIB_WAVE) {
            // the block tier's, or a broken promise
            if (g >= a.nbig && lane == 0) a.err[0] = 1;
            live = false;
        }
    }
    const bool member = live && lane < m;
    const int idx = member ? a.midx[b + lane] : 0;
    if (live && __ballot(member && (idx < 0 || idx >= a.n)) != 0ull) {
        if (lane == 0) a.err[0] = 1;
        live = false;
    }
    if (live && member) {
        const double* p = a.pos + 3 * (int64_t)idx;
        sx[wave][lane] = p[0];
        sy[wave][lane] = p[1];
        sz[wave][lane] = p[2];
    }
    __syncthreads();
    if (!live || m == 0) return;
    const double* x = sx[wave];
    const double* y = sy[wave];
    const double* z = sz[wave];

    unsigned long long adj = 0ull;
    if (lane < m) {
        for (int k = 0; k < m; k++) {
            const double d2 = fib_dist2(x, y, z, lane, k);
            if (k != lane && d2 <= a.r2) adj |= 1ull << k;
        }
    }
    const unsigned long long key = fib_key(a.seed, idx);
    const unsigned long long members =
        m == FIB_WAVE ? ~0ull : (1ull << m) - 1ull;
    unsigned long long active = members;        // wave-uniform
    unsigned long long coll = 0ull;

    for (int round = 0; round < m; round++) {
        FibPick p;
        p.ncoll = (active >> lane) & 1ull ? __popcll(adj & active) : -1;
        p.nother = 0;
        for (unsigned long long rem = active; rem; rem &= rem - 1ull) {
            const int k = __builtin_ctzll(rem);
            const int nk = __shfl(p.ncoll, k);
            if ((adj >> k) & 1ull) p.nother += nk;
        }
        p.key = key;
        p.slot = lane;
        const FibPick first = fib_wave_first(p);
        const int ncoll = __builtin_amdgcn_readfirstlane(first.ncoll);
        const int slot = __builtin_amdgcn_readfirstlane(first.slot);
        if (ncoll <= 0) break;
        coll |= 1ull << slot;
        active &= ~(1ull << slot);
    }

    if (lane >= m) return;
    const int mine = (int)((coll >> lane) & 1ull);
    int nearest = -1;
    if (mine) {
        double best = 0.0;
        for (unsigned long long rem = members & ~coll; rem;
             rem &= rem - 1ull) {
            const int k = __builtin_ctzll(rem);
            const double d2 = fib_dist2(x, y, z, lane, k);
            if (nearest < 0 || d2 < best) {
                best = d2;
                nearest = k;
            }
        }
        if (nearest >= 0) nearest = a.midx[b + nearest];
    }
    a.collided[b + lane] = mine;
    a.neighbor[b + lane] = nearest;
}

// ---- the block tier -------------------------------------------------------

__global__ __launch_bounds__(FIB_BLOCK_THREADS)
void kfib_block(FibArgs a)
{
    extern __shared__ unsigned long long fib_lds[];
    __shared__ unsigned long long s_active[FIB_CAP / 64];
    __shared__ unsigned long long s_coll[FIB_CAP / 64];
    __shared__ FibPick s_first[FIB_BLOCK_WAVES];
    const int tid = threadIdx.x;
    const int wave = tid / FIB_WAVE, lane = tid % FIB_WAVE;

    int b, m;
    fib_range(a, (int)blockIdx.x, &b, &m);
    if (m <= FIB_WAVE) return;          // the wave tier's (block-uniform)
    if (m > FIB_CAP) {
        if (tid == 0) a.err[0] = 1;
        return;
    }
    const int words = (m + 63) >> 6;
    unsigned long long* adj = fib_lds;              // [words][m]
    double* x = reinterpret_cast<double*>(adj + (size_t)words * m);
    double* y = x + m;
    double* z = y + m;
    int* s_ncoll = reinterpret_cast<int*>(z + m);

    const bool member = tid < m;
    const int idx = member ? a.midx[b + tid] : 0;
    if (__syncthreads_or(member && (idx < 0 || idx >= a.n))) {
        if (tid == 0) a.err[0] = 1;
        return;
    }
    if (member) {
        const double* p = a.pos + 3 * (int64_t)idx;
        x[tid] = p[0];
        y[tid] = p[1];
        z[tid] = p[2];
    }
    if (tid < FIB_CAP / 64) {
        const int left = m - tid * 64;
        s_active[tid] = left >= 64 ? ~0ull
                      : (left > 0 ? (1ull << left) - 1ull : 0ull);
        s_coll[tid] = 0ull;
    }
    __syncthreads();

    // the own row of the bit matrix (read by this thread alone)
    if (member) {
        for (int w = 0; w < words; w++) {
            const int k1 = m - w * 64 < 64 ? m - w * 64 : 64;
            unsigned long long bits = 0ull;
            for (int k = 0; k < k1; k++) {
                const int j = w * 64 + k;
                const double d2 = fib_dist2(x, y, z, tid, j);
                if (j != tid && d2 <= a.r2) bits |= 1ull << k;
            }
            adj[(size_t)w * m + tid] = bits;
        }
    }
    const unsigned long long key = fib_key(a.seed, idx);

    for (int round = 0; round < m; round++) {
        const bool act = member && ((s_active[wave] >> lane) & 1ull);
        FibPick p;
        p.ncoll = -1;
        if (act) {
            p.ncoll = 0;
            for (int w = 0; w < words; w++)
                p.ncoll += __popcll(adj[(size_t)w * m + tid] & s_active[w]);
        }
        if (member) s_ncoll[tid] = p.ncoll;
        __syncthreads();
        p.nother = 0;
        if (act) {
            for (int w = 0; w < words; w++) {
                for (unsigned long long rem =
                         adj[(size_t)w * m + tid] & s_active[w];
                     rem; rem &= rem - 1ull)
                    p.nother += s_ncoll[w * 64 + __builtin_ctzll(rem)];
            }
        }
        p.key = key;
        p.slot = tid;
        const FibPick mine = fib_wave_first(p);
        if (lane == 0) s_first[wave] = mine;
        __syncthreads();
        FibPick first = s_first[0];
        for (int v = 1; v < FIB_BLOCK_WAVES; v++) {
            const FibPick q = s_first[v];
            if (fib_before(q, first)) first = q;
        }
        if (first.ncoll <= 0) break;    // block-uniform: all read the same
        if (tid == 0) {
            const unsigned long long bit = 1ull << (first.slot & 63);
            s_active[first.slot >> 6] &= ~bit;
            s_coll[first.slot >> 6] |= bit;
        }
        __syncthreads();
    }

    if (!member) return;
    const int collided = (int)((s_coll[wave] >> lane) & 1ull);
    int nearest = -1;
    if (collided) {
        double best = 0.0;
        for (int w = 0; w < words; w++) {
            const int left = m - w * 64;
            const unsigned long long in_group =
                left >= 64 ? ~0ull : (1ull << left) - 1ull;
            for (unsigned long long rem = in_group & ~s_coll[w]; rem;
                 rem &= rem - 1ull) {
                const int k = w * 64 + __builtin_ctzll(rem);
                const double d2 = fib_dist2(x, y, z, tid, k);
                if (nearest < 0 || d2 < best) {
                    best = d2;
                    nearest = k;
                }
            }
        }
        if (nearest >= 0) nearest = a.midx[b + nearest];
    }
    a.collided[b + tid] = collided;
    a.neighbor[b + tid] = nearest;
}

}  // namespace

extern "C" int nbk_fibers_max_group(void) { return FIB_CAP; }

extern "C" int nbk_fibers_assign_f64(const double* pos_aos, int64_t n,
                                     const int* midx, int64_t nmember,
                                     const int* gstart, int64_t ngroup,
                                     int64_t nbig, double r2, uint64_t seed,
                                     int* collided, int* neighbor, int* err,
                                     void* stream)
{
    const char* who = "nbk_fibers_assign_f64";
    const int64_t lim = (int64_t)1 << 31;
    if (n < 0 || n >= lim || nmember < 0 || nmember >= lim) {
        NBK_SET_ERR("%s: n = %lld, nmember = %lld (0 <= both < 2^31)", who,
                    (long long)n, (long long)nmember);
        return NBK_ERR_ARG;
    }
    if (ngroup < 0 || ngroup >= lim || nbig < 0 || nbig > ngroup) {
        NBK_SET_ERR("%s: ngroup = %lld, nbig = %lld (0 <= nbig <= ngroup "
                    "< 2^31)", who, (long long)ngroup, (long long)nbig);
        return NBK_ERR_ARG;
    }
    if (!(r2 >= 0.0) || !std::isfinite(r2)) {
        NBK_SET_ERR("%s: r2 = %g", who, r2);
        return NBK_ERR_ARG;
    }
    if ((n > 0 && !pos_aos)
        || (nmember > 0 && (!midx || !collided || !neighbor))
        || (ngroup > 0 && (!gstart || !err))) {
        NBK_SET_ERR("%s: a null pointer with a non-zero count", who);
        return NBK_ERR_ARG;
    }
    if (ngroup == 0) return NBK_OK;

    FibArgs a;
    a.pos = pos_aos;
    a.midx = midx;
    a.gstart = gstart;
    a.n = (int)n;
    a.nmember = (int)nmember;
    a.ngroup = (int)ngroup;
    a.nbig = (int)nbig;
    a.r2 = r2;
    a.seed = (unsigned long long)seed;
    a.collided = collided;
    a.neighbor = neighbor;
    a.err = err;
    hipStream_t s = (hipStream_t)stream;
    if (nbig > 0) {
        raise_lds(reinterpret_cast<const void*>(&kfib_block), FIB_BLOCK_LDS);
        hipLaunchKernelGGL(kfib_block, dim3((uint32_t)nbig),
                           dim3(FIB_BLOCK_THREADS), FIB_BLOCK_LDS, s, a);
        NBK_CHECK_HIP(hipGetLastError());
    }
    const int64_t blocks =
        (ngroup + FIB_WAVES_PER_BLOCK - 1) / FIB_WAVES_PER_BLOCK;
    hipLaunchKernelGGL(kfib_wave, dim3((uint32_t)blocks),
                       dim3(FIB_WAVE * FIB_WAVES_PER_BLOCK), 0, s, a);
    NBK_CHECK_HIP(hipGetLastError());
    return NBK_OK;
}
