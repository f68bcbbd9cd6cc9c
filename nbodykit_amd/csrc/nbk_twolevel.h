// The two-level cell grid of nbk_fof.hip and nbk_knn.hip: the grid
// functor of the sort kernels and the argument checks every entry point
// of the two files makes.
//
// ncell[a] = ncoarse[a] * fine[a] cells per axis.  The fine cell of a
// particle is cell_axis() (nbk_cells.h); its coarse cell is that INTEGER
// divided by fine[a] — never a second floor with a coarse inv_cell, whose
// rounding could disagree with the first at a cell face.  Cells are
// numbered block-major: coarse_id * nfine + sub_id, both row-major, so the
// fine cells of one coarse cell are contiguous.
#pragma once
#include "nbk_countsort.h"
#include "nbk_cells.h"

namespace {

struct FofGrid {
    double origin[3];
    double inv_cell[3];
    int ncoarse[3];
    int fine[3];

    // fine cell per axis -> (coarse id, sub id)
    __device__ __forceinline__ void split(const int c[3], int* coarse,
                                          int* sub) const {
        *coarse = ((c[0] / fine[0]) * ncoarse[1] + c[1] / fine[1])
                  * ncoarse[2] + c[2] / fine[2];
        *sub = ((c[0] % fine[0]) * fine[1] + c[1] % fine[1]) * fine[2]
               + c[2] % fine[2];
    }

    __device__ __forceinline__ void locate(double x, double y, double z,
                                           int* coarse, int* sub) const {
        const int c[3] = {
            cell_axis(x, origin[0], inv_cell[0], ncoarse[0] * fine[0]),
            cell_axis(y, origin[1], inv_cell[1], ncoarse[1] * fine[1]),
            cell_axis(z, origin[2], inv_cell[2], ncoarse[2] * fine[2])};
        split(c, coarse, sub);
    }
};

// grid checks of every entry point; `who` names it
[[maybe_unused]] int fof_grid(const char* who, const int ncoarse[3],
                              const int fine[3], int64_t* ncoarse_all,
                              int64_t* nfine)
{
    *ncoarse_all = 1;
    *nfine = 1;
    for (int i = 0; i < 3; i++) {
        if (ncoarse[i] < 1 || fine[i] < 1) {
            NBK_SET_ERR("%s: ncoarse[%d] = %d, fine[%d] = %d", who, i,
                        ncoarse[i], i, fine[i]);
            return NBK_ERR_ARG;
        }
        *ncoarse_all *= ncoarse[i];
        *nfine *= fine[i];
        if (*ncoarse_all > NBK_SORT_LDS_INTS || *nfine > NBK_SORT_LDS_INTS) {
            NBK_SET_ERR("%s: more than %lld coarse cells or sub-cells, the "
                        "LDS histogram", who, (long long)NBK_SORT_LDS_INTS);
            return NBK_ERR_ARG;
        }
    }
    if (*ncoarse_all * *nfine >= ((int64_t)1 << 31)) {
        NBK_SET_ERR("%s: %lld cells, needs fewer than 2^31", who,
                    (long long)(*ncoarse_all * *nfine));
        return NBK_ERR_ARG;
    }
    return NBK_OK;
}

[[maybe_unused]] int fof_key(const char* who, const double origin[3],
                             const double inv_cell[3], const int ncoarse[3],
                             const int fine[3], FofGrid* g,
                             int64_t* ncoarse_all, int64_t* nfine)
{
    const int rc = fof_grid(who, ncoarse, fine, ncoarse_all, nfine);
    if (rc != NBK_OK) return rc;
    for (int i = 0; i < 3; i++) {
        g->origin[i] = origin[i];
        g->inv_cell[i] = inv_cell[i];
        g->ncoarse[i] = ncoarse[i];
        g->fine[i] = fine[i];
    }
    return NBK_OK;
}

[[maybe_unused]] int fof_check_n(const char* who, int64_t n) {
    if (n < 0 || n >= ((int64_t)1 << 31)) {
        NBK_SET_ERR("%s: n=%lld (needs 0 <= n < 2^31)", who, (long long)n);
        return NBK_ERR_ARG;
    }
    return NBK_OK;
}

}  // namespace
