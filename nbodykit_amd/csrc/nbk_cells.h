// The cell of a particle and the neighbour walk of the cell-list kernels
// (nbk_pairs.hip, nbk_3pcf.hip, nbk_fof.hip): one axis of the <= 27
// (cell, shift) neighbours.
#pragma once
#include "nbk_common.h"

// the clamped cell of a coordinate along one axis of n cells
__device__ __forceinline__ int cell_axis(double x, double origin,
                                         double inv_cell, int n) {
    int c = (int)floor((x - origin) * inv_cell);
    c = c < 0 ? 0 : c;
    return c >= n ? n - 1 : c;
}

// one axis of the neighbour walk: offset d = -1, 0, +1 of cell c
__device__ __forceinline__ bool neighbour_axis(int c, int d, int n,
                                               int periodic, double L,
                                               int* c2, double* shift) {
    const int raw = c + d;
    if (raw >= 0 && raw < n) {
        *c2 = raw;
        *shift = 0.0;
        return true;
    }
    if (!periodic) return false;
    if (raw < 0) {
        *c2 = raw + n;
        *shift = -L;
    } else {
        *c2 = raw - n;
        *shift = L;
    }
    return true;
}
