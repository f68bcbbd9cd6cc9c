"""
KDDensity — a proxy density from the distance to the 7th nearest
neighbour (reference nbodykit/algorithms/kdtree.py).  The reference asks
scipy's ``cKDTree(xpos, boxsize=1.0).query(xpos, k=[8])``, whose first
neighbour is the point itself; here it is a k-th-nearest-neighbour search
on the two-level cell list of the FOF finder, csrc/nbk_knn.hip.

Semantics (DESIGN.md "Nearest neighbours"): the squared distance is
``(dx2 + dy2) + dz2`` with the minimum image per axis of a periodic run;
the k-th neighbour is the k-th OTHER particle in the order (r2, input
index), so coincident points are neighbours at distance 0 and the result
is bitwise reproducible.
"""
import logging

import numpy

from nbodykit_amd import hiplib, profiling
from .fof import _as_tensor, fof_grid, two_level_sort

# particles per cell of the search grid (DESIGN.md "Nearest neighbours",
# the per_cell table: the fastest of 1, 2, 4, 8 on the lognormal
# catalogue)
PER_CELL = 2.


def knn(pos, k, box=None, periodic=True, per_cell=PER_CELL, info=None):
    """
    (r2, index) of the k-th nearest other particle of every particle:
    an f64 and an int32 CUDA tensor in input order, ``inf`` and ``-1``
    with fewer than k other particles.

    pos: (n, 3) f64 CUDA rows, already wrapped into ``box`` (3 values) for
    a periodic run.  The grid has about ``per_cell`` particles per cell,
    over the box, or over the bounding box when not periodic.  ``info``,
    if a dict, receives the grid and the start table.
    """
    import torch
    lib = hiplib.require()
    n = int(pos.shape[0])
    k = int(k)
    if not 1 <= k <= int(lib.nbk_knn_max_k()):
        raise ValueError("k must lie in [1, %d], got %d"
                         % (lib.nbk_knn_max_k(), k))
    if not per_cell > 0:
        raise ValueError("per_cell must be positive, got %r" % (per_cell,))
    dev = torch.device('cuda')
    if n == 0:
        return (torch.empty(0, dtype=torch.float64, device=dev),
                torch.empty(0, dtype=torch.int32, device=dev))

    lo = hi = None
    if not periodic:
        lo, hi = pos.amin(dim=0).tolist(), pos.amax(dim=0).tolist()
    grid = fof_grid(periodic, box, 0., n, lo, hi, per_cell=float(per_cell))
    origin, inv_cell, ncoarse, fine = grid
    spos, sindex, fine_start = two_level_sort(pos, grid, stage='knn')

    r2 = torch.empty(n, dtype=torch.float64, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    with profiling.collect('knn_search', units=n):
        hiplib.check(lib.nbk_knn_f64(
            hiplib.dptr(spos), hiplib.dptr(fine_start), hiplib.dptr(sindex),
            n, hiplib.f64_arr(origin), hiplib.f64_arr(inv_cell),
            hiplib.int_arr(ncoarse), hiplib.int_arr(fine),
            hiplib.f64_arr(box if periodic else [0.0, 0.0, 0.0]),
            1 if periodic else 0, k, hiplib.dptr(r2), hiplib.dptr(index),
            hiplib.cur_stream()), 'nbk_knn_f64')
    if info is not None:
        info.update(ncoarse=ncoarse, fine=fine, origin=origin,
                    inv_cell=inv_cell, fine_start=fine_start)
    return r2, index


class KDDensity(object):
    """
    Estimate a proxy density based on the distance to the nearest
    neighbours: ``density = 1 / d**3``, d the distance to the 7th other
    particle under the minimum image (the reference's
    ``1 / (d_unit**3 * V)`` of a cubic box).  The result is proportional
    to the density but the scale is unspecified.

    Parameters follow ``nbodykit.algorithms.KDDensity``: ``source`` must
    hold the 'Position' column and ``attrs['BoxSize']`` (a scalar or three
    values); ``margin`` (the reference's padding of its parallel domains)
    is recorded only.  Columns may be numpy arrays or device tensors.

    A non-cubic box is accepted: the metric here is the physical one.  The
    reference asserts a cubic box only because it rescales the coordinates
    to the unit box before the query.

    The result is :attr:`density`, a numpy f8 array in input order; fewer
    than 8 particles give 0 everywhere, as the reference does.
    """
    logger = logging.getLogger('KDDensity')

    # the reference queries k = [8], the point itself included
    NEIGHBOUR = 7

    def __init__(self, source, margin=1.0):
        if 'Position' not in source:
            raise ValueError("please specify the 'Position' column in the "
                             "input source")
        self.comm = source.comm
        self._source = source

        if 'BoxSize' not in source.attrs:
            raise ValueError("please specify 'BoxSize' in the input source "
                             "'attrs'")
        BoxSize = numpy.array(source.attrs['BoxSize'], dtype='f8')
        if BoxSize.ndim == 0 or len(BoxSize) == 1:
            BoxSize = numpy.ones(3) * BoxSize
        if BoxSize.shape != (3,) or not (numpy.isfinite(BoxSize).all()
                                         and (BoxSize > 0).all()):
            raise ValueError("BoxSize must be a positive scalar or three "
                             "positive values, got %r"
                             % (source.attrs['BoxSize'],))

        self.attrs = {}
        self.attrs['BoxSize'] = BoxSize
        # (the reference's formula, although the name suggests its inverse)
        self.attrs['meansep'] = (source.csize / BoxSize.prod()) \
            ** (1.0 / len(BoxSize))
        self.attrs['margin'] = margin

        position = source['Position']
        if len(position.shape) != 2 or position.shape[1] != 3:
            raise ValueError("the 'Position' column must have shape (N, 3)")
        if source.csize >= 2 ** 31:
            raise ValueError("KDDensity handles fewer than 2^31 particles")

        import torch
        if not bool(torch.isfinite(_as_tensor(position)).all()):
            raise ValueError("'Position' holds non-finite values")

        if self.comm.size > 1:
            raise NotImplementedError("KDDensity runs on a single rank")

        self.run()

    def run(self):
        """Compute the density proxy on the GPU; sets :attr:`density`, a
        unit-less value per particle in input order: the inverse cube of
        the distance to the 7th nearest other particle."""
        from .pair_counters import kernel
        hiplib.require()
        n = len(self._source['Position'])
        if n == 0:
            # no kernel is launched
            self.density = numpy.zeros(0, dtype='f8')
            return
        box = self.attrs['BoxSize']
        pos, _ = kernel.to_device_columns(self._source['Position'], None,
                                          [0, 1, 2])
        pos = kernel.wrap_periodic(pos, box)
        r2, _ = knn(pos, self.NEIGHBOUR, box=box, periodic=True)
        with profiling.collect('knn_density', units=n):
            d = r2.sqrt()
            density = 1.0 / (d * d * d)
        self.density = density.cpu().numpy()
