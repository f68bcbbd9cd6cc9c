"""
Plain numpy references and input catalogues for the kernel-level tests
of the pair counter (test_gpu_pairs_kernels.py), self-checked in
test_paircount_cpu.py.  The pair counts themselves come from
paircount_bruteforce.py.

The cell of a particle is the documented (include/nbk_hip.h)
``clamp(floor((p - origin) * inv_cell), 0, ncell - 1)`` per axis,
flattened as ``(cx * ncell[1] + cy) * ncell[2] + cz`` — the subtraction
and the product each round once (the library is built with
-ffp-contract=off), so the f64 numpy expression is bit-identical.
"""
import functools

import numpy

# the bit-exact multiset comparison and the count-matrix scheme are those
# of the locality sorts
from sort_reference import (canonical_rows, chunk_histograms,  # noqa: F401
                            scan_matrix)


# ---- cell keys and the sorted layout ----------------------------------

def cell_ids(pos, origin, inv_cell, ncell):
    """flattened cell id of every row of ``pos`` (n, 3), int64"""
    pos = numpy.asarray(pos, dtype='f8')
    origin = numpy.asarray(origin, dtype='f8')
    inv_cell = numpy.asarray(inv_cell, dtype='f8')
    n = numpy.asarray(ncell, dtype='i8')
    c = numpy.floor((pos - origin) * inv_cell).astype('i8')
    c = numpy.minimum(numpy.maximum(c, 0), n - 1)
    return (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]


def sorted_reference(pos, w, ids, ncells):
    """(start, rows) of a catalogue sorted by cell: the cell-start table
    (ncells + 1, [ncells] = n) and the canonical (cell, x, y, z, w) rows,
    which do not depend on the order inside a cell."""
    counts = numpy.bincount(ids, minlength=ncells)
    start = numpy.concatenate([[0], numpy.cumsum(counts)])
    return start, canonical_rows(numpy.asarray(pos), w, ids)


def sorted_keys(start):
    """the cell of every slot of a sorted array with start table ``start``"""
    return numpy.repeat(numpy.arange(len(start) - 1), numpy.diff(start))


def uniform_grid(box, ncell):
    """(origin, inv_cell) of ``ncell`` cells over [0, box) per axis"""
    box = numpy.asarray(box, dtype='f8') * numpy.ones(3)
    return numpy.zeros(3), numpy.asarray(ncell, dtype='f8') / box


# ---- catalogues -------------------------------------------------------

HBOX = (40., 50., 64.)
LATBOX = (20., 18., 16.)


def weights(n):
    return numpy.random.RandomState(1).uniform(size=n)


def _slab():
    rng = numpy.random.RandomState(21)
    sheet = rng.uniform(size=(500, 3)) * (300., 120., 35.) \
        + (-50., 7., 1000.)
    blob = rng.normal(size=(600, 3)) * 2. + (100., 60., 1015.)
    return numpy.concatenate([sheet, blob])


def _planar():
    pos = _slab()
    pos[:, 1] = 3.25
    return pos


def _lattice():
    g = numpy.meshgrid(numpy.arange(10.), numpy.arange(9.),
                       numpy.arange(8.), indexing='ij')
    return numpy.stack(g, axis=-1).reshape(-1, 3)


def _latdup():
    g = _lattice()
    return numpy.concatenate([g, g[::18]])


_BUILDERS = {
    # uniform in the anisotropic periodic box HBOX
    'H1': lambda: numpy.random.RandomState(11).uniform(size=(1300, 3))
    * HBOX,
    'H2': lambda: numpy.random.RandomState(12).uniform(size=(700, 3))
    * HBOX,
    # a thin sheet far from the origin plus a blob of 600 points that
    # lands in one or two cells
    'SLAB': _slab,
    # ... the interleaved halves of it (their cross pairs are a subset
    # of SLAB's auto pairs, so SLAB's edge margins bound theirs)
    'SLAB_EVEN': lambda: _slab()[0::2],
    'SLAB_ODD': lambda: _slab()[1::2],
    # ... flattened into a plane that contains the line of sight
    'PLANAR': _planar,
    # the 10 x 9 x 8 integer lattice of LATBOX, and with 40 rows doubled
    'LAT': _lattice,
    'LATDUP': _latdup,
    # ~ one particle per 8 cells of the largest legal grid
    'BIG': lambda: numpy.random.RandomState(31).uniform(size=(5000, 3))
    * HBOX,
}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """(positions (n, 3), weights (n,)) of a named catalogue, read-only"""
    pos = numpy.ascontiguousarray(_BUILDERS[name](), dtype='f8')
    w = weights(len(pos))
    pos.setflags(write=False)
    w.setflags(write=False)
    return pos, w


def bounding_box(*names):
    """joint (lo, hi) of named catalogues"""
    allpos = numpy.concatenate([catalogue(n)[0] for n in names])
    return allpos.min(axis=0), allpos.max(axis=0)


def clamp_rows(origin, inv_cell, ncell, n=3001, seed=41):
    """(n, 3) hand-placed rows for a grid: every coordinate is a value
    below the origin, exactly at it, on an interior cell boundary, at or
    above the top edge — each with its two neighbouring doubles — or
    +-0.0, or (half of the rows) uniform over the grid.  A zero
    ``inv_cell`` (flat axis) puts everything into cell 0 of that axis."""
    rng = numpy.random.RandomState(seed)
    pos = numpy.empty((n, 3), dtype='f8')
    for ax in range(3):
        o, inv, nc = float(origin[ax]), float(inv_cell[ax]), int(ncell[ax])
        side = 1.0 / inv if inv > 0 else 1.0
        top = o + nc * side
        marks = [o, top, o - 0.3 * side, o - 2.5 * side * nc,
                 top + 0.4 * side, top + 3.0 * side * nc]
        marks += [o + k * side for k in sorted(set([1, nc // 2, nc - 1]))
                  if 0 < k < nc]
        pool = []
        for v in marks:
            pool += [v, numpy.nextafter(v, -numpy.inf),
                     numpy.nextafter(v, numpy.inf)]
        pool += [0.0, -0.0]
        pool = numpy.array(pool, dtype='f8')
        fill = rng.uniform(o, top, size=n)
        pick = pool[rng.randint(0, len(pool), size=n)]
        pos[:, ax] = numpy.where(rng.uniform(size=n) < 0.5, pick, fill)
        # every mark at least once
        pos[ax:ax + 3 * len(pool):3, ax] = pool
    return pos
