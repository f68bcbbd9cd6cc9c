"""
Plain numpy references for the locality-sort and gather-paint kernel
tests (test_gpu_sort_kernels.py), self-checked against brute-force
Python loops in test_sort_tables_cpu.py.

Everything here is int64 / float64 numpy.  The cell index is
``floor(x * (N / box))`` with exactly the kernels' operand order — the
library is built with -ffp-contract=off, so the product rounds once and
the result is bit-identical — wrapped with ``numpy.remainder``.
"""
import numpy

WINDOWS = ('cic', 'tsc', 'pcs')


# ---- cell / bucket keys -----------------------------------------------

def inv_h(nmesh, box):
    return numpy.asarray(nmesh, dtype='f8') / numpy.asarray(box, dtype='f8')


def floor_index(pos, nmesh, box):
    """unwrapped integer cell index per axis, shape (n, 3) int64"""
    return numpy.floor(numpy.asarray(pos, dtype='f8')
                       * inv_h(nmesh, box)).astype('i8')


def cell_index(pos, nmesh, box):
    """wrapped (ix, iy, iz), shape (n, 3) int64"""
    return numpy.remainder(floor_index(pos, nmesh, box),
                           numpy.asarray(nmesh, dtype='i8'))


def cell_ids(pos, nmesh, box):
    i = cell_index(pos, nmesh, box)
    n0, n1, n2 = (int(x) for x in nmesh)
    return (i[:, 0] * n1 + i[:, 1]) * n2 + i[:, 2]


def row_ids(pos, nmesh, box):
    i = cell_index(pos, nmesh, box)
    return i[:, 0] * int(nmesh[1]) + i[:, 1]


def coarse_keys(pos, nmesh, box, ys):
    """two-level sort coarse key: ix * (n1 >> ys) + (iy >> ys)"""
    i = cell_index(pos, nmesh, box)
    return i[:, 0] * (int(nmesh[1]) >> ys) + (i[:, 1] >> ys)


def pair_keys(pos, nmesh, box, gs, dlo, dhi):
    """pair-bucket sort keys: (k1, k2) with k2 = -1 where the particle
    has a single copy.  Bucket = (ix // 2) * (n1 >> gs) + group, group
    taken at rows iy+dlo and iy+dhi (wrapped)."""
    n1 = int(nmesh[1])
    ix = cell_index(pos, nmesh, box)[:, 0]
    iy = floor_index(pos, nmesh, box)[:, 1]
    ng = n1 >> gs
    g1 = numpy.remainder(iy + dlo, n1) >> gs
    g2 = numpy.remainder(iy + dhi, n1) >> gs
    base = (ix >> 1) * ng
    return base + g1, numpy.where(g1 == g2, -1, base + g2)


def chunk_histograms(keys, nbuck, chunk):
    """per-chunk histogram matrix (ceil(n/chunk), nbuck) of one or more
    key arrays (entries < 0 are skipped)"""
    if not isinstance(keys, (tuple, list)):
        keys = (keys,)
    n = len(keys[0])
    nblocks = -(-n // chunk)
    mat = numpy.zeros((nblocks, nbuck), dtype='i8')
    for c in range(nblocks):
        for k in keys:
            kc = k[c * chunk:(c + 1) * chunk]
            mat[c] += numpy.bincount(kc[kc >= 0], minlength=nbuck)
    return mat


def scan_matrix(mat):
    """(bases, bucket_bases) of a (nblocks, nbuck) count matrix:
    bucket_bases[b] = sum of all buckets < b over every chunk (total at
    [nbuck]); bases[c][b] = bucket_bases[b] + sum of bucket b over
    chunks < c."""
    mat = numpy.asarray(mat, dtype='i8')
    colsum = mat.sum(axis=0)
    bucket_bases = numpy.concatenate([[0], numpy.cumsum(colsum)])
    within = numpy.cumsum(mat, axis=0) - mat
    return bucket_bases[:-1][None, :] + within, bucket_bases


def row_table(sorted_row_ids, nrows):
    """start of each row in a row-sorted array (without the sentinel)"""
    return numpy.searchsorted(sorted_row_ids, numpy.arange(nrows),
                              side='left')


# ---- bit-exact multiset comparison ------------------------------------

def canonical_rows(pos_rows, mass=None, key=None):
    """int64 bit-pattern rows [key, x, y, z, (m)] in a canonical order:
    two arrays hold the same multiset of (key, position, mass) exactly
    when their canonical forms are equal.  Bit patterns keep -0.0 and
    0.0 apart, as a moved (not recomputed) value must be."""
    cols = [numpy.ascontiguousarray(pos_rows[:, j]).view('i8')
            for j in range(3)]
    if mass is not None:
        cols.append(numpy.ascontiguousarray(mass, dtype='f8').view('i8'))
    if key is not None:
        cols.insert(0, numpy.asarray(key, dtype='i8'))
    a = numpy.stack(cols, axis=1)
    return a[numpy.lexsort(a.T[::-1])]


# ---- input catalogues -------------------------------------------------

def edge_pool(N, L):
    """the adversarial coordinates of one axis: cell boundaries, half
    cells (the TSC / interlacing boundary), the box ends and out-of-box
    values, with their neighbouring doubles"""
    H = L / N
    ks = sorted(set([0, 1, N // 2, max(N - 2, 0), N - 1]))
    pool = []
    for k in ks:
        for v in (k * H, k * H + H / 2):
            pool += [v, numpy.nextafter(v, -numpy.inf),
                     numpy.nextafter(v, numpy.inf)]
    pool += [0.0, -0.0, L, numpy.nextafter(L, 0.0),
             -H / 3, -L - H / 4, L + H / 7, 2.5 * L]
    pool = numpy.array(pool, dtype='f8')
    assert numpy.isfinite(pool).all() and (numpy.abs(pool) <= 3 * L).all()
    return pool


def edge_positions(nmesh, box, n, seed):
    """(n, 3) positions: every coordinate is, with probability 1/2, a
    value of :func:`edge_pool`, otherwise uniform in [0, L)"""
    rng = numpy.random.RandomState(seed)
    pos = numpy.empty((n, 3), dtype='f8')
    for ax in range(3):
        pool = edge_pool(int(nmesh[ax]), float(box[ax]))
        fill = rng.uniform(0, box[ax], size=n)
        pick = pool[rng.randint(0, len(pool), size=n)]
        pos[:, ax] = numpy.where(rng.uniform(size=n) < 0.5, pick, fill)
    return pos


def _in_cell(rng, cell, nmesh, box, n):
    H = numpy.asarray(box, dtype='f8') / numpy.asarray(nmesh, dtype='f8')
    return (numpy.asarray(cell) + rng.uniform(0.01, 0.99, size=(n, 3))) * H


def clustered_positions(nmesh, box, n, seed):
    """every particle inside ONE cell"""
    rng = numpy.random.RandomState(seed)
    cell = [1 % int(nmesh[0]), 5 % int(nmesh[1]), 7 % int(nmesh[2])]
    return _in_cell(rng, cell, nmesh, box, n)


def last_row_positions(nmesh, box, n, seed):
    """every particle in plane n0-1, row n1-1 (the row whose end is the
    row table's sentinel), z uniform over the box"""
    rng = numpy.random.RandomState(seed)
    pos = _in_cell(rng, [int(nmesh[0]) - 1, int(nmesh[1]) - 1, 0],
                   nmesh, box, n)
    pos[:, 2] = rng.uniform(0, box[2], size=n)
    return pos


CATALOGUES = {
    'edge': lambda nmesh, box: edge_positions(nmesh, box, 20011, 101),
    'clustered': lambda nmesh, box: clustered_positions(nmesh, box,
                                                        10000, 102),
    'last_row': lambda nmesh, box: last_row_positions(nmesh, box,
                                                      20011, 103),
}


def masses(n, seed=7):
    return numpy.random.RandomState(seed).uniform(0.5, 1.5, size=n)


# ---- the oracle's deposit stencil along one axis -----------------------

def axis_deposits(x, N, L, window, shift, coords='kernel'):
    """Per-particle weight the ORACLE stencil (oracle.paint's generators)
    deposits at each row offset relative to floor(x * (N / L)), along
    one axis.  Returns (offsets, weights, u) with weights shaped
    (len(offsets), n); the other two axes are summed out (their weights
    are a partition of unity).

    ``coords`` picks the mesh coordinate the stencil is evaluated at:
    'kernel' = x * (N / L) + shift, the expression the floor is taken
    from (and the kernels use); 'oracle' = x / H + shift, the expression
    oracle.paint itself uses — up to ~2 ulp(u) away from the former."""
    import importlib
    # the module, not the oracle.paint() function the package re-exports
    opaint = importlib.import_module('oracle.paint')
    x = numpy.asarray(x, dtype='f8')
    H = L / N
    u = numpy.empty((len(x), 3), dtype='f8')
    if coords == 'oracle':
        u[:, 0] = x / H + shift
    else:
        u[:, 0] = x * (N / L) + shift
    u[:, 1:] = 0.25
    if window == 'cic':
        gen = opaint._cic_offsets_weights(u)
    elif window == 'tsc':
        gen = opaint._centered_offsets_weights(u, (-1, 0, 1),
                                               opaint._tsc_w, nearest=True)
    else:
        gen = opaint._centered_offsets_weights(u, (-1, 0, 1, 2),
                                               opaint._pcs_w, nearest=False)
    ref = numpy.floor(x * (N / L))
    offsets = numpy.arange(-4, 6)
    weights = numpy.zeros((len(offsets), len(x)))
    idx = numpy.arange(len(x))
    for ix, _iy, _iz, w in gen:
        d = (ix - ref).astype('i8') - offsets[0]
        assert d.min() >= 0 and d.max() < len(offsets)
        numpy.add.at(weights, (d, idx), w)
    return offsets, weights, u[:, 0]
