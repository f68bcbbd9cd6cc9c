"""
Plain numpy references and seeded inputs for the FOF tests
(test_fof_cpu.py, test_gpu_fof_kernels.py, test_gpu_fof.py): a brute-force
friends-of-friends, restatements of the reference's label rule and centre
of mass, the block-major cell id of include/nbk_hip.h and the sorted
layout of the two-level cell sort.  Nothing here runs on the GPU.

The brute force rounds like the kernel (the library is built with
-ffp-contract=off): per axis d = (x_i - x_j) - s L, two roundings, for the
images s = -1, 0, 1, the smallest d * d of the three, and
r2 = (dx2 + dy2) + dz2.  Friends iff r2 <= ll * ll.  The ``margin`` it
returns, min |r2 - ll^2| / ll^2 over all off-diagonal pairs, says how far
the nearest pair is from flipping: tests that compare exactly first assert
margin >= 1e-10.
"""
import functools

import numpy

from sort_reference import canonical_rows                   # noqa: F401

MARGIN = 1e-10


# ---- brute-force FOF -----------------------------------------------------

def pair_r2(pos, box=None):
    """(n, n) squared separations, minimum image over s = -1, 0, 1 when
    ``box`` (3 values) is given; every operation rounded separately"""
    pos = numpy.asarray(pos, dtype='f8')
    n = len(pos)
    r2 = None
    for a in range(3):
        d = pos[:, None, a] - pos[None, :, a]
        d2 = d * d
        if box is not None:
            for s in (-1., 1.):
                ds = d - s * float(box[a])
                d2 = numpy.minimum(d2, ds * ds)
        # (dx2 + dy2) + dz2
        r2 = d2 if r2 is None else r2 + d2
    assert r2.shape == (n, n)
    return r2


def brute_fof(pos, ll, box=None):
    """(minid, margin) of a brute-force FOF: minid[i] is the smallest
    index of i's group"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    pos = numpy.asarray(pos, dtype='f8')
    n = len(pos)
    if n == 0:
        return numpy.zeros(0, dtype='i8'), numpy.inf
    r2 = pair_r2(pos, box)
    ll_sq = float(ll) * float(ll)
    linked = r2 <= ll_sq
    off = ~numpy.eye(n, dtype=bool)
    margin = numpy.inf
    if n > 1:
        margin = float((numpy.abs(r2 - ll_sq)[off]).min() / ll_sq)
    _, comp = connected_components(csr_matrix(linked), directed=False)
    smallest = numpy.full(comp.max() + 1, n, dtype='i8')
    numpy.minimum.at(smallest, comp, numpy.arange(n))
    return smallest[comp], margin


# ---- the label rule and the centre of mass --------------------------------

def labels_from_minid(minid, nmin):
    """the reference's _assign_labels on one rank, with its argsort made
    stable: Length <= nmin -> 0, the others 1..Nhalo by decreasing Length,
    among equal Lengths the larger minid first"""
    minid = numpy.asarray(minid, dtype='i8')
    if len(minid) == 0:
        return numpy.zeros(0, dtype='i4')
    uniq, inverse, length = numpy.unique(minid, return_inverse=True,
                                         return_counts=True)
    order = numpy.argsort(length, kind='stable')[::-1]
    label_of_group = numpy.zeros(len(uniq), dtype='i4')
    rank = 0
    for g in order:
        if length[g] > nmin:
            rank += 1
            label_of_group[g] = rank
    return label_of_group[inverse]


def centerofmass(label, pos, box, nhalo0):
    """the reference's centerofmass, group by group; NaN rows for labels
    without particles"""
    pos = numpy.asarray(pos, dtype='f8')
    out = numpy.full((nhalo0, pos.shape[1]), numpy.nan)
    for g in range(nhalo0):
        p = pos[label == g]
        if len(p) == 0:
            continue
        if box is None:
            out[g] = p.sum(axis=0) / len(p)
            continue
        L = numpy.ones(pos.shape[1]) * numpy.asarray(box, dtype='f8')
        pmin = p.min(axis=0)
        d = p - pmin
        d = numpy.where(d < -0.5 * L, d + L, d)
        d = numpy.where(d >= 0.5 * L, d - L, d)
        out[g] = numpy.remainder(pmin + d.sum(axis=0) / len(p), L)
    return out


def periodic_diff(a, b, box):
    """a - b wrapped into [-L/2, L/2): a centre at a face may be 0 or L"""
    L = numpy.asarray(box, dtype='f8')
    d = numpy.asarray(a, dtype='f8') - numpy.asarray(b, dtype='f8')
    return d - L * numpy.round(d / L)


# ---- the two-level cell grid ---------------------------------------------

def fine_cells(pos, origin, inv_cell, ncoarse, fine):
    """(n, 3) clamped fine cell per axis"""
    pos = numpy.asarray(pos, dtype='f8')
    n = numpy.asarray(ncoarse, dtype='i8') * numpy.asarray(fine, dtype='i8')
    c = numpy.floor((pos - numpy.asarray(origin, dtype='f8'))
                    * numpy.asarray(inv_cell, dtype='f8')).astype('i8')
    return numpy.minimum(numpy.maximum(c, 0), n - 1)


def coarse_ids(pos, origin, inv_cell, ncoarse, fine):
    c = fine_cells(pos, origin, inv_cell, ncoarse, fine)
    f = numpy.asarray(fine, dtype='i8')
    nc = [int(v) for v in ncoarse]
    q = c // f
    return (q[:, 0] * nc[1] + q[:, 1]) * nc[2] + q[:, 2]


def cell_ids(pos, origin, inv_cell, ncoarse, fine):
    """block-major cell id: coarse_id * nfine + sub_id, both row-major"""
    c = fine_cells(pos, origin, inv_cell, ncoarse, fine)
    f = [int(v) for v in fine]
    r = c % numpy.asarray(f, dtype='i8')
    sub = (r[:, 0] * f[1] + r[:, 1]) * f[2] + r[:, 2]
    nfine = f[0] * f[1] * f[2]
    return coarse_ids(pos, origin, inv_cell, ncoarse, fine) * nfine + sub


def sorted_reference(pos, index, ids, ncells):
    """(start, rows) of a catalogue sorted by cell: the start table
    (ncells + 1, [ncells] = n) and the canonical (cell, x, y, z, index)
    rows, which do not depend on the order inside a cell"""
    counts = numpy.bincount(ids, minlength=ncells)
    start = numpy.concatenate([[0], numpy.cumsum(counts)])
    return start, canonical_rows(numpy.asarray(pos),
                                 numpy.asarray(index, dtype='f8'), ids)


def sorted_keys(start):
    """the cell of every slot of a sorted array with start table ``start``"""
    return numpy.repeat(numpy.arange(len(start) - 1), numpy.diff(start))


def uniform_grid(box, ncoarse, fine):
    """(origin, inv_cell) of ncoarse * fine cells over [0, box) per axis"""
    box = numpy.asarray(box, dtype='f8') * numpy.ones(3)
    n = numpy.asarray(ncoarse, dtype='f8') * numpy.asarray(fine, dtype='f8')
    return numpy.zeros(3), n / box


# ---- seeded inputs --------------------------------------------------------

SEED = 12345
BOX = 100.


def _clustered():
    """24 Gaussian blobs (sigma 0.8) of 5..119 points, six of them centred
    within 0.2 of a box face, on 1500 uniform points; 3092 in all.

    Measured on this recipe with brute_fof (test_fof_cpu.py asserts the
    ones the tests lean on): at ll = 0.6, 1955 groups periodic and 1975
    non-periodic, the largest of 104, two of Length 72, margin 3.6e-4; at
    ll = 1.0, 1605 and 1622 groups, margin 5.3e-5."""
    rng = numpy.random.RandomState(SEED)
    centres = rng.uniform(size=(24, 3)) * BOX
    sizes = rng.randint(5, 120, 24)
    for k in range(6):
        centres[k, k % 3] = 0.1 if k < 3 else BOX - 0.1
    blobs = [c + 0.8 * rng.normal(size=(s, 3))
             for c, s in zip(centres, sizes)]
    background = rng.uniform(size=(1500, 3)) * BOX
    pos = numpy.remainder(numpy.concatenate(blobs + [background]), BOX)
    return pos[rng.permutation(len(pos))]


FILAMENT_LL = 0.5


def _filament():
    """1200 points spaced 0.9 ll along (1, 1, 1) from (95, 97, 1),
    jittered by +-1e-3, wrapped, on 800 uniform points.  Periodic: one
    group of exactly 1200; non-periodic: 1110 / 59 / 31; margin 1.1e-2."""
    rng = numpy.random.RandomState(SEED)
    step = 0.9 * FILAMENT_LL / numpy.sqrt(3.)
    chain = numpy.array([95., 97., 1.]) \
        + step * numpy.arange(1200)[:, None] * numpy.ones(3)
    chain = chain + rng.uniform(-1e-3, 1e-3, size=chain.shape)
    background = rng.uniform(size=(800, 3)) * BOX
    pos = numpy.remainder(numpy.concatenate([chain, background]), BOX)
    return pos[rng.permutation(len(pos))]


def lattice(nside, box):
    """the reference test's grid: nside^3 points, half-cell shifted"""
    g = numpy.arange(nside) * (float(box) / nside)
    grid = numpy.stack(numpy.meshgrid(g, g, g, indexing='ij'),
                       axis=-1).reshape(-1, 3)
    return grid + 0.5 * box / nside


def lattice_copies():
    """four copies of the 8^3 grid at offsets 0, +0.01, -0.01, +0.02 (the
    -0.01 copy is NOT wrapped here: the finder wraps it)"""
    grid = lattice(8, 8.) - 0.5
    return numpy.concatenate([grid, grid + 0.01, grid - 0.01, grid + 0.02])


_BUILDERS = {'clustered': _clustered, 'filament': _filament}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """positions (n, 3) of a named input, read-only"""
    pos = numpy.ascontiguousarray(_BUILDERS[name](), dtype='f8')
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def reference_minid(name, ll, periodic):
    """(minid, margin) of a named input, computed once"""
    box = [BOX] * 3 if periodic else None
    minid, margin = brute_fof(catalogue(name), ll, box)
    minid.setflags(write=False)
    return minid, margin


def group_lengths(minid):
    return numpy.sort(numpy.unique(minid, return_counts=True)[1])[::-1]
