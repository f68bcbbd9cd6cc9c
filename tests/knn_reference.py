"""
Plain numpy reference for the k-th-nearest-neighbour tests
(test_kddensity_cpu.py, test_gpu_knn_kernels.py, test_gpu_kddensity.py):
a brute force over fof_reference.pair_r2, which rounds like the kernel
(per axis d = x_i - x_j, the smallest of d * d, (d - L) * (d - L),
(d + L) * (d + L) when periodic, r2 = (dx2 + dy2) + dz2), and the
reference's density formula.  Nothing here runs on the GPU.
"""
import functools

import numpy

import fof_reference as ref


MAX_K = 16


def knn_table(pos, box=None):
    """(r2, index), each (n, 16): the 16 nearest OTHER points of every
    point in the order (r2, index), padded with ``inf`` and ``-1`` beyond
    the n - 1 there are.  O(n^2)."""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    n = len(pos)
    r2_out = numpy.full((n, MAX_K), numpy.inf)
    index_out = numpy.full((n, MAX_K), -1, dtype='i4')
    if n < 2:
        return r2_out, index_out
    # every row without its diagonal entry, the columns still in index
    # order: a stable sort by r2 is then the order (r2, index)
    off = ~numpy.eye(n, dtype=bool)
    r2 = ref.pair_r2(pos, box)[off].reshape(n, n - 1)
    idx = numpy.broadcast_to(numpy.arange(n), (n, n))[off].reshape(n, n - 1)
    m = min(MAX_K, n - 1)
    order = numpy.argsort(r2, axis=1, kind='stable')[:, :m]
    r2_out[:, :m] = numpy.take_along_axis(r2, order, axis=1)
    index_out[:, :m] = numpy.take_along_axis(idx, order, axis=1)
    return r2_out, index_out


def knn_brute(pos, k, box=None):
    """(r2, index) of the k-th nearest OTHER point of every point, the
    candidates ordered by the pair (r2, index); ``inf`` and ``-1`` with
    fewer than k other points"""
    assert 1 <= k <= MAX_K
    r2, index = knn_table(pos, box)
    return r2[:, k - 1].copy(), index[:, k - 1].copy()


def density(pos, box):
    """the reference's KDDensity: 1 / (d_unit^3 V) = 1 / d^3, d the
    distance to the 7th other point under the minimum image"""
    box = numpy.ones(3) * numpy.asarray(box, dtype='f8')
    r2, _ = knn_brute(pos, 7, box)
    with numpy.errstate(divide='ignore'):
        return 1.0 / numpy.sqrt(r2) ** 3


def scipy_density(pos, box):
    """(density, d) the way the reference asks scipy: coordinates scaled
    to the unit box, cKDTree(boxsize=1).query(k=[8]); ``box`` a scalar"""
    from scipy.spatial import cKDTree
    L = float(box)
    xpos = numpy.asarray(pos, dtype='f8') / L
    xpos %= 1
    d, _ = cKDTree(xpos, boxsize=1.0).query(xpos, k=[8])
    d = d[:, 0]
    with numpy.errstate(divide='ignore'):
        return 1 / (d ** 3 * L ** 3), d * L


def uniform(n, box, seed=7):
    """n uniform points in [0, box) per axis (box: a scalar or 3 values)"""
    rng = numpy.random.RandomState(seed)
    return rng.uniform(size=(n, 3)) * numpy.asarray(box, dtype='f8')


@functools.lru_cache(maxsize=None)
def reference_table(name, periodic):
    """knn_table of a named input of fof_reference in its box of 100,
    computed once, read-only"""
    r2, index = knn_table(ref.catalogue(name),
                          [ref.BOX] * 3 if periodic else None)
    r2.setflags(write=False)
    index.setflags(write=False)
    return r2, index
