"""
KDDensity without a GPU: the brute force of knn_reference.py against
scipy's kd-tree, the way the reference asks it, and the constructor's
checks, attributes and exports.

Tolerance of the scipy comparison: the reference scales coordinates to the
unit box, which costs about 2^-53 absolute in box units per coordinate;
every input first asserts d_min >= 1e-4 L, so that is at most about 1e-12
relative in d.  rtol = 1e-9 leaves three orders of margin.
"""
import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import fof_reference as ref
import knn_reference as kref
from nbodykit_amd.lab import ArrayCatalog
from nbodykit_amd.algorithms import kdtree


def make_cat(n=64, **attrs):
    pos = numpy.random.RandomState(5).uniform(size=(n, 3)) * 10.
    return ArrayCatalog({'Position': pos}, **attrs)


def constructed(cat, **kwargs):
    """a KDDensity whose constructor ran as far as it gets here: without
    a GPU the attributes are set before the run fails"""
    kd = object.__new__(kdtree.KDDensity)
    try:
        kdtree.KDDensity.__init__(kd, cat, **kwargs)
    except RuntimeError:
        pass
    return kd


# ---- the brute force against scipy ------------------------------------------

@pytest.mark.parametrize('name', ['uniform', 'clustered'])
def test_brute_force_agrees_with_the_kd_tree(name):
    if name == 'uniform':
        pos = kref.uniform(500, ref.BOX)
    else:
        # the blobs and some of the background
        pos = numpy.array(ref.catalogue('clustered'))[:500]
    r2, index = kref.knn_brute(pos, 7, [ref.BOX] * 3)
    want_density, want_d = kref.scipy_density(pos, ref.BOX)
    assert want_d.min() >= 1e-4 * ref.BOX
    assert_allclose(numpy.sqrt(r2), want_d, rtol=1e-9, atol=0)
    assert_allclose(kref.density(pos, ref.BOX), want_density, rtol=1e-9,
                    atol=0)
    assert ((index >= 0) & (index < 500)).all()
    assert (index != numpy.arange(500)).all()


def test_brute_force_order_and_too_few_points():
    # four points on a line; 0 and 3 are coincident
    pos = numpy.array([[1., 0, 0], [2., 0, 0], [4., 0, 0], [1., 0, 0]])
    r2, index = kref.knn_brute(pos, 1)
    assert_array_equal(r2, [0., 1., 4., 0.])
    # point 1 is at distance 1 of both 0 and 3: the smaller index wins
    assert_array_equal(index, [3, 0, 1, 0])
    r2, index = kref.knn_brute(pos, 2)
    assert_array_equal(r2, [1., 1., 9., 1.])
    assert_array_equal(index, [1, 3, 0, 1])
    r2, index = kref.knn_brute(pos, 3, [5., 5., 5.])
    # periodic: 4 is at distance 2 of 1 across the face
    assert_array_equal(r2, [4., 4., 4., 4.])
    assert_array_equal(index, [2, 2, 3, 2])
    for k in (4, 7):
        r2, index = kref.knn_brute(pos, k)
        assert numpy.isinf(r2).all() and (index == -1).all()
    assert_array_equal(kref.density(pos, 5.), 0.)


# ---- constructor, attributes, exports ---------------------------------------

def test_exports():
    from nbodykit_amd import lab
    from nbodykit_amd.algorithms import KDDensity
    assert lab.KDDensity is KDDensity is kdtree.KDDensity


def test_missing_inputs_raise_before_any_gpu_call():
    with pytest.raises(ValueError, match='Position'):
        kdtree.KDDensity(ArrayCatalog({'Velocity': numpy.zeros((4, 3))},
                                      BoxSize=10.))
    with pytest.raises(ValueError, match='BoxSize'):
        kdtree.KDDensity(make_cat())
    for bad in (numpy.nan, numpy.inf):
        cat = make_cat(BoxSize=10.)
        pos = numpy.array(cat['Position'])
        pos[7, 1] = bad
        cat['Position'] = pos
        with pytest.raises(ValueError, match='non-finite'):
            kdtree.KDDensity(cat)


def test_more_than_one_rank_is_not_implemented():
    cat = make_cat(BoxSize=10.)

    class TwoRanks(object):
        size = 2
        rank = 0
    cat.comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        kdtree.KDDensity(cat)


@pytest.mark.parametrize('box', [10., [10.], [10., 10., 10.],
                                 [10., 20., 5.]])
def test_attrs_follow_the_reference(box):
    cat = make_cat(n=64, BoxSize=box)
    kd = constructed(cat, margin=2.5)
    box3 = numpy.ones(3) * numpy.asarray(box, dtype='f8')
    assert sorted(kd.attrs) == ['BoxSize', 'margin', 'meansep']
    assert kd.attrs['BoxSize'].shape == (3,)
    assert kd.attrs['BoxSize'].dtype == numpy.dtype('f8')
    assert_array_equal(kd.attrs['BoxSize'], box3)
    # the reference's formula: (N / V)^(1/3), although the name suggests
    # its inverse
    assert kd.attrs['meansep'] == (64 / box3.prod()) ** (1.0 / 3)
    assert kd.attrs['margin'] == 2.5
    assert constructed(cat).attrs['margin'] == 1.0


def test_the_search_grid_leaves_the_fof_grid_alone():
    from nbodykit_amd.algorithms import fof
    n, L = 100000, 250.
    for ll in (0.3, 2.0):
        a = fof.fof_grid(True, [L] * 3, ll, n)
        b = fof.fof_grid(True, [L] * 3, ll, n, per_cell=2.)
        for u, v in zip(a, b):
            assert_array_equal(u, v)
    # per_cell particles per cell, before the split into two levels
    for per_cell in (1., 2., 4., 8.):
        _, inv_cell, ncoarse, fine = fof.fof_grid(True, [L] * 3, 0., n,
                                                  per_cell=per_cell)
        ncell = numpy.array(ncoarse) * numpy.array(fine)
        side = (per_cell * L ** 3 / n) ** (1. / 3)
        assert_array_equal(ncell[0], ncell)
        assert L / ncell[0] >= side
        assert ncell[0] >= int(L / side) - max(fine)
        assert_allclose(inv_cell, ncell / L, rtol=1e-15)
