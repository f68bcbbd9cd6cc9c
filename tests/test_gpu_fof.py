"""
FOF through the public API on the GPU, against the brute force and the
numpy restatements of fof_reference.py.

``labels`` is compared exactly: the random inputs first assert, on the
reference, that no pair lies within relative 1e-10 of ll^2, and labels
are a function of ``minid`` alone (ties included, DESIGN.md
"Friends-of-friends").  Centres of mass are f4 columns of f64 means:
CMPosition within 2^-22 BoxSize (two f4 ulps at L) of the restatement per
component, as a periodic difference since a centre at a face may come out
as 0 or as L; CMVelocity within 2^-22 max|v|.
"""
import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import fof_reference as ref                                     # noqa: E402
from nbodykit_amd.lab import (FOF, ArrayCatalog, LinearPower,    # noqa: E402
                              LogNormalCatalog, Planck15)
from nbodykit_amd.source.catalog.device import \
    DeviceArrayCatalog                                           # noqa: E402

BOX3 = [ref.BOX] * 3


def catalog(pos, **attrs):
    return ArrayCatalog({'Position': numpy.array(pos)}, **attrs)


def run(pos, ll, nmin, periodic=True, absolute=True, **attrs):
    if periodic or not absolute:
        attrs.setdefault('BoxSize', ref.BOX)
    return FOF(catalog(pos, **attrs), ll, nmin, absolute=absolute,
               periodic=periodic)


def velocities(n):
    return numpy.random.RandomState(3).normal(size=(n, 3)) * 300.


# ---- labels -----------------------------------------------------------------

@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('ll', [0.6, 1.0])
def test_labels_clustered(ll, periodic):
    pos = ref.catalogue('clustered')
    minid, margin = ref.reference_minid('clustered', ll, periodic)
    assert margin >= ref.MARGIN
    for nmin in (0, 5, 20):
        f = run(pos, ll, nmin, periodic)
        want = ref.labels_from_minid(minid, nmin)
        assert f.labels.dtype == numpy.int32
        assert_array_equal(f.labels, want)
        assert f.max_label == [want.max()]
        again = run(pos, ll, nmin, periodic)
        assert_array_equal(again.labels, f.labels)


def test_labels_clustered_relative_linking_length():
    pos = ref.catalogue('clustered')
    mean_sep = (ref.BOX ** 3 / len(pos)) ** (1. / 3)
    for ll in (0.6, 1.0):
        minid, _ = ref.reference_minid('clustered', ll, True)
        b = ll / mean_sep
        # the product b * mean_sep is ll to an ulp, far inside the margin
        assert abs(b * mean_sep - ll) <= 1e-15
        for box in (ref.BOX, BOX3):
            f = run(pos, b, 5, absolute=False, BoxSize=box)
            assert_array_equal(f.labels, ref.labels_from_minid(minid, 5))
            assert f.attrs['linking_length'] == b
            assert not f.attrs['absolute']


@pytest.mark.parametrize('periodic', [True, False])
def test_labels_filament(periodic):
    minid, margin = ref.reference_minid('filament', ref.FILAMENT_LL,
                                        periodic)
    assert margin >= ref.MARGIN
    for nmin in (0, 40):
        f = run(ref.catalogue('filament'), ref.FILAMENT_LL, nmin, periodic)
        assert_array_equal(f.labels, ref.labels_from_minid(minid, nmin))
    if periodic:
        assert numpy.bincount(f.labels)[1] == 1200


def test_lattices_of_the_reference():
    # one particle per group
    grid = ref.lattice(8, 8.)
    f = FOF(catalog(grid, BoxSize=[8., 8., 8.], Nmesh=[8, 8, 8]), 0.9, 0)
    assert_array_equal(numpy.sort(f.labels), numpy.arange(1, 513))
    # 512 chains of 4 across the periodic face
    f = FOF(catalog(ref.lattice_copies(), BoxSize=[8., 8., 8.],
                    Nmesh=[8, 8, 8]),
            0.011 * 3 ** 0.5, 0, absolute=True)
    assert f.labels.max() == 512 and f.labels.min() == 1
    assert (numpy.bincount(f.labels)[1:] == 4).all()
    assert_array_equal(f.labels[:512], f.labels[1024:1536])
    # fully connected: nmin = 63 keeps the group, nmin = 64 drops it
    grid = ref.lattice(4, 4.) - 0.5
    cat = catalog(grid, BoxSize=[4., 4., 4.], Nmesh=[4, 4, 4])
    assert_array_equal(FOF(cat, 2, 63, absolute=True).labels, 1)
    assert_array_equal(FOF(cat, 2, 64, absolute=True).labels, 0)


def test_permuted_rows_give_the_same_partition():
    pos = numpy.array(ref.catalogue('clustered'))
    perm = numpy.random.RandomState(8).permutation(len(pos))
    a = run(pos, 0.6, 5)
    b = run(pos[perm], 0.6, 5)
    la, lb = a.labels[perm], b.labels
    # the same particles are in no group, and the same pairs share one
    assert_array_equal(la == 0, lb == 0)
    assert_array_equal(numpy.bincount(la), numpy.bincount(lb))
    pairs = numpy.unique(numpy.stack([la, lb]), axis=1)
    assert pairs.shape[1] == la.max() + 1
    # Length is unchanged as well
    assert_array_equal(numpy.bincount(a.labels)[1:],
                       numpy.bincount(b.labels)[1:])


def test_device_columns_give_the_same_labels():
    pos = numpy.array(ref.catalogue('clustered'))
    want = run(pos, 0.6, 5).labels
    dcat = DeviceArrayCatalog({'Position': torch.as_tensor(pos).cuda()},
                              BoxSize=ref.BOX)
    assert_array_equal(FOF(dcat, 0.6, 5, absolute=True).labels, want)
    f4 = catalog(pos.astype('f4').astype('f8'), BoxSize=ref.BOX)
    f4b = ArrayCatalog({'Position': pos.astype('f4')}, BoxSize=ref.BOX)
    assert_array_equal(FOF(f4b, 0.6, 5, absolute=True).labels,
                       FOF(f4, 0.6, 5, absolute=True).labels)


def test_nothing_and_one():
    f = run(numpy.zeros((0, 3)), 0.5, 0)
    assert f.labels.shape == (0,) and f.max_label == [0]
    f = run(numpy.array([[1., 2., 3.]]), 0.5, 0)
    assert_array_equal(f.labels, [1])
    f = run(numpy.array([[1., 2., 3.]]), 0.5, 1, periodic=False)
    assert_array_equal(f.labels, [0])


# ---- find_features -------------------------------------------------------------

def test_find_features_clustered():
    pos = numpy.array(ref.catalogue('clustered'))
    vel = velocities(len(pos))
    dens = numpy.random.RandomState(4).uniform(size=len(pos))
    minid, _ = ref.reference_minid('clustered', 0.6, True)
    label = ref.labels_from_minid(minid, 5)
    nh = label.max() + 1
    cat = ArrayCatalog({'Position': pos, 'Velocity': vel, 'Density': dens,
                        'InitialPosition': pos}, BoxSize=ref.BOX)
    f = FOF(cat, 0.6, 5, absolute=True)
    halos = f.find_features(peakcolumn='Density')
    assert halos.csize == nh
    assert halos.attrs['nmin'] == 5 and halos.attrs['BoxSize'] == ref.BOX
    length = numpy.asarray(halos['Length'])
    assert length[0] == 0 and length.dtype == numpy.int32
    assert_array_equal(length[1:], numpy.bincount(label)[1:])
    cm = numpy.asarray(halos['CMPosition'])
    assert cm.dtype == numpy.float32
    want = ref.centerofmass(label, pos, BOX3, nh)
    assert numpy.abs(ref.periodic_diff(cm[1:], want[1:], BOX3)).max() \
        <= 2. ** -22 * ref.BOX
    wantv = ref.centerofmass(label, vel, None, nh)
    assert numpy.abs(numpy.asarray(halos['CMVelocity'])[1:]
                     - wantv[1:]).max() <= 2. ** -22 * numpy.abs(vel).max()
    assert_array_equal(numpy.asarray(halos['InitialPosition'])[1:], cm[1:])
    for g in (1, nh // 2, nh - 1):
        members = numpy.flatnonzero(label == g)
        top = members[numpy.argmax(dens[members])]
        assert_allclose(numpy.asarray(halos['PeakPosition'])[g], pos[top],
                        rtol=1e-6)
    # without the optional columns
    plain = FOF(ArrayCatalog({'Position': pos, 'Velocity': vel},
                             BoxSize=ref.BOX), 0.6, 5,
                absolute=True).find_features()
    assert 'PeakPosition' not in plain and 'InitialPosition' not in plain
    with pytest.raises(ValueError, match='Velocity'):
        run(pos, 0.6, 5).find_features()


def test_shifted_nonperiodic_runs_agree():
    pos = numpy.array(ref.catalogue('clustered'))
    vel = velocities(len(pos))
    dens = numpy.random.RandomState(4).uniform(size=len(pos))
    peaks = []
    for shift in (-100., 100.):
        cat = ArrayCatalog({'Position': pos + shift, 'Velocity': vel,
                            'Density': dens})
        f = FOF(cat, 0.6, 5, periodic=False, absolute=True)
        peaks.append(f.find_features(peakcolumn='Density'))
    p1, p2 = peaks
    assert p1.csize == p2.csize > 10
    for col, add in (('CMPosition', 200.), ('CMVelocity', 0.),
                     ('PeakPosition', 200.), ('PeakVelocity', 0.)):
        assert_allclose(numpy.asarray(p1[col])[1:] + add,
                        numpy.asarray(p2[col])[1:], rtol=1e-6)
    assert_array_equal(numpy.asarray(p1['Length']),
                       numpy.asarray(p2['Length']))


def test_lognormal_invariants():
    Plin = LinearPower(Planck15, redshift=0.55, transfer='EisensteinHu')
    source = LogNormalCatalog(Plin=Plin, nbar=3e-3, BoxSize=128., Nmesh=32,
                              seed=42)
    f = FOF(source, linking_length=0.2, nmin=20)
    n = source.csize
    assert f.labels.shape == (n,)
    counts = numpy.bincount(f.labels)[1:]
    assert (numpy.diff(counts) <= 0).all() and (counts > 20).all()
    halos = f.find_features()
    length = numpy.asarray(halos['Length'])
    assert length.sum() + (f.labels == 0).sum() == n
    assert_array_equal(length[1:], counts)
    again = FOF(source, linking_length=0.2, nmin=20)
    assert_array_equal(again.labels, f.labels)
