"""
FiberCollisions on the GPU against the brute force of fibers_reference.py,
run on the positions the class itself holds (``r.source['Position']``):
exact equality of Label, Collided and NeighborID.
"""
import numpy
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import fibers_reference as fref                                 # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.lab import FiberCollisions                    # noqa: E402

NAMES = ('Label', 'Collided', 'NeighborID')


def columns(r):
    return [numpy.asarray(r.labels[name]) for name in NAMES]


def check_against_brute_force(r):
    pos = numpy.asarray(r.source['Position'])
    want = fref.run(pos, r._collision_radius_rad, r.attrs['seed'])
    for name, got, w in zip(NAMES, columns(r), want):
        assert got.dtype == numpy.dtype('i4'), name
        assert_array_equal(got, w, err_msg=name)
    return want


@pytest.fixture(scope='module')
def reference_run():
    """the input of the reference's test_fibercolls, seed 42"""
    numpy.random.seed(42)
    ra = 10. * numpy.random.random(size=10000)
    dec = 5. * numpy.random.random(size=10000) - 5.0
    return ra, dec, FiberCollisions(ra, dec, degrees=True, seed=42)


def test_reference_input_invariants(reference_run):
    ra, dec, r = reference_run
    pos = numpy.asarray(r.source['Position'])
    collided = numpy.asarray(r.labels['Collided'])
    clean_pairs, lonely = fref.invariants(pos, r._collision_radius_rad,
                                          collided)
    assert clean_pairs == 0, "objects in 'clean' sample within the radius"
    assert lonely == 0, "collided objects that collide with nothing"


def test_reference_input_exact(reference_run):
    ra, dec, r = reference_run
    pos = numpy.asarray(r.source['Position'])
    assert pos.dtype == numpy.dtype('f8') and pos.shape == (10000, 3)
    assert_array_equal(pos, fref.positions(ra, dec))
    label, collided, neighbour = check_against_brute_force(r)
    assert label.max() == 773 and (label > 0).sum() == 1647
    assert collided.sum() == 817
    assert r.attrs == {'collision_radius': 62 / 60. / 60., 'seed': 42,
                       'degrees': True}
    assert r._collision_radius_rad == numpy.deg2rad(62 / 60. / 60.)
    assert_array_equal(r.source.attrs['BoxSize'], [2.2, 2.2, 2.2])
    assert_array_equal(r.labels.attrs['BoxSize'], [2.2, 2.2, 2.2])
    assert r.labels.csize == 10000


@pytest.mark.parametrize('seed', [None, 0, 42])
def test_three_and_four_points(seed):
    r = FiberCollisions([0., 1., 2.], [0., 0., 0.], collision_radius=1.5,
                        seed=seed)
    assert_array_equal(r.labels['Collided'], [0, 1, 0])
    assert_array_equal(r.labels['Label'], [1, 1, 1])
    assert_array_equal(r.labels['NeighborID'], [-1, 0, -1])
    r = FiberCollisions([0., 1., 2., 10.], [0., 0., 0., 0.],
                        collision_radius=1.5, seed=seed)
    assert_array_equal(r.labels['Collided'], [0, 1, 0, 0])
    assert_array_equal(r.labels['Label'], [1, 1, 1, 0])
    assert_array_equal(r.labels['NeighborID'], [-1, 0, -1, -1])


def dense_patch(s):
    rng = numpy.random.RandomState(s)
    return rng.uniform(0, 1, 2000), rng.uniform(-0.5, 0.5, 2000)


def test_dense_patch():
    ra, dec = dense_patch(2)
    r = FiberCollisions(ra, dec, collision_radius=0.025, seed=7)
    label, _, _ = check_against_brute_force(r)
    cap = hiplib.require().nbk_fibers_max_group()
    assert 64 < numpy.bincount(label)[1:].max() <= cap


def test_radians():
    ra, dec = dense_patch(1)
    ra, dec = ra[:500], dec[:500]
    r = FiberCollisions(numpy.deg2rad(ra), numpy.deg2rad(dec),
                        collision_radius=0.05, seed=3, degrees=False)
    # the radius stays in degrees
    assert r._collision_radius_rad == numpy.deg2rad(0.05)
    assert r.attrs['degrees'] is False
    label, collided, _ = check_against_brute_force(r)
    assert collided.sum() > 0


def test_device_tensor_inputs():
    ra, dec = dense_patch(3)
    r = FiberCollisions(torch.from_numpy(ra).cuda(),
                        torch.from_numpy(dec).cuda(),
                        collision_radius=0.02, seed=9)
    pos = numpy.asarray(r.source['Position'])
    assert pos.dtype == numpy.dtype('f8') and pos.shape == (2000, 3)
    # the device's cos and sin may differ from the host's in the last place
    numpy.testing.assert_allclose(pos, fref.positions(ra, dec), rtol=0,
                                  atol=1e-14)
    _, collided, _ = check_against_brute_force(r)
    assert collided.sum() > 0


def test_seeds(reference_run):
    ra, dec, r = reference_run
    again = FiberCollisions(ra, dec, degrees=True, seed=42)
    for a, b in zip(columns(r), columns(again)):
        assert a.tobytes() == b.tobytes()
    other = FiberCollisions(ra, dec, degrees=True, seed=43)
    assert_array_equal(other.labels['Label'], r.labels['Label'])
    assert (numpy.asarray(other.labels['Collided'])
            != numpy.asarray(r.labels['Collided'])).any()
    check_against_brute_force(other)


def test_seed_none_is_recorded():
    ra, dec = dense_patch(1)
    r = FiberCollisions(ra, dec, collision_radius=0.01)
    seed = r.attrs['seed']
    assert 0 <= int(seed) < 4294967295
    again = FiberCollisions(ra, dec, collision_radius=0.01, seed=seed)
    for a, b in zip(columns(r), columns(again)):
        assert_array_equal(a, b)
    check_against_brute_force(r)


@pytest.mark.parametrize('n', [0, 1])
def test_fewer_than_two_objects(n):
    r = FiberCollisions(numpy.arange(n, dtype='f8'), numpy.zeros(n), seed=1)
    label, collided, neighbour = columns(r)
    assert_array_equal(label, numpy.zeros(n))
    assert_array_equal(collided, numpy.zeros(n))
    assert_array_equal(neighbour, numpy.full(n, -1))


def test_group_above_the_cap():
    cap = hiplib.require().nbk_fibers_max_group()
    rng = numpy.random.RandomState(5)
    # 1100 points within 20 arcsec of one another, radius 62 arcsec
    ra = 5. + rng.uniform(0, 1e-2 / 3.6, 1100)
    dec = rng.uniform(0, 1e-2 / 3.6, 1100)
    assert cap < 1100
    with pytest.raises(ValueError, match='1100 members.*up to %d' % cap):
        FiberCollisions(ra, dec, seed=1)


def test_assign_fibers_wants_contiguous_rows():
    from nbodykit_amd.algorithms.fibercollisions import assign_fibers
    label = torch.zeros(5, dtype=torch.int32, device='cuda')
    rows = torch.zeros((3, 5), dtype=torch.float64, device='cuda').T
    with pytest.raises(ValueError, match='contiguous'):
        assign_fibers(rows, label, 0.1, 1)
    with pytest.raises(ValueError, match='contiguous'):
        assign_fibers(rows.contiguous().float(), label, 0.1, 1)
    collided, neighbour = assign_fibers(rows.contiguous(), label, 0.1, 1)
    assert_array_equal(collided.cpu().numpy(), numpy.zeros(5))
    assert_array_equal(neighbour.cpu().numpy(), numpy.full(5, -1))


def test_radius_limit():
    with pytest.raises(ValueError, match='0.2 rad'):
        FiberCollisions([0., 1.], [0., 0.], collision_radius=11.46)
    # just below it runs
    r = FiberCollisions([0., 11., 30.], [0., 0., 0.],
                        collision_radius=11.45, seed=1)
    assert_array_equal(r.labels['Label'], [1, 1, 0])
    check_against_brute_force(r)
