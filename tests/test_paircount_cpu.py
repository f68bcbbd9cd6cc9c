"""
CPU coverage of the pair-counting feature: argument validation (which
runs before the GPU is needed), the loud failure without a GPU, the
weighted pair totals, the analytic-randoms filling factors, the natural
and Landy-Szalay formulas, multipoles and wp of a constant wedge, JSON
round-trips of synthetic results, the cell-grid picker, the
brute-force oracle itself on the lattice, and the references, inputs and
edge margins of the kernel-level tests (pairs_reference.py).
"""
import warnings

import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import paircount_bruteforce as bf
import pairs_reference as pref
from nbodykit_amd.lab import (ArrayCatalog, UniformCatalog,
                              SimulationBoxPairCount, SimulationBox2PCF)
from nbodykit_amd.algorithms.pair_counters import kernel, simbox
from nbodykit_amd.algorithms.pair_counters.simbox import prepare_attrs
from nbodykit_amd.algorithms.paircount_tpcf import (WedgeBinnedStatistic,
                                                    estimators, tpcf)

EDGES = numpy.linspace(10, 150, 10)


@pytest.fixture(scope='module')
def cat():
    return UniformCatalog(nbar=3e-6, BoxSize=512., seed=42)


# ---- validation ---------------------------------------------------------

BAD_ARGUMENTS = {
    'bad mode': dict(mode='3d'),
    'zero edge': dict(edges=[0., 10., 20.]),
    'negative edge': dict(edges=[-1., 10., 20.]),
    '2d without Nmu': dict(mode='2d'),
    'Nmu in 1d': dict(mode='1d', Nmu=10),
    'Nmu in projected': dict(mode='projected', pimax=40, Nmu=10),
    'projected without pimax': dict(mode='projected'),
    'pimax in 1d': dict(mode='1d', pimax=40),
    'pimax in 2d': dict(mode='2d', Nmu=10, pimax=40),
    'pimax below 1': dict(mode='projected', pimax=0.5),
    'los name': dict(los='a'),
    'los index': dict(los=3),
    'los vector': dict(los=[0, 0, 1]),
    'missing position': dict(position='Nope'),
    'missing weight': dict(weight='Nope'),
    'BoxSize keyword mismatch': dict(BoxSize=256.),
    'rmax above half box': dict(edges=[10., 300.]),
    'pimax above half box': dict(mode='projected', pimax=300),
}


@pytest.mark.parametrize('case', sorted(BAD_ARGUMENTS))
def test_validation_raises_value_error(cat, case):
    kw = dict(mode='1d', edges=EDGES)
    kw.update(BAD_ARGUMENTS[case])
    mode, edges = kw.pop('mode'), kw.pop('edges')
    with pytest.raises(ValueError):
        SimulationBoxPairCount(mode, cat, edges, **kw)


def test_boxsize_validation():
    pos = numpy.random.RandomState(0).uniform(size=(10, 3)) * 100
    nobox = ArrayCatalog({'Position': pos})
    with pytest.raises(ValueError, match='BoxSize'):
        SimulationBoxPairCount('1d', nobox, [1., 10.])
    a = ArrayCatalog({'Position': pos}, BoxSize=100.)
    b = ArrayCatalog({'Position': pos}, BoxSize=200.)
    with pytest.raises(ValueError, match='mismatch'):
        SimulationBoxPairCount('1d', a, [1., 10.], second=b)
    # the keyword supplies a missing box
    attrs = prepare_attrs('1d', nobox, [1., 10.], BoxSize=100.)
    assert_array_equal(attrs['BoxSize'], [100., 100., 100.])


def test_negative_los_wraps(cat):
    assert prepare_attrs('1d', cat, EDGES, los=-1)['los'] == 2
    assert prepare_attrs('1d', cat, EDGES, los=-3)['los'] == 0
    assert prepare_attrs('1d', cat, EDGES, los='y')['los'] == 1
    with pytest.raises(ValueError):
        prepare_attrs('1d', cat, EDGES, los=-4)


def test_not_implemented_cases(cat):
    pos = numpy.random.RandomState(0).uniform(size=(10, 3)) * 100
    slab = ArrayCatalog({'Position': pos}, BoxSize=[100., 100., 200.])
    with pytest.raises(NotImplementedError):
        SimulationBoxPairCount('1d', slab, [1., 10.])
    with pytest.raises(NotImplementedError):
        SimulationBoxPairCount('angular', cat, [1., 10.])
    with pytest.raises(NotImplementedError):
        SimulationBox2PCF('angular', cat, [1., 10.])
    # a non-periodic run has no use for a cubic box
    assert prepare_attrs('1d', slab, [1., 10.], periodic=False)


def test_multi_rank_not_implemented(cat):
    class TwoRanks(object):
        size, rank = 2, 0

        def allreduce(self, x, op='sum'):
            return x

    two = ArrayCatalog({'Position': numpy.asarray(cat['Position'])},
                       BoxSize=512.)
    two.comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        SimulationBoxPairCount('1d', two, EDGES)


def test_2pcf_needs_randoms_when_not_periodic(cat):
    with pytest.raises(ValueError, match='randoms'):
        SimulationBox2PCF('1d', cat, EDGES, periodic=False)


def test_compute_fails_loudly_without_gpu(cat):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SimulationBoxPairCount('1d', cat, EDGES)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SimulationBox2PCF('2d', cat, EDGES, Nmu=5)


# ---- attrs --------------------------------------------------------------

def test_attrs_and_weighted_totals():
    rng = numpy.random.RandomState(1)
    pos1 = rng.uniform(size=(50, 3)) * 100
    pos2 = rng.uniform(size=(70, 3)) * 100
    w1, w2 = rng.uniform(size=50), rng.uniform(size=70)
    c1 = ArrayCatalog({'Position': pos1, 'Weight': w1}, BoxSize=100.)
    c2 = ArrayCatalog({'Position': pos2, 'Weight': w2}, BoxSize=100.)

    auto = prepare_attrs('2d', c1, [1., 10., 20.], Nmu=4, los='x',
                         show_progress=True, config=dict(nthreads=2))
    assert sorted(auto) == sorted(
        ['mode', 'edges', 'Nmu', 'pimax', 'show_progress', 'N1', 'N2',
         'total_wnpairs', 'is_cross', 'BoxSize', 'periodic', 'weight',
         'position', 'config', 'los'])
    assert auto['N1'] == 50 and auto['N2'] is None
    assert auto['is_cross'] is False
    assert_allclose(auto['total_wnpairs'],
                    0.5 * (w1.sum() ** 2 - (w1 ** 2).sum()), rtol=1e-14)
    assert auto['los'] == 0 and auto['Nmu'] == 4 and auto['pimax'] is None
    assert auto['config'] == dict(nthreads=2)
    assert auto['show_progress'] is True and auto['periodic'] is True

    # second is first: still an auto-correlation
    same = prepare_attrs('1d', c1, [1., 10.], second=c1)
    assert same['is_cross'] is False and same['N2'] == 50
    assert same['total_wnpairs'] == auto['total_wnpairs']

    cross = prepare_attrs('1d', c1, [1., 10.], second=c2)
    assert cross['is_cross'] is True
    assert cross['N1'] == 50 and cross['N2'] == 70
    assert_allclose(cross['total_wnpairs'], 0.5 * w1.sum() * w2.sum(),
                    rtol=1e-14)

    # the default Weight column counts plain pairs
    plain = prepare_attrs('1d', ArrayCatalog({'Position': pos1},
                                             BoxSize=100.), [1., 10.])
    assert plain['total_wnpairs'] == 0.5 * 50 * 49


# ---- analytic randoms and estimators ------------------------------------

def test_filling_factors():
    r = numpy.linspace(10, 150, 10)
    box = numpy.array([512., 512., 512.])
    V = 512. ** 3
    f1 = estimators.filling_factor('1d', {'r': r}, box)
    assert_allclose(f1, 4. / 3 * numpy.pi * numpy.diff(r ** 3) / V,
                    rtol=1e-14)
    mu = numpy.linspace(0, 1, 11)
    f2 = estimators.filling_factor('2d', {'r': r, 'mu': mu}, box)
    assert f2.shape == (9, 10)
    assert_allclose(f2.sum(axis=-1), f1, rtol=1e-13)
    pi = numpy.linspace(0, 40, 41)
    f3 = estimators.filling_factor('projected', {'rp': r, 'pi': pi}, box)
    assert f3.shape == (9, 40)
    assert_allclose(f3.sum(axis=-1),
                    numpy.pi * numpy.diff(r ** 2) * 2 * 40 / V, rtol=1e-13)


def test_analytic_randoms_counts():
    r = numpy.array([1., 2., 4.])
    auto = estimators.analytic_randoms('1d', ['r'], {'r': r}, 100., 1000)
    fill = 4. / 3 * numpy.pi * numpy.diff(r ** 3) / 1e6
    assert_allclose(auto['npairs'], 1000. ** 2 * fill, rtol=1e-14)
    assert_array_equal(auto['wnpairs'], auto['npairs'])
    assert auto.attrs['total_wnpairs'] == 1000 * 999 / 2.
    cross = estimators.analytic_randoms('1d', ['r'], {'r': r}, 100.,
                                        1000, 500)
    assert_allclose(cross['npairs'], 1000. * 500 * fill, rtol=1e-14)
    assert cross.attrs['total_wnpairs'] == 1000 * 500 / 2.


def test_natural_formula():
    DD = numpy.array([10., 40., 0.])
    RR = numpy.array([20., 20., 5.])
    corr = estimators.natural_corr(DD, 100., RR, 200.)
    assert_allclose(corr, [0., 3., -1.], rtol=1e-15)


def test_landy_szalay_formula_and_nan_branch():
    DD = numpy.array([30., 12., 7.])
    DR = numpy.array([50., 20., 3.])
    RD = numpy.array([40., 22., 5.])
    RR = numpy.array([100., 40., 0.])
    npairs = numpy.array([100, 40, 0], dtype='u8')
    corr = estimators.landy_szalay_corr(DD, DR, RD, RR, 10., 20., 40.,
                                        80., npairs)
    # f = 8, 4, 2
    assert_allclose(corr[:2], [(240. - 200. - 80.) / 100. + 1,
                               (96. - 80. - 44.) / 40. + 1], rtol=1e-15)
    assert numpy.isnan(corr[2])


class FakeCount(object):
    """a pair counter returning prepared counts (no GPU)"""
    table = {}
    calls = []

    def __init__(self, first=None, second=None, **kws):
        FakeCount.calls.append((first.name,
                                None if second is None else second.name))
        key = (first.name, None if second is None else second.name)
        wn, total = FakeCount.table[key]
        data = numpy.zeros(len(wn), dtype=[('r', 'f8'), ('npairs', 'u8'),
                                           ('wnpairs', 'f8')])
        data['npairs'] = wn
        data['wnpairs'] = wn
        data['r'] = 1.0
        self.pairs = simbox.make_pairs('1d', [1., 2., 3.], None, None,
                                       data)
        self.attrs = {'total_wnpairs': total}


class Named(object):
    def __init__(self, name):
        from nbodykit_amd.comm import SerialComm
        self.name, self.comm = name, SerialComm()


def test_landy_szalay_estimator_counts_and_warns():
    D, R = Named('D'), Named('R')
    FakeCount.table = {('R', 'R'): (numpy.array([100., 0.]), 80.),
                       ('D', None): (numpy.array([30., 7.]), 10.),
                       ('D', 'R'): (numpy.array([50., 3.]), 20.)}
    FakeCount.calls = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        D1D2, D1R2, D2R1, R1R2, corr = estimators.LandySzalayEstimator(
            FakeCount, D, None, R, None, mode='1d')
    assert FakeCount.calls == [('R', 'R'), ('D', None), ('D', 'R')]
    assert D2R1 is D1R2
    assert_allclose(corr['corr'][0], (8 * 30. - 2 * 4 * 50.) / 100. + 1)
    assert numpy.isnan(corr['corr'][1])
    assert any('empty separation bins' in str(w.message) for w in caught)
    assert isinstance(corr, WedgeBinnedStatistic)
    assert corr.variables == ['corr', 'r']

    # a supplied R1R2 is reused; a cross-correlation counts D2 x R1 too
    D2 = Named('D2')
    FakeCount.table.update({('D', 'D2'): (numpy.array([30., 7.]), 10.),
                            ('D2', 'R'): (numpy.array([40., 5.]), 40.)})
    R1R2 = FakeCount(first=R, second=R)
    FakeCount.calls = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        out = estimators.LandySzalayEstimator(FakeCount, D, D2, R, None,
                                              R1R2=R1R2, mode='1d')
    assert FakeCount.calls == [('D', 'D2'), ('D', 'R'), ('D2', 'R')]
    assert_allclose(out[4]['corr'][0],
                    (8 * 30. - 4 * 50. - 2 * 40.) / 100. + 1)


def wedge(corr2d, redges, medges, second='mu'):
    x = 'r' if second == 'mu' else 'rp'
    data = numpy.zeros(corr2d.shape, dtype=[('corr', 'f8'), (x, 'f8')])
    data['corr'] = corr2d
    data[x] = (0.5 * (redges[1:] + redges[:-1]))[:, None]
    return WedgeBinnedStatistic([x, second], [redges, medges], data)


def test_to_poles_constant_wedge():
    redges = numpy.array([1., 2., 3., 4.])
    medges = numpy.linspace(0, 1, 6)
    w = wedge(numpy.full((3, 5), 2.5), redges, medges)
    poles = w.to_poles([0, 2])
    assert poles.dims == ['r'] and poles.attrs['poles'] == [0, 2]
    assert_allclose(poles['corr_0'], 2.5, rtol=1e-15)
    mid = 0.5 * (medges[1:] + medges[:-1])
    midpoint = (5 * 0.5 * (3 * mid ** 2 - 1) * 0.2).sum() * 2.5
    # the five terms (each up to 2.5 in size) largely cancel
    assert_allclose(poles['corr_2'], midpoint, rtol=0,
                    atol=2.5 * 16 * 2.0 ** -53)
    assert_allclose(poles['r'], [1.5, 2.5, 3.5])


def test_wp_constant_corr():
    redges = numpy.array([1., 2., 3.])
    piedges = numpy.linspace(0, 40, 41)
    corr = wedge(numpy.full((2, 40), 0.25), redges, piedges, second='pi')
    wp = tpcf.compute_wp(corr)
    assert wp.dims == ['rp'] and wp.shape == (2,)
    assert_allclose(wp['corr'], 2 * 0.25 * 40, rtol=1e-15)
    assert_allclose(wp['rp'], [1.5, 2.5])


# ---- JSON round-trips ---------------------------------------------------

def synthetic_paircount(mode, **kw):
    rng = numpy.random.RandomState(3)
    edges = numpy.array([1., 2., 4., 8.])
    dims, edges2 = simbox.second_dim(mode, kw.get('Nmu'), kw.get('pimax'))
    shape = (3,) if edges2 is None else (3, len(edges2) - 1)
    npairs = rng.randint(0, 100, size=shape).astype('u8')
    data = simbox.pairs_data(dims[0], npairs, rng.uniform(size=shape),
                             npairs * 2.5)
    obj = object.__new__(SimulationBoxPairCount)
    obj.__setstate__({'pairs': data, 'attrs': {
        'mode': mode, 'edges': edges, 'Nmu': kw.get('Nmu'),
        'pimax': kw.get('pimax'), 'total_wnpairs': 12.5,
        'BoxSize': numpy.array([64., 64., 64.]), 'config': {},
        'is_cross': False, 'N1': 7, 'N2': None}})
    from nbodykit_amd.comm import SerialComm
    obj.comm = SerialComm()
    return obj


@pytest.mark.parametrize('mode,kw', [('1d', {}), ('2d', dict(Nmu=4)),
                                     ('projected', dict(pimax=5))])
def test_paircount_json_roundtrip(tmp_path, mode, kw):
    r = synthetic_paircount(mode, **kw)
    out = str(tmp_path / 'pairs.json')
    r.save(out)
    r2 = SimulationBoxPairCount.load(out)
    assert r2.pairs.dims == r.pairs.dims
    assert r2.pairs.data.dtype == r.pairs.data.dtype
    for name in r.pairs.variables:
        assert_array_equal(r2.pairs[name], r.pairs[name])
    for d in r.pairs.dims:
        assert_array_equal(r2.pairs.edges[d], r.pairs.edges[d])
    assert r2.pairs.attrs['total_wnpairs'] == 12.5
    assert r2.attrs['N2'] is None and r2.attrs['mode'] == mode
    assert_array_equal(r2.attrs['BoxSize'], [64., 64., 64.])


def test_2pcf_json_roundtrip(tmp_path):
    DD = synthetic_paircount('projected', pimax=5)
    DD.attrs['periodic'] = True
    R1R2, corr = estimators.NaturalEstimator(DD)
    t = object.__new__(SimulationBox2PCF)
    t.comm = DD.comm
    t.attrs = {'mode': 'projected', 'edges': DD.attrs['edges'],
               'Nmu': None, 'pimax': 5, 'config': {}}
    t.corr, t.D1D2, t.R1R2 = corr, DD.pairs, R1R2
    t.D1R2 = t.D2R1 = None
    t.wp = tpcf.compute_wp(corr)
    out = str(tmp_path / 'tpcf.json')
    t.save(out)
    t2 = SimulationBox2PCF.load(out)
    assert isinstance(t2.corr, WedgeBinnedStatistic)
    assert t2.corr.dims == ['rp', 'pi']
    assert_array_equal(t2.corr['corr'], t.corr['corr'])
    assert_array_equal(t2.wp['corr'], t.wp['corr'])
    assert t2.wp.dims == ['rp']
    assert_array_equal(t2.D1D2['npairs'], DD.pairs['npairs'])
    assert_array_equal(t2.R1R2['wnpairs'], R1R2['wnpairs'])
    assert t2.D1R2 is None and t2.D2R1 is None
    assert t2.attrs['pimax'] == 5


# ---- cell grid ----------------------------------------------------------

def test_cell_grid_picker():
    # periodic: floor(L / rmax) cells of side >= rmax
    _, inv, ncell = kernel.make_grid(True, [100.] * 3, 50.)
    assert ncell == [2, 2, 2]
    assert_allclose(inv, 0.02)
    assert kernel.make_grid(True, [100.] * 3, 40.)[2] == [2, 2, 2]
    assert kernel.make_grid(True, [100.] * 3, 12.)[2] == [8, 8, 8]
    assert kernel.make_grid(True, [512.] * 3, 150.)[2] == [3, 3, 3]
    # projected: the 3-D reach is the diagonal of (rp, pi)
    rmax = kernel.max_3d_separation('projected', [1., 50.], 50.)
    assert_allclose(rmax, numpy.sqrt(5000.))
    assert kernel.make_grid(True, [100.] * 3, rmax)[2] == [1, 1, 1]
    # capped so that the cell histogram fits the LDS
    ncell = kernel.make_grid(True, [1000.] * 3, 1.)[2]
    assert numpy.prod(ncell) <= 40960
    # a cell side within rounding of rmax gives way to a wider cell
    assert kernel.cells_along(300., 100.) == 2
    # non-periodic: over the bounding box, degenerate extents allowed
    origin, inv, ncell = kernel.make_grid(False, None, 32.,
                                          [0., 0., 5.], [56., 56., 5.])
    assert ncell == [1, 1, 1] and inv[2] == 0.
    assert_array_equal(origin, [0., 0., 5.])


def test_candidate_pair_count():
    # 2 cells per axis, periodic: every cell is visited 27 times
    start = numpy.arange(0, 9 * 3, 3)
    assert kernel.candidate_pairs(start, start, [2, 2, 2], True) \
        == 8 * 3 * 27 * 3
    # non-periodic: only the 8 real cells, once each
    assert kernel.candidate_pairs(start, start, [2, 2, 2], False) \
        == 8 * 3 * 8 * 3


# ---- the oracle on the lattice ------------------------------------------

def test_bruteforce_lattice_hand_values():
    """8^3 lattice of spacing 8 in L = 64: 6 neighbours at r = 8, 12 at
    8 sqrt(2), 8 at 8 sqrt(3); r = 8 belongs to [8, 12), r = 32 is
    dropped."""
    pos = bf.lattice_positions()
    edges = [4, 8, 12, 16, 24, 32]
    want = bf.bruteforce_paircount('1d', pos, edges, 64.)
    assert_array_equal(want['npairs'][:3], [0, 18 * 512, 8 * 512])
    assert want['margin0'] == 0.            # pairs exactly on edges
    # all ordered pairs within r < 32 of a point of the periodic lattice
    g = numpy.arange(-4, 4) * 8.
    d2 = (g[:, None, None] ** 2 + g[None, :, None] ** 2
          + g[None, None, :] ** 2).ravel()
    hand = [((d2 >= lo * lo) & (d2 < hi * hi)).sum() * 512
            for lo, hi in zip(edges[:-1], edges[1:])]
    assert_array_equal(want['npairs'], hand)
    assert want['mean'][0] == 0. and want['wnpairs'][0] == 0.
    # a sequential sum of 4096 equal terms
    assert_allclose(want['mean'][2], 8 * numpy.sqrt(3.),
                    rtol=4100 * 2.0 ** -53)
    assert_array_equal(want['wnpairs'], want['npairs'])

    # mu exactly 0 lands in the first bin, exactly 1 in the last
    w2 = bf.bruteforce_paircount('2d', pos, edges, 64., Nmu=4)
    assert_array_equal(w2['npairs'][1], [8 * 512, 0, 8 * 512, 2 * 512])
    assert_array_equal(w2['npairs'].sum(axis=-1), want['npairs'])
    assert w2['n_mu1'] > 0

    # non-periodic: the corner point has 3 neighbours at r = 8
    w3 = bf.bruteforce_paircount('1d', pos, edges, 64., periodic=False)
    assert w3['npairs'][1] == 2 * (3 * 7 * 64) + 2 * (3 * 2 * 49 * 8)


# ---- the references of the kernel-level tests ----------------------------

def test_cell_ids_hand_values():
    """clamp(floor((p - origin) * inv_cell), 0, ncell - 1) per axis,
    flattened (cx * ncy + cy) * ncz + cz, on a 4 x 3 x 2 grid of side
    (2, 0.5, 8) at origin (-1, 10, 0)"""
    origin, inv, ncell = [-1., 10., 0.], [0.5, 2., 0.125], [4, 3, 2]
    up, down = numpy.inf, -numpy.inf
    rows = [
        ([-1., 10., 0.], (0, 0, 0)),                  # exactly at the origin
        ([-1.5, 9., -3.], (0, 0, 0)),                 # below it: clamped
        ([-100., -100., -100.], (0, 0, 0)),
        ([numpy.nextafter(-1., down), 10., -0.0], (0, 0, 0)),
        ([7., 11.5, 16.], (3, 2, 1)),                 # the top edge: clamped
        ([numpy.nextafter(7., down), numpy.nextafter(11.5, down),
          numpy.nextafter(16., down)], (3, 2, 1)),
        ([7.5, 12., 1e3], (3, 2, 1)),                 # above it
        ([1., 10.5, 8.], (1, 1, 1)),                  # interior boundaries
        # just below them; in x the subtraction (1 - 2^-53) + 1 rounds
        # up to 2 and the row belongs to cell 1, in y and z it is exact
        ([numpy.nextafter(1., down), numpy.nextafter(10.5, down),
          numpy.nextafter(8., down)], (1, 0, 0)),
        ([numpy.nextafter(1., up), numpy.nextafter(10.5, up),
          numpy.nextafter(8., up)], (1, 1, 1)),
        ([0.0, 11., 0.0], (0, 2, 0)),
        ([-0.0, 11., -0.0], (0, 2, 0)),
        ([5., 10.75, 4.], (3, 1, 0)),
    ]
    pos = numpy.array([r[0] for r in rows])
    want = [(cx * 3 + cy) * 2 + cz for _, (cx, cy, cz) in rows]
    assert_array_equal(pref.cell_ids(pos, origin, inv, ncell), want)
    # a flat axis (inv_cell = 0) is one cell whatever the coordinate
    flat = pref.cell_ids(pos, origin, [0.5, 0., 0.125], [4, 1, 2])
    assert_array_equal(flat, [cx * 2 + cz for _, (cx, _cy, cz) in rows])
    # anisotropic flattening: the id of a cell is not symmetric in y, z
    assert pref.cell_ids([[-1., 10.5, 0.]], origin, inv, ncell)[0] == 2
    assert pref.cell_ids([[-1., 10., 8.]], origin, inv, ncell)[0] == 1


def test_sorted_reference_and_clamp_rows():
    origin, inv, ncell = [-1., 10., 0.], [0.5, 2., 0.125], [4, 3, 2]
    pos = pref.clamp_rows(origin, inv, ncell, n=500)
    w = pref.weights(len(pos))
    ids = pref.cell_ids(pos, origin, inv, ncell)
    # the hand-placed rows reach every cell of the corner cases
    assert set([0, 23]) <= set(ids) and ids.min() >= 0 and ids.max() < 24
    for ax, (lo, top) in enumerate([(-1., 7.), (10., 11.5), (0., 16.)]):
        x = pos[:, ax]
        for v in (lo, top, 0.0):
            assert (x == v).any()
        assert (x < lo).any() and (x > top).any()
        assert (x == numpy.nextafter(lo, -numpy.inf)).any()
        assert (x == numpy.nextafter(top, -numpy.inf)).any()
        assert numpy.signbit(x[x == 0]).any()
    start, rows = pref.sorted_reference(pos, w, ids, 24)
    assert start[0] == 0 and start[-1] == len(pos)
    assert_array_equal(numpy.diff(start), numpy.bincount(ids, minlength=24))
    # a stable sort by cell holds the same canonical rows; a swapped
    # weight inside one cell does not
    order = numpy.argsort(ids, kind='stable')
    keys = pref.sorted_keys(start)
    assert_array_equal(keys, ids[order])
    assert_array_equal(pref.canonical_rows(pos[order], w[order], keys),
                       rows)
    cell = numpy.flatnonzero(numpy.diff(start) >= 2)[0]
    wrong = w[order].copy()
    a = start[cell]
    wrong[[a, a + 1]] = wrong[[a + 1, a]]
    assert not numpy.array_equal(
        pref.canonical_rows(pos[order], wrong, keys), rows)
    # chunk histograms and their scan
    mat = pref.chunk_histograms(ids, 24, 120)
    assert mat.shape == (5, 24) and mat[-1].sum() == 20
    bases, start2 = pref.scan_matrix(mat)
    assert_array_equal(start2, start)
    assert_array_equal(bases[0], start[:-1])
    assert_array_equal(bases[-1] + mat[-1], start[1:])


# (first, second, mode, edges, keywords, box, periodic) -> the margins
# measured for the kernel-level cases: (r^2 relative, second dimension
# absolute), to two digits
H_EDGES = numpy.linspace(0.5, 18, 8)
HP_EDGES = numpy.linspace(0.5, 14, 7)
S_EDGES = numpy.linspace(1, 30, 8)
SP_EDGES = numpy.linspace(1, 22, 8)
MARGIN_TABLE = {
    'H1 auto 1d': ('H1', None, '1d', H_EDGES, {}, 1.2e-6, None),
    'H1 auto 2d': ('H1', None, '2d', H_EDGES, dict(Nmu=10), 1.2e-6,
                   4.2e-7),
    'H1xH2 1d': ('H1', 'H2', '1d', H_EDGES, {}, 2.1e-8, None),
    'H1xH2 2d': ('H1', 'H2', '2d', H_EDGES, dict(Nmu=10), 2.1e-8, 1.1e-7),
    'H1 auto projected': ('H1', None, 'projected', HP_EDGES,
                          dict(pimax=12), 1.4e-6, 1.6e-6),
    'H1xH2 projected': ('H1', 'H2', 'projected', HP_EDGES, dict(pimax=12),
                        2.4e-7, 6.7e-6),
    'SLAB 1d': ('SLAB', None, '1d', S_EDGES, {}, 1.1e-6, None),
    'SLAB 2d': ('SLAB', None, '2d', S_EDGES, dict(Nmu=6), 1.1e-6, 5.2e-7),
    'SLAB projected': ('SLAB', None, 'projected', SP_EDGES, dict(pimax=20),
                       7.9e-6, 1.8e-6),
    'PLANAR 1d': ('PLANAR', None, '1d', S_EDGES, {}, 6.2e-7, None),
    'PLANAR projected': ('PLANAR', None, 'projected', SP_EDGES,
                         dict(pimax=20), 4.4e-7, 1.8e-6),
}


@pytest.mark.parametrize('case', sorted(MARGIN_TABLE))
def test_kernel_case_margins(case):
    """exact npairs in test_gpu_pairs_kernels.py rests on these: no pair
    within 1e-10 of a bin edge, none at mu = 1"""
    first, second, mode, edges, kw, m0, m1 = MARGIN_TABLE[case]
    pos1, w1 = pref.catalogue(first)
    pos2 = w2 = None
    if second is not None:
        pos2, w2 = pref.catalogue(second)
    periodic = first.startswith('H')
    want = bf.bruteforce_paircount(
        mode, pos1, edges, pref.HBOX if periodic else 0., w1=w1, pos2=pos2,
        w2=w2, periodic=periodic, **kw)
    assert want['margin0'] > 1e-10 and want['margin1'] > 1e-10
    assert want['n_mu1'] == 0
    assert_allclose(want['margin0'], m0, rtol=0.05)
    if m1 is None:
        assert want['margin1'] == numpy.inf
    else:
        assert_allclose(want['margin1'], m1, rtol=0.05)


def test_planar_mu_margin_is_below_the_bar():
    """why PLANAR has no (r, mu) case: in a plane that contains the line
    of sight mu crowds against 1"""
    pos, w = pref.catalogue('PLANAR')
    want = bf.bruteforce_paircount('2d', pos, S_EDGES, 0., w1=w,
                                   periodic=False, Nmu=6)
    assert 0 < want['margin1'] < 1e-10


@pytest.mark.parametrize('Nmu', [10, 100, 200, 512])
def test_copies_case_margins(Nmu):
    pos, w = pref.catalogue('H1')
    want = bf.bruteforce_paircount('2d', pos, numpy.linspace(0.5, 18, 9),
                                   pref.HBOX, w1=w, Nmu=Nmu)
    assert want['margin0'] > 1e-10 and want['margin1'] > 1e-10
    assert want['n_mu1'] == 0


def test_lattice_zero_separation_facts():
    """10 x 9 x 8 integer lattice in the periodic box (20, 18, 16),
    edges[0] = 0: a pair at r = 0 is counted in 1d and projected
    (q = 0 >= 0, pi = 0) and dropped in 2d, where mu = 0/0 has no bin"""
    lat, _ = pref.catalogue('LAT')
    dup, _ = pref.catalogue('LATDUP')
    assert lat.shape == (720, 3) and dup.shape == (760, 3)
    edges = [0, 1, 2, 3, 5, 6, 7]
    totals = {}
    for mode, kw in [('1d', {}), ('2d', dict(Nmu=5)),
                     ('projected', dict(pimax=4))]:
        with numpy.errstate(invalid='ignore', divide='ignore'):
            auto = bf.bruteforce_paircount(mode, lat, edges, pref.LATBOX,
                                           **kw)
            cross = bf.bruteforce_paircount(mode, lat, edges, pref.LATBOX,
                                            pos2=lat.copy(), **kw)
            both = bf.bruteforce_paircount(mode, dup, edges, pref.LATBOX,
                                           **kw)
        totals[mode] = [int(r['npairs'].sum())
                        for r in (auto, cross, both)]
        diff = cross['npairs'].astype('i8') - auto['npairs'].astype('i8')
        if mode == '2d':
            assert not diff.any()
            assert auto['n_mu1'] == 4860
        else:
            # all of them in the very first bin
            assert diff.ravel()[0] == 720 and diff.sum() == 720
    assert totals['1d'][:2] == [336804, 336804 + 720]
    assert totals['2d'][:2] == [336804, 336804]
    assert totals['projected'][1] - totals['projected'][0] == 720
    assert totals['1d'][2] == 376504 and totals['2d'][2] == 376424
    # mu = 3/5 sits one ulp below the published edge
    assert numpy.linspace(0, 1., 6)[3] == numpy.nextafter(0.6, 1.) > 3. / 5


def test_slab_grid_is_anisotropic():
    """extents 298.8 x 119.8 x 34.8: floor(extent / 30) = (9, 3, 1), and
    (10, 4, 1) for the projected reach sqrt(22^2 + 20^2) = 29.73"""
    lo, hi = pref.bounding_box('SLAB')
    assert_allclose(hi - lo, [298.788, 119.766, 34.763], atol=1e-3)
    origin, inv, ncell = kernel.make_grid(False, None, 30., lo, hi)
    assert ncell == [9, 3, 1]
    assert_array_equal(origin, lo)
    assert_allclose(inv, numpy.array(ncell) / (hi - lo), rtol=1e-15)
    rmax = kernel.max_3d_separation('projected', SP_EDGES, 20)
    assert kernel.make_grid(False, None, rmax, lo, hi)[2] == [10, 4, 1]
    # the blob: one cell holds more than a 256-particle tile
    pos, _ = pref.catalogue('SLAB')
    ids = pref.cell_ids(pos, origin, inv, ncell)
    assert numpy.bincount(ids, minlength=27).max() > 256
    # flattened: a single cell of zero extent along y
    lo, hi = pref.bounding_box('PLANAR')
    origin, inv, ncell = kernel.make_grid(False, None, 30., lo, hi)
    assert ncell == [9, 1, 1] and inv[1] == 0. and origin[1] == 3.25
