"""
CPU coverage of survey pair counting: hand values of the numpy oracle
(survey_bruteforce.py, the contract of DESIGN.md "Survey pair counting"),
argument validation of SurveyDataPairCount (which runs before the GPU is
needed), its attrs, the loud failure without a GPU, the grid reach of
every mode and JSON round-trips of synthetic results.
"""
import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import survey_bruteforce as sb
from nbodykit_amd.lab import (ArrayCatalog, Planck15, SurveyDataPairCount,
                              SurveyData2PCF, transform)
from nbodykit_amd.algorithms.pair_counters import kernel, mocksurvey
from nbodykit_amd.algorithms.pair_counters.mocksurvey import prepare_attrs
from nbodykit_amd.algorithms.paircount_tpcf import (WedgeBinnedStatistic,
                                                    estimators, tpcf)

EDGES = numpy.linspace(10, 150, 10)


def sky_catalog(n=60, seed=0, weight=True):
    ra, dec, z = sb.sky_survey(seed, n)
    cols = {'RA': ra, 'DEC': dec, 'Redshift': z}
    if weight:
        cols['Weight'] = sb.sky_weights(seed, n)
    return ArrayCatalog(cols)


@pytest.fixture(scope='module')
def cat():
    return sky_catalog()


# ---- hand values on the oracle -------------------------------------------

def count(mode, p1, p2, edges, **kw):
    return sb.bruteforce_survey_paircount(
        mode, numpy.array(p1, dtype='f8'), edges,
        pos2=numpy.array(p2, dtype='f8'), **kw)


def test_same_sight_line():
    """p1 = 3 u and p2 = 5 u with u = (1, 2, 2) / 3 exactly representable
    products: d = -2u, l = 8u, mu = 1 exactly, pi = |r1 - r2| = 6,
    rp^2 = 0"""
    p1, p2 = [[3., 6., 6.]], [[5., 10., 10.]]          # |p| = 9, 15
    r = count('2d', p1, p2, [1., 5., 7.], Nmu=4)
    assert_array_equal(r['npairs'], [[0, 0, 0, 0], [0, 0, 0, 1]])
    assert r['n_top'] == 1 and r['mean'][1, 3] == 6.
    # rp^2 = 0 fails q >= edges[0]^2 > 0 ...
    r = count('projected', p1, p2, [1., 5., 7.], pimax=8)
    assert r['npairs'].sum() == 0
    # ... and pi = 6 exactly: with an (illegal, oracle-only) zero edge
    # the pair sits in rp bin 0, pi bin [6, 7)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        r = count('projected', p1, p2, [0., 5., 7.], pimax=8)
    assert r['npairs'][0, 6] == 1 and r['npairs'].sum() == 1
    assert r['mean'][0, 6] == 0.
    # pi >= pimax is dropped
    with numpy.errstate(invalid='ignore', divide='ignore'):
        r = count('projected', p1, p2, [0., 5., 7.], pimax=6)
    assert r['npairs'].sum() == 0


def test_equal_distance():
    """|p1| = |p2|: d . l = |p1|^2 - |p2|^2 = 0, so mu = 0 and pi = 0"""
    p1, p2 = [[3., 4., 0.]], [[0., 4., 3.]]
    r = count('2d', p1, p2, [1., 5., 7.], Nmu=4)
    assert_array_equal(r['npairs'], [[1, 0, 0, 0], [0, 0, 0, 0]])
    assert_allclose(r['mean'][0, 0], numpy.sqrt(18.), rtol=2e-16)
    r = count('projected', p1, p2, [1., 5., 7.], pimax=3)
    assert_array_equal(r['npairs'], [[1, 0, 0], [0, 0, 0]])
    assert_allclose(r['mean'][0, 0], numpy.sqrt(18.), rtol=2e-16)


def test_opposite_points_have_no_line_of_sight():
    """p2 = -p1: l = 0, so no mu and no pi; '1d' counts the pair"""
    p1, p2 = [[1., 2., 2.]], [[-1., -2., -2.]]         # s = 6
    r = count('1d', p1, p2, [1., 5., 7.])
    assert_array_equal(r['npairs'], [0, 1])
    assert r['mean'][1] == 6.
    r = count('2d', p1, p2, [1., 5., 7.], Nmu=4)
    assert r['npairs'].sum() == 0 and r['n_nan'] == 1
    r = count('projected', p1, p2, [1., 5., 7.], pimax=8)
    assert r['npairs'].sum() == 0


def test_antipodal_directions():
    """antipodes: q = 4 exactly, the squared chord of 180 degrees, which
    the open top edge drops; 179.99 degrees is kept"""
    assert sb.chord_edges_sq([180.])[0] == 4.
    u1, u2 = [[0., 0., 1.]], [[0., 0., -1.]]
    r = count('angular', u1, u2, [90., 180.])
    assert r['npairs'].sum() == 0 and r['margin0'] == 0.
    ra, dec = numpy.array([10., 190.]), numpy.array([20., -19.99])
    u = transform.SkyToUnitSphere(ra, dec)
    r = sb.bruteforce_survey_paircount('angular', u, [90., 180.])
    assert_array_equal(r['npairs'], [2])
    assert_allclose(r['mean'], [179.99], rtol=1e-9)


def test_angle_of_a_chord():
    """theta = 2 asin(chord / 2) in degrees; the chord keeps arcsecond
    separations that 1 - cos(theta) loses"""
    assert_allclose(sb.chord_to_degrees(2.), 90., rtol=4e-16)
    assert_allclose(sb.chord_to_degrees(4.), 180., rtol=4e-16)
    # a chord that rounding made longer than the diameter is clamped
    assert sb.chord_to_degrees(numpy.nextafter(4., 5.)) \
        == sb.chord_to_degrees(4.)
    arcsec = 1. / 3600
    u = transform.SkyToUnitSphere([0., arcsec], [0., 0.])
    r = sb.bruteforce_survey_paircount('angular', u,
                                       [0.5 * arcsec, 2 * arcsec])
    assert_array_equal(r['npairs'], [2])
    assert_allclose(r['mean'], [arcsec], rtol=1e-9)


def test_oracle_against_direct_geometry():
    """(s, mu) and (rp, pi) of random pairs from norms and the angle to
    the midpoint direction, written another way"""
    rng = numpy.random.RandomState(7)
    p1 = rng.normal(size=(40, 3)) * 50 + (300., 0., 0.)
    p2 = rng.normal(size=(30, 3)) * 50 + (300., 0., 0.)
    d = p1[:, None] - p2[None]
    mid = 0.5 * (p1[:, None] + p2[None])
    s = numpy.linalg.norm(d, axis=-1)
    para = numpy.abs((d * mid).sum(-1)) / numpy.linalg.norm(mid, axis=-1)
    mu, rp = para / s, numpy.sqrt(s ** 2 - para ** 2)
    edges = numpy.array([5., 40., 90., 160.])
    r = sb.bruteforce_survey_paircount('2d', p1, edges, pos2=p2, Nmu=5)
    assert r['margin0'] > 1e-10 and r['margin1'] > 1e-10
    want, _, _ = numpy.histogram2d(s.ravel(), mu.ravel(),
                                   [edges, numpy.linspace(0, 1, 6)])
    assert_array_equal(r['npairs'], want)
    r = sb.bruteforce_survey_paircount('projected', p1, edges, pos2=p2,
                                       pimax=30)
    assert r['margin0'] > 1e-10 and r['margin1'] > 1e-10
    want, _, _ = numpy.histogram2d(rp.ravel(), para.ravel(),
                                   [edges, numpy.linspace(0, 30, 31)])
    assert_array_equal(r['npairs'], want)
    # auto-correlation: ordered pairs, no self pairs, weights multiply
    w = rng.uniform(size=40)
    a = sb.bruteforce_survey_paircount('1d', p1, [1e-3, 1e4], w1=w)
    assert a['npairs'][0] == 40 * 39
    assert_allclose(a['wnpairs'][0], w.sum() ** 2 - (w ** 2).sum(),
                    rtol=1e-13)


# ---- validation ---------------------------------------------------------

BAD_ARGUMENTS = {
    'bad mode': dict(mode='3d'),
    'zero edge': dict(edges=[0., 10., 20.]),
    'negative edge': dict(edges=[-1., 10., 20.]),
    'decreasing edges': dict(edges=[20., 10.]),
    'missing cosmo': dict(cosmo=None),
    'missing ra': dict(ra='Nope'),
    'missing dec': dict(dec='Nope'),
    'missing redshift': dict(redshift='Nope'),
    'missing weight': dict(weight='Nope'),
    'theta above 180': dict(mode='angular', edges=[1., 90., 180.5]),
    'zero theta edge': dict(mode='angular', edges=[0., 1.]),
    '2d without Nmu': dict(mode='2d'),
    'Nmu in 1d': dict(mode='1d', Nmu=10),
    'Nmu zero': dict(mode='2d', Nmu=0),
    'Nmu in projected': dict(mode='projected', pimax=40, Nmu=10),
    'Nmu in angular': dict(mode='angular', edges=[1., 2.], Nmu=10),
    'projected without pimax': dict(mode='projected'),
    'pimax in 1d': dict(mode='1d', pimax=40),
    'pimax in 2d': dict(mode='2d', Nmu=10, pimax=40),
    'pimax in angular': dict(mode='angular', edges=[1., 2.], pimax=40),
    'pimax below 1': dict(mode='projected', pimax=0.5),
}


@pytest.mark.parametrize('case', sorted(BAD_ARGUMENTS))
def test_validation_raises_value_error(cat, case):
    kw = dict(mode='1d', edges=EDGES, cosmo=Planck15)
    kw.update(BAD_ARGUMENTS[case])
    mode, edges = kw.pop('mode'), kw.pop('edges')
    with pytest.raises(ValueError):
        SurveyDataPairCount(mode, cat, edges, **kw)
    with pytest.raises(ValueError):
        SurveyData2PCF(mode, cat, cat, edges, **kw)


def test_second_source_columns_are_checked(cat):
    other = ArrayCatalog({'RA': numpy.zeros(3), 'DEC': numpy.zeros(3)})
    with pytest.raises(ValueError, match='Redshift'):
        SurveyDataPairCount('1d', cat, EDGES, cosmo=Planck15, second=other)
    # angular mode needs neither a redshift nor a cosmology
    attrs = prepare_attrs('angular', other, [0.1, 1., 180.])
    assert attrs['cosmo'] is None and attrs['total_wnpairs'] == 3.


def test_multi_rank_not_implemented(cat):
    class TwoRanks(object):
        size, rank = 2, 0

        def allreduce(self, x, op='sum'):
            return x

    two = sky_catalog()
    two.comm = TwoRanks()
    with pytest.raises(NotImplementedError):
        SurveyDataPairCount('1d', two, EDGES, cosmo=Planck15)


def test_compute_fails_loudly_without_gpu(cat):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SurveyDataPairCount('1d', cat, EDGES, cosmo=Planck15)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SurveyDataPairCount('angular', cat, [0.1, 1.])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SurveyData2PCF('2d', cat, cat, EDGES, cosmo=Planck15, Nmu=5)


# ---- attrs, dimensions, grid reach ---------------------------------------

def test_attrs_and_weighted_totals():
    c1, c2 = sky_catalog(50, 1), sky_catalog(70, 2)
    w1, w2 = sb.sky_weights(1, 50), sb.sky_weights(2, 70)
    auto = prepare_attrs('2d', c1, [1., 10., 20.], cosmo=Planck15, Nmu=4,
                         show_progress=True, domain_factor=2,
                         config=dict(nthreads=2))
    assert sorted(auto) == sorted(
        ['mode', 'edges', 'Nmu', 'pimax', 'show_progress', 'N1', 'N2',
         'total_wnpairs', 'is_cross', 'cosmo', 'ra', 'dec', 'redshift',
         'weight', 'domain_factor', 'config'])
    assert auto['N1'] == 50 and auto['N2'] is None
    assert auto['is_cross'] is False and auto['cosmo'] is Planck15
    assert_allclose(auto['total_wnpairs'],
                    0.5 * (w1.sum() ** 2 - (w1 ** 2).sum()), rtol=1e-14)
    assert auto['config'] == dict(nthreads=2)
    assert auto['domain_factor'] == 2 and auto['show_progress'] is True

    same = prepare_attrs('1d', c1, [1., 10.], cosmo=Planck15, second=c1)
    assert same['is_cross'] is False and same['N2'] == 50
    assert same['total_wnpairs'] == auto['total_wnpairs']

    cross = prepare_attrs('1d', c1, [1., 10.], cosmo=Planck15, second=c2)
    assert cross['is_cross'] is True
    assert cross['N1'] == 50 and cross['N2'] == 70
    assert_allclose(cross['total_wnpairs'], 0.5 * w1.sum() * w2.sum(),
                    rtol=1e-14)

    # the default Weight column counts plain pairs
    plain = prepare_attrs('1d', sky_catalog(50, 1, weight=False),
                          [1., 10.], cosmo=Planck15)
    assert plain['total_wnpairs'] == 0.5 * 50 * 49


def test_dimensions_of_every_mode():
    assert mocksurvey.second_dim('angular', None, None) == (['theta'], None)
    assert mocksurvey.second_dim('1d', None, None) == (['r'], None)
    dims, e2 = mocksurvey.second_dim('2d', 4, None)
    assert dims == ['r', 'mu']
    assert_array_equal(e2, numpy.linspace(0, 1., 5))
    dims, e2 = mocksurvey.second_dim('projected', None, 7.5)
    assert dims == ['rp', 'pi'] and len(e2) == 8 and e2[-1] == 7.5
    # the simulation box has no theta
    from nbodykit_amd.algorithms.pair_counters import simbox
    with pytest.raises(ValueError):
        simbox.second_dim('angular', None, None)


def test_positions_from_the_sky(cat):
    attrs = prepare_attrs('1d', cat, EDGES, cosmo=Planck15)
    pos = mocksurvey.sky_positions(cat, attrs)
    ra, dec, z = sb.sky_survey(0, 60)
    assert_array_equal(pos, transform.SkyToCartesian(ra, dec, z, Planck15))
    assert_allclose(numpy.linalg.norm(pos, axis=-1),
                    Planck15.comoving_distance(z), rtol=1e-14)
    attrs = prepare_attrs('angular', cat, [0.1, 1.])
    unit = mocksurvey.sky_positions(cat, attrs)
    assert_array_equal(unit, transform.SkyToUnitSphere(ra, dec))
    # f4 columns are widened before the trigonometry
    cat4 = ArrayCatalog({'RA': ra.astype('f4'), 'DEC': dec.astype('f4')})
    assert_array_equal(
        mocksurvey.sky_positions(cat4, attrs),
        transform.SkyToUnitSphere(ra.astype('f4').astype('f8'),
                                  dec.astype('f4').astype('f8')))


def test_grid_reach_of_every_mode():
    assert kernel.max_3d_separation('1d', [1., 50.], None) == 50.
    assert kernel.max_3d_separation('2d', [1., 50.], None) == 50.
    assert_allclose(kernel.max_3d_separation('projected', [1., 30.], 40.),
                    50.)
    # the largest chord: 2 sin(theta / 2)
    assert_allclose(kernel.max_3d_separation('angular', [1., 60.], None),
                    1., rtol=1e-15)
    assert kernel.max_3d_separation('angular', [1., 180.], None) == 2.
    assert_array_equal(kernel.chord_edges_sq([0.5, 60., 180.]),
                       sb.chord_edges_sq([0.5, 60., 180.]))
    assert kernel.SKY_MODE_IDS == {'2d': 3, 'projected': 4, 'angular': 5}


# ---- JSON round-trips ---------------------------------------------------

def synthetic_paircount(mode, **kw):
    rng = numpy.random.RandomState(3)
    edges = numpy.array([1., 2., 4., 8.])
    dims, edges2 = mocksurvey.second_dim(mode, kw.get('Nmu'),
                                         kw.get('pimax'))
    shape = (3,) if edges2 is None else (3, len(edges2) - 1)
    npairs = rng.randint(0, 100, size=shape).astype('u8')
    data = mocksurvey.pairs_data(dims[0], npairs, rng.uniform(size=shape),
                                 npairs * 2.5)
    obj = object.__new__(SurveyDataPairCount)
    obj.__setstate__({'pairs': data, 'attrs': {
        'mode': mode, 'edges': edges, 'Nmu': kw.get('Nmu'),
        'pimax': kw.get('pimax'), 'total_wnpairs': 12.5,
        'cosmo': None if mode == 'angular' else Planck15, 'config': {},
        'is_cross': False, 'N1': 7, 'N2': None}})
    from nbodykit_amd.comm import SerialComm
    obj.comm = SerialComm()
    return obj


@pytest.mark.parametrize('mode,kw', [('1d', {}), ('2d', dict(Nmu=4)),
                                     ('projected', dict(pimax=5)),
                                     ('angular', {})])
def test_paircount_json_roundtrip(tmp_path, mode, kw):
    r = synthetic_paircount(mode, **kw)
    out = str(tmp_path / 'pairs.json')
    r.save(out)
    r2 = SurveyDataPairCount.load(out)
    assert r2.pairs.dims == r.pairs.dims
    assert r2.pairs.dims[0] == {'1d': 'r', '2d': 'r', 'projected': 'rp',
                                'angular': 'theta'}[mode]
    assert r2.pairs.data.dtype == r.pairs.data.dtype
    for name in r.pairs.variables:
        assert_array_equal(r2.pairs[name], r.pairs[name])
    for d in r.pairs.dims:
        assert_array_equal(r2.pairs.edges[d], r.pairs.edges[d])
    assert r2.pairs.attrs['total_wnpairs'] == 12.5
    assert r2.attrs['N2'] is None and r2.attrs['mode'] == mode
    if mode == 'angular':
        assert r2.attrs['cosmo'] is None
    else:
        assert dict(r2.attrs['cosmo'].pars) == dict(Planck15.pars)


def test_2pcf_json_roundtrip(tmp_path):
    DD = synthetic_paircount('projected', pimax=5)
    corr = estimators.make_corr(
        DD.pairs, numpy.linspace(-1, 1, 15).reshape(3, 5))
    t = object.__new__(SurveyData2PCF)
    t.comm = DD.comm
    t.attrs = {'mode': 'projected', 'edges': DD.attrs['edges'],
               'cosmo': Planck15, 'Nmu': None, 'pimax': 5, 'config': {}}
    t.corr = corr
    t.D1D2 = t.D1R2 = t.D2R1 = t.R1R2 = DD.pairs
    t.wp = tpcf.compute_wp(corr)
    out = str(tmp_path / 'tpcf.json')
    t.save(out)
    t2 = SurveyData2PCF.load(out)
    assert isinstance(t2.corr, WedgeBinnedStatistic)
    assert t2.corr.dims == ['rp', 'pi']
    assert_array_equal(t2.corr['corr'], t.corr['corr'])
    assert_array_equal(t2.wp['corr'], t.wp['corr'])
    assert t2.wp.dims == ['rp'] and t2.wp.shape == (3,)
    for name in tpcf.PAIR_COUNTS:
        assert_array_equal(getattr(t2, name)['npairs'], DD.pairs['npairs'])
    assert dict(t2.attrs['cosmo'].pars) == dict(Planck15.pars)
