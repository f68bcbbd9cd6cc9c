"""
SimulationBoxPairCount / SimulationBox2PCF on the GPU against the
brute-force numpy oracle (paircount_bruteforce.py).

``npairs`` must equal the oracle exactly.  That is fair because each
case first asserts, on the oracle, that no pair lies within relative
1e-10 of a squared first-dimension edge nor within absolute 1e-10 of a
mu or pi edge (measured margins are >= 1.0e-8 for every A and B case);
the lattice cases are exempt, their arithmetic is exact.  ``wnpairs``
and the mean separation are sums of n_bin positive terms in another
order, so they match to rtol = 4 (n_bin + 4) 2^-53 per bin.

Inputs: A = uniform_positions(3e-6, 512., seed 42 / 84) (395 / 355
particles, the reference's own test catalogues), B =
uniform_positions(2e-3, 100., seed 7 / 8) (1921 / 2058), weights
RandomState(1).uniform(size=N), and the 8^3 lattice of spacing 8 in
L = 64.  From pairs_reference.py (the kernel-level tests' catalogues):
SLAB, a thin anisotropic sheet far from the origin with a dense blob,
PLANAR, the same flattened to zero extent in y, and the 10 x 9 x 8
integer lattice LAT of the box (20, 18, 16) with its 40 doubled rows
(LATDUP).  B1W is B1 with rows moved out of the box by -L and +2L and
one row set to (L, 0, L), which the driver has to wrap.
"""
import functools

import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import paircount_bruteforce as bf                               # noqa: E402
import pairs_reference as pref                                  # noqa: E402
from conftest import uniform_positions                          # noqa: E402
from nbodykit_amd.lab import (ArrayCatalog, SimulationBoxPairCount,  # noqa
                              SimulationBox2PCF)
from nbodykit_amd.source.catalog.device import DeviceArrayCatalog  # noqa
from nbodykit_amd.algorithms.pair_counters import kernel       # noqa: E402

EPS = 2.0 ** -53
MARGIN = 1e-10

EDGES_A = numpy.linspace(10, 150, 10)
EDGES_B = numpy.linspace(1, 50, 15)
EDGES_B2 = numpy.linspace(2, 40, 11)
EDGES_B8 = numpy.geomspace(0.5, 12, 9)
EDGES_LAT = [4, 8, 12, 16, 24, 32]
EDGES_SLAB = numpy.linspace(1, 30, 8)
EDGES_SLAB_P = numpy.linspace(1, 22, 8)


@functools.lru_cache(maxsize=None)
def positions(name):
    if name == 'lattice':
        pos, box = bf.lattice_positions(), 64.
    elif name in ('SLAB', 'PLANAR'):
        # non-periodic only: the box is required but has no use
        pos, box = pref.catalogue(name)[0], 2048.
    elif name == 'B1W':
        b1, box = positions('B1')
        pos = b1.copy()
        pos[0::3] -= box
        pos[1::3] += 2 * box
        pos[2] = (box, 0., box)
    else:
        nbar, box, seed = {'A1': (3e-6, 512., 42), 'A2': (3e-6, 512., 84),
                           'B1': (2e-3, 100., 7),
                           'B2': (2e-3, 100., 8)}[name]
        pos = uniform_positions(nbar, box, seed)
    pos.setflags(write=False)
    return pos, box


def weights(n):
    return numpy.random.RandomState(1).uniform(size=n)


def over_capacity_nmu():
    """Nmu for 8 r bins x Nmu = 1.5 x the single-pass capacity"""
    return int(1.5 * kernel.single_pass_capacity()) // 8


# name -> (first, second, edges, periodic, keywords); the mode follows
# from the keywords
def _cases():
    c = {}
    modes_a = [('1d', {}), ('2d_z', dict(Nmu=10)),
               ('2d_x', dict(Nmu=10, los='x')),
               ('projected', dict(pimax=40))]
    for tag, kw in modes_a:
        c['A_auto_' + tag] = ('A1', None, EDGES_A, True, kw)
    c['A_auto_nonperiodic_1d'] = ('A1', None, EDGES_A, False, {})
    c['A_auto_nonperiodic_2d'] = ('A1', None, EDGES_A, False,
                                  dict(Nmu=10))
    c['A_cross_1d'] = ('A1', 'A2', EDGES_A, True, {})
    c['A_cross_2d'] = ('A1', 'A2', EDGES_A, True, dict(Nmu=10))
    modes_b = [('1d', {}), ('2d', dict(Nmu=7)),
               ('projected', dict(pimax=50))]
    for tag, kw in modes_b:
        c['B_auto_' + tag] = ('B1', None, EDGES_B, True, kw)
        c['B_cross_' + tag] = ('B1', 'B2', EDGES_B, True, kw)
    c['B_auto_third_1d'] = ('B1', None, EDGES_B2, True, {})
    c['B2_auto_third_1d'] = ('B2', None, EDGES_B2, True, {})
    c['B_cross_third_1d'] = ('B1', 'B2', EDGES_B2, True, {})
    c['B_auto_8cells_1d'] = ('B1', None, EDGES_B8, True, {})
    c['B_auto_nonperiodic_1d'] = ('B1', None, EDGES_B2, False, {})
    for per in (True, False):
        tag = 'periodic' if per else 'nonperiodic'
        c['lattice_%s_1d' % tag] = ('lattice', None, EDGES_LAT, per, {})
        c['lattice_%s_2d' % tag] = ('lattice', None, EDGES_LAT, per,
                                    dict(Nmu=4))
    c['A_auto_empty_bin'] = ('A1', None, [0.01, 0.02, 150], True, {})
    # anisotropic grids with a 1-cell axis and a cell above 256
    # particles; los='y' moves the 1-cell axis
    modes_s = [('1d', EDGES_SLAB, {}), ('2d', EDGES_SLAB, dict(Nmu=6)),
               ('projected', EDGES_SLAB_P, dict(pimax=20))]
    for tag, edges, kw in modes_s:
        c['SLAB_nonperiodic_' + tag] = ('SLAB', None, edges, False, kw)
        c['SLAB_nonperiodic_%s_y' % tag] = ('SLAB', None, edges, False,
                                            dict(kw, los='y'))
        # zero extent along y; in (r, mu) the margin is 5.8e-11, below
        # the bar, so that mode is left out
        if tag != '2d':
            c['PLANAR_nonperiodic_' + tag] = ('PLANAR', None, edges, False,
                                              kw)
    # rows outside [0, L) (margins 1.8e-7, 1.8e-8)
    c['B_wrapped_auto_2d'] = ('B1W', None, EDGES_B, True, dict(Nmu=7))
    return c


CASES = _cases()


def mode_of(kw):
    return '2d' if 'Nmu' in kw else ('projected' if 'pimax' in kw else '1d')


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The brute-force result of a case: computed once, shared."""
    first, second, edges, periodic, kw = CASES[name]
    return _oracle(first, second, tuple(edges), periodic,
                   tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def _oracle(first, second, edges, periodic, kw_items):
    kw = dict(kw_items)
    los = kw.pop('los', 'z')
    pos1, box = positions(first)
    lattice = first == 'lattice'
    w1 = None if lattice else weights(len(pos1))
    pos2 = w2 = None
    if second is not None:
        pos2, _ = positions(second)
        w2 = weights(len(pos2))
    want = bf.bruteforce_paircount(
        mode_of(kw), pos1, numpy.array(edges), box, w1=w1, pos2=pos2,
        w2=w2, periodic=periodic, los='xyz'.index(los), **kw)
    for v in want.values():
        if isinstance(v, numpy.ndarray):
            v.setflags(write=False)
    return want


def catalog(name, dtype='f8', device=False):
    pos, box = positions(name)
    w = numpy.ones(len(pos)) if name == 'lattice' else weights(len(pos))
    if device:
        return DeviceArrayCatalog(
            {'Position': torch.as_tensor(numpy.array(pos)).to('cuda'),
             'Weight': torch.as_tensor(w).to('cuda')}, BoxSize=box)
    return ArrayCatalog({'Position': pos.astype(dtype),
                         'Weight': w.astype(dtype if dtype[0] in '<>'
                                            else 'f8')}, BoxSize=box)


def run_case(name, first=None, second=None):
    f, s, edges, periodic, kw = CASES[name]
    first = catalog(f) if first is None else first
    if s is not None and second is None:
        second = catalog(s)
    return SimulationBoxPairCount(mode_of(kw), first, edges,
                                  periodic=periodic, second=second, **kw)


def check_precondition(name, want):
    """exact npairs is only fair when no pair sits on a bin edge"""
    if name.startswith('lattice'):
        return
    assert want['margin0'] > MARGIN, (name, want['margin0'])
    assert want['margin1'] > MARGIN, (name, want['margin1'])
    assert want['n_mu1'] == 0


def check_pairs(pairs, want):
    dim0 = pairs.dims[0]
    print('npairs total %d, margins %.3g %.3g'
          % (want['npairs'].sum(), want['margin0'], want['margin1']))
    assert pairs.data.dtype == numpy.dtype(
        [(dim0, 'f8'), ('npairs', 'u8'), ('wnpairs', 'f8')])
    assert_array_equal(pairs['npairs'], want['npairs'])
    rtol = 4 * (want['npairs'].astype('f8') + 4) * EPS
    for got, ref in [(pairs['wnpairs'], want['wnpairs']),
                     (pairs[dim0], want['mean'])]:
        err = numpy.abs(got - ref)
        print('max err / bound: %.3g'
              % (err / (rtol * numpy.abs(ref) + 1e-300)).max())
        assert (err <= rtol * numpy.abs(ref)).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_pair_counts(name):
    want = oracle(name)
    check_precondition(name, want)
    r = run_case(name)
    check_pairs(r.pairs, want)
    assert r.pairs.attrs['total_wnpairs'] == r.attrs['total_wnpairs']
    # bitwise reproducible integer counts
    again = run_case(name)
    assert_array_equal(again.pairs['npairs'], r.pairs['npairs'])


def test_lattice_hand_values():
    r = run_case('lattice_periodic_1d')
    assert_array_equal(r.pairs['npairs'][:3], [0, 18 * 512, 8 * 512])
    assert r.pairs['r'][0] == 0.          # empty bin: 0, not NaN
    # exactly transverse pairs in the first mu bin, exactly
    # line-of-sight ones in the last
    r2 = run_case('lattice_periodic_2d')
    # (r = 8: 4 transverse + 2 line-of-sight; r = 8 sqrt(2): 4 at mu = 0
    # and 8 at mu = 1/sqrt(2))
    assert_array_equal(r2.pairs['npairs'][1],
                       [8 * 512, 0, 8 * 512, 2 * 512])


def test_empty_bin_is_zero_not_nan():
    r = run_case('A_auto_empty_bin')
    assert r.pairs['npairs'][0] == 0
    assert r.pairs['wnpairs'][0] == 0.
    assert r.pairs['r'][0] == 0.


def test_mixed_precision_cross():
    """first in f4, second in f8: the oracle sees the same f4 values"""
    pos1, box = positions('A1')
    pos2, _ = positions('A2')
    p4 = pos1.astype('f4')
    w1, w2 = weights(len(pos1)), weights(len(pos2))
    want = bf.bruteforce_paircount('2d', p4, EDGES_A, box, w1=w1,
                                   pos2=pos2, w2=w2, Nmu=10)
    assert want['margin0'] > MARGIN and want['margin1'] > MARGIN
    first = ArrayCatalog({'Position': p4, 'Weight': w1}, BoxSize=box)
    r = SimulationBoxPairCount('2d', first, EDGES_A, second=catalog('A2'),
                               Nmu=10)
    check_pairs(r.pairs, want)
    assert r.attrs['is_cross'] and r.attrs['N2'] == len(pos2)


def test_device_catalog():
    r = run_case('A_auto_2d_z', first=catalog('A1', device=True))
    check_pairs(r.pairs, oracle('A_auto_2d_z'))
    r = run_case('A_cross_1d', first=catalog('A1', device=True),
                 second=catalog('A2', device=True))
    check_pairs(r.pairs, oracle('A_cross_1d'))


def test_big_endian_columns():
    r = run_case('A_auto_projected', first=catalog('A1', dtype='>f8'))
    check_pairs(r.pairs, oracle('A_auto_projected'))


def test_over_capacity_runs_in_passes():
    """8 r bins x 768 mu bins = 6144 bins = 1.5 x the single-pass
    capacity of 4096, so the count runs as two passes over mu slices.
    Seed 42 (catalogue A) satisfies the edge precondition: margins
    6.4e-6 (relative, r^2) and 9.1e-8 (absolute, mu)."""
    cap = kernel.single_pass_capacity()
    Nmu = over_capacity_nmu()
    edges = numpy.linspace(10, 150, 9)
    assert 8 * Nmu * 2 == 3 * cap
    pos, box = positions('A1')
    w = weights(len(pos))
    want = bf.bruteforce_paircount('2d', pos, edges, box, w1=w, Nmu=Nmu)
    print('margins %.3g %.3g' % (want['margin0'], want['margin1']))
    assert want['margin0'] > MARGIN and want['margin1'] > MARGIN
    assert want['n_mu1'] == 0

    info = {}
    orig = kernel.count_pairs

    def spy(*args, **kwargs):
        return orig(*args, info=info, **kwargs)

    kernel.count_pairs = spy
    try:
        r = SimulationBoxPairCount('2d', catalog('A1'), edges, Nmu=Nmu)
    finally:
        kernel.count_pairs = orig
    assert info['npasses'] == 2
    check_pairs(r.pairs, want)


# ---- SimulationBox2PCF -------------------------------------------------

def natural_expected(want, mode, edges, kw, N, box, total_wnpairs):
    """the natural estimator applied to the oracle's counts, with the
    analytic randoms written out here"""
    V = box ** 3
    e = numpy.asarray(edges, dtype='f8')
    if mode == '1d':
        fill = numpy.diff(4. / 3 * numpy.pi * e ** 3) / V
    elif mode == '2d':
        mu = numpy.linspace(0, 1, kw['Nmu'] + 1)
        fill = numpy.diff(numpy.diff(
            4. / 3 * numpy.pi * numpy.outer(e ** 3, mu), axis=0),
            axis=1) / V
    else:
        pi = numpy.linspace(0, kw['pimax'], int(kw['pimax'] + 1))
        fill = numpy.diff(numpy.diff(
            numpy.pi * numpy.outer(e ** 2, 2 * pi), axis=0), axis=1) / V
    RR = float(N) ** 2 * fill
    RR_total = 0.5 * N * (N - 1)
    return want['wnpairs'] * (RR_total / total_wnpairs) / RR - 1.


@pytest.mark.parametrize('name', ['A_auto_1d', 'A_auto_2d_z',
                                  'A_auto_projected', 'B_auto_1d',
                                  'B_auto_2d', 'B_auto_projected'])
def test_2pcf_natural(name):
    f, _, edges, _, kw = CASES[name]
    mode = mode_of(kw)
    want = oracle(name)
    check_precondition(name, want)
    pos, box = positions(f)
    w = weights(len(pos))
    cat = catalog(f)
    r = SimulationBox2PCF(mode, cat, edges, **kw)
    total = 0.5 * (w.sum() ** 2 - (w ** 2).sum())
    expected = natural_expected(want, mode, edges, kw, len(pos), box,
                                total)
    # corr + 1 carries the relative error of wnpairs (+ the estimator's
    # own handful of roundings)
    rtol = 4 * (want['npairs'].astype('f8') + 8) * EPS
    err = numpy.abs(r.corr['corr'] - expected)
    assert (err <= rtol * numpy.abs(expected + 1.)).all()
    assert_array_equal(r.D1D2['npairs'], want['npairs'])
    assert r.D1R2 is None and r.D2R1 is None
    if mode == 'projected':
        dpi = numpy.diff(r.corr.edges['pi'])
        assert_allclose(r.wp['corr'],
                        (2 * r.corr['corr'] * dpi).sum(axis=-1),
                        rtol=1e-14)
        assert r.wp.dims == ['rp']
    else:
        assert r.wp is None


def ls_expected(DD, DR, RD, RR, tDD, tDR, tRD, tRR):
    return ((tRR / tDD) * DD['wnpairs'] - (tRR / tDR) * DR['wnpairs']
            - (tRR / tRD) * RD['wnpairs']) / RR['wnpairs'] + 1


def auto_total(w):
    return 0.5 * (w.sum() ** 2 - (w ** 2).sum())


def test_2pcf_landy_szalay_auto(monkeypatch):
    """data seed 7, randoms seed 8; a supplied R1R2 skips the RR count"""
    calls = []
    orig = kernel.count_pairs
    monkeypatch.setattr(kernel, 'count_pairs',
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    data, randoms = catalog('B1'), catalog('B2')
    r = SimulationBox2PCF('1d', data, EDGES_B2, randoms1=randoms)
    assert len(calls) == 3

    DD, RR, DR = (oracle('B_auto_third_1d'), oracle('B2_auto_third_1d'),
                  oracle('B_cross_third_1d'))
    for name, want in [('B_auto_third_1d', DD), ('B2_auto_third_1d', RR),
                       ('B_cross_third_1d', DR)]:
        check_precondition(name, want)
    w1 = weights(len(positions('B1')[0]))
    w2 = weights(len(positions('B2')[0]))
    tDD, tRR = auto_total(w1), auto_total(w2)
    tDR = 0.5 * w1.sum() * w2.sum()
    expected = ls_expected(DD, DR, DR, RR, tDD, tDR, tDR, tRR)
    # three sums of up to n_bin terms each, scaled by O(1) factors
    scale = ((tRR / tDD) * DD['wnpairs'] + 2 * (tRR / tDR) * DR['wnpairs']
             ) / RR['wnpairs'] + 1
    nmax = numpy.maximum(numpy.maximum(DD['npairs'], DR['npairs']),
                         RR['npairs']).astype('f8')
    atol = 4 * (nmax + 8) * EPS * scale * 2
    assert (numpy.abs(r.corr['corr'] - expected) <= atol).all()
    assert_array_equal(r.D1D2['npairs'], DD['npairs'])
    assert_array_equal(r.D1R2['npairs'], DR['npairs'])
    assert_array_equal(r.R1R2['npairs'], RR['npairs'])

    # sanity: a uniform catalogue has no correlation (the oracle alone
    # gives at most 2.4 sigma here)
    assert (numpy.abs(r.corr['corr'])
            < 5 / numpy.sqrt(DD['npairs'] / 2.)).all()

    # R1R2 supplied: the randoms-randoms count is not repeated
    R1R2 = SimulationBoxPairCount('1d', randoms, EDGES_B2)
    del calls[:]
    r2 = SimulationBox2PCF('1d', data, EDGES_B2, randoms1=randoms,
                           R1R2=R1R2)
    assert len(calls) == 2
    assert_array_equal(r2.R1R2['npairs'], RR['npairs'])
    assert (numpy.abs(r2.corr['corr'] - expected) <= atol).all()


def test_2pcf_landy_szalay_cross(monkeypatch):
    """data1 seed 7 x data2 seed 8, randoms seed 8 for both"""
    calls = []
    orig = kernel.count_pairs
    monkeypatch.setattr(kernel, 'count_pairs',
                        lambda *a, **k: calls.append(1) or orig(*a, **k))
    data1, data2 = catalog('B1'), catalog('B2')
    r = SimulationBox2PCF('1d', data1, EDGES_B2, data2=data2,
                          randoms1=data2)
    assert len(calls) == 4
    # D1D2 = D1R2 = B1 x B2 (cross), D2R1 = R1R2 = B2 auto
    X, RR = oracle('B_cross_third_1d'), oracle('B2_auto_third_1d')
    w1 = weights(len(positions('B1')[0]))
    w2 = weights(len(positions('B2')[0]))
    tX, tRR = 0.5 * w1.sum() * w2.sum(), auto_total(w2)
    expected = ls_expected(X, X, RR, RR, tX, tX, tRR, tRR)
    scale = (2 * (tRR / tX) * X['wnpairs'] + RR['wnpairs']) \
        / RR['wnpairs'] + 1
    nmax = numpy.maximum(X['npairs'], RR['npairs']).astype('f8')
    atol = 4 * (nmax + 8) * EPS * scale * 2
    assert (numpy.abs(r.corr['corr'] - expected) <= atol).all()
    assert_array_equal(r.D2R1['npairs'], RR['npairs'])


def test_save_load_roundtrip(tmp_path):
    r = run_case('A_auto_2d_z')
    out = str(tmp_path / 'pairs.json')
    r.save(out)
    r2 = SimulationBoxPairCount.load(out)
    for name in r.pairs.variables:
        assert_array_equal(r2.pairs[name], r.pairs[name])
    assert r2.pairs.dims == ['r', 'mu']
    assert r2.attrs['total_wnpairs'] == r.attrs['total_wnpairs']
    assert_array_equal(r2.attrs['edges'], EDGES_A)

    t = SimulationBox2PCF('projected', catalog('A1'), EDGES_A, pimax=40)
    out = str(tmp_path / 'tpcf.json')
    t.save(out)
    t2 = SimulationBox2PCF.load(out)
    assert_array_equal(t2.corr['corr'], t.corr['corr'])
    assert_array_equal(t2.wp['corr'], t.wp['corr'])
    assert_array_equal(t2.D1D2['npairs'], t.D1D2['npairs'])
    assert t2.D1R2 is None
    assert t2.attrs['pimax'] == 40


# ---- gaps of the driver ------------------------------------------------

def test_slab_grids_are_anisotropic():
    """what the SLAB / PLANAR cases are there for"""
    for name, los, ncell in [('SLAB_nonperiodic_2d', 'z', [9, 3, 1]),
                             ('SLAB_nonperiodic_2d_y', 'y', [9, 1, 3]),
                             ('SLAB_nonperiodic_projected', 'z', [10, 4, 1]),
                             ('PLANAR_nonperiodic_1d', 'z', [9, 1, 1])]:
        info = {}
        orig = kernel.count_pairs
        kernel.count_pairs = lambda *a, **k: orig(*a, info=info, **k)
        try:
            run_case(name)
        finally:
            kernel.count_pairs = orig
        assert info['ncell'] == ncell, name
        if name.startswith('SLAB'):
            assert numpy.diff(info['start1']).max() > 256


def test_wrapped_case_has_rows_outside_the_box():
    """what B_wrapped_auto_2d (in test_pair_counts) is there for"""
    pos, box = positions('B1W')
    assert (pos < 0).any() and (pos > box).any() and (pos == box).any()
    assert (pos.min(axis=0) < -0.9 * box).all()
    assert (pos.max(axis=0) > 2.9 * box).all()


@pytest.mark.parametrize('case', ['cross-copy', 'duplicated-rows'])
def test_zero_separation_has_no_mu(case):
    """edges[0] = 0 (which the class rejects, so through the driver): a
    pair at r = 0 has mu = 0/0 and is dropped in '2d', as in the oracle;
    LAT x a copy of LAT then equals LAT auto, and the 80 coincident
    pairs of LATDUP are not counted."""
    edges = numpy.array([0., 1, 2, 3, 5, 6, 7])
    mu = bf.second_edges('2d', Nmu=5)
    lat, _ = pref.catalogue('LAT')
    first = pref.catalogue('LAT' if case == 'cross-copy' else 'LATDUP')[0]
    w1 = weights(len(first))
    second = w2 = None
    if case == 'cross-copy':
        second, w2 = lat.copy(), weights(len(lat))
    with numpy.errstate(invalid='ignore', divide='ignore'):
        want = bf.bruteforce_paircount('2d', first, edges, pref.LATBOX,
                                       w1=w1, pos2=second, w2=w2, Nmu=5)
    assert want['npairs'].sum() == (336804 if case == 'cross-copy'
                                    else 376424)

    def cols(pos, w):
        return (torch.as_tensor(numpy.array(pos)).to('cuda'),
                torch.as_tensor(w).to('cuda'))

    pos1, w1_t = cols(first, w1)
    pos2, w2_t = (None, None) if second is None else cols(second, w2)
    npairs, wsum, xsum = kernel.count_pairs(
        '2d', pos1, w1_t, pos2, w2_t, edges, mu, pref.LATBOX, True)
    assert_array_equal(npairs, want['npairs'])
    rtol = 4 * (want['npairs'].astype('f8') + 4) * EPS
    assert (numpy.abs(wsum - want['wnpairs'])
            <= rtol * want['wnpairs']).all()
    full = npairs > 0
    mean = numpy.zeros(xsum.shape)
    mean[full] = xsum[full] / npairs[full]
    assert (numpy.abs(mean - want['mean']) <= rtol * want['mean']).all()


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('mode,kw', [('1d', {}), ('2d', dict(Nmu=10)),
                                     ('projected', dict(pimax=40))])
def test_empty_second_catalogue(mode, kw, periodic):
    empty = ArrayCatalog({'Position': numpy.zeros((0, 3)),
                          'Weight': numpy.zeros(0)}, BoxSize=512.)
    r = SimulationBoxPairCount(mode, catalog('A1'), EDGES_A, second=empty,
                               periodic=periodic, **kw)
    assert r.attrs['is_cross'] and r.attrs['N2'] == 0
    assert r.attrs['total_wnpairs'] == 0.
    assert r.pairs['npairs'].shape == ((9,) if mode == '1d' else
                                       (9, 10) if mode == '2d' else (9, 40))
    assert (r.pairs['npairs'] == 0).all()
    assert (r.pairs['wnpairs'] == 0.).all()
    assert (r.pairs[r.pairs.dims[0]] == 0.).all()
