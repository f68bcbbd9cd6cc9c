"""
Kernel-level tests of nbk_cgm_resolve_f64, nbk_cgm_host_f64 and
nbk_cgm_count_f64 (csrc/nbk_cgm.hip), called through the C ABI with
hand-picked grids over a layout sorted by the nbk_fof_* sort calls, and
compared with the brute force of cgm_reference.py — never with another GPU
kernel.

Every comparison is exact equality of integers: the brute force rounds
every operation like the kernel (the library is built with
-ffp-contract=off), so the lattice, the coincident points and the pair at
half a box need no margin.
"""
from types import SimpleNamespace

import numpy
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import cgm_reference as cref                                    # noqa: E402
import fof_reference as ref                                     # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.algorithms import cgm                         # noqa: E402

DEVICE = 'cuda'
NBK_ERR_ARG = -2
SENTINEL = -7
MARGIN = 64
BOX = 100.
BOX3 = [BOX] * 3
Z = [0., 0., 1.]
OBLIQUE = [1. / 3, 2. / 3, 2. / 3]


def dev(arr):
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def filled(n, value, dtype):
    return torch.full((int(n),), value, dtype=dtype, device=DEVICE)


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def last_error(lib):
    return lib.nbk_last_error_string().decode()


def two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, chunk=1024):
    """count -> scan -> scatter -> fine pass; the start table and the
    index column are checked against the reference before the walk reads
    through them"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    n = len(pos)
    ncoarse_all = int(numpy.prod(ncoarse))
    ncells = ncoarse_all * int(numpy.prod(fine))
    grid = (hiplib.f64_arr(origin), hiplib.f64_arr(inv_cell),
            hiplib.int_arr(ncoarse), hiplib.int_arr(fine))
    ids = ref.cell_ids(pos, origin, inv_cell, ncoarse, fine)
    pos_t = dev(pos)
    index_t = dev(numpy.arange(n, dtype='f8'))
    cpos = filled(3 * n, float('nan'), torch.float64)
    cindex = filled(n, float('nan'), torch.float64)
    cstart = filled(ncoarse_all + 1, SENTINEL, torch.int32)
    if n:
        nchunks = -(-n // chunk)
        mat = filled(nchunks * ncoarse_all, SENTINEL, torch.int32)
        hiplib.check(lib.nbk_fof_cell_count_f64(
            hiplib.dptr(pos_t), n, chunk, *grid, hiplib.dptr(mat), None),
            'fof_cell_count')
        colsum = filled(9 * ncoarse_all, SENTINEL, torch.int32)
        bases = filled(nchunks * ncoarse_all, SENTINEL, torch.int32)
        hiplib.check(lib.nbk_scan_matrix_i32(
            hiplib.dptr(mat), nchunks, ncoarse_all, hiplib.dptr(colsum),
            hiplib.dptr(bases), hiplib.dptr(cstart), None), 'scan')
        hiplib.check(lib.nbk_fof_cell_scatter_f64(
            hiplib.dptr(pos_t), hiplib.dptr(index_t), n, chunk, *grid,
            hiplib.dptr(bases), hiplib.dptr(cpos), hiplib.dptr(cindex),
            None), 'fof_cell_scatter')
    spos = filled(3 * n, float('nan'), torch.float64)
    sindex = filled(n, SENTINEL, torch.int32)
    fstart = filled(ncells + 1, SENTINEL, torch.int32)
    hiplib.check(lib.nbk_fof_fine_sort_f64(
        hiplib.dptr(cpos), hiplib.dptr(cindex), n, *grid,
        hiplib.dptr(cstart), hiplib.dptr(spos), hiplib.dptr(sindex),
        hiplib.dptr(fstart), None), 'fof_fine_sort')
    want_start = numpy.concatenate(
        [[0], numpy.cumsum(numpy.bincount(ids, minlength=ncells))])
    assert_array_equal(host(fstart), want_start)
    got_index = host(sindex)
    assert_array_equal(numpy.sort(got_index), numpy.arange(n))
    assert_array_equal(ids[got_index], ref.sorted_keys(want_start))
    assert_array_equal(host(spos).reshape(3, n).T, pos[got_index])
    return SimpleNamespace(n=n, pos=spos, index=got_index, start=fstart,
                           ncoarse=list(ncoarse), fine=list(fine))


def common_args(s, sprio, box, periodic, los, rperp, rpar, replace=None):
    """the arguments the three calls share; ``replace`` overrides them by
    name"""
    a = dict(n=s.n, ncoarse=s.ncoarse, fine=s.fine,
             box=box if periodic else [0.] * 3, los_mode=0 if los else 1,
             los=los if los else [0.] * 3, rperp2=float(rperp) * float(rperp),
             rpar2=float(rpar) * float(rpar))
    a.update(replace or {})
    return (hiplib.dptr(s.pos), hiplib.dptr(s.start), hiplib.dptr(sprio),
            a['n'], hiplib.int_arr(a['ncoarse']), hiplib.int_arr(a['fine']),
            hiplib.f64_arr(a['box']), 1 if periodic else 0, a['los_mode'],
            hiplib.f64_arr(a['los']), a['rperp2'], a['rpar2'])


def sweep(lib, common, state):
    """one resolve sweep; (decided, undecided)"""
    flags = filled(2 + MARGIN, 0, torch.int32)
    hiplib.check(lib.nbk_cgm_resolve_f64(
        *common, hiplib.dptr(state), hiplib.dptr(flags), None),
        'nbk_cgm_resolve')
    flags_h = host(flags)
    assert (flags_h[2:] == 0).all() and set(flags_h[:2]) <= {0, 1}
    return int(flags_h[0]), int(flags_h[1])


def run_cgm(lib, s, prio, box, periodic, los, rperp, rpar):
    """sweeps to the fixpoint, host and count over a sorted layout:
    (state, host, nsat) in INPUT order, host as input indices, and the
    number of sweeps.  Every output has a margin behind it that must come
    back untouched."""
    n = s.n
    sprio = dev(numpy.asarray(prio, dtype='i4')[s.index])
    common = common_args(s, sprio, box, periodic, los, rperp, rpar)
    state = filled(n + MARGIN, SENTINEL, torch.int32)
    state[:n] = 0
    sweeps = 0
    while True:
        decided, undecided = sweep(lib, common, state)
        sweeps += 1
        if not undecided:
            break
        assert decided and sweeps <= n
    # one more sweep leaves a final state alone
    before = host(state).copy()
    assert sweep(lib, common, state) == (0, 0)
    assert_array_equal(host(state), before)

    host_t = filled(n + MARGIN, SENTINEL, torch.int32)
    nsat_t = filled(n + MARGIN, SENTINEL, torch.int32)
    hiplib.check(lib.nbk_cgm_host_f64(
        *common, hiplib.dptr(state), hiplib.dptr(host_t), None),
        'nbk_cgm_host')
    hiplib.check(lib.nbk_cgm_count_f64(
        *common, hiplib.dptr(state), hiplib.dptr(host_t),
        hiplib.dptr(nsat_t), None), 'nbk_cgm_count')
    state_h, host_h, nsat_h = host(state), host(host_t), host(nsat_t)
    for out in (state_h, host_h, nsat_h):
        assert (out[n:] == SENTINEL).all()
    assert ((host_h[:n] >= 0) & (host_h[:n] < max(n, 1))).all()
    state_in = numpy.empty(n, dtype='i4')
    host_in = numpy.empty(n, dtype='i8')
    nsat_in = numpy.empty(n, dtype='i8')
    state_in[s.index] = state_h[:n]
    host_in[s.index] = s.index[host_h[:n]]
    nsat_in[s.index] = nsat_h[:n]
    return state_in, host_in, nsat_in, sweeps


def check_cgm(lib, pos, prio, box, periodic, los, rperp, rpar, ncoarse, fine,
              origin=None, inv_cell=None):
    """sort, run and compare with the brute force; returns the brute
    force's (state, host, nsat) and the number of sweeps"""
    pos = numpy.asarray(pos, dtype='f8')
    prio = numpy.asarray(prio)
    if origin is None:
        origin, inv_cell = ref.uniform_grid(box, ncoarse, fine)
    adj = cref.neighbours(pos, box, rperp, rpar, los, periodic)
    want_state, want_host = cref.greedy(adj, prio)
    want_nsat = numpy.bincount(want_host[want_state == 2],
                               minlength=len(pos))
    s = two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine)
    state, host_in, nsat, sweeps = run_cgm(lib, s, prio, box, periodic, los,
                                           rperp, rpar)
    assert_array_equal(state, want_state)
    assert_array_equal(host_in, want_host)
    assert_array_equal(nsat, want_nsat)
    return want_state, want_host, want_nsat, sweeps


def uniform(n, box=BOX, seed=21):
    rng = numpy.random.RandomState(seed)
    return rng.uniform(size=(n, 3)) * box, rng.permutation(n)


# ---- 1. a uniform box, every line of sight -----------------------------------

@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('los', [Z, OBLIQUE, None], ids=['z', 'oblique',
                                                         'observer'])
def test_uniform_box(lib, los, periodic):
    # cells of 12.5 cover the largest extent, 11.4 (the observer's rmax,
    # or 8 sqrt(1 - 4/9) + 8 * 2/3 on the oblique axes)
    pos, prio = uniform(1500)
    assert cgm.cylinder_extent(8., 8., los).max() < 12.5
    state, _, nsat, sweeps = check_cgm(lib, pos, prio, BOX3, periodic, los,
                                       8., 8., (2, 2, 2), (4, 4, 4))
    assert 1 < sweeps < 20
    assert 300 < (state == 1).sum() < 1200 and nsat.max() > 2


def test_observer_far_from_the_origin(lib):
    pos, prio = uniform(1500)
    origin, inv_cell = ref.uniform_grid(BOX3, (2, 2, 2), (4, 4, 4))
    check_cgm(lib, pos + 300., prio, None, False, None, 8., 8., (2, 2, 2),
              (4, 4, 4), origin=origin + 300., inv_cell=inv_cell)


def test_long_and_flat_cylinders(lib):
    pos, prio = uniform(1500)
    # (4, 4, 2) cells of (25, 25, 50)
    check_cgm(lib, pos, prio, BOX3, True, Z, 4., 40., (2, 2, 2), (2, 2, 1))
    # (3, 4, 3) cells of (33, 25, 33) for a disc of 30 across y
    check_cgm(lib, pos, prio, BOX3, False, [0., 1., 0.], 30., 3., (1, 1, 1),
              (3, 4, 3))


# ---- 2. few cells on an axis ---------------------------------------------------

@pytest.mark.parametrize('ncoarse, fine', [
    ((1, 1, 1), (1, 1, 1)), ((2, 1, 1), (1, 2, 1)), ((1, 1, 1), (2, 1, 2)),
    ((1, 2, 4), (1, 1, 1)), ((1, 1, 3), (2, 3, 1))])
@pytest.mark.parametrize('periodic', [True, False])
def test_1_to_4_cells_per_axis(lib, ncoarse, fine, periodic):
    # no cell is visited twice: nsat would count a satellite twice
    pos, prio = uniform(500)
    _, _, nsat, _ = check_cgm(lib, pos, prio, BOX3, periodic, Z, 12., 12.,
                              ncoarse, fine)
    assert nsat.max() > 2


def test_everything_in_one_cell(lib):
    # 300 objects, more than a block, in one cell of 216
    pos, prio = uniform(300)
    pos = 41. + 0.3 * pos / BOX
    for periodic in (True, False):
        state, _, _, _ = check_cgm(lib, pos, prio, BOX3, periodic, Z, 0.04,
                                   0.04, (3, 3, 3), (2, 2, 2))
        assert 10 < (state == 1).sum() < 290
    # and in the only cell of a grid
    check_cgm(lib, pos, prio, BOX3, True, OBLIQUE, 0.04, 0.04, (1, 1, 1),
              (1, 1, 1))


@pytest.mark.parametrize('periodic', [True, False])
def test_mostly_empty_cells(lib, periodic):
    pos, prio = uniform(200)
    state, _, _, _ = check_cgm(lib, pos, prio, BOX3, periodic, Z, 8., 8.,
                               (3, 4, 2), (4, 3, 6))
    assert (state == 2).sum() > 10


# ---- 3. ties of the predicate ----------------------------------------------------

def test_coincident_points(lib):
    pos = numpy.ones((70, 3)) * [12.5, 50., 99.]
    prio = numpy.random.RandomState(4).permutation(70)
    for los in (Z, None):
        state, host_in, nsat, sweeps = check_cgm(
            lib, pos, prio, BOX3, True, los, 1., 1., (2, 2, 2), (2, 2, 2))
        top = numpy.argmax(prio)
        assert (state == 1).sum() == 1 and state[top] == 1
        assert (host_in == top).all()
        assert nsat[top] == 69 and nsat.sum() == 69
        # (a sweep may already see the central it has just made)
        assert sweeps <= 2


@pytest.mark.parametrize('periodic', [True, False])
def test_unit_lattice_with_unit_radii(lib, periodic):
    # every separation is an integer: <= decides on the exact boundary
    pos = ref.lattice(8, 8.)
    prio = numpy.random.RandomState(6).permutation(len(pos))
    adj = cref.neighbours(pos, [8.] * 3, 1., 1., Z, periodic)
    if periodic:
        # dz in {-1, 0, 1} and dx2 + dy2 <= 1: 14 neighbours each
        assert (adj.sum(axis=1) == 14).all()
    check_cgm(lib, pos, prio, [8.] * 3, periodic, Z, 1., 1., (2, 2, 2),
              (2, 2, 2))
    check_cgm(lib, pos, prio, [8.] * 3, periodic, None, 1., 1., (2, 2, 2),
              (2, 2, 2))


def test_pair_at_exactly_half_a_box(lib):
    box = [16.] * 3
    rng = numpy.random.RandomState(9)
    others = rng.uniform(size=(40, 3)) * 16.
    for pair in ([[10., 10., 2.], [10., 10., 10.]],
                 [[2., 10., 10.], [10., 10., 10.]]):
        pos = numpy.concatenate([pair, others])
        for prio in (numpy.arange(42), numpy.arange(42)[::-1]):
            for rperp, rpar in ((8., 8.), (1., 8.), (8., 1.), (7.999, 7.999)):
                adj = cref.neighbours(pos, box, rperp, rpar, Z, True)
                assert adj[0, 1] == adj[1, 0]
                check_cgm(lib, pos, prio, box, True, Z, rperp, rpar,
                          (1, 1, 1), (2, 2, 2))
    # the two alone: a central and its satellite, or two centrals
    pos = [[10., 10., 2.], [10., 10., 10.]]
    state, _, nsat, _ = check_cgm(lib, pos, [0, 1], box, True, Z, 1., 8.,
                                  (1, 1, 1), (2, 2, 2))
    assert_array_equal(state, [2, 1])
    assert_array_equal(nsat, [0, 1])
    state, _, _, _ = check_cgm(lib, pos, [0, 1], box, True, Z, 1., 7.999,
                               (1, 1, 1), (2, 2, 2))
    assert_array_equal(state, [1, 1])


def test_nan_pair_about_the_observer(lib):
    # 0 and 1 lie symmetrically about the observer: 0 / 0, no pair,
    # although either is a neighbour of 2
    pos = [[3., 4., 5.], [-3., -4., -5.], [3., 4., 5.5]]
    state, host_in, nsat, _ = check_cgm(
        lib, pos, [2, 1, 0], None, False, None, 100., 100., (1, 1, 1),
        (1, 1, 1), origin=[-3., -4., -5.], inv_cell=[0.1] * 3)
    assert_array_equal(state, [1, 1, 2])
    assert_array_equal(host_in, [0, 1, 0])
    assert_array_equal(nsat, [1, 0, 0])


# ---- 4. the thin cylinder ----------------------------------------------------------

def test_thin_cylinder_on_the_grid_of_cgm_grid(lib):
    # rpar / rperp = 1e4: pairs at the rim, on cells of the bare minimum
    # side along the line of sight (10 cells of 10.00000001)
    box = [100.0000001] * 3
    rng = numpy.random.RandomState(17)
    m = 400
    centre = rng.uniform(size=(m, 3)) * box[0]
    angle = rng.uniform(size=m) * 2 * numpy.pi
    shrink = 1. - 10. ** rng.uniform(-16, -3, size=(m, 1))
    half = 0.5 * shrink * numpy.stack(
        [1e-3 * numpy.cos(angle), 1e-3 * numpy.sin(angle),
         10. * rng.choice([-1., 1.], size=m)], axis=1)
    pos = numpy.remainder(numpy.concatenate([centre + half, centre - half]),
                          box[0])
    prio = rng.permutation(2 * m)
    # (cells of 1 across the line of sight: 99 x 99 x 10)
    origin, inv_cell, ncoarse, fine = cgm.cgm_grid(True, box, 1e-3, 10., Z,
                                                   2 * 10 ** 6, per_cell=2.)
    ncell = numpy.array(ncoarse) * numpy.array(fine)
    assert ncell[2] == 10 and ncell[0] * ncell[1] * ncell[2] < 2 * 10 ** 5
    state, _, _, _ = check_cgm(lib, pos, prio, box, True, Z, 1e-3, 10.,
                               ncoarse, fine, origin=origin,
                               inv_cell=inv_cell)
    assert (state == 2).sum() > m // 4


# ---- 5. the adversarial line ----------------------------------------------------------

def test_line_of_200_points(lib):
    pos, prio = cref.line(200)
    # 100 cells of 1.99 along x; y and z are flat
    state, _, nsat, sweeps = check_cgm(
        lib, pos, prio, None, False, Z, 1.5, 1.5, (25, 1, 1), (4, 1, 1),
        origin=[0.5, 0., 0.], inv_cell=[100 / 199., 0., 0.])
    assert_array_equal(state, numpy.tile([1, 2], 100))
    assert_array_equal(nsat, numpy.tile([1, 0], 100))
    assert 1 < sweeps <= 200


# ---- 6. nothing and one ----------------------------------------------------------------

def test_nothing_launches_nothing(lib):
    s = two_level_sort(lib, numpy.zeros((0, 3)), [0.] * 3, [0.04] * 3,
                       (2, 2, 2), (2, 2, 2))
    state, host_in, nsat, sweeps = run_cgm(lib, s, numpy.zeros(0, 'i4'),
                                           BOX3, True, Z, 1., 1.)
    assert len(state) == len(host_in) == len(nsat) == 0 and sweeps == 1


@pytest.mark.parametrize('periodic', [True, False])
def test_one_object(lib, periodic):
    state, host_in, nsat, sweeps = check_cgm(
        lib, [[99., 0.5, 50.]], [0], BOX3, periodic, Z, 60., 60., (1, 1, 1),
        (1, 2, 1))
    assert (state[0], host_in[0], nsat[0], sweeps) == (1, 0, 0, 1)


# ---- 7. bad arguments --------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(lib):
    pos, prio = uniform(100)
    origin, inv_cell = ref.uniform_grid(BOX3, (2, 2, 2), (2, 2, 2))
    s = two_level_sort(lib, pos, origin, inv_cell, (2, 2, 2), (2, 2, 2))
    sprio = dev(prio.astype('i4')[s.index])
    outs = [filled(100, SENTINEL, torch.int32) for _ in range(4)]
    state, flags, host_t, nsat = outs
    nan, inf = float('nan'), float('inf')
    cases = [dict(rperp2=-1.), dict(rperp2=nan), dict(rperp2=inf),
             dict(rpar2=-1e-300), dict(rpar2=nan), dict(rpar2=inf),
             dict(los_mode=2), dict(los_mode=-1), dict(los=[0., nan, 1.]),
             dict(los=[inf, 0., 0.]), dict(box=[100., 0., 100.]),
             dict(box=[100., 100., -1.]), dict(box=[nan, 100., 100.]),
             dict(n=-1), dict(n=2 ** 31), dict(ncoarse=[2, 0, 2]),
             dict(fine=[2, 2, -1]), dict(ncoarse=[64, 64, 64]),
             dict(fine=[64, 64, 64])]
    for case in cases:
        common = common_args(s, sprio, BOX3, True, Z, 8., 8., case)
        calls = [
            ('nbk_cgm_resolve_f64', lambda: lib.nbk_cgm_resolve_f64(
                *common, hiplib.dptr(state), hiplib.dptr(flags), None)),
            ('nbk_cgm_host_f64', lambda: lib.nbk_cgm_host_f64(
                *common, hiplib.dptr(state), hiplib.dptr(host_t), None)),
            ('nbk_cgm_count_f64', lambda: lib.nbk_cgm_count_f64(
                *common, hiplib.dptr(state), hiplib.dptr(host_t),
                hiplib.dptr(nsat), None))]
        for name, call in calls:
            assert call() == NBK_ERR_ARG, (name, case)
            assert name in last_error(lib)
        for out in outs:
            assert (host(out) == SENTINEL).all(), case
    # box and los are not read when not periodic / in observer mode
    state = filled(100, 0, torch.int32)
    common = common_args(s, sprio, None, False, None, 8., 8.,
                         dict(los=[nan] * 3, box=[nan] * 3))
    flags = filled(2, 0, torch.int32)
    hiplib.check(lib.nbk_cgm_resolve_f64(
        *common, hiplib.dptr(state), hiplib.dptr(flags), None), 'resolve')
    assert host(flags)[0] == 1
