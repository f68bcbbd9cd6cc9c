"""
Kernel-level tests of the sky modes of the pair counter
(nbk_pairs_count_sky_f64 in csrc/nbk_pairs.hip: 3 = (s, mu), 4 = (rp, pi)
with the midpoint line of sight, 5 = theta), called through the C ABI
with grids, block counts and bin slices the Python driver never picks,
and compared with the brute-force oracle (survey_bruteforce.py) — never
with another GPU kernel.

The project's bars (DESIGN.md "Reproducibility"): ``npairs`` equals the
oracle exactly and is bitwise equal between two runs; the sum of weights
and the mean s or rp are within 4 (n_bin + 4) 2^-53 relative, per bin.
The mean theta gets 12 x 2^-53 on top: 4 ulp for the device asin (the
OpenCL bound for a double asin, which the device math library is assumed
to meet), 1 ulp for the host's, and correctly rounded sqrt, division and
products on bit-identical inputs.  Exact counts are fair because every
random catalogue first asserts, on the oracle, that no pair lies within
relative 1e-10 of a squared first-dimension edge nor within absolute
1e-10 of a mu or pi edge; the hand-built cases are exempt, their
arithmetic is exact.

Every cell-start table is compared with the reference before a count
kernel reads through it.
"""
import functools
from types import SimpleNamespace

import numpy
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import pairs_reference as ref                                   # noqa: E402
import survey_bruteforce as sb                                  # noqa: E402
from nbodykit_amd import hiplib, transform                      # noqa: E402
from nbodykit_amd.cosmology import Planck15                     # noqa: E402
from nbodykit_amd.algorithms.pair_counters import kernel       # noqa: E402

DEVICE = 'cuda'
NBK_ERR_ARG = -2
EPS = 2.0 ** -53
MARGIN = 1e-10
MODES = {0: '1d', 3: '2d', 4: 'projected', 5: 'angular'}
SENTINEL = -7


def dev(arr):
    # (a copy: the cached catalogues are read-only arrays)
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def filled(n, value, dtype):
    return torch.full((int(n),), value, dtype=dtype, device=DEVICE)


def nan_f64(n):
    """outputs start as NaN so a slot the kernel never wrote shows up"""
    return filled(n, float('nan'), torch.float64)


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def last_error(lib):
    return lib.nbk_last_error_string().decode()


# ---- catalogues ----------------------------------------------------------

def _cartesian(sky, seed, n):
    ra, dec, z = sky(seed, n)
    return transform.SkyToCartesian(ra, dec, z, Planck15)


def _unit(sky, seed, n):
    return transform.SkyToUnitSphere(*sky(seed, n))


def _rays():
    """integer multiples m = 1..5 of five integer directions of norm 3,
    one of them opposite to another: pairs on one ray have mu = 1
    exactly, the m = m pairs of the opposite rays have l = 0"""
    dirs = numpy.array([[1., 2., 2.], [2., 1., 2.], [2., 2., 1.],
                        [-1., 2., 2.], [-1., -2., -2.]])
    m = numpy.arange(1., 6.)
    return (dirs[:, None, :] * m[None, :, None]).reshape(-1, 3)


_BUILDERS = {
    'SURVEY1': lambda: _cartesian(sb.sky_survey, 42, 1000),
    'SURVEY2': lambda: _cartesian(sb.sky_survey, 84, 700),
    'CLUMP1': lambda: _cartesian(sb.sky_clump, 5, 700),
    'CLUMP2': lambda: _cartesian(sb.sky_clump, 6, 450),
    'CLUMP1-256': lambda: _cartesian(sb.sky_clump, 5, 700)[:256],
    'CLUMP1-257': lambda: _cartesian(sb.sky_clump, 5, 700)[:257],
    'CLUMP1-513': lambda: _cartesian(sb.sky_clump, 5, 700)[:513],
    'PATCH1': lambda: _unit(sb.sky_patch, 3, 1500),
    'PATCH2': lambda: _unit(sb.sky_patch, 4, 900),
    'CAP1': lambda: _unit(sb.sky_cap, 3, 1500),
    'CAP2': lambda: _unit(sb.sky_cap, 4, 900),
    'SPHERE1': lambda: _unit(sb.sky_sphere, 3, 600),
    'SPHERE2': lambda: _unit(sb.sky_sphere, 4, 400),
    'RAYS': _rays,
}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """(positions (n, 3), weights (n,)) of a named catalogue, read-only"""
    pos = numpy.ascontiguousarray(_BUILDERS[name](), dtype='f8')
    w = ref.weights(len(pos))
    pos.setflags(write=False)
    w.setflags(write=False)
    return pos, w


def driver_grid(names, rmax):
    """the driver's grid over the joint bounding box of ``names``"""
    allpos = numpy.concatenate([catalogue(n)[0] for n in names])
    return kernel.make_grid(False, None, rmax, allpos.min(axis=0),
                            allpos.max(axis=0))


def one_cell_grid(names):
    """a forced (1, 1, 1) grid: inv_cell = 0 puts every row in cell 0"""
    allpos = numpy.concatenate([catalogue(n)[0] for n in names])
    return allpos.min(axis=0), numpy.zeros(3), [1, 1, 1]


# ---- the cell sort, checked against the reference -------------------------

_sorted = {}


def sorted_cat(name, grid):
    """device-resident cell-sorted catalogue, built once per (catalogue,
    grid); the cursors, the cell-start table and the sorted rows are
    compared with the reference before anything reads through them"""
    origin, inv_cell, ncell = grid
    key = (name, tuple(origin), tuple(inv_cell), tuple(ncell))
    if key in _sorted:
        return _sorted[key]
    lib = hiplib.require()
    pos, w = catalogue(name)
    n = len(pos)
    ncells = int(numpy.prod(ncell))
    chunk = n // 5 + 1
    nchunks = -(-n // chunk)
    og, iv, nc = (hiplib.f64_arr(origin), hiplib.f64_arr(inv_cell),
                  hiplib.int_arr(ncell))
    pos_t, w_t = dev(pos), dev(w)
    mat = filled(nchunks * ncells, -1, torch.int32)
    hiplib.check(lib.nbk_pairs_cell_count_f64(
        hiplib.dptr(pos_t), n, chunk, og, iv, nc, hiplib.dptr(mat), None),
        'pairs_cell_count')
    colsum = filled(9 * ncells, -1, torch.int32)
    bases = filled(nchunks * ncells, -1, torch.int32)
    start = filled(ncells + 1, -1, torch.int32)
    hiplib.check(lib.nbk_scan_matrix_i32(
        hiplib.dptr(mat), nchunks, ncells, hiplib.dptr(colsum),
        hiplib.dptr(bases), hiplib.dptr(start), None), 'scan')

    ids = ref.cell_ids(pos, origin, inv_cell, ncell)
    want_mat = ref.chunk_histograms(ids, ncells, chunk)
    want_bases, want_start = ref.scan_matrix(want_mat)
    assert_array_equal(host(mat).reshape(nchunks, ncells), want_mat)
    assert_array_equal(host(bases).reshape(nchunks, ncells), want_bases)
    assert_array_equal(host(start), want_start)

    out, out_w = nan_f64(3 * n), nan_f64(n)
    hiplib.check(lib.nbk_pairs_cell_scatter_f64(
        hiplib.dptr(pos_t), hiplib.dptr(w_t), n, chunk, og, iv, nc,
        hiplib.dptr(bases), hiplib.dptr(out), hiplib.dptr(out_w), None),
        'pairs_cell_scatter')
    want_start, want_rows = ref.sorted_reference(pos, w, ids, ncells)
    assert_array_equal(host(start), want_start)
    got_rows = ref.canonical_rows(host(out).reshape(3, n).T, host(out_w),
                                  ref.sorted_keys(want_start))
    assert_array_equal(got_rows, want_rows)
    s = SimpleNamespace(n=n, pos=out, w=out_w, start=start, ncells=ncells,
                        ncell=[int(k) for k in ncell],
                        occupancy=numpy.diff(want_start))
    _sorted[key] = s
    return s


def empty_sorted(ncell):
    ncells = int(numpy.prod(ncell))
    return SimpleNamespace(
        n=0, pos=None, w=None,
        start=filled(ncells + 1, 0, torch.int32), ncells=ncells)


# ---- the oracle -----------------------------------------------------------

def second_edges(mode, nb1):
    """nb1 = Nmu (mode 3) or pimax (mode 4)"""
    if mode == 3:
        return numpy.linspace(0, 1., nb1 + 1)
    if mode == 4:
        return numpy.linspace(0, nb1, int(nb1 + 1))
    return None


@functools.lru_cache(maxsize=None)
def oracle(first, second, mode, edges, nb1):
    """The brute-force result of a case: computed once, shared."""
    pos1, w1 = catalogue(first)
    pos2 = w2 = None
    if second is not None:
        pos2, w2 = catalogue(second)
    kw = {3: dict(Nmu=nb1), 4: dict(pimax=nb1)}.get(mode, {})
    want = sb.bruteforce_survey_paircount(
        MODES[mode], pos1, numpy.array(edges), w1=w1, pos2=pos2, w2=w2,
        **kw)
    for v in want.values():
        if isinstance(v, numpy.ndarray):
            v.setflags(write=False)
    return want


def check_margins(want):
    """exact npairs is only fair when no pair sits on a bin edge"""
    print('npairs total %d, margins %.3g %.3g, mu >= 1: %d, no mu: %d'
          % (want['npairs'].sum(), want['margin0'], want['margin1'],
             want['n_top'], want['n_nan']))
    assert want['margin0'] > MARGIN
    assert want['margin1'] > MARGIN


class Outputs(object):
    """(nb0, nb1) device outputs prefilled with sentinels"""

    def __init__(self, nb0, nb1):
        self.shape = (nb0, nb1)
        self.npairs = filled(nb0 * nb1, SENTINEL, torch.int64)
        self.wsum = nan_f64(nb0 * nb1)
        self.xsum = nan_f64(nb0 * nb1)

    def arrays(self):
        return (host(self.npairs).reshape(self.shape),
                host(self.wsum).reshape(self.shape),
                host(self.xsum).reshape(self.shape))


def first_edges_sq(mode, edges):
    edges = numpy.asarray(edges, dtype='f8')
    return sb.chord_edges_sq(edges) if mode == 5 else edges * edges


def call_sky(lib, s1, s2, ncell, mode, edges, nb1, nblocks, out=None, j0=0,
             j1=None, autocorr=None, e0sq_mode=None):
    """one nbk_pairs_count_sky_f64 call; ``s2 is None`` is the
    auto-correlation.  ``partials`` starts as NaN."""
    nb0 = len(edges) - 1
    j1 = nb1 if j1 is None else j1
    auto = s2 is None
    if auto:
        s2 = s1
    out = Outputs(nb0, nb1) if out is None else out
    e0sq = dev(first_edges_sq(mode if e0sq_mode is None else e0sq_mode,
                              edges))
    e1 = second_edges(mode, nb1)
    if e1 is None and mode not in (0, 5):
        e1 = numpy.linspace(0, 1., nb1 + 1)    # (a rejected mode's)
    e1_t = None if e1 is None else dev(e1)
    partials = nan_f64(3 * max(nblocks, 1) * nb0 * max(j1 - j0, 1))
    rc = lib.nbk_pairs_count_sky_f64(
        hiplib.dptr(s1.pos), hiplib.dptr(s1.w), hiplib.dptr(s1.start), s1.n,
        hiplib.dptr(s2.pos), hiplib.dptr(s2.w), hiplib.dptr(s2.start), s2.n,
        int(auto) if autocorr is None else autocorr,
        hiplib.int_arr(ncell), mode, hiplib.dptr(e0sq), nb0,
        hiplib.dptr(e1_t), nb1, j0, j1, nblocks, hiplib.dptr(partials),
        hiplib.dptr(out.npairs), hiplib.dptr(out.wsum),
        hiplib.dptr(out.xsum), None)
    torch.cuda.synchronize()
    return rc, out


def check_counts(got, want, mode, columns=slice(None)):
    """``got`` = (npairs, wsum, xsum) as (nb0, nb1); the oracle's arrays
    are (nb0,) or (nb0, nb1)"""
    npairs, wsum, xsum = (a[:, columns] for a in got)
    wn, ww, wm = (want[k].reshape(got[0].shape)[:, columns]
                  for k in ('npairs', 'wnpairs', 'mean'))
    assert_array_equal(npairs, wn.astype('i8'))
    mean = numpy.zeros(xsum.shape)
    full = npairs > 0
    mean[full] = xsum[full] / npairs[full]
    assert (xsum[~full] == 0).all() and (wsum[~full] == 0).all()
    rtol = 4 * (wn.astype('f8') + 4) * EPS
    # the angle goes through asin on either side
    rtol_mean = rtol + (12 * EPS if mode == 5 else 0.)
    for name, g, r, tol in [('wnpairs', wsum, ww, rtol),
                            ('mean', mean, wm, rtol_mean)]:
        err = numpy.abs(g - r)
        print('%s: max err / bound: %.3g'
              % (name, (err / (tol * numpy.abs(r) + 1e-300)).max()))
        assert (err <= tol * numpy.abs(r)).all()


def count_and_check(lib, s1, s2, ncell, mode, edges, nb1, nblocks, want):
    rc, out = call_sky(lib, s1, s2, ncell, mode, edges, nb1, nblocks)
    assert rc == 0, last_error(lib)
    got = out.arrays()
    check_counts(got, want, mode)
    # bitwise reproducible integer counts
    rc, again = call_sky(lib, s1, s2, ncell, mode, edges, nb1, nblocks)
    assert rc == 0
    assert_array_equal(again.arrays()[0], got[0])
    return got


def run_slices(lib, s1, s2, ncell, mode, edges, nb1, nblocks, slices, want):
    """count the second-dimension slices [j0, j1) one call each, in the
    order given; after every call the columns not yet counted still hold
    the sentinel and the counted ones the oracle's values"""
    out = Outputs(len(edges) - 1, nb1)
    done = numpy.zeros(nb1, dtype=bool)
    for j0, j1 in slices:
        rc, _ = call_sky(lib, s1, s2, ncell, mode, edges, nb1, nblocks,
                         out=out, j0=j0, j1=j1)
        assert rc == 0, last_error(lib)
        done[j0:j1] = True
        npairs, wsum, xsum = out.arrays()
        assert (npairs[:, ~done] == SENTINEL).all()
        assert numpy.isnan(wsum[:, ~done]).all()
        assert numpy.isnan(xsum[:, ~done]).all()
        check_counts((npairs, wsum, xsum), want, mode, columns=done)
    assert done.all()


# ---- 1. the survey and the clump on the driver's grid ---------------------

# (catalogues, mode) -> (first-dimension edges, nb1)
SKY_BINS = {
    ('SURVEY', 3): (tuple(numpy.linspace(10, 1000, 10)), 50),
    ('SURVEY', 4): (tuple(numpy.linspace(5, 100, 9)), 40),
    ('CLUMP', 3): (tuple(numpy.linspace(2, 60, 8)), 10),
    ('CLUMP', 4): (tuple(numpy.linspace(1, 40, 9)), 30),
}


def sky_rmax(mode, edges, nb1):
    return kernel.max_3d_separation(MODES[mode], edges,
                                    nb1 if mode == 4 else None)


@pytest.mark.parametrize('pair', ['auto', 'cross'])
@pytest.mark.parametrize('mode', [3, 4])
@pytest.mark.parametrize('cat', ['SURVEY', 'CLUMP'])
def test_count_sky_fixtures(lib, cat, mode, pair):
    """SURVEY (1000 and 700 points over a quarter of the sky, z ~ 0.5):
    the driver's grid is (1, 3, 1) cells of side >= 1000 in (s, mu) and
    thousands of cells of side >= sqrt(100^2 + 40^2) in (rp, pi).  CLUMP
    (700 and 450 points about 70 Mpc/h across): one cell of more than
    256 points, so the tile loop takes two or three trips."""
    edges, nb1 = SKY_BINS[cat, mode]
    names = [cat + '1', cat + '2']
    second = names[1] if pair == 'cross' else None
    want = oracle(names[0], second, mode, edges, nb1)
    check_margins(want)
    grid = driver_grid(names, sky_rmax(mode, edges, nb1))
    s1 = sorted_cat(names[0], grid)
    s2 = None if second is None else sorted_cat(second, grid)
    if cat == 'CLUMP':
        assert s1.ncell == [1, 1, 1] and s1.occupancy.max() > 512
    elif mode == 3:
        assert s1.ncell == [1, 3, 1]
    else:
        assert s1.ncells > 1000
    count_and_check(lib, s1, s2, s1.ncell, mode, edges, nb1, 7, want)


# ---- 2. more bins than one pass holds -------------------------------------

EDGES17 = tuple(numpy.linspace(2, 60, 18))


def test_count_sky_over_capacity(lib):
    """CLUMP1 auto with 17 x 241 = 4097 bins: refused in one pass, and
    the same counts from two slices of the mu bins"""
    assert 17 * 241 == lib.nbk_pairs_max_bins() + 1
    want = oracle('CLUMP1', None, 3, EDGES17, 241)
    check_margins(want)
    s = sorted_cat('CLUMP1', driver_grid(['CLUMP1'], 60.))
    out = Outputs(17, 241)
    rc, _ = call_sky(lib, s, None, s.ncell, 3, EDGES17, 241, 6, out=out)
    assert rc == NBK_ERR_ARG
    assert 'nbk_pairs_count_sky_f64' in last_error(lib)
    assert (out.arrays()[0] == SENTINEL).all()
    run_slices(lib, s, None, s.ncell, 3, EDGES17, 241, 6,
               [(120, 241), (0, 120)], want)


RAY_EDGES = (0.5, 4., 8., 16., 40.)


@pytest.mark.parametrize('quarters', [((0, 4),), ((0, 2), (2, 4)),
                                      ((2, 4), (0, 2)),
                                      ((3, 4), (0, 1), (1, 3))])
@pytest.mark.parametrize('mode', [3, 4])
def test_count_sky_closed_top_bin_in_slices(lib, mode, quarters):
    """RAYS: the ordered pairs on a common line through the origin have
    mu = 1 exactly and belong to the last mu bin, which is closed above
    only in the slice that ends at nb1: a slice [0, 2) must not take
    them for its own top bin.  The 10 ordered pairs p2 = -p1 have no mu
    and no pi in any slice.  Integer coordinates: the arithmetic is
    exact.  The slices are given in quarters of the nb1 = 4 mu bins or
    8 pi bins."""
    nb1 = 4 if mode == 3 else 8
    want = oracle('RAYS', None, mode, RAY_EDGES, nb1)
    if mode == 3:
        # 20 ordered pairs on each of the 5 rays, and the 40 pairs of
        # unequal multiples on the two opposite rays
        assert want['n_top'] == 5 * 20 + 40 and want['n_nan'] == 10
        assert want['npairs'][:, -1].sum() >= want['n_top']
    s = sorted_cat('RAYS', one_cell_grid(['RAYS']))
    slices = [(a * nb1 // 4, b * nb1 // 4) for a, b in quarters]
    run_slices(lib, s, None, [1, 1, 1], mode, RAY_EDGES, nb1, 3, slices,
               want)


# ---- 3. tiles, blocks and the work split ----------------------------------

@pytest.mark.parametrize('nblocks', [1, 300])
@pytest.mark.parametrize('n', [256, 257, 513])
@pytest.mark.parametrize('mode', [3, 4])
def test_count_sky_one_cell_tiles(lib, mode, n, nblocks):
    """The first 256, 257 and 513 points of CLUMP1 in a forced (1, 1, 1)
    grid: exactly one tile, one tile and one row, two tiles and one row.
    One block walks everything (split = 4); 300 blocks give split = 64,
    more work items than 256-particle slices and more blocks than work
    items, so blocks that store all-zero partials."""
    edges, nb1 = SKY_BINS['CLUMP', mode]
    name = 'CLUMP1-%d' % n
    want = oracle(name, None, mode, edges, nb1)
    check_margins(want)
    s = sorted_cat(name, one_cell_grid([name]))
    assert s.occupancy.tolist() == [n]
    count_and_check(lib, s, None, [1, 1, 1], mode, edges, nb1, nblocks,
                    want)


EDGES8 = tuple(numpy.linspace(2, 60, 9))


@pytest.mark.parametrize('nb1', [63, 64, 65, 127, 128, 129])
def test_count_sky_histogram_copies(lib, nb1):
    """CLUMP1 auto in (s, mu) with 8 s bins and Nmu on either side of 64
    and 128: 504, 512, 520, 1016, 1024 and 1032 bins, where the
    histogram copies per block go from 4 to 2 and from 2 to 1"""
    want = oracle('CLUMP1', None, 3, EDGES8, nb1)
    check_margins(want)
    s = sorted_cat('CLUMP1', driver_grid(['CLUMP1'], 60.))
    count_and_check(lib, s, None, s.ncell, 3, EDGES8, nb1, 8, want)


@pytest.mark.parametrize('empty', ['first', 'second', 'both', 'auto'])
@pytest.mark.parametrize('mode', [3, 4, 5])
def test_count_sky_empty_sides(lib, mode, empty):
    """n1 = 0, n2 = 0 or both: NBK_OK, and the outputs are written as
    zeros, not left at the sentinel"""
    if mode == 5:
        name, edges, nb1 = 'CAP1', tuple(numpy.linspace(0.001, 1, 10)), 1
        rmax = sky_rmax(5, edges, None)
    else:
        name = 'CLUMP1'
        edges, nb1 = SKY_BINS['CLUMP', mode]
        rmax = sky_rmax(mode, edges, nb1)
    full = sorted_cat(name, driver_grid([name], rmax))
    s1 = full if empty == 'second' else empty_sorted(full.ncell)
    s2 = full if empty == 'first' else empty_sorted(full.ncell)
    if empty == 'auto':
        s2 = None
    rc, out = call_sky(lib, s1, s2, full.ncell, mode, edges, nb1, 5)
    assert rc == 0, last_error(lib)
    npairs, wsum, xsum = out.arrays()
    assert (npairs == 0).all() and (wsum == 0).all() and (xsum == 0).all()


# ---- 4. angles -------------------------------------------------------------

THETA_SMALL = tuple(numpy.linspace(0.001, 1, 10))
THETA_WIDE = (0.5, 5., 30., 60., 90., 120., 179.)
# catalogue -> [(edges, cells per axis: 0 = the driver's grid, whatever it
# is, n > 0 = the driver's grid, which has n, -n = a forced grid of n)]
ANGULAR_CASES = {
    'PATCH': [(THETA_SMALL, 0)],
    'CAP': [(THETA_SMALL, 0)],
    'SPHERE': [(THETA_WIDE[:3], 3), (THETA_WIDE[:3], -2), (THETA_WIDE, 1)],
}


@pytest.mark.parametrize('pair', ['auto', 'cross'])
@pytest.mark.parametrize('cat,case', [(c, k) for c in sorted(ANGULAR_CASES)
                                      for k in range(len(ANGULAR_CASES[c]))])
def test_count_sky_angular(lib, cat, case, pair):
    """PATCH: 12 x 10 degrees straddling RA = 0 / 360, a slab of cells
    thin in x.  CAP: 4 degrees around the pole, flat in z.  SPHERE: the
    whole sky, an extent of 2: a top edge of 30 degrees (a chord of
    0.52) gives three cells per axis, and is also run on a forced grid
    of two (cells of side 1 >= 0.52); 179 degrees gives one cell."""
    edges, ncell = ANGULAR_CASES[cat][case]
    names = [cat + '1', cat + '2']
    second = names[1] if pair == 'cross' else None
    want = oracle(names[0], second, 5, edges, 1)
    check_margins(want)
    assert want['npairs'].min() > 0
    rmax = sky_rmax(5, edges, None)
    grid = driver_grid(names, rmax)
    if ncell < 0:
        origin, inv_cell, n3 = grid
        assert n3 == [3, 3, 3]
        grid = (origin, inv_cell * (-ncell / 3.), [-ncell] * 3)
        assert (1. / grid[1] >= rmax).all()
    s1 = sorted_cat(names[0], grid)
    s2 = None if second is None else sorted_cat(second, grid)
    if ncell != 0:
        assert s1.ncell == [abs(ncell)] * 3
    else:
        assert s1.ncells > 20 and 1 in s1.ncell
    count_and_check(lib, s1, s2, s1.ncell, 5, edges, 1, 7, want)


# ---- 5. hand values --------------------------------------------------------

def one_by_one(lib, mode, p1, p2, edges, nb1):
    """the pair (p1, p2) as a 1 x 1 cross-correlation in one cell"""
    def single(p):
        return SimpleNamespace(n=1, pos=dev(numpy.array(p, dtype='f8')),
                               w=dev(numpy.array([1.])),
                               start=dev(numpy.array([0, 1], dtype='i4')))
    s1, s2 = single(p1), single(p2)
    kw = {3: dict(Nmu=nb1), 4: dict(pimax=nb1)}.get(mode, {})
    want = sb.bruteforce_survey_paircount(
        MODES[mode], numpy.array([p1], dtype='f8'), numpy.array(edges),
        pos2=numpy.array([p2], dtype='f8'), **kw)
    if mode == 0:
        # the existing entry point on a non-periodic grid
        out = Outputs(len(edges) - 1, 1)
        e0sq = dev(first_edges_sq(0, edges))
        partials = nan_f64(3 * 2 * (len(edges) - 1))
        rc = lib.nbk_pairs_count_f64(
            hiplib.dptr(s1.pos), hiplib.dptr(s1.w), hiplib.dptr(s1.start),
            1, hiplib.dptr(s2.pos), hiplib.dptr(s2.w),
            hiplib.dptr(s2.start), 1, 0, hiplib.int_arr([1, 1, 1]),
            hiplib.f64_arr([0., 0., 0.]), 0, 0, hiplib.dptr(e0sq),
            len(edges) - 1, None, 1, 0, 1, 2, hiplib.dptr(partials),
            hiplib.dptr(out.npairs), hiplib.dptr(out.wsum),
            hiplib.dptr(out.xsum), None)
    else:
        rc, out = call_sky(lib, s1, s2, [1, 1, 1], mode, edges, nb1, 2)
    assert rc == 0, last_error(lib)
    got = out.arrays()
    check_counts(got, want, mode)
    return got


def test_hand_same_sight_line(lib):
    """(3, 6, 6) and (5, 10, 10): mu = 1 exactly, pi = 6, rp^2 = 0"""
    p1, p2 = [3., 6., 6.], [5., 10., 10.]
    npairs, _, xsum = one_by_one(lib, 3, p1, p2, (1., 5., 7.), 4)
    assert_array_equal(npairs, [[0, 0, 0, 0], [0, 0, 0, 1]])
    assert xsum[1, 3] == 6.
    # rp^2 = 0 is below the first edge
    npairs, _, _ = one_by_one(lib, 4, p1, p2, (1., 5., 7.), 8)
    assert npairs.sum() == 0


def test_hand_equal_distance(lib):
    """|p1| = |p2|: mu = 0 and pi = 0"""
    p1, p2 = [3., 4., 0.], [0., 4., 3.]
    npairs, _, _ = one_by_one(lib, 3, p1, p2, (1., 5., 7.), 4)
    assert_array_equal(npairs, [[1, 0, 0, 0], [0, 0, 0, 0]])
    npairs, _, xsum = one_by_one(lib, 4, p1, p2, (1., 5., 7.), 3)
    assert_array_equal(npairs, [[1, 0, 0], [0, 0, 0]])
    assert xsum[0, 0] == numpy.sqrt(18.)


def test_hand_opposite_points(lib):
    """p2 = -p1 has no mu and no pi, and is counted in '1d'"""
    p1, p2 = [1., 2., 2.], [-1., -2., -2.]
    assert one_by_one(lib, 3, p1, p2, (1., 5., 7.), 4)[0].sum() == 0
    assert one_by_one(lib, 4, p1, p2, (1., 5., 7.), 8)[0].sum() == 0
    npairs, _, xsum = one_by_one(lib, 0, p1, p2, (1., 5., 7.), 1)
    assert_array_equal(npairs[:, 0], [0, 1])
    assert xsum[1, 0] == 6.


def test_hand_antipodes(lib):
    """antipodal directions give q = 4, dropped at a 180 degree top edge;
    0.01 degrees short of it the pair is kept"""
    assert one_by_one(lib, 5, [0., 0., 1.], [0., 0., -1.], (90., 180.),
                      1)[0].sum() == 0
    u = transform.SkyToUnitSphere([10., 190.], [20., -19.99])
    npairs, _, xsum = one_by_one(lib, 5, list(u[0]), list(u[1]),
                                 (90., 180.), 1)
    assert npairs[0, 0] == 1
    assert abs(xsum[0, 0] - 179.99) < 1e-7


# ---- 6. rejections ---------------------------------------------------------

def test_count_sky_rejects_bad_arguments(lib):
    edges, nb1 = SKY_BINS['CLUMP', 3]               # 7 bins x 10
    s = sorted_cat('CLUMP1', driver_grid(['CLUMP1'], 60.))
    ncell = tuple(s.ncell)
    # the same catalogue in arrays of its own
    other = SimpleNamespace(**vars(s))
    other.pos, other.w, other.start = (s.pos.clone(), s.w.clone(),
                                       s.start.clone())
    out = Outputs(17, 241)

    def rc(mode=3, edges=edges, nb1=nb1, j0=0, j1=None, nblocks=4,
           ncell=ncell, s2=None, autocorr=None):
        code, _ = call_sky(lib, s, s2, ncell, mode, edges, nb1, nblocks,
                           out=out, j0=j0, j1=j1, autocorr=autocorr,
                           e0sq_mode=3)
        return code

    bad = {
        'mode 2': dict(mode=2),
        'mode 0': dict(mode=0, nb1=1),
        'mode 6': dict(mode=6),
        'mode -1': dict(mode=-1),
        'angular with nb1 = 2': dict(mode=5, nb1=2),
        'j0 == j1': dict(j0=4, j1=4),
        'j0 > j1': dict(j0=5, j1=4),
        'j0 < 0': dict(j0=-1, j1=4),
        'j1 > nb1': dict(j1=11),
        '4097 bins in one pass': dict(edges=EDGES17, nb1=241),
        'nblocks = 0': dict(nblocks=0),
        'ncell with a 0': dict(ncell=(1, 0, 1)),
        'too many cells': dict(ncell=(40961, 1, 1)),
        'autocorr with distinct arrays': dict(s2=other, autocorr=1),
    }
    for name, kw in sorted(bad.items()):
        assert rc(**kw) == NBK_ERR_ARG, name
        assert 'nbk_pairs_count_sky_f64' in last_error(lib), name
    # nothing was launched: the outputs are as they were
    npairs, wsum, xsum = out.arrays()
    assert (npairs == SENTINEL).all()
    assert numpy.isnan(wsum).all() and numpy.isnan(xsum).all()
    # and the same call with good arguments goes through
    assert rc() == 0
    assert rc(s2=other) == 0
    assert rc(mode=4, nb1=30) == 0
    assert rc(mode=5, nb1=1) == 0
