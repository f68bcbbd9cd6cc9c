"""
Kernel-level tests of the 3PCF (csrc/nbk_3pcf.hip), called through the C
ABI with grids, block counts, multipoles and bin counts the Python driver
never picks, and compared only with the numpy restatement of
threeptcf_reference.py — never with another GPU kernel.

The bar: |zeta_l(b1, b2) - reference| <= 1e-10 sqrt(zeta_l(b1, b1)
zeta_l(b2, b2)), the Cauchy-Schwarz scale (valid for positive weights).
The sums have fewer than 10^3 terms and the recurrence fewer than 10^2
roundings, so reordering costs about 1e-13, while one mis-binned pair
moves an entry by >~ 1e-3 of the scale.  Entries whose scale is 0 must be
exactly 0.  That is fair because every random catalogue (weights in
[0.5, 1.5]) first asserts, on the host, that no pair lies within relative
1e-10 of an edge.  Outputs and scratch start as NaN.
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

import pairs_reference as pref                                  # noqa: E402
import threeptcf_reference as ref                               # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.algorithms.pair_counters import kernel       # noqa: E402

NBK_ERR_ARG = -2
RTOL = 1e-10
MARGIN = 1e-10

CUBE = (96., 96., 96.)
SLAB = (128., 99., 165.)
EDGES3 = (0., 10., 20., 30.)


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """name -> (pos, w), read-only"""
    if name == 'cube':              # 300 in the periodic cube
        rng = numpy.random.RandomState(101)
        pos = rng.uniform(size=(300, 3)) * CUBE
    elif name == 'slab':            # 300 in the non-cubic periodic box
        rng = numpy.random.RandomState(102)
        pos = rng.uniform(size=(300, 3)) * SLAB
    elif name == 'clusters':        # two blobs 200 apart: empty cells
        rng = numpy.random.RandomState(103)
        pos = rng.uniform(size=(300, 3)) * 40.
        pos[150:, 0] += 200.
    elif name == 'dense':           # 700 in one cell
        rng = numpy.random.RandomState(104)
        pos = rng.uniform(size=(700, 3)) * 20.
    elif name == 'few':             # 64 for the widest binning
        rng = numpy.random.RandomState(105)
        pos = rng.uniform(size=(64, 3)) * 100.
    elif name == 'dup':             # 120 rows, the first 40 once more
        rng = numpy.random.RandomState(106)
        pos = rng.uniform(size=(120, 3)) * CUBE
        pos = numpy.concatenate([pos, pos[:40]])
    elif name == 'one':
        rng = numpy.random.RandomState(107)
        pos = rng.uniform(size=(1, 3)) * CUBE
    else:
        raise KeyError(name)
    w = numpy.random.RandomState(len(pos)).uniform(0.5, 1.5, size=len(pos))
    pos.setflags(write=False)
    w.setflags(write=False)
    return pos, w


@functools.lru_cache(maxsize=None)
def reference(name, edges, lmax, box):
    """The restatement's zeta of a case, computed once and shared; the
    edge precondition is asserted with it"""
    pos, w = catalogue(name)
    margin = ref.edge_margin(pos, box, numpy.array(edges))
    print('%s: edge margin %.3g' % (name, margin))
    assert margin > MARGIN
    want = ref.alm_zeta(pos, w, numpy.array(edges), lmax, box=box)
    want.setflags(write=False)
    return want


def dev(arr):
    return torch.as_tensor(numpy.array(arr, order='C')).to('cuda')


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def nan_f64(n):
    return torch.full((int(n),), float('nan'), dtype=torch.float64,
                      device='cuda')


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


_sorted = {}


def sorted_cat(name, grid_key, grid):
    """device-resident cell-sorted catalogue, its cell-start table checked
    against the host's cell ids before a kernel reads through it"""
    key = (name, grid_key)
    if key not in _sorted:
        lib = hiplib.require()
        origin, inv_cell, ncell = grid
        pos, w = catalogue(name)
        spos, sw, start = kernel.cell_sort(lib, dev(pos), dev(w), origin,
                                           inv_cell, ncell)
        ncells = int(numpy.prod(ncell))
        ids = pref.cell_ids(pos, origin, inv_cell, ncell)
        want_start = numpy.concatenate(
            [[0], numpy.cumsum(numpy.bincount(ids, minlength=ncells))])
        assert_array_equal(host(start), want_start)
        _sorted[key] = SimpleNamespace(
            n=len(pos), pos=spos, w=sw, start=start,
            ncell=[int(k) for k in ncell], occupancy=numpy.diff(want_start))
    return _sorted[key]


def periodic_sorted(name, box, ncell):
    grid = pref.uniform_grid(box, ncell) + (list(ncell),)
    return sorted_cat(name, ('periodic', tuple(box), tuple(ncell)), grid)


def bbox_sorted(name, rmax):
    pos, _ = catalogue(name)
    grid = kernel.make_grid(False, None, rmax, pos.min(axis=0),
                            pos.max(axis=0))
    return sorted_cat(name, ('bbox', rmax), grid)


def call_zeta(lib, s, box, periodic, edges, lmax, nblocks):
    """one nbk_3pcf_zeta_f64 call; scratch and output start as NaN"""
    edges = numpy.asarray(edges, dtype='f8')
    nbins = len(edges) - 1
    esq = dev(edges * edges)
    nl = max(lmax, 0) + 1           # (lmax = -1 is a rejection case)
    nent = nl * nbins * (nbins + 1) // 2
    partials = nan_f64(max(nblocks, 1) * nent)
    zeta = nan_f64(nl * nbins * nbins)
    rc = lib.nbk_3pcf_zeta_f64(
        hiplib.dptr(s.pos), hiplib.dptr(s.w), hiplib.dptr(s.start), s.n,
        hiplib.int_arr(s.ncell), hiplib.f64_arr(box), int(periodic),
        hiplib.dptr(esq), nbins, lmax, nblocks, hiplib.dptr(partials),
        hiplib.dptr(zeta), None)
    return rc, host(zeta).reshape(nl, nbins, nbins), host(partials)


def run_and_check(lib, s, box, periodic, edges, lmax, nblocks, want):
    rc, got, _ = call_zeta(lib, s, box, periodic, edges, lmax, nblocks)
    assert rc == 0, lib.nbk_last_error_string().decode()
    assert numpy.isfinite(got).all()
    assert numpy.abs(want).max() > 0
    ref.assert_zeta_close(got, want, RTOL)
    # symmetric by construction (one triangle is computed)
    assert_array_equal(got, got.transpose(0, 2, 1))
    return got


# ---- any grid, any work split ---------------------------------------------

@pytest.mark.parametrize('ncell', [(1, 1, 1), (2, 2, 2), (3, 3, 3)])
def test_periodic_cube_any_grid(lib, ncell):
    """300 points, lmax = 10, 3 bins: (1, 1, 1) aliases cell 0 under three
    shifts per axis and holds more than one tile; (2, 2, 2) aliases -1 and
    +1; (3, 3, 3) has cells exactly 32 >= rmax = 30 wide"""
    want = reference('cube', EDGES3, 10, CUBE)
    s = periodic_sorted('cube', CUBE, ncell)
    run_and_check(lib, s, CUBE, True, EDGES3, 10, 7, want)


def test_periodic_non_cubic_box(lib):
    """box (128, 99, 165) on a (4, 3, 5) grid"""
    want = reference('slab', EDGES3, 10, SLAB)
    s = periodic_sorted('slab', SLAB, (4, 3, 5))
    run_and_check(lib, s, SLAB, True, EDGES3, 10, 7, want)


def test_non_periodic_with_empty_cells(lib):
    """two blobs 200 apart on the bounding-box grid: the cells between
    them are empty, and box is not read"""
    want = reference('clusters', EDGES3, 10, None)
    s = bbox_sorted('clusters', 30.)
    assert (s.occupancy == 0).any() and len(s.occupancy) > 1
    run_and_check(lib, s, [0., 0., 0.], False, EDGES3, 10, 5, want)


def test_many_primaries_in_one_cell(lib):
    """700 points in one non-periodic cell: three tiles, and 175 trips of
    four primaries for a block"""
    edges = (0., 4., 8., 12.)
    want = reference('dense', edges, 10, None)
    s = bbox_sorted('dense', 12.)
    assert s.ncell == [1, 1, 1]
    run_and_check(lib, s, [0., 0., 0.], False, edges, 10, 3, want)


@pytest.mark.parametrize('nblocks', [1, 3, 40])
def test_any_block_count(lib, nblocks):
    """27 cells: one block takes them all (split 1), 3 blocks split 1,
    40 blocks are more than the cells (split 6, 162 work items)"""
    want = reference('cube', EDGES3, 10, CUBE)
    s = periodic_sorted('cube', CUBE, (3, 3, 3))
    run_and_check(lib, s, CUBE, True, EDGES3, 10, nblocks, want)


def test_more_blocks_than_work_items(lib):
    """one cell of 300, 500 blocks: 64 work items, idle blocks store zero
    partials"""
    want = reference('cube', EDGES3, 10, CUBE)
    s = periodic_sorted('cube', CUBE, (1, 1, 1))
    run_and_check(lib, s, CUBE, True, EDGES3, 10, 500, want)


# ---- multipoles and bins ---------------------------------------------------

@pytest.mark.parametrize('lmax', [0, 1, 15])
def test_lmax(lib, lmax):
    assert lib.nbk_3pcf_max_ell() == 15
    want = reference('cube', EDGES3, lmax, CUBE)
    s = periodic_sorted('cube', CUBE, (2, 2, 2))
    got = run_and_check(lib, s, CUBE, True, EDGES3, lmax, 7, want)
    assert got.shape == (lmax + 1, 3, 3)


def test_one_bin(lib):
    edges = (0., 30.)
    want = reference('cube', edges, 10, CUBE)
    s = periodic_sorted('cube', CUBE, (2, 2, 2))
    run_and_check(lib, s, CUBE, True, edges, 10, 7, want)


def test_bins_at_capacity(lib):
    """nbk_3pcf_max_bins(10) bins (one wave per block) with 64 points"""
    cap = lib.nbk_3pcf_max_bins(10)
    assert cap >= 20
    assert lib.nbk_3pcf_max_bins(15) < cap < lib.nbk_3pcf_max_bins(0)
    assert lib.nbk_3pcf_max_bins(16) == 0 and lib.nbk_3pcf_max_bins(-1) == 0
    box = (100., 100., 100.)
    edges = tuple(numpy.linspace(0., 50., cap + 1))
    want = reference('few', edges, 10, box)
    s = periodic_sorted('few', box, (1, 1, 1))
    run_and_check(lib, s, box, True, edges, 10, 4, want)


def test_twenty_bins_at_lmax_10(lib):
    box = (100., 100., 100.)
    edges = tuple(numpy.linspace(0., 50., 21))
    want = reference('few', edges, 10, box)
    s = periodic_sorted('few', box, (2, 2, 2))
    run_and_check(lib, s, box, True, edges, 10, 4, want)


def test_above_capacity_is_rejected(lib):
    s = periodic_sorted('cube', CUBE, (2, 2, 2))
    cap = lib.nbk_3pcf_max_bins(10)
    bad = {
        'one bin too many': (tuple(numpy.linspace(0., 30., cap + 2)), 10, 4),
        'one l too many': (EDGES3, 16, 4),
        'negative l': (EDGES3, -1, 4),
        'nblocks = 0': (EDGES3, 10, 0),
    }
    for name, (edges, lmax, nblocks) in sorted(bad.items()):
        rc, zeta, partials = call_zeta(lib, s, CUBE, True, edges, lmax,
                                       nblocks)
        assert rc == NBK_ERR_ARG, name
        assert 'nbk_3pcf_zeta_f64' in lib.nbk_last_error_string().decode()
        # nothing was launched: outputs and scratch are as they were
        assert numpy.isnan(zeta).all(), name
        assert numpy.isnan(partials).all(), name
    s.ncell = [2, 0, 2]
    try:
        rc, zeta, _ = call_zeta(lib, s, CUBE, True, EDGES3, 10, 4)
    finally:
        s.ncell = [2, 2, 2]
    assert rc == NBK_ERR_ARG and numpy.isnan(zeta).all()
    # and the same call with good arguments goes through
    rc, zeta, _ = call_zeta(lib, s, CUBE, True, EDGES3, 10, 4)
    assert rc == 0 and numpy.isfinite(zeta).all()


# ---- empty, single, excluded ------------------------------------------------

@pytest.mark.parametrize('n', [0, 1])
def test_no_pairs_gives_zeros(lib, n):
    """n = 0 and n = 1: NBK_OK, the output written as zeros, not left NaN"""
    ncell = (2, 2, 2)
    if n == 0:
        s = SimpleNamespace(
            n=0, pos=None, w=None, ncell=list(ncell),
            start=torch.zeros(9, dtype=torch.int32, device='cuda'))
    else:
        s = periodic_sorted('one', CUBE, ncell)
    rc, zeta, _ = call_zeta(lib, s, CUBE, True, EDGES3, 10, 4)
    assert rc == 0, lib.nbk_last_error_string().decode()
    assert (zeta == 0).all()


def test_pairs_below_the_first_edge(lib):
    """edges[0] = 12 > 0: the pairs closer than that are in no bin"""
    edges = (12., 20., 30.)
    pos, _ = catalogue('cube')
    close = 0
    for i in range(len(pos)):
        _, q = ref.separations(pos, i, CUBE)
        close += int(((q > 0) & (q <= 144.)).sum())
    assert close > 100
    want = reference('cube', edges, 10, CUBE)
    s = periodic_sorted('cube', CUBE, (2, 2, 2))
    run_and_check(lib, s, CUBE, True, edges, 10, 7, want)


def test_duplicated_points_are_dropped(lib):
    """40 rows twice, edges[0] = 0: a duplicate is at r = 0 of its twin and
    in no bin of it, but still a primary and a secondary of all others"""
    want = reference('dup', EDGES3, 10, CUBE)
    s = periodic_sorted('dup', CUBE, (2, 2, 2))
    run_and_check(lib, s, CUBE, True, EDGES3, 10, 7, want)


# ---- reproducibility --------------------------------------------------------

def test_two_launches_are_bitwise_equal(lib):
    s = periodic_sorted('cube', CUBE, (3, 3, 3))
    rc1, first, p1 = call_zeta(lib, s, CUBE, True, EDGES3, 10, 11)
    rc2, again, p2 = call_zeta(lib, s, CUBE, True, EDGES3, 10, 11)
    assert rc1 == 0 and rc2 == 0
    assert_array_equal(first.view('u8'), again.view('u8'))
    assert_array_equal(p1.view('u8'), p2.view('u8'))
