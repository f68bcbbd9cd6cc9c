"""
Kernel-level tests of the pair counter (csrc/nbk_pairs.hip), called
through the C ABI with grids, chunks, block counts and bin slices the
Python driver never picks, and compared with plain numpy
(pairs_reference.py) and the brute-force oracle
(paircount_bruteforce.py) — never with another GPU kernel.

Cell sort: the integers (histogram rows, cursor seeds, cell-start table)
are exact, and every cell's output range holds exactly its multiset of
(x, y, z, w) rows, bit for bit (they are moved, not computed).

Counts, the project's bars (DESIGN.md "Reproducibility"): ``npairs``
equals the oracle exactly and is bitwise equal between two runs; the sum
of weights and the mean separation are within 4 (n_bin + 4) 2^-53
relative, per bin.  Exact counts are fair because every random catalogue
first asserts, on the oracle, that no pair lies within relative 1e-10 of
a squared first-dimension edge nor within absolute 1e-10 of a mu or pi
edge; the lattice cases are exempt, their arithmetic is exact.

Every cell-start table is compared with the reference before a count
kernel reads through it, and every cursor matrix before the scatter
writes through it.
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

import paircount_bruteforce as bf                               # noqa: E402
import pairs_reference as ref                                   # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.algorithms.pair_counters import kernel       # noqa: E402

DEVICE = 'cuda'
NBK_ERR_ARG = -2
EPS = 2.0 ** -53
MARGIN = 1e-10
MODES = {0: '1d', 1: '2d', 2: 'projected'}
SENTINEL = -7


def dev(arr):
    # (a copy: the cached catalogues are read-only arrays)
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


def host(t):
    if DEVICE == 'cuda':
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


# ---- the cell sort ------------------------------------------------------

def chunk_for(n, kind):
    """'one': a single chunk; 'partial': 5 chunks, the last partial;
    'exact': n an exact multiple of the chunk (4 chunks)"""
    if kind == 'one':
        return n + 1000
    if kind == 'partial':
        chunk = n // 5 + 1
        assert -(-n // chunk) == 5 and n % chunk != 0
        return chunk
    assert n % 4 == 0
    return n // 4


def run_cell_sort(lib, pos, w, origin, inv_cell, ncell, chunk):
    """count -> scan -> scatter; the cursors are checked against the
    reference before the scatter writes through them"""
    n = len(pos)
    ncells = int(numpy.prod(ncell))
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
    return SimpleNamespace(n=n, pos=out, w=out_w, start=start, ids=ids,
                           ncells=ncells)


def check_sorted(s, pos, w):
    want_start, want_rows = ref.sorted_reference(pos, w, s.ids, s.ncells)
    assert_array_equal(host(s.start), want_start)
    got_rows = ref.canonical_rows(host(s.pos).reshape(3, s.n).T, host(s.w),
                                  ref.sorted_keys(want_start))
    assert_array_equal(got_rows, want_rows)


def slab_grid(name, rmax=30.):
    lo, hi = ref.bounding_box(name)
    return kernel.make_grid(False, None, rmax, lo, hi)


# name -> (catalogue, (origin, inv_cell, ncell))
def _sort_cases():
    c = {}
    for ncell in [(1, 1, 1), (2, 2, 3), (5, 1, 3)]:
        tag = 'x'.join(str(k) for k in ncell)
        grid = ref.uniform_grid(ref.HBOX, ncell) + (list(ncell),)
        c['H1-' + tag] = ('H1', grid)
        c['clamp-' + tag] = ('clamp', grid)
    c['SLAB-bbox'] = ('SLAB', slab_grid('SLAB'))
    c['clamp-SLAB-bbox'] = ('clamp', slab_grid('SLAB'))
    c['PLANAR-flat-y'] = ('PLANAR', slab_grid('PLANAR'))
    c['clamp-PLANAR-flat-y'] = ('clamp', slab_grid('PLANAR'))
    big = ref.uniform_grid(ref.HBOX, (32, 32, 40)) + ([32, 32, 40],)
    c['BIG-32x32x40'] = ('BIG', big)
    c['clamp-32x32x40'] = ('clamp', big)
    return c


SORT_CASES = _sort_cases()


def sort_input(case):
    cat, (origin, inv_cell, ncell) = SORT_CASES[case]
    if cat == 'clamp':
        pos = ref.clamp_rows(origin, inv_cell, ncell)
        w = ref.weights(len(pos))
    else:
        pos, w = ref.catalogue(cat)
    return pos, w, origin, inv_cell, ncell


@pytest.mark.parametrize('chunks', ['one', 'partial', 'exact'])
@pytest.mark.parametrize('case', sorted(SORT_CASES))
def test_cell_sort(lib, case, chunks):
    pos, w, origin, inv_cell, ncell = sort_input(case)
    if chunks == 'exact':
        keep = len(pos) - len(pos) % 4
        pos, w = pos[:keep], w[:keep]
    if case == 'SLAB-bbox':
        assert list(ncell) == [9, 3, 1]
    if case == 'PLANAR-flat-y':
        assert list(ncell) == [9, 1, 1] and inv_cell[1] == 0.
    if case.endswith('32x32x40'):
        assert int(numpy.prod(ncell)) == 40960      # the documented maximum
    s = run_cell_sort(lib, pos, w, origin, inv_cell, ncell,
                      chunk_for(len(pos), chunks))
    check_sorted(s, pos, w)


def test_cell_sort_rejects_bad_arguments(lib):
    pos, w = ref.catalogue('H1')
    n = len(pos)
    pos_t, w_t = dev(pos), dev(w)
    mat = filled(40961, 0, torch.int32)
    out, out_w = nan_f64(3 * n), nan_f64(n)
    origin, inv = hiplib.f64_arr([0.] * 3), hiplib.f64_arr([1.] * 3)

    def count(ncell, chunk):
        return lib.nbk_pairs_cell_count_f64(
            hiplib.dptr(pos_t), n, chunk, origin, inv,
            hiplib.int_arr(ncell), hiplib.dptr(mat), None)

    def scatter(ncell, chunk):
        return lib.nbk_pairs_cell_scatter_f64(
            hiplib.dptr(pos_t), hiplib.dptr(w_t), n, chunk, origin, inv,
            hiplib.int_arr(ncell), hiplib.dptr(mat), hiplib.dptr(out),
            hiplib.dptr(out_w), None)

    for fn, name in [(count, 'nbk_pairs_cell_count_f64'),
                     (scatter, 'nbk_pairs_cell_scatter_f64')]:
        for ncell, chunk in [([40961, 1, 1], 4096), ([1, 13, 3151], 4096),
                             ([2, 0, 2], 4096), ([2, 2, -1], 4096),
                             ([2, 2, 2], 0)]:
            assert fn(ncell, chunk) == NBK_ERR_ARG, (name, ncell, chunk)
            assert name in last_error(lib)
    # nothing was launched: the outputs are as they were
    assert numpy.isnan(host(out)).all() and numpy.isnan(host(out_w)).all()
    assert (host(mat) == 0).all()


def test_weighted_cell_sort_beside_unweighted_mesh_sorts(lib):
    """One scatter template serves all three keys, its mass pointer
    nullable: in one process the cell sort moves its weights while the
    two mesh sorts run with mass = NULL and leave `mass_out` alone.
    Mesh and grid [8, 8, 8] over HBOX, 3 chunks."""
    import sort_reference as sref
    pos, w = ref.catalogue('H1')
    n = len(pos)
    nmesh = [8, 8, 8]
    chunk = n // 3 + 1
    assert -(-n // chunk) == 3
    grid = ref.uniform_grid(ref.HBOX, nmesh) + (nmesh,)

    def check_cell_sort():
        check_sorted(run_cell_sort(lib, pos, w, *grid, chunk), pos, w)

    def run_mesh_sort(count, scatter, keys, nbuck, extra):
        """count -> scan -> scatter with mass = NULL; returns the number
        of placed rows"""
        nm, bx = hiplib.i64_arr(nmesh), hiplib.f64_arr(ref.HBOX)
        pos_t = dev(pos)
        mat = filled(3 * nbuck, -1, torch.int32)
        tail = (None,) if count is lib.nbk_xsort_count_f64 else ()
        hiplib.check(count(hiplib.dptr(pos_t), n, chunk, nm, bx, *extra,
                           hiplib.dptr(mat), *tail, None), 'count')
        want_mat = sref.chunk_histograms(keys, nbuck, chunk)
        want_bases, want_bb = sref.scan_matrix(want_mat)
        assert_array_equal(host(mat).reshape(3, nbuck), want_mat)
        bases, _ = hiplib.scan_count_matrix(lib, mat, 3, nbuck, None)
        assert_array_equal(host(bases).reshape(3, nbuck), want_bases)
        n_out = int(want_bb[-1])
        out, out_m = nan_f64(3 * n_out), nan_f64(n_out)
        tail = (n_out,) if scatter is lib.nbk_psort_scatter_f64 else ()
        hiplib.check(scatter(hiplib.dptr(pos_t), None, n, chunk, nm, bx,
                             *extra, hiplib.dptr(bases), *tail,
                             hiplib.dptr(out), hiplib.dptr(out_m), None),
                     'scatter')
        assert numpy.isnan(host(out_m)).all()       # NULL mass: untouched
        dup = numpy.concatenate([k[k >= 0] for k in keys])
        rows = numpy.concatenate([pos[k >= 0] for k in keys])
        got_key = numpy.repeat(numpy.arange(nbuck), numpy.diff(want_bb))
        assert_array_equal(
            ref.canonical_rows(host(out).reshape(3, n_out).T, None, got_key),
            ref.canonical_rows(rows, None, dup))
        return n_out

    check_cell_sort()
    ys = 1
    assert run_mesh_sort(
        lib.nbk_xsort_count_f64, lib.nbk_xsort_scatter_f64,
        (sref.coarse_keys(pos, nmesh, ref.HBOX, ys),), 8 * (8 >> ys),
        (ys,)) == n
    gs, dlo, dhi = 2, 0, 1
    assert run_mesh_sort(
        lib.nbk_psort_count_f64, lib.nbk_psort_scatter_f64,
        sref.pair_keys(pos, nmesh, ref.HBOX, gs, dlo, dhi),
        (8 >> 1) * (8 >> gs), (gs, dlo, dhi)) > n
    check_cell_sort()


# ---- the count kernel ---------------------------------------------------

_sorted = {}


def sorted_cat(name, grid_key, grid):
    """device-resident cell-sorted catalogue, built once per (catalogue,
    grid) and checked against the reference"""
    key = (name, grid_key)
    if key not in _sorted:
        lib = hiplib.require()
        origin, inv_cell, ncell = grid
        pos, w = ref.catalogue(name)
        s = run_cell_sort(lib, pos, w, origin, inv_cell, ncell,
                          chunk_for(len(pos), 'partial'))
        check_sorted(s, pos, w)
        s.ncell = [int(k) for k in ncell]
        _sorted[key] = s
    return _sorted[key]


def periodic_sorted(name, box, ncell):
    grid = ref.uniform_grid(box, ncell) + (list(ncell),)
    return sorted_cat(name, ('periodic', tuple(box), tuple(ncell)), grid)


def second_edges(mode, nb1):
    """nb1 = Nmu (mode 1) or pimax (mode 2)"""
    if mode == 1:
        return bf.second_edges('2d', Nmu=nb1)
    if mode == 2:
        return bf.second_edges('projected', pimax=nb1)
    return None


@functools.lru_cache(maxsize=None)
def oracle(first, second, mode, edges, nb1, box, periodic):
    """The brute-force result of a case: computed once, shared."""
    pos1, w1 = ref.catalogue(first)
    pos2 = w2 = None
    if second is not None:
        pos2, w2 = ref.catalogue(second)
    kw = {1: dict(Nmu=nb1), 2: dict(pimax=nb1)}.get(mode, {})
    # (edges[0] = 0 has no relative margin: 0/0 in the margin itself)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        want = bf.bruteforce_paircount(
            MODES[mode], pos1, numpy.array(edges), numpy.array(box), w1=w1,
            pos2=pos2, w2=w2, periodic=periodic, los=2, **kw)
    for v in want.values():
        if isinstance(v, numpy.ndarray):
            v.setflags(write=False)
    return want


def check_margins(want):
    """exact npairs is only fair when no pair sits on a bin edge"""
    print('npairs total %d, margins %.3g %.3g'
          % (want['npairs'].sum(), want['margin0'], want['margin1']))
    assert want['margin0'] > MARGIN
    assert want['margin1'] > MARGIN
    assert want['n_mu1'] == 0


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


def call_count(lib, s1, s2, ncell, box, periodic, mode, edges, nb1, nblocks,
               out=None, j0=0, j1=None, autocorr=None):
    """one nbk_pairs_count_f64 call; ``s2 is None`` is the
    auto-correlation.  ``partials`` starts as NaN."""
    edges = numpy.asarray(edges, dtype='f8')
    nb0 = len(edges) - 1
    j1 = nb1 if j1 is None else j1
    auto = s2 is None
    if auto:
        s2 = s1
    out = Outputs(nb0, nb1) if out is None else out
    e0sq = dev(edges * edges)
    e1 = second_edges(mode, nb1)
    e1_t = None if e1 is None else dev(e1)
    partials = nan_f64(3 * max(nblocks, 1) * nb0 * max(j1 - j0, 1))
    rc = lib.nbk_pairs_count_f64(
        hiplib.dptr(s1.pos), hiplib.dptr(s1.w), hiplib.dptr(s1.start), s1.n,
        hiplib.dptr(s2.pos), hiplib.dptr(s2.w), hiplib.dptr(s2.start), s2.n,
        int(auto) if autocorr is None else autocorr,
        hiplib.int_arr(ncell), hiplib.f64_arr(box), int(periodic), mode,
        hiplib.dptr(e0sq), nb0, hiplib.dptr(e1_t), nb1, j0, j1, nblocks,
        hiplib.dptr(partials), hiplib.dptr(out.npairs),
        hiplib.dptr(out.wsum), hiplib.dptr(out.xsum), None)
    if DEVICE == 'cuda':
        torch.cuda.synchronize()
    return rc, out


def check_counts(got, want, columns=slice(None)):
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
    for g, r in [(wsum, ww), (mean, wm)]:
        err = numpy.abs(g - r)
        print('max err / bound: %.3g'
              % (err / (rtol * numpy.abs(r) + 1e-300)).max())
        assert (err <= rtol * numpy.abs(r)).all()


def count_and_check(lib, s1, s2, ncell, box, periodic, mode, edges, nb1,
                    nblocks, want):
    rc, out = call_count(lib, s1, s2, ncell, box, periodic, mode, edges,
                         nb1, nblocks)
    assert rc == 0, last_error(lib)
    got = out.arrays()
    check_counts(got, want)
    # bitwise reproducible integer counts
    rc, again = call_count(lib, s1, s2, ncell, box, periodic, mode, edges,
                           nb1, nblocks)
    assert rc == 0
    assert_array_equal(again.arrays()[0], got[0])
    return got


# mode -> (first-dimension edges, nb1) of the H cases
H_BINS = {0: (tuple(numpy.linspace(0.5, 18, 8)), 1),
          1: (tuple(numpy.linspace(0.5, 18, 8)), 10),
          2: (tuple(numpy.linspace(0.5, 14, 7)), 12)}


# ---- 1. the same pairs on any grid and any work split --------------------

@pytest.mark.parametrize('nblocks', [1, 3, 300])
@pytest.mark.parametrize('ncell', [(1, 1, 1), (2, 2, 3), (1, 2, 3)])
@pytest.mark.parametrize('second', [None, 'H2'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_count_any_grid_any_split(lib, mode, second, ncell, nblocks):
    """H1 (1300) auto and H1 x H2 (700) in the periodic box (40, 50, 64).
    (1, 1, 1) is one cell of 1300: every loop runs several trips and
    every axis aliases cell 0 under three shifts; (2, 2, 3) with one
    block has split = 1; (1, 1, 1) with 300 blocks has split = 64 and
    more blocks than its 64 work items, so blocks that store all-zero
    partials."""
    edges, nb1 = H_BINS[mode]
    want = oracle('H1', second, mode, edges, nb1, ref.HBOX, True)
    check_margins(want)
    s1 = periodic_sorted('H1', ref.HBOX, ncell)
    s2 = None if second is None else periodic_sorted(second, ref.HBOX,
                                                     ncell)
    count_and_check(lib, s1, s2, ncell, ref.HBOX, True, mode, edges, nb1,
                    nblocks, want)


# ---- 2./3. anisotropic non-periodic grids, offset origin, flat axis ------

# mode -> (edges, nb1, rmax of the grid)
SLAB_BINS = {0: (tuple(numpy.linspace(1, 30, 8)), 1, 30.),
             1: (tuple(numpy.linspace(1, 30, 8)), 6, 30.),
             2: (tuple(numpy.linspace(1, 22, 8)), 20,
                 kernel.max_3d_separation('projected', [22.], 20))}


def slab_sorted(name, mode, bbox_of):
    rmax = SLAB_BINS[mode][2]
    grid = slab_grid(bbox_of, rmax)
    return sorted_cat(name, ('bbox', bbox_of, rmax), grid)


@pytest.mark.parametrize('pair', ['auto', 'halves'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_count_slab_nonperiodic(lib, mode, pair):
    """SLAB: a 300 x 120 x 35 sheet at (-50, 7, 1000) plus a blob of 600
    in one or two cells; box = 0, periodic = 0, the driver's grid on its
    bounding box.  The extents 298.8 x 119.8 x 34.8 give floor(extent /
    rmax) = (9, 3, 1) cells for rmax = 30 and (10, 4, 1) for the
    projected reach sqrt(22^2 + 20^2) = 29.73.  'halves' counts the even
    rows against the odd rows on the same grid: those pairs are a subset
    of the auto-correlation's, whose margins therefore hold for it."""
    edges, nb1, rmax = SLAB_BINS[mode]
    auto = oracle('SLAB', None, mode, edges, nb1, (0., 0., 0.), False)
    check_margins(auto)
    s = slab_sorted('SLAB', mode, 'SLAB')
    ncell = s.ncell
    assert ncell == ([10, 4, 1] if mode == 2 else [9, 3, 1])
    assert ncell[2] == 1 and len(set(ncell)) == 3
    assert numpy.diff(host(s.start)).max() > 256
    if pair == 'auto':
        s1, s2, want = s, None, auto
    else:
        s1 = slab_sorted('SLAB_EVEN', mode, 'SLAB')
        s2 = slab_sorted('SLAB_ODD', mode, 'SLAB')
        want = oracle('SLAB_EVEN', 'SLAB_ODD', mode, edges, nb1,
                      (0., 0., 0.), False)
        assert want['n_mu1'] == 0
    count_and_check(lib, s1, s2, ncell, [0., 0., 0.], False, mode, edges,
                    nb1, 7, want)


@pytest.mark.parametrize('mode', [0, 2])
def test_count_planar_zero_extent(lib, mode):
    """PLANAR = SLAB with y = 3.25: one cell with inv_cell = 0 on the
    flat axis.  In a plane that contains the line of sight mu crowds
    against 1 and the (r, mu) margin is 5.8e-11, below the 1e-10 bar, so
    mode 1 is left out rather than the bar lowered."""
    edges, nb1, rmax = SLAB_BINS[mode]
    want = oracle('PLANAR', None, mode, edges, nb1, (0., 0., 0.), False)
    check_margins(want)
    s = slab_sorted('PLANAR', mode, 'PLANAR')
    assert s.ncell == ([10, 1, 1] if mode == 2 else [9, 1, 1])
    count_and_check(lib, s, None, s.ncell, [0., 0., 0.], False, mode, edges,
                    nb1, 5, want)


# ---- 4./5. the lattice: pairs on edges, mu = 1, zero separation ----------

LAT_EDGES = (0., 1., 2., 3., 5., 6., 7.)
LAT_NB1 = {0: 1, 1: 5, 2: 4}


@pytest.mark.parametrize('ncell', [(2, 2, 2), (1, 2, 2)])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_count_lattice_on_edges(lib, mode, ncell):
    """The 10 x 9 x 8 integer lattice in the periodic box (20, 18, 16):
    exact arithmetic, many pairs exactly on r and pi edges (q = 49 on
    the open top edge is dropped), mu = 3/5 one ulp below linspace's
    0.6000000000000001, and 4860 pairs at mu = 1 closing the last bin."""
    nb1 = LAT_NB1[mode]
    want = oracle('LAT', None, mode, LAT_EDGES, nb1, ref.LATBOX, True)
    if mode == 1:
        assert want['n_mu1'] == 4860
        assert bf.second_edges('2d', Nmu=5)[3] > 3. / 5
    s = periodic_sorted('LAT', ref.LATBOX, ncell)
    count_and_check(lib, s, None, ncell, ref.LATBOX, True, mode, LAT_EDGES,
                    nb1, 6, want)


def run_slices(lib, s1, s2, ncell, box, mode, edges, nb1, nblocks, slices,
               want):
    """count the second-dimension slices [j0, j1) one call each, in the
    order given; after every call the columns not yet counted still hold
    the sentinel and the counted ones the oracle's values"""
    out = Outputs(len(edges) - 1, nb1)
    done = numpy.zeros(nb1, dtype=bool)
    for j0, j1 in slices:
        rc, _ = call_count(lib, s1, s2, ncell, box, True, mode, edges, nb1,
                           nblocks, out=out, j0=j0, j1=j1)
        assert rc == 0, last_error(lib)
        done[j0:j1] = True
        npairs, wsum, xsum = out.arrays()
        assert (npairs[:, ~done] == SENTINEL).all()
        assert numpy.isnan(wsum[:, ~done]).all()
        assert numpy.isnan(xsum[:, ~done]).all()
        check_counts((npairs, wsum, xsum), want, columns=done)
    assert done.all()


@pytest.mark.parametrize('case', ['cross-copy', 'duplicated-rows'])
@pytest.mark.parametrize('mode,passes', [(0, 'single'), (1, 'single'),
                                         (1, 'sliced'), (2, 'single'),
                                         (2, 'sliced')])
def test_count_zero_separation(lib, mode, passes, case):
    """Pairs at r = 0 with edges[0] = 0: LAT x a copy of LAT
    (autocorr = 0, 720 coincident pairs) and LATDUP auto (40 rows
    doubled, 80 coincident pairs).  Modes 0 and 2 count them in their
    first bin (q = 0 >= 0, pi = 0); in mode 1 mu = 0/0 has no bin and
    the pair is dropped — in every pass, however the bins are sliced."""
    nb1 = LAT_NB1[mode]
    ncell = (2, 2, 2)
    if case == 'cross-copy':
        first, second = 'LAT', 'LAT'
        s1 = periodic_sorted('LAT', ref.LATBOX, ncell)
        # sorted again into arrays of its own
        s2 = sorted_cat('LAT', 'copy', ref.uniform_grid(ref.LATBOX, ncell)
                        + (list(ncell),))
        assert s2.pos.data_ptr() != s1.pos.data_ptr()
    else:
        first, second = 'LATDUP', None
        s1, s2 = periodic_sorted('LATDUP', ref.LATBOX, ncell), None
    want = oracle(first, second, mode, LAT_EDGES, nb1, ref.LATBOX, True)
    base = oracle('LAT', None, mode, LAT_EDGES, nb1, ref.LATBOX, True)
    if case == 'cross-copy':
        extra = int(want['npairs'].sum()) - int(base['npairs'].sum())
        assert extra == (0 if mode == 1 else 720)
    else:
        assert want['npairs'].sum() == (376424 if mode == 1 else
                                        {0: 376504, 2: 304280}[mode])
    if passes == 'single':
        count_and_check(lib, s1, s2, ncell, ref.LATBOX, True, mode,
                        LAT_EDGES, nb1, 6, want)
    else:
        slices = [(3, nb1), (0, 1), (1, 3)]
        run_slices(lib, s1, s2, ncell, ref.LATBOX, mode, LAT_EDGES, nb1, 6,
                   slices, want)


# ---- 6. histogram copies and slices --------------------------------------

EDGES8 = tuple(numpy.linspace(0.5, 18, 9))


@pytest.mark.parametrize('passes', ['single', 'sliced'])
@pytest.mark.parametrize('nb1', [10, 100, 200, 512])
def test_count_copies_and_slices(lib, nb1, passes):
    """H1 auto in (r, mu) with 8 r bins and Nmu = 10, 100, 200, 512:
    80, 800, 1600 and 4096 bins in one pass, so 4, 2, 1 and 1 histogram
    copies, the last exactly the capacity.  'sliced' runs three slices
    of unequal width (1/5, 1/2 and the rest of the mu bins) in a
    scrambled order; the narrower histograms take as many copies as
    their own bin count allows.  Seed 11 passes the edge precondition
    for every Nmu: mu margins 4.2e-7, 3.7e-8, 3.7e-8, 2.1e-9 (r^2:
    3.7e-7)."""
    assert 8 * 512 == lib.nbk_pairs_max_bins()
    want = oracle('H1', None, 1, EDGES8, nb1, ref.HBOX, True)
    check_margins(want)
    ncell = (2, 2, 3)
    s = periodic_sorted('H1', ref.HBOX, ncell)
    if passes == 'single':
        count_and_check(lib, s, None, ncell, ref.HBOX, True, 1, EDGES8,
                        nb1, 8, want)
    else:
        a, b = nb1 // 5, nb1 // 5 + nb1 // 2
        run_slices(lib, s, None, ncell, ref.HBOX, 1, EDGES8, nb1, 8,
                   [(b, nb1), (0, a), (a, b)], want)


# ---- 7. empty sides -------------------------------------------------------

def empty_sorted(ncell):
    ncells = int(numpy.prod(ncell))
    return SimpleNamespace(
        n=0, pos=None, w=None,
        start=filled(ncells + 1, 0, torch.int32), ncells=ncells)


@pytest.mark.parametrize('empty', ['first', 'second', 'both', 'auto'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_count_empty_sides(lib, mode, empty):
    """n1 = 0, n2 = 0 or both: NBK_OK, and the outputs are written as
    zeros, not left at the sentinel"""
    edges, nb1 = H_BINS[mode]
    ncell = (2, 2, 3)
    full = periodic_sorted('H1', ref.HBOX, ncell)
    s1 = full if empty == 'second' else empty_sorted(ncell)
    s2 = full if empty == 'first' else empty_sorted(ncell)
    if empty == 'auto':
        s2 = None
    rc, out = call_count(lib, s1, s2, ncell, ref.HBOX, True, mode, edges,
                         nb1, 5)
    assert rc == 0, last_error(lib)
    npairs, wsum, xsum = out.arrays()
    assert (npairs == 0).all() and (wsum == 0).all() and (xsum == 0).all()


# ---- 8. rejections --------------------------------------------------------

def test_count_rejects_bad_arguments(lib):
    ncell = (2, 2, 3)
    s = periodic_sorted('H1', ref.HBOX, ncell)
    # the same catalogue in arrays of its own
    other = SimpleNamespace(**vars(s))
    other.pos, other.w, other.start = (s.pos.clone(), s.w.clone(),
                                       s.start.clone())
    edges = H_BINS[1][0]                    # 7 bins
    edges17 = tuple(numpy.linspace(0.5, 18, 18))    # 17 bins
    out = Outputs(17, 241)

    def rc(mode=1, edges=edges, nb1=10, j0=0, j1=None, nblocks=4,
           ncell=ncell, s2=None, autocorr=None):
        code, _ = call_count(lib, s, s2, ncell, ref.HBOX, True, mode, edges,
                             nb1, nblocks, out=out, j0=j0, j1=j1,
                             autocorr=autocorr)
        return code

    bad = {
        'mode 3': dict(mode=3),
        'mode -1': dict(mode=-1),
        '1d with nb1 = 2': dict(mode=0, nb1=2),
        'j0 == j1': dict(j0=4, j1=4),
        'j0 > j1': dict(j0=5, j1=4),
        'j0 < 0': dict(j0=-1, j1=4),
        'j1 > nb1': dict(j1=11),
        '4097 bins in one pass': dict(edges=edges17, nb1=241),
        'nblocks = 0': dict(nblocks=0),
        'ncell with a 0': dict(ncell=(2, 0, 3)),
        'too many cells': dict(ncell=(40961, 1, 1)),
        'autocorr with distinct arrays': dict(s2=other, autocorr=1),
    }
    assert 17 * 241 == 4097
    for name, kw in sorted(bad.items()):
        assert rc(**kw) == NBK_ERR_ARG, name
        assert 'nbk_pairs_count_f64' in last_error(lib), name
    # nothing was launched: the outputs are as they were
    npairs, wsum, xsum = out.arrays()
    assert (npairs == SENTINEL).all()
    assert numpy.isnan(wsum).all() and numpy.isnan(xsum).all()
    # and the same call with good arguments goes through
    assert rc() == 0
    assert rc(s2=other) == 0
