"""
Kernel-level tests of the FOF kernels (csrc/nbk_fof.hip), called through
the C ABI with grids and chunks the Python driver never picks, and
compared with plain numpy (fof_reference.py) — never with another GPU
kernel.

Two-level sort: the integers (histogram rows, cursor seeds, coarse and
fine start tables) are exact, and every fine cell's output range holds
exactly its multiset of (x, y, z, index) rows, bit for bit.  Every start
table and cursor matrix is compared with the reference BEFORE a later
kernel reads through it.

Link and flatten: ``minid`` equals the brute force exactly and is equal
between two runs.  Exact equality is fair because every random input
first asserts, on the reference, that no pair lies within relative 1e-10
of ll^2; the lattices are exempt (their pairs at exactly ll do not
decide connectivity).
"""
from types import SimpleNamespace

import numpy
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import fof_reference as ref                                     # noqa: E402
import pairs_reference as pref                                  # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402

DEVICE = 'cuda'
NBK_ERR_ARG = -2
SENTINEL = -7
BOX3 = [ref.BOX] * 3


def dev(arr):
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def filled(n, value, dtype):
    return torch.full((int(n),), value, dtype=dtype, device=DEVICE)


def nan_f64(n):
    return filled(n, float('nan'), torch.float64)


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def last_error(lib):
    return lib.nbk_last_error_string().decode()


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


# ---- the two-level sort ------------------------------------------------------

def two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, chunk):
    """count -> scan -> scatter -> fine pass, every table checked against
    the reference before the next kernel reads through it; returns the
    checked sorted layout"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    n = len(pos)
    ncoarse_all = int(numpy.prod(ncoarse))
    nfine = int(numpy.prod(fine))
    ncells = ncoarse_all * nfine
    grid = (hiplib.f64_arr(origin), hiplib.f64_arr(inv_cell),
            hiplib.int_arr(ncoarse), hiplib.int_arr(fine))
    index = numpy.arange(n, dtype='f8')
    ids = ref.cell_ids(pos, origin, inv_cell, ncoarse, fine)
    cids = ref.coarse_ids(pos, origin, inv_cell, ncoarse, fine)
    want_cstart = numpy.concatenate(
        [[0], numpy.cumsum(numpy.bincount(cids, minlength=ncoarse_all))])

    pos_t, index_t = dev(pos), dev(index)
    cpos, cindex = nan_f64(3 * n), nan_f64(n)
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
        want_mat = pref.chunk_histograms(cids, ncoarse_all, chunk)
        want_bases, want_edges = pref.scan_matrix(want_mat)
        assert_array_equal(host(mat).reshape(nchunks, ncoarse_all), want_mat)
        assert_array_equal(host(bases).reshape(nchunks, ncoarse_all),
                           want_bases)
        assert_array_equal(want_edges, want_cstart)
        assert_array_equal(host(cstart), want_cstart)
        hiplib.check(lib.nbk_fof_cell_scatter_f64(
            hiplib.dptr(pos_t), hiplib.dptr(index_t), n, chunk, *grid,
            hiplib.dptr(bases), hiplib.dptr(cpos), hiplib.dptr(cindex),
            None), 'fof_cell_scatter')
        # the coarse-sorted rows, before the fine pass reads them
        got = pref.canonical_rows(host(cpos).reshape(3, n).T, host(cindex),
                                  ref.sorted_keys(want_cstart))
        assert_array_equal(got, pref.canonical_rows(pos, index, cids))

    spos = nan_f64(3 * n)
    sindex = filled(n, SENTINEL, torch.int32)
    fstart = filled(ncells + 1, SENTINEL, torch.int32)
    hiplib.check(lib.nbk_fof_fine_sort_f64(
        hiplib.dptr(cpos), hiplib.dptr(cindex), n, *grid,
        hiplib.dptr(cstart), hiplib.dptr(spos), hiplib.dptr(sindex),
        hiplib.dptr(fstart), None), 'fof_fine_sort')
    want_start, want_rows = ref.sorted_reference(pos, index, ids, ncells)
    assert_array_equal(host(fstart), want_start)
    got_index = host(sindex)
    got_rows = pref.canonical_rows(host(spos).reshape(3, n).T,
                                   got_index.astype('f8'),
                                   ref.sorted_keys(want_start))
    assert_array_equal(got_rows, want_rows)
    assert_array_equal(numpy.sort(got_index), numpy.arange(n))
    return SimpleNamespace(n=n, pos=spos, index=sindex, start=fstart,
                           ncoarse=list(ncoarse), fine=list(fine))


SORT_GRIDS = [((3, 2, 2), (4, 4, 4)), ((1, 1, 1), (1, 1, 1)),
              ((5, 5, 5), (1, 1, 1)), ((2, 3, 1), (7, 1, 5))]


@pytest.mark.parametrize('kind', ['one', 'partial', 'exact'])
@pytest.mark.parametrize('ncoarse, fine', SORT_GRIDS)
def test_two_level_sort(lib, ncoarse, fine, kind):
    pos = ref.catalogue('clustered')
    origin, inv_cell = ref.uniform_grid(ref.BOX, ncoarse, fine)
    two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine,
                   chunk_for(len(pos), kind))


def test_sort_with_empty_coarse_cells_and_clamping(lib):
    # the grid covers [25, 225)^3: most coarse cells are empty, and a
    # quarter of the points per axis clamp into the first cells
    pos = ref.catalogue('clustered')
    ncoarse, fine = (4, 3, 5), (3, 5, 2)
    n = numpy.array(ncoarse) * numpy.array(fine)
    two_level_sort(lib, pos, [25.] * 3, n / 200., ncoarse, fine, 1000)


def test_sort_with_everything_in_one_fine_cell(lib):
    pos = 41. + 0.3 * numpy.array(ref.catalogue('clustered')) / ref.BOX
    ncoarse, fine = (3, 3, 3), (8, 8, 8)
    origin, inv_cell = ref.uniform_grid(ref.BOX, ncoarse, fine)
    s = two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, 700)
    assert (numpy.diff(host(s.start)) == len(pos)).sum() == 1


def test_sort_at_the_largest_fine_histogram(lib):
    # 34^3 sub-cells in one coarse cell: the 1024-thread scan
    pos = ref.catalogue('clustered')
    ncoarse, fine = (1, 1, 2), (34, 34, 34)
    origin, inv_cell = ref.uniform_grid(ref.BOX, ncoarse, fine)
    two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, 4096)


@pytest.mark.parametrize('n', [0, 1])
def test_sort_of_nothing_and_of_one(lib, n):
    pos = numpy.array(ref.catalogue('clustered'))[5:5 + n]
    ncoarse, fine = (2, 3, 1), (7, 1, 5)
    origin, inv_cell = ref.uniform_grid(ref.BOX, ncoarse, fine)
    two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, 64)


@pytest.mark.parametrize('ncoarse, fine', [
    ((35, 35, 35), (1, 1, 1)), ((1, 1, 1), (35, 35, 35)),
    ((0, 1, 1), (1, 1, 1)), ((1, 1, 1), (1, -2, 1))])
def test_bad_geometry_is_refused_before_any_launch(lib, ncoarse, fine):
    n = 10
    pos = dev(numpy.zeros((n, 3)))
    mat = filled(8, SENTINEL, torch.int32)
    out = nan_f64(3 * n)
    grid = (hiplib.f64_arr([0.] * 3), hiplib.f64_arr([1.] * 3),
            hiplib.int_arr(ncoarse), hiplib.int_arr(fine))
    box = hiplib.f64_arr(BOX3)
    assert lib.nbk_fof_cell_count_f64(
        hiplib.dptr(pos), n, 64, *grid, hiplib.dptr(mat),
        None) == NBK_ERR_ARG
    assert 'nbk_fof_cell_count_f64' in last_error(lib)
    assert lib.nbk_fof_cell_scatter_f64(
        hiplib.dptr(pos), hiplib.dptr(out), n, 64, *grid, hiplib.dptr(mat),
        hiplib.dptr(out), hiplib.dptr(out), None) == NBK_ERR_ARG
    assert lib.nbk_fof_fine_sort_f64(
        hiplib.dptr(out), hiplib.dptr(out), n, *grid, hiplib.dptr(mat),
        hiplib.dptr(out), hiplib.dptr(mat), hiplib.dptr(mat),
        None) == NBK_ERR_ARG
    assert lib.nbk_fof_link_f64(
        hiplib.dptr(out), hiplib.dptr(mat), n, grid[2], grid[3], box, 1,
        1.0, hiplib.dptr(mat), hiplib.dptr(mat), None) == NBK_ERR_ARG
    assert 'nbk_fof_link_f64' in last_error(lib)
    assert (host(mat) == SENTINEL).all() and numpy.isnan(host(out)).all()


def test_bad_n_and_linking_length_are_refused(lib):
    mat = filled(8, SENTINEL, torch.int32)
    out = nan_f64(8)
    one = hiplib.int_arr([1, 1, 1])
    box = hiplib.f64_arr(BOX3)
    for n, ll_sq in ((2 ** 31, 1.0), (-1, 1.0), (2, -1.0),
                     (2, float('nan')), (2, float('inf'))):
        assert lib.nbk_fof_link_f64(
            hiplib.dptr(out), hiplib.dptr(mat), n, one, one, box, 1, ll_sq,
            hiplib.dptr(mat), hiplib.dptr(mat), None) == NBK_ERR_ARG
    assert lib.nbk_fof_flatten_i32(hiplib.dptr(mat), 2 ** 31,
                                   hiplib.dptr(mat), hiplib.dptr(mat),
                                   None) == NBK_ERR_ARG
    assert (host(mat) == SENTINEL).all()


# ---- link and flatten -----------------------------------------------------------

def link_minid(lib, s, box, periodic, ll):
    """link + flatten over a checked sorted layout -> minid in input order,
    reduced on the host"""
    n = s.n
    parent = torch.arange(n, dtype=torch.int32, device=DEVICE)
    err = torch.zeros(1, dtype=torch.int32, device=DEVICE)
    hiplib.check(lib.nbk_fof_link_f64(
        hiplib.dptr(s.pos), hiplib.dptr(s.start), n,
        hiplib.int_arr(s.ncoarse), hiplib.int_arr(s.fine),
        hiplib.f64_arr(box if periodic else [0.] * 3),
        1 if periodic else 0, float(ll) * float(ll), hiplib.dptr(parent),
        hiplib.dptr(err), None), 'fof_link')
    parent_h = host(parent)
    assert host(err)[0] == 0
    # a forest whose links only go down
    assert (parent_h <= numpy.arange(n)).all() and (parent_h >= 0).all()
    root = filled(n, SENTINEL, torch.int32)
    hiplib.check(lib.nbk_fof_flatten_i32(
        hiplib.dptr(parent), n, hiplib.dptr(root), hiplib.dptr(err), None),
        'fof_flatten')
    assert host(err)[0] == 0
    root_h, index_h = host(root).astype('i8'), host(s.index).astype('i8')
    # the parent array is left as it was, and every root is its own root
    assert_array_equal(host(parent), parent_h)
    assert_array_equal(parent_h[root_h], root_h)
    smallest = numpy.full(n, n, dtype='i8')
    numpy.minimum.at(smallest, root_h, index_h)
    minid = numpy.empty(n, dtype='i8')
    minid[index_h] = smallest[root_h]
    return minid


def check_fof(lib, pos, box, periodic, ll, ncoarse, fine, want,
              origin=None, inv_cell=None):
    if origin is None:
        origin, inv_cell = ref.uniform_grid(box, ncoarse, fine)
    ncell = numpy.array(ncoarse) * numpy.array(fine)
    # the grid is a legal one: cells at least ll wide
    assert (ncell <= 2).all() or \
        (1. / numpy.asarray(inv_cell)[ncell > 2] >= ll).all()
    s = two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, 1024)
    first = link_minid(lib, s, box, periodic, ll)
    assert_array_equal(first, want)
    assert_array_equal(link_minid(lib, s, box, periodic, ll), first)


# grids of 1, 2, 3 and many cells on an axis (cell sides >= 1.0)
LINK_GRIDS = [((1, 1, 1), (1, 1, 1)), ((2, 1, 1), (1, 2, 1)),
              ((3, 1, 1), (1, 1, 3)), ((5, 5, 5), (4, 4, 4)),
              ((33, 11, 9), (3, 9, 11))]


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('ncoarse, fine', LINK_GRIDS)
@pytest.mark.parametrize('ll', [0.6, 1.0])
def test_link_clustered(lib, ll, ncoarse, fine, periodic):
    want, margin = ref.reference_minid('clustered', ll, periodic)
    assert margin >= ref.MARGIN
    check_fof(lib, ref.catalogue('clustered'), BOX3, periodic, ll, ncoarse,
              fine, want)


@pytest.mark.parametrize('periodic', [True, False])
@pytest.mark.parametrize('ncoarse, fine', LINK_GRIDS)
def test_link_filament(lib, ncoarse, fine, periodic):
    want, margin = ref.reference_minid('filament', ref.FILAMENT_LL, periodic)
    assert margin >= ref.MARGIN
    check_fof(lib, ref.catalogue('filament'), BOX3, periodic,
              ref.FILAMENT_LL, ncoarse, fine, want)


@pytest.mark.parametrize('ll', [0.6, 1.0])
def test_link_with_a_cell_side_within_1e_9_of_ll(lib, ll):
    # a non-periodic grid from the origin whose side is ll (1 + 1e-9)
    want, margin = ref.reference_minid('clustered', ll, False)
    assert margin >= ref.MARGIN
    side = ll * (1 + 1e-9)
    ncoarse, fine = (28, 28, 28), (6, 6, 6)
    assert 168 * side > ref.BOX
    check_fof(lib, ref.catalogue('clustered'), None, False, ll, ncoarse,
              fine, want, origin=[0.] * 3, inv_cell=[1. / side] * 3)


def test_link_duplicated_rows(lib):
    base = numpy.array(ref.catalogue('clustered'))[:600]
    pos = numpy.concatenate([base, base[:80], base[:20]])
    want, _ = ref.brute_fof(pos, 1.0, BOX3)
    # duplicates link (distance 0), so the copies share their original's
    # group
    assert_array_equal(want[600:680], want[:80])
    off_dupes = numpy.abs(ref.pair_r2(base, BOX3) - 1.0)
    numpy.fill_diagonal(off_dupes, 1.)
    assert off_dupes.min() >= ref.MARGIN
    for ncoarse, fine in (((1, 1, 1), (1, 1, 1)), ((5, 5, 5), (4, 4, 4))):
        check_fof(lib, pos, BOX3, True, 1.0, ncoarse, fine, want)


@pytest.mark.parametrize('periodic', [True, False])
def test_link_anisotropic_box(lib, periodic):
    pos, _ = pref.catalogue('H1')
    box = list(pref.HBOX)
    ll = 2.5
    want, margin = ref.brute_fof(pos, ll, box if periodic else None)
    assert margin >= ref.MARGIN
    assert 1 < len(numpy.unique(want)) < len(pos)
    for ncoarse, fine in (((4, 4, 1), (3, 4, 2)), ((2, 1, 25), (1, 1, 1))):
        check_fof(lib, pos, box, periodic, ll, ncoarse, fine, want)


def test_link_lattices(lib):
    # 8^3 singletons at ll = 0.9 of the unit spacing
    grid = ref.lattice(8, 8.)
    check_fof(lib, grid, [8.] * 3, True, 0.9, (2, 2, 2), (4, 4, 4),
              numpy.arange(512))
    # four copies: 512 chains of 4, the -0.01 copy wrapped to the far face
    pos = numpy.remainder(ref.lattice_copies(), 8.)
    ll = 0.011 * 3 ** 0.5
    want = numpy.tile(numpy.arange(512), 4)
    for ncoarse, fine in (((2, 2, 2), (4, 4, 4)), ((8, 8, 8), (20, 20, 20))):
        check_fof(lib, pos, [8.] * 3, True, ll, ncoarse, fine, want)
    # 4^3 at ll = 2: one group
    grid = ref.lattice(4, 4.) - 0.5
    for ncoarse, fine in (((1, 1, 1), (1, 1, 1)), ((2, 1, 1), (1, 2, 2))):
        check_fof(lib, grid, [4.] * 3, True, 2.0, ncoarse, fine,
                  numpy.zeros(64, dtype='i8'))


def test_flatten_stops_at_a_cycle(lib):
    n = 1000
    parent_h = numpy.arange(n, dtype='i4')
    parent_h[1:] = numpy.arange(n - 1)          # one chain of 1000
    parent_h[300], parent_h[301] = 301, 300     # ... with a 2-cycle in it
    parent = dev(parent_h)
    root = filled(n + 64, SENTINEL, torch.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEVICE)
    rc = lib.nbk_fof_flatten_i32(hiplib.dptr(parent), n, hiplib.dptr(root),
                                 hiplib.dptr(err), None)
    assert rc == NBK_ERR_ARG
    assert 'nbk_fof_flatten_i32' in last_error(lib)
    assert host(err)[0] != 0
    root_h = host(root)
    # below the cycle the walk still ends at 0; from it on it gives up
    assert_array_equal(root_h[:300], 0)
    assert_array_equal(root_h[300:n], -1)
    assert_array_equal(root_h[n:], SENTINEL)
    assert_array_equal(host(parent), parent_h)


def test_flatten_of_a_long_chain(lib):
    n = 5000
    parent_h = numpy.arange(n, dtype='i4')
    parent_h[1:] = numpy.arange(n - 1)
    parent_h[4000] = 4000                       # two chains
    root = filled(n, SENTINEL, torch.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEVICE)
    hiplib.check(lib.nbk_fof_flatten_i32(
        hiplib.dptr(dev(parent_h)), n, hiplib.dptr(root), hiplib.dptr(err),
        None), 'fof_flatten')
    want = numpy.where(numpy.arange(n) < 4000, 0, 4000)
    assert_array_equal(host(root), want)
    assert host(err)[0] == 0
