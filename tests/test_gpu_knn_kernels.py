"""
Kernel-level tests of nbk_knn_f64 (csrc/nbk_knn.hip), called through the
C ABI with hand-picked grids over a layout sorted by the nbk_fof_* sort
calls, and compared with the brute force of knn_reference.py — never with
another GPU kernel.

Both outputs are compared for exact equality: the brute force rounds every
operation like the kernel (the library is built with -ffp-contract=off),
and the order (r2, input index) decides every tie, so the lattices and the
coincident points need no margin.
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
import knn_reference as kref                                    # noqa: E402
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


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def last_error(lib):
    return lib.nbk_last_error_string().decode()


def two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine, chunk=1024):
    """count -> scan -> scatter -> fine pass; the start table and the
    index column are checked against the reference before the search
    reads through them"""
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
        cids = ref.coarse_ids(pos, origin, inv_cell, ncoarse, fine)
        assert_array_equal(host(cstart), numpy.concatenate(
            [[0], numpy.cumsum(numpy.bincount(cids,
                                              minlength=ncoarse_all))]))
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
    # every slot holds a particle of its cell, bit for bit
    assert_array_equal(ids[got_index], ref.sorted_keys(want_start))
    assert_array_equal(host(spos).reshape(3, n).T, pos[got_index])
    return SimpleNamespace(n=n, pos=spos, index=sindex, start=fstart,
                           origin=list(origin), inv_cell=list(inv_cell),
                           ncoarse=list(ncoarse), fine=list(fine))


def knn_call(lib, s, box, periodic, k, r2, index, n=None, **replace):
    """nbk_knn_f64 over a sorted layout into r2 / index; returns the code"""
    g = dict(origin=s.origin, inv_cell=s.inv_cell, ncoarse=s.ncoarse,
             fine=s.fine)
    g.update(replace)
    return lib.nbk_knn_f64(
        hiplib.dptr(s.pos), hiplib.dptr(s.start), hiplib.dptr(s.index),
        s.n if n is None else n, hiplib.f64_arr(g['origin']),
        hiplib.f64_arr(g['inv_cell']), hiplib.int_arr(g['ncoarse']),
        hiplib.int_arr(g['fine']),
        hiplib.f64_arr(box if periodic else [0.] * 3),
        1 if periodic else 0, k, hiplib.dptr(r2), hiplib.dptr(index), None)


def search(lib, s, box, periodic, k):
    """(r2, index) on the host, with a margin behind both outputs that
    must come back untouched"""
    r2 = filled(s.n + 64, float('nan'), torch.float64)
    index = filled(s.n + 64, SENTINEL, torch.int32)
    hiplib.check(knn_call(lib, s, box, periodic, k, r2, index), 'nbk_knn')
    r2_h, index_h = host(r2), host(index)
    assert numpy.isnan(r2_h[s.n:]).all() and (index_h[s.n:] == SENTINEL).all()
    return r2_h[:s.n], index_h[:s.n]


def check_knn(lib, pos, box, periodic, ks, ncoarse, fine, origin=None,
              inv_cell=None, table=None):
    """sort once, then every k against the brute force (``table``: a
    knn_table computed before); returns the results for the callers that
    compare runs"""
    if origin is None:
        origin, inv_cell = ref.uniform_grid(box, ncoarse, fine)
    if table is None:
        table = kref.knn_table(pos, box if periodic else None)
    s = two_level_sort(lib, pos, origin, inv_cell, ncoarse, fine)
    out = []
    for k in ks:
        r2, index = search(lib, s, box, periodic, k)
        assert_array_equal(r2, table[0][:, k - 1])
        assert_array_equal(index, table[1][:, k - 1])
        out.append((r2, index))
    return out


# ---- 1. an ordinary grid, every template ------------------------------------

UNIFORM_2000 = kref.uniform(2000, ref.BOX)
ALL_K = [1, 2, 7, 8, 16]


@pytest.fixture(scope='module')
def uniform_table():
    """the brute force of UNIFORM_2000, computed once per geometry"""
    tables = {}

    def get(periodic):
        if periodic not in tables:
            tables[periodic] = kref.knn_table(UNIFORM_2000,
                                              BOX3 if periodic else None)
        return tables[periodic]
    return get


@pytest.mark.parametrize('periodic', [True, False])
def test_ordinary_grid_every_template(lib, uniform_table, periodic):
    check_knn(lib, UNIFORM_2000, BOX3, periodic, ALL_K, (3, 3, 3),
              (2, 2, 2), table=uniform_table(periodic))


# ---- 2. few cells per axis --------------------------------------------------

@pytest.mark.parametrize('ncoarse, fine', [
    ((1, 1, 1), (1, 1, 1)), ((2, 1, 1), (1, 2, 2)), ((1, 3, 1), (3, 1, 3)),
    ((2, 4, 1), (2, 1, 4))])
def test_periodic_with_1_to_4_cells_per_axis(lib, ncoarse, fine):
    pos = UNIFORM_2000[:700]
    assert len(set(numpy.array(ncoarse) * numpy.array(fine))) == 1
    check_knn(lib, pos, BOX3, True, [7], ncoarse, fine)


@pytest.mark.parametrize('periodic', [True, False])
def test_mixed_grid_in_a_non_cubic_box(lib, periodic):
    box = [100., 60., 140.]
    pos = kref.uniform(700, box, seed=11)
    check_knn(lib, pos, box, periodic, [3, 7], (1, 2, 5), (1, 1, 1))
    check_knn(lib, pos, box, periodic, [7], (1, 1, 1), (1, 2, 5))


# ---- 3. many rings ------------------------------------------------------------

@pytest.mark.parametrize('periodic', [True, False])
def test_many_rings_clustered(lib, periodic):
    # 1728 cells for 3092 points, a third of them in 24 blobs
    check_knn(lib, ref.catalogue('clustered'), BOX3, periodic, [7, 16],
              (4, 4, 4), (3, 3, 3),
              table=kref.reference_table('clustered', periodic))


@pytest.mark.parametrize('periodic', [True, False])
def test_many_rings_sparse(lib, periodic):
    # 300 points in 1728 cells: most cells are empty, k = 16 needs rings
    # out to full coverage for some
    pos = UNIFORM_2000[:300]
    check_knn(lib, pos, BOX3, periodic, [1, 7, 16], (3, 4, 2), (4, 3, 6))


def test_everything_in_one_cell_of_a_large_grid(lib):
    # the worst case: every thread walks every start-table entry
    pos = 41. + 0.3 * UNIFORM_2000[:200] / ref.BOX
    for periodic in (True, False):
        check_knn(lib, pos, BOX3, periodic, [7], (3, 3, 3), (4, 4, 4))


# ---- 4. too few particles -------------------------------------------------------

@pytest.mark.parametrize('k', [1, 7, 16])
def test_too_few_particles(lib, k):
    for n, finite in ((1, False), (k, False), (k + 1, True)):
        pos = UNIFORM_2000[:n]
        for periodic in (True, False):
            (r2, index), = check_knn(lib, pos, BOX3, periodic, [k],
                                     (2, 2, 2), (2, 2, 2))
            if finite:
                assert numpy.isfinite(r2).all() and (index >= 0).all()
            else:
                assert numpy.isinf(r2).all() and (index == -1).all()


def test_nothing_launches_nothing(lib):
    s = two_level_sort(lib, numpy.zeros((0, 3)), [0.] * 3, [0.04] * 3,
                       (2, 2, 2), (2, 2, 2))
    r2, index = search(lib, s, BOX3, True, 7)
    assert len(r2) == 0 and len(index) == 0


# ---- 5. ties ----------------------------------------------------------------------

def test_lattices_and_coincident_points(lib):
    box = [8.] * 3
    # half-cell shifted: every point has 6 neighbours at exactly 1, 12 at
    # exactly sqrt 2
    grid = ref.lattice(8, 8.)
    check_knn(lib, grid, box, True, [1, 6, 7, 16], (2, 2, 2), (2, 2, 2))
    # points exactly on cell faces and corners
    corners = ref.lattice(8, 8.) - 0.5
    check_knn(lib, corners, box, True, [1, 7], (2, 2, 2), (4, 4, 4))
    check_knn(lib, corners, box, False, [7], (2, 2, 2), (4, 4, 4))
    # four copies at small offsets, and the grid once more: coincident
    # points are neighbours at distance 0, the smaller index first
    pos = numpy.remainder(numpy.concatenate(
        [ref.lattice_copies(), corners]), 8.)
    (r2, index), _ = check_knn(lib, pos, box, True, [1, 7], (2, 2, 2),
                               (4, 4, 4))
    assert_array_equal(r2[:512], 0.)
    assert_array_equal(index[:512], numpy.arange(512) + 2048)
    assert_array_equal(index[2048:], numpy.arange(512))


# ---- 6. a flat axis ---------------------------------------------------------------

def test_flat_axis(lib):
    pos = numpy.array(UNIFORM_2000[:900])
    pos[:, 2] = 12.5
    origin = [0., 0., 12.5]
    inv_cell = [0.06, 0.06, 0.]
    check_knn(lib, pos, None, False, [1, 7], (2, 3, 1), (3, 2, 1),
              origin=origin, inv_cell=inv_cell)


def test_grid_that_clamps_outliers(lib):
    # a non-periodic grid over [25, 75)^3 only: the points outside clamp
    # into the edge cells
    pos = UNIFORM_2000[:900]
    check_knn(lib, pos, None, False, [7], (2, 2, 2), (3, 3, 3),
              origin=[25.] * 3, inv_cell=[6 / 50.] * 3)


# ---- 7. reproducibility -------------------------------------------------------------

def test_two_runs_are_bitwise_equal(lib, uniform_table):
    pos = numpy.remainder(ref.lattice_copies(), 8.)
    table = kref.knn_table(pos, [8.] * 3)
    runs = []
    for _ in range(2):
        # (each run sorts again: the order inside a cell may differ)
        runs.append(
            check_knn(lib, UNIFORM_2000, BOX3, True, ALL_K, (3, 3, 3),
                      (2, 2, 2), table=uniform_table(True))
            + check_knn(lib, pos, [8.] * 3, True, [7], (2, 2, 2), (4, 4, 4),
                        table=table))
    first, again = runs
    for (r2_a, index_a), (r2_b, index_b) in zip(first, again):
        assert r2_a.tobytes() == r2_b.tobytes()
        assert index_a.tobytes() == index_b.tobytes()


# ---- 8. bad arguments -----------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(lib):
    pos = UNIFORM_2000[:100]
    origin, inv_cell = ref.uniform_grid(BOX3, (2, 2, 2), (2, 2, 2))
    s = two_level_sort(lib, pos, origin, inv_cell, (2, 2, 2), (2, 2, 2))
    r2 = filled(100, float('nan'), torch.float64)
    index = filled(100, SENTINEL, torch.int32)
    cases = [dict(k=0), dict(k=17), dict(k=7, n=-1),
             dict(k=7, ncoarse=[2, 0, 2]),
             dict(k=7, box=[0., 100., 100.]),
             dict(k=7, inv_cell=[0.04, float('nan'), 0.04])]
    for case in cases:
        case = dict(case)
        rc = knn_call(lib, s, case.pop('box', BOX3), True, case.pop('k'),
                      r2, index, **case)
        assert rc == NBK_ERR_ARG, case
        assert 'nbk_knn_f64' in last_error(lib)
        assert numpy.isnan(host(r2)).all()
        assert (host(index) == SENTINEL).all()
    # box is not read when not periodic
    hiplib.check(knn_call(lib, s, [0.] * 3, False, 7, r2, index), 'knn')
    want_r2, want_index = kref.knn_brute(pos, 7)
    assert_array_equal(host(r2), want_r2)
    assert_array_equal(host(index), want_index)


def test_index_entry_out_of_range_is_skipped(lib):
    pos = UNIFORM_2000[:500]
    origin, inv_cell = ref.uniform_grid(BOX3, (2, 2, 2), (2, 2, 2))
    s = two_level_sort(lib, pos, origin, inv_cell, (2, 2, 2), (2, 2, 2))
    want_r2, want_index = kref.knn_brute(pos, 7, BOX3)
    index_h = host(s.index).copy()
    for slot, bad in ((123, 500), (321, -1), (17, -2 ** 31)):
        victim = index_h[slot]
        corrupt = index_h.copy()
        corrupt[slot] = bad
        s.index = dev(corrupt)
        r2, index = search(lib, s, BOX3, True, 7)
        # the row of the slot is never written ...
        assert numpy.isnan(r2[victim]) and index[victim] == SENTINEL
        # ... and every other row is right; where the victim is the 7th
        # neighbour itself, the index reads what the column says
        others = numpy.arange(500) != victim
        assert_array_equal(r2[others], want_r2[others])
        named = others & (want_index == victim)
        plain = others & (want_index != victim)
        assert_array_equal(index[plain], want_index[plain])
        assert_array_equal(index[named], bad)


# ---- 9. the limit ---------------------------------------------------------------------

def test_max_k(lib):
    assert lib.nbk_knn_max_k() == 16
