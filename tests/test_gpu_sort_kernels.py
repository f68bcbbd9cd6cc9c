"""
Kernel-level tests of the paint locality sorts, the ownership-gather
paint, the scatter paints and the readout, called through the C ABI and
compared with plain numpy (sort_reference.py) and with oracle.paint /
oracle.readout — never with another GPU kernel.

Integers (counts, bases, row tables) are compared exactly; positions
and masses are moved, not computed, so they are compared bit for bit.
Paints keep the project's paint bar, rtol = atol = 1e-12 against the
oracle (test_gpu_kernels.py), the fused z-spectrum the r2c bar of 1e-12
of the line's largest magnitude.

Inputs sit where floor(x * invH), the index wrap, the stencil-span
tables and the tile masks have to agree: exact cell and half-cell
boundaries and their neighbouring doubles, +-0.0, BoxSize itself,
positions outside the box, every particle in one cell, every particle
in the last row — on a non-dyadic anisotropic box and on meshes that
are thin in x (fewer planes than the gather tile's source span),
non-power-of-two in x and z, or the smallest legal pair-bucket mesh.
"""
import functools
from types import SimpleNamespace

import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import sort_reference as ref                                    # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.source.mesh.catalog import (                  # noqa: E402
    _PAIR_GHOST, _two_level_ys, _pair_gs)
from oracle import MeshGeometry, paint, readout                 # noqa: E402

DEVICE = 'cuda'
NBK_ERR_ARG = -2

# non-dyadic, anisotropic: no invH is a power of two
BOX = (10.0, 100.0 / 3, 7.3)
MESHES = {
    'n32': [32, 32, 32],
    'thin4': [4, 32, 32],       # n0 < P + span for the TSC/PCS gather tile
    'thin8': [8, 64, 32],       # same with P = 8; also the slab-halves mesh
    'pair2': [2, 32, 32],       # smallest legal pair-bucket mesh
    'npot': [6, 64, 48],        # generic-modulo wrap in x and z
}
NBLOCKS = (1, 5, 9, 17)
PAIR_TEST_GS = 3                # 8-row groups: several groups per plane


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


def geom_args(nmesh):
    return hiplib.i64_arr(nmesh), hiplib.f64_arr(BOX)


def chunk_for(n, nblocks):
    """a chunk size giving exactly ``nblocks`` chunks, the last partial"""
    if nblocks == 1:
        return n + 1000
    chunk = n // nblocks + 1
    assert -(-n // chunk) == nblocks and n % chunk != 0
    return chunk


# ---- inputs and oracle results, computed once --------------------------

@functools.lru_cache(maxsize=None)
def catalogue(mesh, cat):
    """(positions (n, 3), masses or None).  The clustered catalogue is
    unweighted so the NULL-mass path of every kernel runs too."""
    nmesh = MESHES[mesh]
    pos = ref.CATALOGUES[cat](nmesh, BOX)
    mass = None if cat == 'clustered' else ref.masses(len(pos))
    pos.setflags(write=False)
    if mass is not None:
        mass.setflags(write=False)
    return pos, mass


@functools.lru_cache(maxsize=None)
def oracle_mesh(mesh, cat, window, shift):
    pos, mass = catalogue(mesh, cat)
    nmesh = MESHES[mesh]
    want = numpy.zeros(nmesh)
    paint(pos, 1.0 if mass is None else mass, want,
          MeshGeometry(nmesh, BOX), resampler=window, shift=shift)
    want.setflags(write=False)
    return want


def total_mass(mesh, cat):
    pos, mass = catalogue(mesh, cat)
    return float(len(pos)) if mass is None else mass.sum()


# ---- drivers of the sort pipelines -------------------------------------

def run_scan(lib, mat_t, nblocks, nbuck):
    colsum = filled(9 * nbuck, -1, torch.int32)   # 8 partials + sums
    bases = filled(nblocks * nbuck, -1, torch.int32)
    bucket_bases = filled(nbuck + 1, -1, torch.int32)
    hiplib.check(lib.nbk_scan_matrix_i32(
        hiplib.dptr(mat_t), nblocks, nbuck, hiplib.dptr(colsum),
        hiplib.dptr(bases), hiplib.dptr(bucket_bases), None), 'scan')
    return bases, bucket_bases


def check_cursors(mat, bases, bucket_bases, nblocks, nbuck, n_out):
    """The scatter passes write through these cursors: make sure they
    stay inside the output arrays before launching them."""
    m = host(mat).reshape(nblocks, nbuck)
    assert m.min() >= 0 and m.sum() == n_out
    want_bases, want_bb = ref.scan_matrix(m)
    assert_array_equal(host(bucket_bases), want_bb)
    assert_array_equal(host(bases).reshape(nblocks, nbuck), want_bases)


def run_two_level(lib, pos, mass, nmesh, ys, chunk, rows_only):
    n = len(pos)
    n0, n1, n2 = nmesh
    nm, bx = geom_args(nmesh)
    nbuck = n0 * (n1 >> ys)
    nblocks = -(-n // chunk)
    pos_t = dev(pos)
    mass_t = None if mass is None else dev(mass)
    mat = filled(nblocks * nbuck, -1, torch.int32)
    flag = filled(1, 0, torch.int32)
    hiplib.check(lib.nbk_xsort_count_f64(
        hiplib.dptr(pos_t), n, chunk, nm, bx, ys, hiplib.dptr(mat),
        hiplib.dptr(flag), None), 'xsort_count')
    bases, bucket_bases = run_scan(lib, mat, nblocks, nbuck)
    check_cursors(mat, bases, bucket_bases, nblocks, nbuck, n)
    coarse = nan_f64(3 * n)
    mass_c = None if mass is None else nan_f64(n)
    hiplib.check(lib.nbk_xsort_scatter_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n, chunk, nm, bx, ys,
        hiplib.dptr(bases), hiplib.dptr(coarse), hiplib.dptr(mass_c),
        None), 'xsort_scatter')
    out = nan_f64(3 * n)
    out_m = None if mass is None else nan_f64(n)
    rowtab = filled(n0 * n1 + 1, -7, torch.int32)
    rowtab[-1] = n                        # the caller's sentinel
    hiplib.check(lib.nbk_bucket_fine_f64(
        hiplib.dptr(coarse), hiplib.dptr(mass_c), n, nm, bx, ys,
        hiplib.dptr(bucket_bases), hiplib.dptr(out), hiplib.dptr(out_m),
        hiplib.dptr(rowtab), int(rows_only), None), 'bucket_fine')
    return SimpleNamespace(
        n=n, nbuck=nbuck, nblocks=nblocks, mat=mat, flag=flag,
        bases=bases, bucket_bases=bucket_bases, coarse=coarse,
        coarse_mass=mass_c, pos=out, mass=out_m, table=rowtab, pair_gs=-1)


def run_pair_sort(lib, pos, mass, nmesh, gs, dlo, dhi, chunk):
    n = len(pos)
    n0, n1, n2 = nmesh
    nm, bx = geom_args(nmesh)
    nbuck = (n0 >> 1) * (n1 >> gs)
    nblocks = -(-n // chunk)
    pos_t = dev(pos)
    mass_t = None if mass is None else dev(mass)
    mat = filled(nblocks * nbuck, -1, torch.int32)
    hiplib.check(lib.nbk_psort_count_f64(
        hiplib.dptr(pos_t), n, chunk, nm, bx, gs, dlo, dhi,
        hiplib.dptr(mat), None), 'psort_count')
    bases, bucket_bases = run_scan(lib, mat, nblocks, nbuck)
    n_out = int(host(bucket_bases)[-1])
    check_cursors(mat, bases, bucket_bases, nblocks, nbuck, n_out)
    # the reference copy count bounds the allocation before the scatter
    # writes through the scanned bases
    k1, k2 = ref.pair_keys(pos, nmesh, BOX, gs, dlo, dhi)
    assert n_out == n + int((k2 >= 0).sum())
    out = nan_f64(3 * n_out)
    out_m = None if mass is None else nan_f64(n_out)
    hiplib.check(lib.nbk_psort_scatter_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n, chunk, nm, bx, gs,
        dlo, dhi, hiplib.dptr(bases), n_out, hiplib.dptr(out),
        hiplib.dptr(out_m), None), 'psort_scatter')
    return SimpleNamespace(
        n=n_out, nbuck=nbuck, nblocks=nblocks, mat=mat, bases=bases,
        bucket_bases=bucket_bases, pos=out, mass=out_m,
        table=bucket_bases, pair_gs=gs, keys=(k1, k2))


def soa_rows(t, n):
    """(n, 3) host rows of a device SoA block x[n] y[n] z[n]"""
    return host(t).reshape(3, n).T


def host_mass(t):
    return None if t is None else host(t)


def assert_same_particles(got_rows, got_mass, pos, mass, key_got=None,
                          key_want=None):
    assert_array_equal(ref.canonical_rows(got_rows, got_mass, key_got),
                       ref.canonical_rows(pos, mass, key_want))


_sorted_cache = {}


def sorted_table(mesh, cat, mode, window='cic', interlaced=False):
    """device-resident sorted particles + table for the gather paint,
    built once per (mesh, catalogue, table mode[, pair ghost row])"""
    lib = hiplib.require()
    nmesh = MESHES[mesh]
    if mode == 'row':
        key = (mesh, cat, mode)
    else:
        key = (mesh, cat, mode, _PAIR_GHOST[(window, interlaced)])
    if key not in _sorted_cache:
        pos, mass = catalogue(mesh, cat)
        chunk = chunk_for(len(pos), 5)
        if mode == 'row':
            ys = _two_level_ys(SimpleNamespace(Nmesh=nmesh))
            s = run_two_level(lib, pos, mass, nmesh, ys, chunk,
                              rows_only=1)
            tab = host(s.table)
            assert tab[0] == 0 and tab[-1] == s.n \
                and (numpy.diff(tab) >= 0).all()
            _sorted_cache[key] = s
        else:
            gs = PAIR_TEST_GS if mode == 'pair' else _pair_gs(nmesh)
            dlo, dhi = key[3]
            assert dhi - dlo < (1 << gs)
            _sorted_cache[key] = run_pair_sort(lib, pos, mass, nmesh, gs,
                                               dlo, dhi, chunk)
    return _sorted_cache[key]


# ---- (a) nbk_scan_matrix_i32 --------------------------------------------

@pytest.mark.parametrize('nblocks,nbuck', [
    (1, 1), (1, 1024), (3, 7), (7, 1000), (8, 1025), (9, 4097),
    (17, 40960)])
def test_scan_matrix(lib, nblocks, nbuck):
    rng = numpy.random.RandomState(nblocks * 100003 + nbuck)
    mat = rng.randint(0, 50, size=(nblocks, nbuck)).astype('i4')
    mat[:, rng.uniform(size=nbuck) < 0.2] = 0       # all-zero columns
    bases, bucket_bases = run_scan(lib, dev(mat), nblocks, nbuck)
    want_bases, want_bb = ref.scan_matrix(mat)
    assert_array_equal(host(bucket_bases), want_bb)
    assert_array_equal(host(bases).reshape(nblocks, nbuck), want_bases)


# ---- (b) nbk_bucket_count_f64 -------------------------------------------

def run_bucket_count(lib, pos, nmesh, shift):
    nm, bx = geom_args(nmesh)
    nb = (nmesh[0] * nmesh[1] * nmesh[2]) >> shift
    pos_t = dev(pos)
    counts = filled(nb, 0, torch.int32)
    flag = filled(1, 0, torch.int32)
    hiplib.check(lib.nbk_bucket_count_f64(
        hiplib.dptr(pos_t), len(pos), nm, bx, shift, hiplib.dptr(counts),
        hiplib.dptr(flag), None), 'bucket_count')
    return host(counts), int(host(flag)[0])


@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('mesh', ['n32', 'pair2', 'npot'])
def test_bucket_count(lib, mesh, shift):
    nmesh = MESHES[mesh]
    pos, _ = catalogue(mesh, 'edge')
    ids = ref.cell_ids(pos, nmesh, BOX)
    nb = (nmesh[0] * nmesh[1] * nmesh[2]) >> shift
    counts, flag = run_bucket_count(lib, pos, nmesh, shift)
    assert_array_equal(counts, numpy.bincount(ids >> shift, minlength=nb))
    assert flag == 1                      # the catalogue is scrambled

    # reference-sorted input: no false positive (callers skip the sort)
    order = numpy.argsort(ids, kind='stable')
    spos = pos[order]
    counts, flag = run_bucket_count(lib, spos, nmesh, shift)
    assert_array_equal(counts, numpy.bincount(ids >> shift, minlength=nb))
    assert flag == 0

    # one inversion between two neighbouring lanes of the same wave
    sid = ids[order] >> shift
    k = numpy.flatnonzero((sid[:-1] < sid[1:])
                          & (numpy.arange(1, len(sid)) % 64 != 0))[0]
    inv = spos.copy()
    inv[[k, k + 1]] = inv[[k + 1, k]]
    _, flag = run_bucket_count(lib, inv, nmesh, shift)
    assert flag == 1


# ---- (c) nbk_bucket_scatter_f64 -----------------------------------------

@pytest.mark.parametrize('soa_out', [0, 1])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('mesh', ['n32', 'npot'])
def test_bucket_scatter(lib, mesh, shift, weighted, soa_out):
    nmesh = MESHES[mesh]
    nm, bx = geom_args(nmesh)
    pos, mass = catalogue(mesh, 'edge')
    if not weighted:
        mass = None
    n = len(pos)
    nb = (nmesh[0] * nmesh[1] * nmesh[2]) >> shift
    counts = numpy.bincount(ref.cell_ids(pos, nmesh, BOX) >> shift,
                            minlength=nb)
    pos_t = dev(pos)
    mass_t = None if mass is None else dev(mass)
    offsets = dev(numpy.cumsum(counts).astype('i4'))   # INCLUSIVE cumsum
    out = nan_f64(3 * n)
    out_m = None if mass is None else nan_f64(n)
    hiplib.check(lib.nbk_bucket_scatter_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n, nm, bx, shift,
        soa_out, hiplib.dptr(offsets), hiplib.dptr(out),
        hiplib.dptr(out_m), None), 'bucket_scatter')
    rows = soa_rows(out, n) if soa_out else host(out).reshape(n, 3)
    assert_same_particles(rows, host_mass(out_m), pos, mass)
    # slots [base_b, base_b + count_b) hold exactly bucket b
    assert_array_equal(ref.cell_ids(rows, nmesh, BOX) >> shift,
                       numpy.repeat(numpy.arange(nb), counts))
    # the tickets counted down to the exclusive bases
    assert_array_equal(host(offsets), numpy.cumsum(counts) - counts)


# ---- (d) xsort_count -> scan -> xsort_scatter -> bucket_fine ------------

def two_level_modes(nmesh):
    ys = _two_level_ys(SimpleNamespace(Nmesh=nmesh))
    # cell mode needs the production ys (fine window % 1024); the
    # rows-only mode also runs at 4-row groups, several per plane
    return [(0, ys), (1, ys), (1, 2)]


_row_tables = {}


@pytest.mark.parametrize('nblocks', NBLOCKS)
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('mesh', list(MESHES))
def test_two_level_sort(lib, mesh, mode, nblocks):
    nmesh = MESHES[mesh]
    n0, n1, n2 = nmesh
    rows_only, ys = two_level_modes(nmesh)[mode]
    pos, mass = catalogue(mesh, 'edge')
    n = len(pos)
    chunk = chunk_for(n, nblocks)
    s = run_two_level(lib, pos, mass, nmesh, ys, chunk, rows_only)
    assert s.nblocks == nblocks

    # pass A: one histogram row per chunk
    ckeys = ref.coarse_keys(pos, nmesh, BOX, ys)
    want_mat = ref.chunk_histograms(ckeys, s.nbuck, chunk)
    assert_array_equal(host(s.mat).reshape(nblocks, s.nbuck), want_mat)
    assert int(host(s.flag)[0]) == 1
    want_bases, want_bb = ref.scan_matrix(want_mat)
    assert_array_equal(host(s.bucket_bases), want_bb)
    assert_array_equal(host(s.bases).reshape(nblocks, s.nbuck), want_bases)

    # pass C: the same particles, grouped by coarse bucket
    crow = soa_rows(s.coarse, n)
    assert_same_particles(crow, host_mass(s.coarse_mass), pos, mass)
    assert_array_equal(ref.coarse_keys(crow, nmesh, BOX, ys),
                       numpy.repeat(numpy.arange(s.nbuck),
                                    numpy.diff(want_bb)))

    # fine pass: the same particles in cell (or row) order + row table
    rows = soa_rows(s.pos, n)
    assert_same_particles(rows, host_mass(s.mass), pos, mass)
    rid = ref.row_ids(rows, nmesh, BOX)
    if rows_only:
        assert (numpy.diff(rid) >= 0).all()
    else:
        assert (numpy.diff(ref.cell_ids(rows, nmesh, BOX)) >= 0).all()
    rowtab = host(s.table)
    assert_array_equal(rowtab[:-1], ref.row_table(rid, n0 * n1))
    assert rowtab[-1] == n                # sentinel left as set

    # the tables do not depend on the chunking
    first = _row_tables.setdefault((mesh, mode), rowtab)
    assert_array_equal(rowtab, first)


def test_xsort_count_sorted_input_not_flagged(lib):
    nmesh = MESHES['npot']
    pos, _ = catalogue('npot', 'edge')
    pos = pos[numpy.argsort(ref.cell_ids(pos, nmesh, BOX), kind='stable')]
    ys = _two_level_ys(SimpleNamespace(Nmesh=nmesh))
    s = run_two_level(lib, pos, None, nmesh, ys, chunk_for(len(pos), 9), 1)
    assert int(host(s.flag)[0]) == 0
    assert_same_particles(soa_rows(s.pos, len(pos)), None, pos, None)


# ---- (e) psort_count -> scan -> psort_scatter ---------------------------

@pytest.mark.parametrize('variant', ['gs3-9blocks', 'gsmax-5blocks'])
@pytest.mark.parametrize('ghost', sorted(_PAIR_GHOST))
@pytest.mark.parametrize('mesh', ['n32', 'pair2', 'npot', 'thin4'])
def test_pair_sort(lib, mesh, ghost, variant):
    nmesh = MESHES[mesh]
    dlo, dhi = _PAIR_GHOST[ghost]
    gs, nblocks = ((PAIR_TEST_GS, 9) if variant == 'gs3-9blocks'
                   else (_pair_gs(nmesh), 5))
    assert dhi - dlo < (1 << gs)
    pos, mass = catalogue(mesh, 'edge')
    n = len(pos)
    chunk = chunk_for(n, nblocks)
    s = run_pair_sort(lib, pos, mass, nmesh, gs, dlo, dhi, chunk)
    k1, k2 = s.keys
    dup = k2 >= 0
    if variant == 'gs3-9blocks':
        assert dup.any() and not dup.all()

    want_mat = ref.chunk_histograms((k1, k2), s.nbuck, chunk)
    assert_array_equal(host(s.mat).reshape(nblocks, s.nbuck), want_mat)
    want_bases, want_bb = ref.scan_matrix(want_mat)
    assert_array_equal(host(s.bucket_bases), want_bb)
    assert_array_equal(host(s.bases).reshape(nblocks, s.nbuck), want_bases)
    assert s.n == n + dup.sum()           # 1 copy, + 1 across a group edge

    # every bucket range holds exactly its multiset of (position, mass)
    want_pos = numpy.concatenate([pos, pos[dup]])
    want_mass = numpy.concatenate([mass, mass[dup]])
    want_key = numpy.concatenate([k1, k2[dup]])
    got_key = numpy.repeat(numpy.arange(s.nbuck), numpy.diff(want_bb))
    assert_same_particles(soa_rows(s.pos, s.n), host(s.mass), want_pos,
                          want_mass, got_key, want_key)


def test_pair_sort_rejects_bad_geometry(lib):
    pos, _ = catalogue('n32', 'edge')
    pos_t = dev(pos[:1000])
    mat = filled(40960, 0, torch.int32)
    bx = hiplib.f64_arr(BOX)

    def count(nmesh, gs, dlo, dhi):
        return lib.nbk_psort_count_f64(
            hiplib.dptr(pos_t), 1000, 4096, hiplib.i64_arr(nmesh), bx, gs,
            dlo, dhi, hiplib.dptr(mat), None)

    assert count([32, 32, 32], 2, -1, 2) == 0
    assert count([32, 32, 32], 1, -1, 2) == NBK_ERR_ARG   # span >= group
    assert count([32, 32, 32], 2, -1, 3) == NBK_ERR_ARG
    assert count([3, 32, 32], 3, 0, 1) == NBK_ERR_ARG     # odd n0
    assert count([32, 48, 32], 5, 0, 1) == NBK_ERR_ARG    # n1 % group


def test_count_matrix_steps_reject_bad_arguments(lib):
    """chunk < 1, n >= 2^31 and, for the pair scatter, the geometries
    its count step rejects: NBK_ERR_ARG, nothing launched.  Every
    particle sits in cell (0, 0, .) and `bases` is all zero, so a scatter
    step that did run would stay inside the 2000-row outputs."""
    n = 1000
    pos = numpy.full((n, 3), 0.1)
    pos[:, 2] = numpy.linspace(0., BOX[2], n, endpoint=False)
    pos_t = dev(pos)
    mat = filled(40960, -7, torch.int32)
    bases = filled(40960, 0, torch.int32)
    out, out_m = nan_f64(3 * 2 * n), nan_f64(2 * n)
    bx = hiplib.f64_arr(BOX)
    n32 = hiplib.i64_arr(MESHES['n32'])
    ys = _two_level_ys(SimpleNamespace(Nmesh=MESHES['n32']))

    def xcount(n, chunk):
        return lib.nbk_xsort_count_f64(
            hiplib.dptr(pos_t), n, chunk, n32, bx, ys, hiplib.dptr(mat),
            None, None)

    def xscatter(n, chunk):
        return lib.nbk_xsort_scatter_f64(
            hiplib.dptr(pos_t), None, n, chunk, n32, bx, ys,
            hiplib.dptr(bases), hiplib.dptr(out), None, None)

    def pcount(n, chunk):
        return lib.nbk_psort_count_f64(
            hiplib.dptr(pos_t), n, chunk, n32, bx, PAIR_TEST_GS, 0, 1,
            hiplib.dptr(mat), None)

    def pscatter(n, chunk, nmesh=MESHES['n32'], gs=PAIR_TEST_GS, dlo=0,
                 dhi=1):
        return lib.nbk_psort_scatter_f64(
            hiplib.dptr(pos_t), None, n, chunk, hiplib.i64_arr(nmesh), bx,
            gs, dlo, dhi, hiplib.dptr(bases), 2 * n, hiplib.dptr(out),
            hiplib.dptr(out_m), None)

    for fn, name in [(xcount, 'nbk_xsort_count_f64'),
                     (xscatter, 'nbk_xsort_scatter_f64'),
                     (pcount, 'nbk_psort_count_f64'),
                     (pscatter, 'nbk_psort_scatter_f64')]:
        for bad_n, bad_chunk in [(n, 0), (2 ** 31, 4096)]:
            assert fn(bad_n, bad_chunk) == NBK_ERR_ARG, (name, bad_n)
            assert name in lib.nbk_last_error_string().decode()

    # the geometries of test_pair_sort_rejects_bad_geometry
    for nmesh, gs, dlo, dhi in [([32, 32, 32], 1, -1, 2),
                                ([32, 32, 32], 2, -1, 3),
                                ([3, 32, 32], 3, 0, 1),
                                ([32, 48, 32], 5, 0, 1)]:
        assert pscatter(n, 4096, nmesh, gs, dlo, dhi) == NBK_ERR_ARG, \
            (nmesh, gs, dlo, dhi)
        assert 'nbk_psort_scatter_f64' in lib.nbk_last_error_string().decode()

    # nothing was launched: the outputs are as they were
    assert (host(mat) == -7).all()
    assert numpy.isnan(host(out)).all() and numpy.isnan(host(out_m)).all()


# ---- (f) nbk_paint_gather_f64 vs oracle.paint ---------------------------

def run_gather(lib, s, nmesh, window, shift, x0=0, nx=None, accumulate=0,
               mesh_t=None):
    nm, bx = geom_args(nmesh)
    nx = nmesh[0] if nx is None else nx
    if mesh_t is None:
        mesh_t = nan_f64(nx * nmesh[1] * nmesh[2])
    hiplib.check(lib.nbk_paint_gather_f64(
        hiplib.dptr(s.pos), hiplib.dptr(s.mass), s.n, nm, bx,
        hiplib.WINDOW_IDS[window], shift, hiplib.dptr(s.table),
        hiplib.dptr(mesh_t), x0, nx, accumulate, s.pair_gs, None),
        'paint_gather')
    return mesh_t


@pytest.mark.parametrize('mode', ['row', 'pair'])
@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('cat', list(ref.CATALOGUES))
@pytest.mark.parametrize('mesh', list(MESHES))
def test_gather_paint_matches_oracle(lib, mesh, cat, window, shift, mode):
    """Every window x shift x table mode x mesh x catalogue.  The thin
    meshes pin the source-plane walk: a tile reads P + span consecutive
    planes, and where the mesh has fewer ('thin4', 'thin8', 'pair2' for
    TSC, PCS and shifted CIC in row-table mode) an unbounded walk
    deposits the revisited planes twice — relative errors of 1 to 2.
    In pair mode 'thin4' is the case: 4 planes walked from an odd one
    visit pairs q, q', q', q."""
    nmesh = MESHES[mesh]
    s = sorted_table(mesh, cat, mode, window, shift != 0.0)
    got = host(run_gather(lib, s, nmesh, window, shift)).reshape(nmesh)
    want = oracle_mesh(mesh, cat, window, shift)
    assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert_allclose(got.sum(), total_mass(mesh, cat), rtol=1e-12)


@pytest.mark.parametrize('window', ref.WINDOWS)
def test_gather_paint_pair_interlaced_table_serves_both_shifts(lib, window):
    # the interlaced ghost row feeds ONE sorted array to both paints
    nmesh = MESHES['thin8']
    s = sorted_table('thin8', 'edge', 'pairmax', window, True)
    for shift in (0.0, 0.5):
        got = host(run_gather(lib, s, nmesh, window, shift)).reshape(nmesh)
        assert_allclose(got, oracle_mesh('thin8', 'edge', window, shift),
                        rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('mode', ['row', 'pair', 'pairmax'])
@pytest.mark.parametrize('window', ref.WINDOWS)
def test_gather_paint_accumulates(lib, window, mode):
    nmesh = MESHES['thin8']
    s = sorted_table('thin8', 'edge', mode, window, False)
    mesh_t = filled(nmesh[0] * nmesh[1] * nmesh[2], 0.0, torch.float64)
    for _ in range(2):
        run_gather(lib, s, nmesh, window, 0.0, accumulate=1, mesh_t=mesh_t)
    assert_allclose(host(mesh_t).reshape(nmesh),
                    2 * oracle_mesh('thin8', 'edge', window, 0.0),
                    rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('mode', ['row', 'pair'])
@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('window', ref.WINDOWS)
def test_gather_paint_slab_halves(lib, window, shift, mode):
    nmesh = MESHES['thin8']
    s = sorted_table('thin8', 'edge', mode, window, shift != 0.0)
    half = nmesh[0] // 2
    parts = [host(run_gather(lib, s, nmesh, window, shift, x0=x0, nx=half))
             for x0 in (0, half)]
    got = numpy.concatenate(parts).reshape(nmesh)
    assert_allclose(got, oracle_mesh('thin8', 'edge', window, shift),
                    rtol=1e-12, atol=1e-12)


# ---- (g) nbk_paint_gather_fft_f64 vs the oracle's z transform -----------

@pytest.mark.parametrize('mode', ['row', 'pair', 'pairmax'])
@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('window', ['cic', 'tsc'])
@pytest.mark.parametrize('mesh', ['n32', 'thin4'])
def test_gather_paint_fft_matches_oracle(lib, mesh, window, shift, mode):
    nmesh = MESHES[mesh]
    n0, n1, n2 = nmesh
    nm, bx = geom_args(nmesh)
    s = sorted_table(mesh, 'edge', mode, window, shift != 0.0)
    scale = 1.0 / (n0 * n1 * n2)
    nzh = n2 // 2 + 1
    zspec = torch.full((n0, n1, nzh), complex('nan'),
                       dtype=torch.complex128, device=DEVICE)
    hiplib.check(lib.nbk_paint_gather_fft_f64(
        hiplib.dptr(s.pos), hiplib.dptr(s.mass), s.n, nm, bx,
        hiplib.WINDOW_IDS[window], shift, hiplib.dptr(s.table),
        hiplib.dptr(zspec), 0, n0, scale, s.pair_gs, None),
        'paint_gather_fft')
    got = host(zspec)
    # the z stage of oracle.r2c (rfftn = rfft along z, then y, x), with
    # the 1/Ntotal normalisation passed as `scale`
    want = numpy.fft.rfft(oracle_mesh(mesh, 'edge', window, shift),
                          axis=2) * scale
    err = numpy.abs(got - want).max(axis=2)
    assert numpy.isfinite(err).all()
    assert (err <= 1e-12 * numpy.abs(want).max(axis=2)).all(), \
        (err / numpy.abs(want).max(axis=2)).max()


# ---- (h) the scatter paints on the same edge catalogues -----------------

def run_scatter_paint(lib, fn, pos, mass, nmesh, window, shift):
    nm, bx = geom_args(nmesh)
    pos_soa = dev(pos).t().contiguous()
    mass_t = None if mass is None else dev(mass)
    mesh_t = filled(nmesh[0] * nmesh[1] * nmesh[2], 0.0, torch.float64)
    hiplib.check(fn(
        hiplib.dptr(pos_soa), hiplib.dptr(mass_t), len(pos), nm, bx,
        hiplib.WINDOW_IDS[window], shift, hiplib.dptr(mesh_t), 0,
        nmesh[0], None), 'paint')
    return host(mesh_t).reshape(nmesh)


@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('cat', list(ref.CATALOGUES))
@pytest.mark.parametrize('mesh', list(MESHES))
def test_scatter_paint_edges_match_oracle(lib, mesh, cat, window, shift):
    pos, mass = catalogue(mesh, cat)
    got = run_scatter_paint(lib, lib.nbk_paint_f64, pos, mass,
                            MESHES[mesh], window, shift)
    assert_allclose(got, oracle_mesh(mesh, cat, window, shift),
                    rtol=1e-12, atol=1e-12)
    assert_allclose(got.sum(), total_mass(mesh, cat), rtol=1e-12)


@pytest.mark.parametrize('order', ['sorted', 'unsorted'])
@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('cat', list(ref.CATALOGUES))
@pytest.mark.parametrize('mesh', list(MESHES))
def test_sorted_paint_edges_match_oracle(lib, mesh, cat, window, shift,
                                         order):
    """nbk_paint_sorted_f64 wants cell-ordered input but documents a
    correct (slower) fallback for blocks whose particles are spread
    out: unsorted input must give the same mesh."""
    nmesh = MESHES[mesh]
    pos, mass = catalogue(mesh, cat)
    if order == 'sorted':
        o = numpy.argsort(ref.cell_ids(pos, nmesh, BOX), kind='stable')
        pos = pos[o]
        mass = None if mass is None else mass[o]
    got = run_scatter_paint(lib, lib.nbk_paint_sorted_f64, pos, mass,
                            nmesh, window, shift)
    assert_allclose(got, oracle_mesh(mesh, cat, window, shift),
                    rtol=1e-12, atol=1e-12)


# ---- (i) nbk_readout_f64 vs oracle.readout ------------------------------

# 'nnb' (nearest grid point) exists for the readout only
READOUT_IDS = dict(hiplib.WINDOW_IDS, nnb=3)


@functools.lru_cache(maxsize=None)
def readout_values(mesh):
    values = numpy.random.RandomState(211).normal(size=MESHES[mesh])
    values.setflags(write=False)
    return values


@functools.lru_cache(maxsize=None)
def oracle_readout(mesh, cat, window):
    pos, _ = catalogue(mesh, cat)
    want = readout(pos, readout_values(mesh),
                   MeshGeometry(MESHES[mesh], BOX), resampler=window)
    want.setflags(write=False)
    return want


def readout_comparable(pos, nmesh, window):
    """Mask of the particles the oracle and the kernel must agree on.
    The B-spline windows are continuous: all of them.  nnb is a step
    function of the mesh coordinate, which the oracle computes as
    x / H and the kernel as x * (N / L); where the two round to
    different sides of a half-cell boundary they legitimately read
    different cells, so those particles are left out — a condition on
    the input, worked out from the two reference expressions alone."""
    if window != 'nnb':
        return numpy.ones(len(pos), dtype=bool)
    N = numpy.asarray(nmesh, dtype='f8')
    L = numpy.asarray(BOX, dtype='f8')
    keep = (numpy.floor(pos * (N / L) + 0.5)
            == numpy.floor(pos / (L / N) + 0.5)).all(axis=1)
    assert (~keep).mean() <= 1.0 / 8
    return keep


def run_readout(lib, pos, values, nmesh, window, x0=0, nx=None):
    nm, bx = geom_args(nmesh)
    nx = nmesh[0] if nx is None else nx
    pos_soa = dev(pos).t().contiguous()
    values_t = dev(values[x0:x0 + nx])
    out = nan_f64(len(pos))
    hiplib.check(lib.nbk_readout_f64(
        hiplib.dptr(pos_soa), len(pos), nm, bx, READOUT_IDS[window],
        hiplib.dptr(values_t), x0, nx, hiplib.dptr(out), None), 'readout')
    return host(out)


@pytest.mark.parametrize('window', list(READOUT_IDS))
@pytest.mark.parametrize('cat', list(ref.CATALOGUES))
@pytest.mark.parametrize('mesh', list(MESHES))
def test_readout_edges_match_oracle(lib, mesh, cat, window):
    nmesh = MESHES[mesh]
    pos, _ = catalogue(mesh, cat)
    keep = readout_comparable(pos, nmesh, window)
    got = run_readout(lib, pos, readout_values(mesh), nmesh, window)
    assert_allclose(got[keep], oracle_readout(mesh, cat, window)[keep],
                    rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('window', list(READOUT_IDS))
def test_readout_slab_halves(lib, window):
    """each half of the mesh contributes its partial (cells outside the
    slab read as 0); the partials sum to the full readout"""
    nmesh = MESHES['thin8']
    pos, _ = catalogue('thin8', 'edge')
    keep = readout_comparable(pos, nmesh, window)
    half = nmesh[0] // 2
    got = sum(run_readout(lib, pos, readout_values('thin8'), nmesh, window,
                          x0=x0, nx=half) for x0 in (0, half))
    assert_allclose(got[keep], oracle_readout('thin8', 'edge', window)[keep],
                    rtol=1e-12, atol=1e-12)


# ---- the driver on a thin mesh, end to end ------------------------------

@pytest.mark.parametrize('mode', ['real', 'complex'])
@pytest.mark.parametrize('window', ['tsc', 'pcs'])
def test_to_mesh_thin_mesh_matches_oracle(window, mode):
    """The thin-mesh plane walk through the public API: with the sort
    thresholds shrunk, to_mesh on the 8-plane mesh runs the two-level
    sort and the gather paint ('real') or its fused z-FFT variant
    ('complex'), whose TSC/PCS tile spans 11 source planes."""
    from nbodykit_amd import set_options
    from nbodykit_amd.lab import ArrayCatalog
    from oracle import r2c
    nmesh = MESHES['thin8']
    pos, mass = catalogue('thin8', 'edge')
    cat = ArrayCatalog({'Position': numpy.array(pos),
                        'Weight': numpy.array(mass)})
    with set_options(sort_min_n=1024, sort_two_level_min_n=1024,
                     sort_two_level_min_cells=1):
        field = cat.to_mesh(Nmesh=nmesh, BoxSize=list(BOX), dtype='f8',
                            resampler=window, compensated=False
                            ).compute(mode=mode)
    nbar = mass.sum() / float(numpy.prod(nmesh))        # 1 + delta
    want = oracle_mesh('thin8', 'edge', window, 0.0) / nbar
    got = field.value.cpu().numpy()
    if mode == 'real':
        assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    else:
        # the r2c bar of test_gpu_kernels.py
        assert_allclose(got, r2c(want), rtol=1e-11, atol=1e-13)
