"""
Range lengths against the batch structure of the gather paint's
software-pipelined particle loop (csrc/nbk_paint.hip, kpaint_gather).

The loop stages U particles per thread and trip (U * 1024 per block) and
issues the next batch's loads before it deposits the current one, across
the ranges a tile reads.  What can go wrong is tied to the LENGTH of a
range against that batch — a slot past the range's end deposited or
read, the last partial batch dropped, a batch of the next range consumed
with the previous range's end — so these tests sweep the lengths around
k * 1024 for every plausible U, with one, two and many ranges per tile,
at the smallest meshes that have them.  The sort kernels are not
involved: the sorted SoA array and its table are built with numpy
(sort_reference.py), and the device array holds exactly 3 * n_out
doubles, so the last range ends where the allocation ends.

Paints are compared with oracle.paint at the project's paint bar,
rtol = atol = 1e-12, and in total mass at rtol = 1e-12; the fused
z-spectrum with numpy.fft.rfft of the oracle mesh at the r2c bar of
1e-12 of each line's largest magnitude.  Outputs start NaN-filled, so a
cell the kernel never wrote shows up.  (The deposits are f64 atomic adds
in varying order: nothing is compared bit for bit.)
"""
import functools

import numpy
import pytest
from numpy.testing import assert_allclose

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import sort_reference as ref                                    # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402
from nbodykit_amd.source.mesh.catalog import _PAIR_GHOST        # noqa: E402
from oracle import MeshGeometry, paint                          # noqa: E402

DEVICE = 'cuda'

# non-dyadic, anisotropic: no invH is a power of two
BOX = (10.0, 100.0 / 3, 7.3)
PAIR_MESH = [4, 32, 32]
PAIR_GS = 3                     # 8-row groups: 2 pairs x 4 groups
ROW_MESH = [8, 64, 32]

# brackets U * 1024 and 2 * U * 1024 for every plausible batch size U
# without knowing U
SWEEP = (0, 1, 63, 64, 65) + tuple(
    k * 1024 + d for k in range(1, 10) for d in (-1, 0, 1))
TWO_RANGES = ((0, 4097), (4097, 0), (1, 1023), (1025, 4096), (3000, 3000))
ROW_SWEEP = (1, 1023, 1024, 1025, 4096, 4097, 8193)


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def dev(arr):
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- inputs and oracle results, computed once ---------------------------

def in_cells(rng, nmesh, lo, hi, n):
    """(n, 3) positions uniform over the cells [lo, hi) of each axis,
    kept 1e-3 of a cell off the two ends of the block"""
    H = numpy.asarray(BOX) / numpy.asarray(nmesh, dtype='f8')
    lo = numpy.asarray(lo, dtype='f8')
    hi = numpy.asarray(hi, dtype='f8')
    pos = (lo + 1e-3 + (hi - lo - 2e-3) * rng.uniform(size=(n, 3))) * H
    cells = ref.floor_index(pos, nmesh, BOX)
    assert (cells >= lo).all() and (cells < hi).all()
    return pos


@functools.lru_cache(maxsize=None)
def pair_case(lengths):
    """Particles of the pair-bucket cases: ``lengths`` = (L,) puts L
    particles in the LAST bucket (plane pair 1, row group 3: the range
    that ends the sorted array); (L1, L2) puts them in row group 1 of
    plane pairs 0 and 1.  Rows span the whole group, so the particles of
    its last row need the duplicated copy in the next group's bucket
    (about L/8 entries there; every other bucket is empty, and no copy
    comes INTO the buckets under test, whose lengths are exactly L)."""
    n0, n1, n2 = PAIR_MESH
    rg = 1 << PAIR_GS
    rng = numpy.random.RandomState(1000 + sum(lengths) + len(lengths))
    if len(lengths) == 1:
        blocks = [((2, n1 - rg, 0), (4, n1, n2), lengths[0])]
    else:
        blocks = [((0, rg, 0), (2, 2 * rg, n2), lengths[0]),
                  ((2, rg, 0), (4, 2 * rg, n2), lengths[1])]
    pos = numpy.concatenate([in_cells(rng, PAIR_MESH, lo, hi, L)
                             for lo, hi, L in blocks])
    mass = ref.masses(len(pos), seed=11)
    pos.setflags(write=False)
    mass.setflags(write=False)
    return pos, mass


@functools.lru_cache(maxsize=None)
def pair_sorted(lengths):
    """host-built pair-bucket sort: (SoA positions [3 * n_out], masses
    [n_out], bucket table [nbuck + 1] int32, n_out)"""
    pos, mass = pair_case(lengths)
    n0, n1, n2 = PAIR_MESH
    nbuck = (n0 >> 1) * (n1 >> PAIR_GS)
    dlo, dhi = _PAIR_GHOST[('cic', False)]
    k1, k2 = ref.pair_keys(pos, PAIR_MESH, BOX, PAIR_GS, dlo, dhi)
    dup = k2 >= 0
    keys = numpy.concatenate([k1, k2[dup]])
    order = numpy.argsort(keys, kind='stable')
    spos = numpy.concatenate([pos, pos[dup]])[order]
    smass = numpy.concatenate([mass, mass[dup]])[order]
    counts = numpy.bincount(keys, minlength=nbuck)
    table = numpy.concatenate([[0], numpy.cumsum(counts)]).astype('i4')
    # the buckets under test hold exactly the lengths asked for
    if len(lengths) == 1:
        assert counts[-1] == lengths[0] and table[-1] == len(spos)
        assert lengths[0] < 64 or dup.any()
    else:
        ng = n1 >> PAIR_GS
        assert (counts[1], counts[ng + 1]) == lengths
    return spos.T.ravel().copy(), smass, table, len(spos)


@functools.lru_cache(maxsize=None)
def row_case(L):
    """L particles in plane n0-1, row n1-1 (the row whose end is the row
    table's sentinel and the end of the array), z over the whole box"""
    n0, n1, n2 = ROW_MESH
    rng = numpy.random.RandomState(2000 + L)
    pos = in_cells(rng, ROW_MESH, (n0 - 1, n1 - 1, 0), (n0, n1, n2), L)
    mass = ref.masses(L, seed=12)
    rid = ref.row_ids(pos, ROW_MESH, BOX)
    assert (rid == n0 * n1 - 1).all()
    table = numpy.concatenate(
        [ref.row_table(rid, n0 * n1), [L]]).astype('i4')
    pos.setflags(write=False)
    mass.setflags(write=False)
    return pos, mass, table


@functools.lru_cache(maxsize=None)
def oracle_mesh(kind, key, weighted, window, shift):
    if kind == 'pair':
        pos, mass = pair_case(key)
        nmesh = PAIR_MESH
    else:
        pos, mass, _ = row_case(key)
        nmesh = ROW_MESH
    want = numpy.zeros(nmesh)
    paint(pos, mass if weighted else 1.0, want, MeshGeometry(nmesh, BOX),
          resampler=window, shift=shift)
    want.setflags(write=False)
    return want


def total_mass(kind, key, weighted):
    mass = (pair_case(key) if kind == 'pair' else row_case(key))[1]
    return mass.sum() if weighted else float(len(mass))


# ---- launchers ----------------------------------------------------------

def run_gather(lib, soa, mass, n, table, pair_gs, nmesh, window, shift):
    pos_t = dev(soa)
    assert pos_t.numel() == 3 * n          # the last range ends the array
    mass_t = None if mass is None else dev(mass)
    table_t = dev(table)
    mesh_t = torch.full((int(numpy.prod(nmesh)),), float('nan'),
                        dtype=torch.float64, device=DEVICE)
    hiplib.check(lib.nbk_paint_gather_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n, hiplib.i64_arr(nmesh),
        hiplib.f64_arr(BOX), hiplib.WINDOW_IDS[window], shift,
        hiplib.dptr(table_t), hiplib.dptr(mesh_t), 0, nmesh[0], 0, pair_gs,
        None), 'paint_gather')
    return host(mesh_t).reshape(nmesh)


def run_gather_fft(lib, soa, mass, n, table, pair_gs, nmesh, window, shift):
    n0, n1, n2 = nmesh
    pos_t = dev(soa)
    assert pos_t.numel() == 3 * n
    mass_t = None if mass is None else dev(mass)
    table_t = dev(table)
    scale = 1.0 / (n0 * n1 * n2)
    zspec = torch.full((n0, n1, n2 // 2 + 1), complex('nan'),
                       dtype=torch.complex128, device=DEVICE)
    hiplib.check(lib.nbk_paint_gather_fft_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n, hiplib.i64_arr(nmesh),
        hiplib.f64_arr(BOX), hiplib.WINDOW_IDS[window], shift,
        hiplib.dptr(table_t), hiplib.dptr(zspec), 0, n0, scale, pair_gs,
        None), 'paint_gather_fft')
    return host(zspec), scale


def check_paint(got, kind, key, weighted, window, shift):
    want = oracle_mesh(kind, key, weighted, window, shift)
    assert_allclose(got, want, rtol=1e-12, atol=1e-12)
    assert_allclose(got.sum(), total_mass(kind, key, weighted), rtol=1e-12)


def check_zspec(got, scale, want_mesh):
    want = numpy.fft.rfft(want_mesh, axis=2) * scale
    err = numpy.abs(got - want).max(axis=2)
    assert numpy.isfinite(err).all()
    bar = 1e-12 * numpy.abs(want).max(axis=2)
    assert (err <= bar).all(), (err - bar).max()


# ---- 1. single range, length sweep, pair mode ---------------------------

@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('L', SWEEP)
def test_pair_single_range_length_sweep(lib, L, weighted):
    soa, mass, table, n = pair_sorted((L,))
    got = run_gather(lib, soa, mass if weighted else None, n, table,
                     PAIR_GS, PAIR_MESH, 'cic', 0.0)
    check_paint(got, 'pair', (L,), weighted, 'cic', 0.0)


# ---- 2. two ranges per tile ---------------------------------------------

@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('lengths', TWO_RANGES)
def test_pair_two_ranges_per_tile(lib, lengths, weighted):
    """Even-plane tiles of the row group read both buckets back to back
    (planes p-1 and p lie in different pairs), odd-plane tiles one."""
    soa, mass, table, n = pair_sorted(lengths)
    got = run_gather(lib, soa, mass if weighted else None, n, table,
                     PAIR_GS, PAIR_MESH, 'cic', 0.0)
    check_paint(got, 'pair', lengths, weighted, 'cic', 0.0)


# ---- 3. row-table mode with wrapped intervals ---------------------------

def run_row_case(lib, L, weighted, window, shift):
    pos, mass, table = row_case(L)
    soa = pos.T.ravel().copy()            # one row: any order is sorted
    got = run_gather(lib, soa, mass if weighted else None, L, table, -1,
                     ROW_MESH, window, shift)
    check_paint(got, 'row', L, weighted, window, shift)


@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('shift', [0.0, 0.5])
@pytest.mark.parametrize('L', ROW_SWEEP)
def test_row_table_wrapped_interval_tsc(lib, L, shift, weighted):
    """Row n1-1 of plane n0-1: the tiles at the top and the bottom of
    the y axis reach it through a wrapped row interval (two ranges per
    source plane, one of them empty), from a multi-plane tile that walks
    the x wrap."""
    run_row_case(lib, L, weighted, 'tsc', shift)


def test_row_table_wrapped_interval_pcs(lib):
    run_row_case(lib, 4097, True, 'pcs', 0.0)


# ---- 4. fused paint + z-FFT on the same inputs --------------------------

@pytest.mark.parametrize('weighted', [True, False])
@pytest.mark.parametrize('lengths', [(0,), (1025,), (4097,), (0, 4097),
                                     (4097, 0), (1025, 4096)])
def test_pair_fused_fft(lib, lengths, weighted):
    soa, mass, table, n = pair_sorted(lengths)
    got, scale = run_gather_fft(lib, soa, mass if weighted else None, n,
                                table, PAIR_GS, PAIR_MESH, 'cic', 0.0)
    check_zspec(got, scale,
                oracle_mesh('pair', lengths, weighted, 'cic', 0.0))

