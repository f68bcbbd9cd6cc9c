"""
The fused z-FFT of the gather paint kernel (csrc/nbk_paint.hip,
kpaint_gather with DOFFT; zfft_row) at the C ABI, entry point
nbk_paint_gather_fft_f64.

Row lengths n2 = 128 ... 1024 take the register-resident radix-8
transform, one compile-time instance per length (m = n2/2 = R * 8 * 8
points, R = 1, 2, 4, 8 per lane in the first pass); every other length
keeps the LDS radix-4 network.  What can go wrong is an index of an
exchange, a twiddle of a lane, the lanes that idle below n2 = 1024, a
wave that transforms no row, one row or two rows with the same resident
twiddles, and the choice of the instance itself.  So the cases are

  * every length that takes the new routine (128 the smallest, 1024 the
    largest), and 64 and 2048 on the two sides of it, and 4096;
  * at n2 = 128, tiles of 8 rows (half the block's 16 waves idle), of 16
    rows, and a row-table TSC tile of 4 planes x 8 rows = 32 rows (two
    rows per wave);
  * one particle (each row is an impulse pair with a closed-form
    spectrum, every other row exactly 0), one occupied row among empty
    ones, a dense random fill, and masses once.

The sort kernels are not involved: the sorted SoA array and its table
are built with numpy (sort_reference.py).  The z-spectrum is compared
with numpy.fft.rfft of the oracle paint at the r2c bar of
tests/test_gpu_paint_pipeline.py, 1e-12 of each line's largest
magnitude; a line whose mesh row is empty has bar 0 and must be exactly
0.  The k = 0 and the Nyquist bin are also checked on their own against
the row's plain and alternating sums.  Outputs start NaN-filled, so a
bin the kernel never wrote shows up.
"""
import functools

import numpy
import pytest

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

# n2 of the register-resident instances, and of the LDS network around
NEW_PATH = (128, 256, 512, 1024)
FALLBACK = (64, 2048, 4096)


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def dev(arr):
    return torch.as_tensor(numpy.array(arr, order='C')).to(DEVICE)


# ---- inputs, sorted arrays and oracle results, computed once -------------

@functools.lru_cache(maxsize=None)
def particles(kind, nmesh):
    """positions (n, 3) and masses (n,) of one content kind"""
    n0, n1, n2 = nmesh
    H = numpy.asarray(BOX) / numpy.asarray(nmesh, dtype='f8')
    rng = numpy.random.RandomState(n2 + 7 * n1 + len(kind))
    if kind == 'dense':
        pos = rng.uniform(size=(6000, 3)) * numpy.asarray(BOX)
    elif kind == 'one':
        # last z cell: the impulse pair wraps to z = 0
        pos = (numpy.array([[1, n1 - 3, n2 - 1]]) + [0.25, 0.625, 0.3]) * H
    elif kind == 'row':
        # every particle in plane 2, row 5; z over the whole box
        pos = (numpy.array([2, 5, 0])
               + rng.uniform(0.01, 0.99, size=(3000, 3)) * [1, 1, n2]) * H
    else:
        raise ValueError(kind)
    mass = ref.masses(len(pos), seed=13)
    pos.setflags(write=False)
    mass.setflags(write=False)
    return pos, mass


@functools.lru_cache(maxsize=None)
def pair_sorted(kind, nmesh, gs):
    """host-built pair-bucket sort of CIC: (SoA positions [3 * n_out],
    masses [n_out], bucket table [nbuck + 1] int32, n_out)"""
    pos, mass = particles(kind, nmesh)
    n0, n1, n2 = nmesh
    nbuck = (n0 >> 1) * (n1 >> gs)
    dlo, dhi = _PAIR_GHOST[('cic', False)]
    k1, k2 = ref.pair_keys(pos, nmesh, BOX, gs, dlo, dhi)
    dup = k2 >= 0
    keys = numpy.concatenate([k1, k2[dup]])
    order = numpy.argsort(keys, kind='stable')
    spos = numpy.concatenate([pos, pos[dup]])[order]
    smass = numpy.concatenate([mass, mass[dup]])[order]
    counts = numpy.bincount(keys, minlength=nbuck)
    table = numpy.concatenate([[0], numpy.cumsum(counts)]).astype('i4')
    return spos.T.ravel().copy(), smass, table, len(spos)


@functools.lru_cache(maxsize=None)
def row_sorted(kind, nmesh):
    """host-built row sort: (SoA positions, masses, row table with its
    sentinel [n0 * n1 + 1] int32, n)"""
    pos, mass = particles(kind, nmesh)
    n0, n1, n2 = nmesh
    rid = ref.row_ids(pos, nmesh, BOX)
    order = numpy.argsort(rid, kind='stable')
    table = numpy.concatenate(
        [ref.row_table(rid[order], n0 * n1), [len(pos)]]).astype('i4')
    return pos[order].T.ravel().copy(), mass[order], table, len(pos)


@functools.lru_cache(maxsize=None)
def oracle_mesh(kind, nmesh, weighted, window):
    pos, mass = particles(kind, nmesh)
    want = numpy.zeros(nmesh)
    paint(pos, mass if weighted else 1.0, want, MeshGeometry(nmesh, BOX),
          resampler=window, shift=0.0)
    want.setflags(write=False)
    return want


# ---- launcher and checks -------------------------------------------------

def run_gather_fft(lib, soa, mass, n, table, pair_gs, nmesh, window):
    n0, n1, n2 = nmesh
    pos_t = dev(soa)
    assert pos_t.numel() == 3 * n
    mass_t = None if mass is None else dev(mass)
    table_t = dev(table)
    scale = 1.0 / (n0 * n1 * n2)
    zspec = torch.full((n0, n1, n2 // 2 + 1), complex('nan'),
                       dtype=torch.complex128, device=DEVICE)
    hiplib.check(lib.nbk_paint_gather_fft_f64(
        hiplib.dptr(pos_t), hiplib.dptr(mass_t), n,
        hiplib.i64_arr(list(nmesh)), hiplib.f64_arr(BOX),
        hiplib.WINDOW_IDS[window], 0.0, hiplib.dptr(table_t),
        hiplib.dptr(zspec), 0, n0, scale, pair_gs, None),
        'paint_gather_fft')
    torch.cuda.synchronize()
    return zspec.cpu().numpy(), scale


def check_zspec(got, scale, want_mesh):
    """rfft bar on every line; exact zeros on empty lines; the k = 0 and
    Nyquist bins against the row sums"""
    want = numpy.fft.rfft(want_mesh, axis=2) * scale
    bar = 1e-12 * numpy.abs(want).max(axis=2)
    err = numpy.abs(got - want).max(axis=2)
    assert numpy.isfinite(err).all()
    print('largest err / bar: %.3g' % (err[bar > 0] / bar[bar > 0]).max())
    assert (err <= bar).all(), (err - bar).max()
    assert (got[~want_mesh.any(axis=2)] == 0).all()
    n2 = want_mesh.shape[2]
    sign = 1.0 - 2.0 * (numpy.arange(n2) % 2)
    dc = want_mesh.sum(axis=2) * scale
    ny = (want_mesh * sign).sum(axis=2) * scale
    assert (numpy.abs(got[:, :, 0] - dc) <= bar).all()
    assert (numpy.abs(got[:, :, n2 // 2] - ny) <= bar).all()


def pair_run(lib, kind, nmesh, gs, weighted):
    soa, mass, table, n = pair_sorted(kind, nmesh, gs)
    got, scale = run_gather_fft(lib, soa, mass if weighted else None, n,
                                table, gs, nmesh, 'cic')
    check_zspec(got, scale, oracle_mesh(kind, nmesh, weighted, 'cic'))
    return got, scale


# ---- 1. every length, dense fill -----------------------------------------

@pytest.mark.parametrize('n2', NEW_PATH + FALLBACK)
def test_lengths_dense(lib, n2):
    """[4, 32, n2], pair mode, 8-row tiles (4-row at n2 = 4096, where 8
    rows do not fit the LDS): the four register-resident instances and
    the LDS network on both sides of them"""
    pair_run(lib, 'dense', (4, 32, n2), 3 if n2 < 4096 else 2, False)


def test_weighted_dense(lib):
    pair_run(lib, 'dense', (4, 32, 1024), 3, True)


# ---- 2. rows per tile against the 16 waves of a block --------------------

def test_rows_16_per_tile(lib):
    """pair mode, gs = 4: 16 rows, one per wave (gs = 3, 8 rows and half
    the waves idle, is test_lengths_dense[128])"""
    pair_run(lib, 'dense', (4, 32, 128), 4, False)


@pytest.mark.parametrize('weighted', [False, True])
def test_rows_32_per_tile_row_table(lib, weighted):
    """row-table TSC on [4, 8, 128]: the launcher's tile is all 4 planes
    x all 8 rows, so every wave transforms two rows with the twiddles it
    loaded once"""
    nmesh = (4, 8, 128)
    soa, mass, table, n = row_sorted('dense', nmesh)
    got, scale = run_gather_fft(lib, soa, mass if weighted else None, n,
                                table, -1, nmesh, 'tsc')
    check_zspec(got, scale, oracle_mesh('dense', nmesh, weighted, 'tsc'))


# ---- 3. content that singles out index errors ----------------------------

@pytest.mark.parametrize('n2', NEW_PATH)
def test_one_particle_closed_form(lib, n2):
    """One particle of unit mass: the four rows it reaches hold the
    impulse pair w * (1 - f) at iz and w * f at iz + 1 (wrapped), whose
    spectrum is w * ((1 - f) W^(k iz) + f W^(k (iz + 1))),
    W = exp(-2 pi i / n2); every other row is exactly 0."""
    nmesh = (4, 32, n2)
    got, scale = pair_run(lib, 'one', nmesh, 3, False)
    pos, _ = particles('one', nmesh)
    u = pos[0] * ref.inv_h(nmesh, BOX)
    i = numpy.floor(u).astype('i8')
    f = u - i
    k = numpy.arange(n2 // 2 + 1)
    W = lambda e: numpy.exp(-2j * numpy.pi * ((k * e) % n2) / n2)
    line = (1 - f[2]) * W(i[2]) + f[2] * W(i[2] + 1)
    want = numpy.zeros_like(got)
    for dx, wx in ((0, 1 - f[0]), (1, f[0])):
        for dy, wy in ((0, 1 - f[1]), (1, f[1])):
            want[(i[0] + dx) % 4, (i[1] + dy) % 32] = wx * wy * scale * line
    err = numpy.abs(got - want).max(axis=2)
    bar = 1e-12 * numpy.abs(want).max(axis=2)
    assert (err <= bar).all(), (err - bar).max()
    assert (bar > 0).sum() == 4


@pytest.mark.parametrize('n2', (128, 1024))
def test_one_occupied_row(lib, n2):
    """3000 particles in one (plane, row) of cells: CIC reaches 2 planes
    x 2 rows, the other 124 lines are exactly 0 (check_zspec)"""
    nmesh = (4, 32, n2)
    pair_run(lib, 'row', nmesh, 3, False)
    assert oracle_mesh('row', nmesh, False, 'cic').any(axis=2).sum() == 4
