"""
Kernel-level tests of the FFT passes and the k-space kernels through the C
ABI, at every launch branch their launchers take.

A. nbk_fft_r2c_z, nbk_fft_c2r_z, nbk_fft_c_strided and pm.fft_axis1
   (Bluestein on the same kernels) against numpy.fft in LONG DOUBLE
   (kspace_reference.fft_ref), at every length 8..4096.
B. nbk_bin_power_f64 / nbk_power_bin_f64 (all four binning kernels) and the
   elementwise kernels against kspace_reference.bin_sums_ref: the raw
   [xsum|musum|Nsum|ysum] block, unfolded, under every layout.
C. nbk_fft_x_bin_f64 at every tile width, register cap, LDS raise, chunked
   grid, slab offset and rejection.

FFT error measure: e = max|got - want| / rms(want) per call, asserted as
e <= C * eps * log2(N), eps = 2^-52.  C per kernel is the smallest power of
two that is at least twice the worst e / (eps log2 N) measured on an MI355X
(a radix-4 network with host-computed table twiddles; numpy's own f64
transform measures 0.3 against the same reference):

    e / (eps log2 N), the worse of the two signs where there are two:
    N                      8    16    32    64   128   256   512  1024  2048  4096   worst   C
    r2c_z               0.25  0.24  0.47  0.49  0.46  0.40  0.63  0.53  0.77  0.62   0.77    2
    c2r_z               0.20  0.35  0.40  0.46  0.58  0.81  0.67  0.70  0.77  0.87   0.87    2
    c_strided ni=5      0.47  0.40  0.41  0.76  0.71  0.67  0.63  0.78  0.95  0.75   0.95    2
    c_strided ni=1,3    0.51     -     -  0.64     -     -     -     -  0.75  0.78   0.78    2
    Bluestein, N = the convolution length M (r2c/c2r include the untwiddle;
    Bluestein is three transforms and two chirps, hence its own C):
    n (M)           12 (32)   27 (64)   96 (256)   1500 (4096)   worst   C
    forward          1.082     1.251      1.059         1.173
    inverse          1.252     1.139      0.844         1.245    1.252   4
    No C is above 8: none of the passes is far from pocketfft's 0.3, and
    the ratio does not grow with N as a twiddle recurrence (eps N) would.

Bin sums: integer counts exactly equal; each float sum within
n_terms * eps * abs_sum of the long-double sum of the same f64 terms (the
reordering bound of a sum of n_terms terms whose magnitudes add to abs_sum),
rows 0..Nx; the overflow row Nx+1 exactly zero (the kernels skip
k2 >= last edge).
"""
import math
import os

import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import kspace_reference as ref                                  # noqa: E402
from kspace_reference import EPS, LD                            # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402

NBK_ERR_ARG = -2
NBK_ERR_UNSUPPORTED = -3

# e <= C * eps * log2(N) per kernel (see the table above)
C_R2C = 2.0
C_C2R = 2.0
C_STRIDED = 2.0
C_BLUESTEIN = 4.0


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


def dev(arr):
    # a fresh contiguous copy: the shared fields are read-only arrays
    return torch.as_tensor(numpy.array(arr, order='C')).to('cuda')


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def crandn(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def skip_if_env(*names):
    """The library reads these overrides once into statics; a test whose
    point is a launch branch they move cannot run under one (and never
    sets one itself)."""
    for name in names:
        if os.environ.get(name):
            pytest.skip('%s is set: it overrides the launch branch this '
                        'test is about' % name)


FFT_ENV = ('NBK_FFT_TI', 'NBK_FFT_BLOCK')
XBIN_ENV = ('NBK_XBIN_TI', 'NBK_XBIN_GRID', 'NBK_XBIN_PHASES')


# =========================================================================
# A. FFT passes
# =========================================================================

LENGTHS = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096]


def fft_error(got, want):
    want = numpy.asarray(want)
    d = numpy.abs(numpy.asarray(got, dtype=want.dtype) - want).max()
    rms = numpy.sqrt(numpy.mean(numpy.abs(want) ** 2))
    return float(d / rms)


def check_fft(name, n, got, want, C):
    e = fft_error(got, want)
    unit = EPS * math.log2(n)
    print('FFTERR %s N=%d e=%.3e e/(eps log2 N)=%.3f C=%g'
          % (name, n, e, e / unit, C))
    assert e <= C * unit, (name, n, e / unit)


@pytest.mark.parametrize('n', LENGTHS)
def test_r2c_z_matches_long_double(lib, n):
    x = numpy.random.RandomState(100 + n).normal(size=(3, n))
    out_t = torch.zeros((3, n // 2 + 1), dtype=torch.complex128,
                        device='cuda')
    x_t = dev(x)
    hiplib.check(lib.nbk_fft_r2c_z(hiplib.dptr(x_t), hiplib.dptr(out_t),
                                   3, n, 0.37, None), 'r2c')
    check_fft('r2c_z', n, host(out_t), ref.rfft_ref(x) * LD(0.37), C_R2C)


def test_r2c_z_no_lines_leaves_output(lib):
    out = crandn(numpy.random.RandomState(1), (2, 9))
    out_t, x_t = dev(out), dev(numpy.zeros(16))
    assert lib.nbk_fft_r2c_z(hiplib.dptr(x_t), hiplib.dptr(out_t), 0, 16,
                             0.37, None) == 0
    assert_array_equal(host(out_t), out)


@pytest.mark.parametrize('n', LENGTHS)
def test_c2r_z_matches_long_double(lib, n):
    """a half-spectrum of its own, not r2c's output (a round trip cannot
    see an error common to both directions), whose DC and Nyquist entries
    carry imaginary parts that c2r must drop"""
    X = crandn(numpy.random.RandomState(200 + n), (3, n // 2 + 1))
    assert numpy.abs(X[:, 0].imag).min() > 0
    assert numpy.abs(X[:, -1].imag).min() > 0
    out_t = torch.zeros((3, n), dtype=torch.float64, device='cuda')
    X_t = dev(X)
    hiplib.check(lib.nbk_fft_c2r_z(hiplib.dptr(X_t), hiplib.dptr(out_t),
                                   3, n, None), 'c2r')
    check_fft('c2r_z', n, host(out_t), ref.irfft_ref(X, n), C_C2R)


STRIDED_CASES = [(n, 5) for n in LENGTHS] \
    + [(n, ni) for n in (8, 64, 2048, 4096) for ni in (1, 3)]


@pytest.mark.parametrize('sign', [-1, 1])
@pytest.mark.parametrize('n,n_inner', STRIDED_CASES)
def test_c_strided_matches_long_double(lib, n, n_inner, sign):
    """a (2, n, 7) buffer of which only the first n_inner columns are
    transformed: the column tile is 4, narrowed to 2 at n = 2048 and 1 at
    4096 and clamped to n_inner below 4, with a partial last tile at 5"""
    if n >= 2048 or n_inner < 4:
        skip_if_env(*FFT_ENV)
    x = crandn(numpy.random.RandomState(300 + n + n_inner), (2, n, 7))
    x_t = dev(x)
    hiplib.check(lib.nbk_fft_c_strided(hiplib.dptr(x_t), n, 7, 2, 7 * n,
                                       n_inner, sign, None), 'strided')
    got = host(x_t)
    assert_array_equal(got[:, :, n_inner:], x[:, :, n_inner:])
    check_fft('c_strided[%+d,ni=%d]' % (sign, n_inner), n,
              got[:, :, :n_inner],
              ref.fft_ref(x[:, :, :n_inner], 1, sign), C_STRIDED)


def _fft3d_passes(lib, cplx_t, n0, n1, nzh, sign):
    # forward: y then x; inverse: x then y
    passes = [(n1, nzh, n0, n1 * nzh, nzh), (n0, n1 * nzh, 1, 0, n1 * nzh)]
    if sign > 0:
        passes.reverse()
    for nfft, stride, n_outer, ostride, n_inner in passes:
        hiplib.check(lib.nbk_fft_c_strided(
            hiplib.dptr(cplx_t), nfft, stride, n_outer, ostride, n_inner,
            sign, None), 'strided')


def test_fft3d_noncubic_composition(lib):
    """(16, 8, 64) through the z, y, x passes against the long-double
    rfftn, and the inverse chain against the long-double inverse of ITS
    OWN input.  The passes' bounds add: each is relative to the rms, which
    the other (unitary up to scale) passes carry along."""
    n0, n1, n2 = 16, 8, 64
    nzh = n2 // 2 + 1
    unit = EPS * (C_R2C * math.log2(n2) + C_STRIDED * math.log2(n1)
                  + C_STRIDED * math.log2(n0))
    rng = numpy.random.RandomState(41)
    x = rng.normal(size=(n0, n1, n2))
    scale = 1.0 / (n0 * n1 * n2)
    want = ref.fft_ref(ref.fft_ref(ref.rfft_ref(x) * LD(scale), 1, -1),
                       0, -1)
    assert_allclose(want.astype('c16'), numpy.fft.rfftn(x) * scale,
                    rtol=0, atol=1e-13)          # the reference composes
    x_t = dev(x)
    c_t = torch.zeros((n0, n1, nzh), dtype=torch.complex128, device='cuda')
    hiplib.check(lib.nbk_fft_r2c_z(hiplib.dptr(x_t), hiplib.dptr(c_t),
                                   n0 * n1, n2, scale, None), 'z')
    _fft3d_passes(lib, c_t, n0, n1, nzh, -1)
    e = fft_error(host(c_t), want)
    print('FFTERR fft3d forward e=%.3e bound=%.3e' % (e, unit))
    assert e <= unit

    H = crandn(rng, (n0, n1, nzh))
    want = ref.irfft_ref(ref.fft_ref(ref.fft_ref(H, 0, +1), 1, +1), n2)
    h_t = dev(H)
    r_t = torch.zeros((n0, n1, n2), dtype=torch.float64, device='cuda')
    _fft3d_passes(lib, h_t, n0, n1, nzh, +1)
    hiplib.check(lib.nbk_fft_c2r_z(hiplib.dptr(h_t), hiplib.dptr(r_t),
                                   n0 * n1, n2, None), 'zi')
    unit = EPS * (C_C2R * math.log2(n2) + C_STRIDED * math.log2(n1)
                  + C_STRIDED * math.log2(n0))
    e = fft_error(host(r_t), want)
    print('FFTERR fft3d inverse e=%.3e bound=%.3e' % (e, unit))
    assert e <= unit


@pytest.mark.parametrize('sign', [-1, 1])
@pytest.mark.parametrize('n', [12, 27, 96, 1500])
def test_bluestein_axis1_matches_long_double(lib, n, sign):
    """pm.fft_axis1 at lengths that are no power of two: a chirp, three
    power-of-two transforms of length M >= 2n - 1 (4096 at n = 1500) and a
    second chirp; the error unit takes N = M."""
    from nbodykit_amd.pm import fft_axis1
    M = 8
    while M < 2 * n - 1:
        M *= 2
    x = crandn(numpy.random.RandomState(400 + n), (2, n, 3))
    x_t = dev(x)
    fft_axis1(x_t, sign, hiplib.cur_stream())
    check_fft('bluestein[%+d,n=%d]' % (sign, n), M, host(x_t),
              ref.fft_ref(x, 1, sign), C_BLUESTEIN)


# =========================================================================
# B. binning and elementwise kernels
# =========================================================================

BOX = (32., 30., 25.)
LOSES = {'z': (0., 0., 1.), 'x': (1., 0., 0.),
         'tilt': (1. / 3, 2. / 3, 2. / 3)}
POLES = [[0], [0, 2, 4], [0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6, 7]]


def nyquist(nmesh, box):
    return min(numpy.pi * n / b for n, b in zip(nmesh, box))


def make_edges(nmesh, box, nk, nmu, real_field=False, last=0.6):
    """kmin > 0 (row 0 fills) and a last edge at ``last`` of the smallest
    Nyquist (half the smallest box side for a real field)"""
    top = last * (0.5 * min(box) if real_field else nyquist(nmesh, box))
    xedges = numpy.linspace(0.07 * top, top, nk + 1)
    muedges = numpy.linspace(0 if real_field else -1, 1, nmu + 1)
    return xedges ** 2, muedges


@pytest.fixture(scope='module')
def fields():
    """the fields of section B, made once and never written to"""
    rng = numpy.random.RandomState(77)
    out = {
        'even': ((10, 7, 12), BOX, crandn(rng, (10, 7, 7))),
        'odd': ((10, 7, 9), BOX, crandn(rng, (10, 7, 5))),
        'long': ((6, 5, 64), BOX, crandn(rng, (6, 5, 33))),
        'real': ((10, 7, 12), BOX, rng.normal(size=(10, 7, 12))),
    }
    for _, _, f in out.values():
        f.setflags(write=False)
    return out


def unpack(block, nx_edges, nmu_edges, nell):
    """the contiguous [xsum|musum|Nsum|ysum] block as a namespace of
    (Nx+2, Nmu+2) arrays, nothing folded"""
    shape = (nx_edges + 1, nmu_edges + 1)
    NB = shape[0] * shape[1]
    assert block.shape == ((3 + 2 * nell) * NB,)
    ys = block[3 * NB:].reshape(nell, 2, NB)
    return dict(xsum=block[:NB].reshape(shape),
                musum=block[NB:2 * NB].reshape(shape),
                Nsum=block[2 * NB:3 * NB].reshape(shape),
                ysum=(ys[:, 0] + 1j * ys[:, 1]).reshape((nell,) + shape))


def new_sums(nx_edges, nmu_edges, nell):
    NB = (nx_edges + 1) * (nmu_edges + 1)
    return torch.zeros((3 + 2 * nell) * NB, dtype=torch.float64,
                       device='cuda'), NB


def sums_ptrs(sums, NB):
    return (hiplib.dptr(sums), hiplib.dptr(sums[NB:]),
            hiplib.dptr(sums[2 * NB:]), hiplib.dptr(sums[3 * NB:]))


def run_bin(lib, block, nmesh, box, k2e, mue, los, ells, real_field=0,
            off=(0, 0, 0), axis_map=None, sums=None):
    """nbk_bin_power_f64 on one local block; accumulates into ``sums``"""
    block = numpy.ascontiguousarray(block)
    if sums is None:
        sums, NB = new_sums(len(k2e), len(mue), len(ells))
    else:
        NB = (len(k2e) + 1) * (len(mue) + 1)
    b_t, k_t, m_t = dev(block), dev(k2e), dev(mue)
    rc = lib.nbk_bin_power_f64(
        hiplib.dptr(b_t), hiplib.i64_arr(nmesh), hiplib.f64_arr(box),
        hiplib.i64_arr(block.shape), hiplib.i64_arr(off),
        hiplib.int_arr(axis_map) if axis_map is not None else None,
        hiplib.dptr(k_t), len(k2e), hiplib.dptr(m_t), len(mue),
        hiplib.f64_arr(los), hiplib.int_arr(ells), len(ells), real_field,
        *sums_ptrs(sums, NB), None)
    torch.cuda.synchronize()
    return rc, sums


def assert_block(got, want, label, extra=0.0, err_ysum=None):
    """got: unpack() of a kernel's block; want: bin_sums_ref's namespace.
    Rows 0..Nx under the reordering bound (ysum with ``extra`` more eps of
    abs_sum and the absolute ``err_ysum`` on its real part), Nsum exact,
    the overflow row exactly zero."""
    n = want.n_terms[:-1].astype('f8')
    for name in ('xsum', 'musum', 'Nsum', 'ysum'):
        assert not numpy.any(got[name][..., -1, :]), \
            '%s: overflow row of %s written' % (label, name)
    assert_array_equal(got['Nsum'][:-1], want.Nsum[:-1],
                       err_msg='%s: Nsum' % label)
    assert want.Nsum[:-1].sum() > 0
    worst = 0.0
    for name in ('xsum', 'musum'):
        d = numpy.abs(got[name][:-1] - getattr(want, name)[:-1])
        bound = n * EPS * getattr(want, 'abs_' + name)[:-1]
        assert numpy.all(d <= bound), '%s: %s' % (label, name)
        worst = max(worst, (d / numpy.where(bound > 0, bound, 1)).max())
    for part in ('real', 'imag'):
        g = getattr(got['ysum'][:, :-1], part)
        w = getattr(want.ysum[:, :-1], part)
        bound = (n + extra) * EPS * getattr(want.abs_ysum[:, :-1], part)
        if err_ysum is not None and part == 'real':
            bound = bound + err_ysum[:, :-1]
        d = numpy.abs(g - w)
        assert numpy.all(d <= bound), '%s: ysum.%s' % (label, part)
        worst = max(worst, (d / numpy.where(bound > 0, bound, 1)).max())
    print('BINERR %s worst |diff|/bound = %.3f over %d filled bins'
          % (label, worst, (want.n_terms[:-1] > 0).sum()))


def reference_sums(field_entry, k2e, mue, los, ells, real_field=False):
    nmesh, box, f = field_entry
    fx, fy, fz = ref.grid_freqs(nmesh, real_field=real_field)
    return ref.bin_sums_ref(f, fx, fy, fz, nmesh, box, k2e, mue, los, ells,
                            hermitian=not real_field, real_field=real_field)


@pytest.mark.parametrize('los', sorted(LOSES))
@pytest.mark.parametrize('ells', POLES, ids=lambda p: 'l%d' % len(p))
@pytest.mark.parametrize('nmu', [1, 5])
@pytest.mark.parametrize('name', ['even', 'odd', 'long', 'real'])
def test_bin_power_identity(lib, fields, name, nmu, ells, los):
    """kbin_run<true> for the complex fields (a partial 32-line group and
    16-element runs that wrap lines at d2 = 7 and 5; d2 = 33 longer than a
    run), kbin<true> for the real field"""
    nmesh, box, f = fields[name]
    real = name == 'real'
    k2e, mue = make_edges(nmesh, box, 6, nmu, real_field=real)
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES[los], ells,
                       real_field=int(real))
    assert rc == 0
    want = reference_sums(fields[name], k2e, mue, LOSES[los], ells, real)
    assert want.Nsum[0].sum() > 0 and want.Nsum[-1].sum() > 0
    got = unpack(host(sums), len(k2e), len(mue), len(ells))
    assert_block(got, want, 'bin %s' % name)
    if real:
        assert not numpy.any(got['ysum'].imag)


def test_bin_power_rejects_nine_poles(lib, fields):
    nmesh, box, f = fields['even']
    k2e, mue = make_edges(nmesh, box, 6, 1)
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES['z'],
                       list(range(9)))
    assert rc == NBK_ERR_ARG
    assert not numpy.any(host(sums))


@pytest.mark.parametrize('real', [0, 1])
def test_bin_power_modes_on_edges(lib, real):
    """a cubic mesh binned at its own fundamental: every axis mode sits
    exactly ON an edge, where one ulp of k2 or `<` for `<=` moves it"""
    nmesh, box = (8, 8, 8), (20., 20., 20.)
    rng = numpy.random.RandomState(5)
    f = rng.normal(size=nmesh) if real else crandn(rng, (8, 8, 5))
    fund = box[0] / 8 if real else 2 * numpy.pi / box[0]
    k2e = (numpy.arange(0, 4) * fund) ** 2
    mue = numpy.linspace(0 if real else -1, 1, 5)
    ells = [0, 1, 2]
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES['z'], ells,
                       real_field=real)
    assert rc == 0
    want = reference_sums((nmesh, box, f), k2e, mue, LOSES['z'], ells,
                          bool(real))
    assert_block(unpack(host(sums), 4, 5, 3), want, 'on-edge real=%d' % real)


@pytest.mark.parametrize('real', [0, 1])
def test_bin_power_histograms_beyond_lds(lib, fields, real):
    """302 * 10 bins * 9 planes of doubles = 212 KiB > the 160 KiB LDS: the
    histograms go to global atomics, kbin_run<false> for the complex field
    and kbin<false> for the real one"""
    name = 'real' if real else 'even'
    nmesh, box, f = fields[name]
    ells = [0, 2, 4]
    k2e, mue = make_edges(nmesh, box, 300, 8, real_field=bool(real))
    assert (len(k2e) + 1) * (len(mue) + 1) * 9 * 8 > 160 * 1024
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES['tilt'], ells,
                       real_field=real)
    assert rc == 0
    want = reference_sums(fields[name], k2e, mue, LOSES['tilt'], ells,
                          bool(real))
    assert_block(unpack(host(sums), 301, 9, 3), want,
                 'global-atomic real=%d' % real)


@pytest.mark.parametrize('nx_edges', [1262, 1263, 1278])
def test_bin_power_at_the_lds_limit(lib, fields, nx_edges):
    """kbin_run keeps 8 (16 nx + 31) bytes of histograms, edges and z
    tables in dynamic LDS for this field (d2 = 7, two mu edges, one
    multipole) and 1056 B more statically; the launcher keeps 2 KiB of
    the 160 KiB for the latter.  1262 edges are the most that stay in
    LDS, 1263 go to global atomics, and 1278 fit 160 KiB only without
    the static arrays (an invalid launch before the reserve)."""
    nmesh, box, f = fields['even']
    k2e = numpy.linspace(0.05, 0.9 * nyquist(nmesh, box), nx_edges) ** 2
    mue = numpy.linspace(-1, 1, 2)
    assert (8 * (16 * 1262 + 31) <= 160 * 1024 - 2048
            < 8 * (16 * 1263 + 31))
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES['tilt'], [0])
    assert rc == 0
    want = reference_sums(fields['even'], k2e, mue, LOSES['tilt'], [0])
    assert_block(unpack(host(sums), nx_edges, 2, 1), want,
                 'bin at the LDS limit nx=%d' % nx_edges)


@pytest.mark.parametrize('nx_edges', [20200, 20300])
def test_bin_power_edge_tables_at_the_lds_limit(lib, fields, nx_edges):
    """With the histograms in global memory kbin_run still stages
    8 (nx + 2 + 2 * 7) bytes of edges and z tables in dynamic LDS: 20200
    edges fit the 160 KiB less the 2 KiB reserve (and need the attribute
    raised above 64 KiB), 20300 do not and go to the general kernel, which
    reads the edges from global memory."""
    nmesh, box, f = fields['even']
    assert (8 * (20200 + 16) <= 160 * 1024 - 2048 < 8 * (20300 + 16))
    k2e = numpy.linspace(0.05, 0.9 * nyquist(nmesh, box), nx_edges) ** 2
    mue = numpy.linspace(-1, 1, 2)
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, LOSES['tilt'], [0])
    assert rc == 0
    want = reference_sums(fields['even'], k2e, mue, LOSES['tilt'], [0])
    assert_block(unpack(host(sums), nx_edges, 2, 1), want,
                 'bin edge tables nx=%d' % nx_edges)


@pytest.mark.parametrize('name', ['even', 'odd', 'long'])
def test_bin_power_layouts(lib, fields, name):
    """every layout of one field gives the identity layout's sums: the
    transposed pencil (1,0,2) whole and split with off = (y0, 0, 0), the
    general kernel's (0,2,1), and an identity split along the half axis
    with off = (0, 0, z0); split parts accumulate into one buffer"""
    nmesh, box, f = fields[name]
    ells = [0, 1, 2, 4]
    k2e, mue = make_edges(nmesh, box, 6, 5)
    los = LOSES['tilt']
    want = reference_sums(fields[name], k2e, mue, los, ells)
    rc, sums = run_bin(lib, f, nmesh, box, k2e, mue, los, ells)
    assert rc == 0
    ident = unpack(host(sums), 7, 6, 4)
    ft = f.transpose(1, 0, 2)
    y0, z0 = 3, 2
    layouts = {
        'pencil whole': [(ft, (0, 0, 0), (1, 0, 2))],
        'pencil split': [(ft[:y0], (0, 0, 0), (1, 0, 2)),
                         (ft[y0:], (y0, 0, 0), (1, 0, 2))],
        'general (0,2,1)': [(f.transpose(0, 2, 1), (0, 0, 0), (0, 2, 1))],
        'general split': [(f.transpose(0, 2, 1)[:, :z0], (0, 0, 0),
                           (0, 2, 1)),
                          (f.transpose(0, 2, 1)[:, z0:], (0, z0, 0),
                           (0, 2, 1))],
        'half-axis split': [(f[:, :, :z0], (0, 0, 0), None),
                            (f[:, :, z0:], (0, 0, z0), None)],
    }
    for label, parts in layouts.items():
        sums = None
        for block, off, amap in parts:
            rc, sums = run_bin(lib, block, nmesh, box, k2e, mue, los, ells,
                               off=off, axis_map=amap, sums=sums)
            assert rc == 0
        got = unpack(host(sums), 7, 6, 4)
        assert_array_equal(got['Nsum'], ident['Nsum'], err_msg=label)
        assert_block(got, want, '%s %s' % (name, label))


# ---- nbk_power_bin_f64 ---------------------------------------------------

def run_power_bin(lib, c1, c2, V, win1, il1, win2, il2, clear, nmesh, box,
                  k2e, mue, los, ells, c2_mode='ptr'):
    sums, NB = new_sums(len(k2e), len(mue), len(ells))
    c1_t = dev(c1)
    c2_t = None if c2_mode == 'null' else c1_t if c2_mode == 'same' \
        else dev(c2)
    k_t, m_t = dev(k2e), dev(mue)
    rc = lib.nbk_power_bin_f64(
        hiplib.dptr(c1_t), hiplib.dptr(c2_t), V, win1, il1, win2, il2,
        clear, hiplib.i64_arr(nmesh), hiplib.f64_arr(box),
        hiplib.i64_arr(c1.shape), hiplib.i64_arr((0, 0, 0)), None,
        hiplib.dptr(k_t), len(k2e), hiplib.dptr(m_t), len(mue),
        hiplib.f64_arr(los), hiplib.int_arr(ells), len(ells),
        *sums_ptrs(sums, NB), None)
    torch.cuda.synchronize()
    return rc, sums


POWER_BIN_CASES = {
    # c2 mode, (win1, il1), (win2, il2)
    'auto null': ('null', (0, 0), (0, 0)),
    'auto same': ('same', (1, 1), (1, 1)),
    'auto same, windows differ': ('same', (0, 0), (2, 1)),
    'cross cic x pcs-interlaced': ('ptr', (0, 0), (2, 1)),
    'cross none x tsc': ('ptr', (-1, 0), (1, 0)),
    'cross pcs x none': ('ptr', (2, 0), (-1, 0)),
}


@pytest.mark.parametrize('clear', [0, 1])
@pytest.mark.parametrize('nmu', [1, 5])
@pytest.mark.parametrize('case', sorted(POWER_BIN_CASES))
def test_power_bin_matches_reference(lib, fields, case, nmu, clear):
    """comp1 c1 conj(comp2 c2) V with the zero mode cleared or kept; the
    products are taken in long double from the f64 compensated fields, and
    the bound gains 4 eps abs_sum for the kernel's reciprocal-product
    composition of the factors"""
    mode, (w1, i1), (w2, i2) = POWER_BIN_CASES[case]
    nmesh, box, c1 = fields['even']
    c2 = c1 if mode != 'ptr' \
        else crandn(numpy.random.RandomState(78), c1.shape)
    V = float(numpy.prod(box))
    ells = [0, 1, 2, 3]
    nyq = nyquist(nmesh, box)
    k2e = numpy.linspace(0., 0.9 * nyq, 7) ** 2      # the zero mode bins
    mue = numpy.linspace(-1, 1, nmu + 1)
    los = LOSES['tilt']
    rc, sums = run_power_bin(lib, c1, c2, V, w1, i1, w2, i2, clear, nmesh,
                             box, k2e, mue, los, ells, c2_mode=mode)
    assert rc == 0

    fx, fy, fz = ref.grid_freqs(nmesh)
    w = ref.circular(fx, fy, fz, nmesh)
    a = (c1 * ref.comp_factor(w1, i1, w)).astype(ref.CLD)
    b = (c2 * ref.comp_factor(w2, i2, w)).astype(ref.CLD)
    p = (a * numpy.conj(b) * LD(V)).astype('c16')
    assert p[0, 0, 0] != 0
    if clear:
        p[0, 0, 0] = 0
    want = ref.bin_sums_ref(p, fx, fy, fz, nmesh, box, k2e, mue, los, ells)
    assert_block(unpack(host(sums), 7, nmu + 1, 4), want,
                 'power_bin %s clear=%d' % (case, clear), extra=4)


# ---- elementwise ----------------------------------------------------------

def layouts_of(arr, y0=3):
    """(label, local block, off, axis_map) of a full identity-layout array"""
    return [('identity', arr, (0, 0, 0), None),
            ('pencil+off', arr.transpose(1, 0, 2)[y0:], (y0, 0, 0),
             (1, 0, 2)),
            ('(0,2,1)', arr.transpose(0, 2, 1), (0, 0, 0), (0, 2, 1))]


@pytest.mark.parametrize('interlaced', [0, 1])
@pytest.mark.parametrize('window', [0, 1, 2])
@pytest.mark.parametrize('name', ['even', 'odd'])
def test_compensate_layouts(lib, fields, name, window, interlaced):
    nmesh, _, f = fields[name]
    fx, fy, fz = ref.grid_freqs(nmesh)
    fac = ref.comp_factor(window, interlaced,
                          ref.circular(fx, fy, fz, nmesh))
    for (label, blk, off, amap), (_, fb, _, _) in zip(layouts_of(f),
                                                     layouts_of(fac)):
        b_t = dev(blk)
        hiplib.check(lib.nbk_compensate_f64(
            hiplib.dptr(b_t), hiplib.i64_arr(nmesh),
            hiplib.i64_arr(blk.shape), hiplib.i64_arr(off),
            hiplib.int_arr(amap) if amap else None, window, interlaced,
            None), 'compensate')
        want = numpy.ascontiguousarray(blk) * fb
        got = host(b_t)
        assert_allclose(got.real, want.real, rtol=1e-13, atol=0,
                        err_msg=label)
        assert_allclose(got.imag, want.imag, rtol=1e-13, atol=0,
                        err_msg=label)


@pytest.mark.parametrize('name', ['even', 'odd'])
def test_interlace_combine_layouts(lib, fields, name):
    nmesh, box, c1 = fields[name]
    c2 = crandn(numpy.random.RandomState(79), c1.shape)
    fx, fy, fz = ref.grid_freqs(nmesh)
    want_full = (c1 * LD(0.5) + c2 * LD(0.5)
                 * ref.interlace_phase(fx, fy, fz, nmesh))
    for (label, b1, off, amap), (_, b2, _, _), (_, wb, _, _) in zip(
            layouts_of(c1), layouts_of(c2), layouts_of(want_full)):
        b1_t, b2_t = dev(b1), dev(b2)
        hiplib.check(lib.nbk_interlace_combine_f64(
            hiplib.dptr(b1_t), hiplib.dptr(b2_t), hiplib.i64_arr(nmesh),
            hiplib.f64_arr(box), hiplib.i64_arr(b1.shape),
            hiplib.i64_arr(off), hiplib.int_arr(amap) if amap else None,
            None), 'interlace')
        assert_allclose(host(b1_t), wb.astype('c16'), rtol=1e-13, atol=0,
                        err_msg=label)
        assert_array_equal(host(b2_t), numpy.ascontiguousarray(b2))


def test_power3d_zero_mode_and_offsets(lib, fields):
    _, box, c1 = fields['even']
    c2 = crandn(numpy.random.RandomState(80), c1.shape)
    V = float(numpy.prod(box))
    want = (c1.astype(ref.CLD) * numpy.conj(c2) * LD(V)).astype('c16')
    c1_t, c2_t = dev(c1), dev(c2)
    for off, clear in (((0, 0, 0), 1), ((0, 0, 0), 0), ((0, 3, 0), 1),
                       ((2, 0, 0), 1), ((0, 0, 1), 1)):
        out_t = torch.zeros(c1.shape, dtype=torch.complex128, device='cuda')
        hiplib.check(lib.nbk_power3d_f64(
            hiplib.dptr(out_t), hiplib.dptr(c1_t), hiplib.dptr(c2_t), V,
            hiplib.i64_arr(c1.shape), hiplib.i64_arr(off), clear, None),
            'power3d')
        got = host(out_t)
        cleared = clear and off == (0, 0, 0)
        assert (got.flat[0] == 0) == bool(cleared), (off, clear)
        assert numpy.count_nonzero(got == 0) == int(cleared)
        d = numpy.abs(got - want)
        d.flat[0] = 0 if cleared else d.flat[0]
        assert numpy.all(d <= 4 * EPS * numpy.abs(want))


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_recon_displacement_matches_reference(lib, fields, axis):
    nmesh, box, f = fields['even']
    R, bias, growth = 2.5, 1.7, 0.6
    los = LOSES['tilt']
    f_t = dev(f)
    out_t = torch.full(f.shape, 9 + 9j, dtype=torch.complex128,
                       device='cuda')
    hiplib.check(lib.nbk_recon_displacement_f64(
        hiplib.dptr(out_t), hiplib.dptr(f_t), hiplib.i64_arr(nmesh),
        hiplib.f64_arr(box), hiplib.i64_arr(f.shape),
        hiplib.i64_arr((0, 0, 0)), axis, R, bias, growth,
        hiplib.f64_arr(los), None), 'recon')
    fx, fy, fz = ref.grid_freqs(nmesh)
    want = (ref.recon_factor(fx, fy, fz, box, axis, R, bias, growth, los)
            * f).astype('c16')
    got = host(out_t)
    assert got[0, 0, 0] == 0
    assert numpy.count_nonzero(want) > 0.8 * want.size
    assert_allclose(got.real, want.real, rtol=1e-13, atol=0)
    assert_allclose(got.imag, want.imag, rtol=1e-13, atol=0)


def test_recon_displacement_rejects_axis_3(lib, fields):
    nmesh, box, f = fields['even']
    f_t = dev(f)
    out_t = torch.zeros(f.shape, dtype=torch.complex128, device='cuda')
    rc = lib.nbk_recon_displacement_f64(
        hiplib.dptr(out_t), hiplib.dptr(f_t), hiplib.i64_arr(nmesh),
        hiplib.f64_arr(box), hiplib.i64_arr(f.shape),
        hiplib.i64_arr((0, 0, 0)), 3, 2.5, 1.7, 0.6,
        hiplib.f64_arr(LOSES['z']), None)
    assert rc == NBK_ERR_ARG
    assert not numpy.any(host(out_t))


# =========================================================================
# C. nbk_fft_x_bin_f64
# =========================================================================

def xbin_box(nmesh):
    # anisotropic cells, the z Nyquist (pi/1.25) the smallest: the Nyquist
    # plane lies inside the last edge, so whether a call visits it shows
    return tuple(n * h for n, h in zip(nmesh, (1.0, 0.8, 1.25)))


def xbin_edges(nmesh, box, nk, nmu, kmin_frac=0.0, last=1.05):
    top = last * nyquist(nmesh, box)
    kedges = numpy.linspace(kmin_frac * top, top, nk + 1)
    return kedges, numpy.linspace(-1, 1, nmu + 1)


def hints_of(kedges, muedges):
    return [float(kedges[0]), 1.0 / float(kedges[1] - kedges[0]),
            float(muedges[0]), 1.0 / float(muedges[1] - muedges[0])]


def run_xbin(lib, pre, pre2, nmesh, box, y_off, window, il_flag, clear, V,
             kedges, mue, los, ells, hints=None, sums=None):
    """nbk_fft_x_bin_f64 on the pre-x block(s) (n0, ny_local, nzh);
    accumulates into ``sums``"""
    nell = len(ells)
    if sums is None:
        sums, _ = new_sums(len(kedges), len(mue), nell)
    p_t = dev(pre)
    p2_t = dev(pre2) if pre2 is not None else None
    k_t, m_t = dev(numpy.asarray(kedges) ** 2), dev(mue)
    rc = lib.nbk_fft_x_bin_f64(
        hiplib.dptr(p_t), hiplib.dptr(p2_t), hiplib.i64_arr(nmesh),
        pre.shape[1] * pre.shape[2], y_off, hiplib.f64_arr(box),
        window, il_flag, clear, V, hiplib.dptr(k_t), len(kedges),
        hiplib.dptr(m_t), len(mue),
        hiplib.f64_arr(hints if hints is not None
                       else hints_of(kedges, mue)),
        hiplib.f64_arr(los), hiplib.int_arr(ells), nell,
        hiplib.dptr(sums), None)
    torch.cuda.synchronize()
    return rc, sums


def xbin_reference(pre, pre2, nmesh, box, y_off, window, il_flag, clear, V,
                   kedges, mue, los, ells):
    """x FFT in long double, the interlaced combine, compensation,
    |a|^2 V with the zero mode cleared, then bin_sums_ref over exactly the
    elements the kernel is documented to visit: all of them, or for an
    interlaced pair all but the iz = 0 plane and the even-n2 Nyquist
    plane.  Also the propagated FFT term err_ysum, from
    delta = C_STRIDED eps log2(n0) rms(line) per column."""
    n0, nyl, nzh = pre.shape
    n1, n2 = int(nmesh[1]), int(nmesh[2])
    assert nzh == n2 // 2 + 1
    fx, fy, fz = numpy.broadcast_arrays(
        ref.freq_full(numpy.arange(n0), n0)[:, None, None],
        ref.freq_full(numpy.arange(nyl) + y_off, n1)[None, :, None],
        ref.freq_half(numpy.arange(nzh), n2)[None, None, :])

    def transformed(x):
        X = ref.fft_ref(x, 0, -1)
        rms = numpy.sqrt(numpy.mean(numpy.abs(X) ** 2, axis=0,
                                    keepdims=True)).astype('f8')
        return X, C_STRIDED * EPS * math.log2(n0) * rms

    X, delta = transformed(pre)
    if pre2 is not None:
        X2, delta2 = transformed(pre2)
        X = X * LD(0.5) + X2 * LD(0.5) \
            * ref.interlace_phase(fx, fy, fz, nmesh)
        delta = 0.5 * (delta + delta2)
    comp = ref.comp_factor(window, il_flag,
                           ref.circular(fx, fy, fz, nmesh))
    val = (numpy.abs(X * comp) ** 2 * LD(V)).astype('f8')
    if clear and y_off == 0:
        assert val[0, 0, 0] != 0
        val[0, 0, 0] = 0.0
    keep = numpy.ones(pre.shape, dtype=bool)
    if pre2 is not None:
        keep[:, :, 0] = False
        if n2 % 2 == 0:
            keep[:, :, -1] = False
    delta = numpy.broadcast_to(delta, pre.shape)
    return ref.bin_sums_ref(
        val[keep], fx[keep], fy[keep], fz[keep], nmesh, box,
        numpy.asarray(kedges) ** 2, mue, los, ells,
        absx=numpy.abs(X).astype('f8')[keep], delta=delta[keep],
        err_scale=(comp * comp * V)[keep])


def check_xbin(lib, shape, interlaced_pair, window=0, il_flag=0, clear=1,
               nmu=1, ells=(0,), los='tilt', kmin_frac=0.0, last=1.05,
               nk=8, seed=0):
    skip_if_env(*XBIN_ENV)
    n0, n1, n2 = shape
    box = xbin_box(shape)
    V = float(numpy.prod(box))
    rng = numpy.random.RandomState(500 + seed + n0 + n1)
    pre = crandn(rng, (n0, n1, n2 // 2 + 1))
    pre2 = crandn(rng, pre.shape) if interlaced_pair else None
    kedges, mue = xbin_edges(shape, box, nk, nmu, kmin_frac, last)
    ells = list(ells)
    args = (shape, box, 0, window, il_flag, clear, V, kedges, mue,
            LOSES[los], ells)
    rc, sums = run_xbin(lib, pre, pre2, *args)
    assert rc == 0, hiplib.load().nbk_last_error_string()
    want = xbin_reference(pre, pre2, *args)
    got = unpack(host(sums), len(kedges), len(mue), len(ells))
    assert not numpy.any(got['ysum'].imag), 'imaginary multipole planes'
    assert_block(got, want, 'xbin %s il=%d' % (shape, interlaced_pair),
                 err_ysum=want.err_ysum)
    return want


# option sets that between them take every value the issue lists; each
# runs on every small shape, plain and as an interlaced pair
XBIN_OPTIONS = [
    dict(window=-1, il_flag=0, clear=1, nmu=1, ells=(0,)),
    dict(window=0, il_flag=0, clear=1, nmu=5, ells=(0, 2, 4)),
    dict(window=0, il_flag=1, clear=0, nmu=1, ells=(0, 1, 2, 3)),
    dict(window=1, il_flag=0, clear=1, nmu=5, ells=tuple(range(8))),
    dict(window=1, il_flag=1, clear=1, nmu=1, ells=(0,), kmin_frac=0.1),
    dict(window=2, il_flag=0, clear=0, nmu=5, ells=(0,), los='z'),
    dict(window=2, il_flag=1, clear=1, nmu=5, ells=(0, 2, 4), last=0.45),
    dict(window=-1, il_flag=1, clear=1, nmu=1, ells=(0, 2, 4), los='x',
         kmin_frac=0.1, last=0.45),
]
XBIN_SMALL = [(8, 6, 10), (16, 5, 12), (32, 4, 8)]
XBIN_SMALL_IL = [(8, 6, 10), (16, 5, 9)]


@pytest.mark.parametrize('opt', range(len(XBIN_OPTIONS)))
@pytest.mark.parametrize('shape', XBIN_SMALL, ids=str)
def test_xbin_small_shapes(lib, shape, opt):
    """n0 = 8..32: the fused final stage is the whole network after one
    radix-2 (8, 32) or radix-4 (16) stage; (16, 5, 12) has 35 columns, a
    partial last tile"""
    want = check_xbin(lib, shape, False, seed=opt, **XBIN_OPTIONS[opt])
    if XBIN_OPTIONS[opt].get('last', 1.05) < 1:
        # whole columns lie beyond the last edge and are skipped unloaded
        assert want.n_terms[-1].sum() > 0.5 * want.n_terms.sum()


@pytest.mark.parametrize('opt', range(len(XBIN_OPTIONS)))
@pytest.mark.parametrize('shape', XBIN_SMALL_IL, ids=str)
def test_xbin_small_shapes_interlaced_pair(lib, shape, opt):
    """the pair mode skips the iz = 0 plane and, for even n2 only, the
    Nyquist plane"""
    check_xbin(lib, shape, True, seed=opt, **XBIN_OPTIONS[opt])


@pytest.mark.parametrize('shape', [(1024, 3, 8), (2048, 3, 8),
                                   (8, 128, 128)], ids=str)
def test_xbin_launch_branches(lib, shape):
    """(1024, 3, 8): n0 * TI exactly at the 4096 register cap;
    (2048, 3, 8): TI = 2 and an LDS tile above 64 KiB;
    (8, 128, 128): 8320 columns = 2080 tiles over 2048 blocks, so two
    tiles per block and about half the blocks without one"""
    check_xbin(lib, shape, False, window=0, nmu=5, ells=(0, 2, 4))


@pytest.mark.parametrize('shape', [(512, 3, 8), (1024, 3, 8)], ids=str)
def test_xbin_launch_branches_interlaced_pair(lib, shape):
    """the pair halves the register cap: TI = 4 at 512, 2 at 1024"""
    check_xbin(lib, shape, True, window=2, il_flag=1, nmu=5,
               ells=(0, 2, 4))


@pytest.mark.parametrize('shape,pair', [((4096, 2, 8), False),
                                        ((2048, 2, 8), True)])
def test_xbin_unsupported_sizes_leave_output(lib, shape, pair):
    """the TI = 1 tile(s) and the n0-entry tables alone fill the LDS: the
    launcher rejects the size before any launch"""
    skip_if_env(*XBIN_ENV)
    box = xbin_box(shape)
    pre = numpy.zeros((shape[0], shape[1], shape[2] // 2 + 1), dtype='c16')
    kedges, mue = xbin_edges(shape, box, 4, 1)
    sums, _ = new_sums(len(kedges), len(mue), 1)
    sums += 7.0
    rc, sums = run_xbin(lib, pre, pre if pair else None, shape, box, 0, 0,
                        0, 1, 1.0, kedges, mue, LOSES['z'], [0], sums=sums)
    assert rc == NBK_ERR_UNSUPPORTED
    assert numpy.all(host(sums) == 7.0)


def test_xbin_rejects_nine_poles(lib):
    shape = (8, 6, 10)
    box = xbin_box(shape)
    pre = numpy.zeros((8, 6, 6), dtype='c16')
    kedges, mue = xbin_edges(shape, box, 4, 1)
    rc, sums = run_xbin(lib, pre, None, shape, box, 0, 0, 0, 1, 1.0,
                        kedges, mue, LOSES['z'], list(range(9)))
    assert rc == NBK_ERR_ARG
    assert not numpy.any(host(sums))


def test_xbin_slab_split_accumulates(lib):
    """rows [0, 2) and [2, 6) of a (16, 6, 12) field in two calls with
    y_off = 0 and 2 into one out_sums == the single full call"""
    skip_if_env(*XBIN_ENV)
    shape = (16, 6, 12)
    box = xbin_box(shape)
    V = float(numpy.prod(box))
    pre = crandn(numpy.random.RandomState(61), (16, 6, 7))
    kedges, mue = xbin_edges(shape, box, 8, 5)
    ells = [0, 2, 4]
    tail = (1, 0, 1, V, kedges, mue, LOSES['tilt'], ells)
    rc, full = run_xbin(lib, pre, None, shape, box, 0, *tail)
    assert rc == 0
    sums = None
    for y0, y1 in ((0, 2), (2, 6)):
        rc, sums = run_xbin(lib, pre[:, y0:y1], None, shape, box, y0,
                            *tail, sums=sums)
        assert rc == 0
    want = xbin_reference(pre, None, shape, box, 0, *tail)
    got = unpack(host(sums), 9, 6, 3)
    one = unpack(host(full), 9, 6, 3)
    assert_array_equal(got['Nsum'], one['Nsum'])
    assert_block(got, want, 'xbin slab split',
                 err_ysum=want.err_ysum)
    assert_block(one, want, 'xbin slab whole',
                 err_ysum=want.err_ysum)


def assert_same_terms(a, b, want, label):
    """two runs over the same f64 terms in different orders: Nsum equal
    bit for bit, the sums within the reordering bound of each other"""
    assert_array_equal(a['Nsum'], b['Nsum'], err_msg=label)
    n = want.n_terms.astype('f8')
    for name in ('xsum', 'musum'):
        assert numpy.all(numpy.abs(a[name] - b[name])
                         <= n * EPS * getattr(want, 'abs_' + name)), \
            '%s: %s' % (label, name)
    assert numpy.all(numpy.abs(a['ysum'].real - b['ysum'].real)
                     <= n * EPS * want.abs_ysum.real), label
    assert not numpy.any(a['ysum'].imag) and not numpy.any(b['ysum'].imag)


def test_xbin_wrong_dig_hints_change_nothing(lib):
    """the hints only seed the digitize: k_invd three times too large and
    mu_lo shifted by 0.4 must give the same bins"""
    skip_if_env(*XBIN_ENV)
    shape = (16, 5, 12)
    box = xbin_box(shape)
    V = float(numpy.prod(box))
    pre = crandn(numpy.random.RandomState(62), (16, 5, 7))
    kedges, mue = xbin_edges(shape, box, 8, 5, kmin_frac=0.1)
    ells = [0, 1, 2]
    args = (shape, box, 0, 1, 0, 1, V, kedges, mue, LOSES['tilt'], ells)
    good = hints_of(kedges, mue)
    bad = [good[0], 3.0 * good[1], good[2] + 0.4, good[3]]
    rc, s_good = run_xbin(lib, pre, None, *args, hints=good)
    assert rc == 0
    rc, s_bad = run_xbin(lib, pre, None, *args, hints=bad)
    assert rc == 0
    want = xbin_reference(pre, None, *args)
    assert_same_terms(unpack(host(s_good), 9, 6, 3),
                      unpack(host(s_bad), 9, 6, 3), want, 'wrong hints')


@pytest.mark.parametrize('n0', [16, 2048])
def test_xbin_equals_unfused_pass(lib, n0):
    """nbk_fft_c_strided along x then nbk_power_bin_f64(c1 == c2): the
    header claims bit-identical element values, so the two differ by the
    order of the sums alone"""
    skip_if_env(*XBIN_ENV)
    skip_if_env(*FFT_ENV)
    shape = (n0, 3, 8)
    box = xbin_box(shape)
    V = float(numpy.prod(box))
    pre = crandn(numpy.random.RandomState(63 + n0), (n0, 3, 5))
    kedges, mue = xbin_edges(shape, box, 8, 5)
    ells = [0, 2, 4]
    args = (shape, box, 0, 2, 0, 1, V, kedges, mue, LOSES['tilt'], ells)
    rc, fused = run_xbin(lib, pre, None, *args)
    assert rc == 0
    c_t = dev(pre)
    hiplib.check(lib.nbk_fft_c_strided(hiplib.dptr(c_t), n0, 15, 1, 0, 15,
                                       -1, None), 'x pass')
    rc, unfused = run_power_bin(lib, host(c_t), None, V, 2, 0, 2, 0, 1,
                                shape, box, numpy.asarray(kedges) ** 2, mue,
                                LOSES['tilt'], ells, c2_mode='same')
    assert rc == 0
    want = xbin_reference(pre, None, *args)
    assert_same_terms(unpack(host(fused), 9, 6, 3),
                      unpack(host(unfused), 9, 6, 3), want,
                      'fused vs unfused n0=%d' % n0)


@pytest.mark.parametrize('n0,pair,nx_fit,nx_dyn', [(2048, False, 606, 638),
                                                   (1024, True, 542, 574)])
def test_xbin_gate_agrees_with_kernel(lib, n0, pair, nx_fit, nx_dyn):
    """_xbin_lds_fits must answer as the launcher does on both sides of
    the LDS limit, or FFTPower raises in production.  With two mu edges
    and one multipole the launcher needs, at TI = 1,
    8 (16 nx + 17 + n0) + 32 n0 bytes plain and
    8 (16 nx + 17 + n0) + 16 n0 + 64 n0 for a pair, against 160 KiB less
    the 4 KiB it reserves for the kernel's static arrays: nx <= 606 at
    n0 = 2048 plain, nx <= 542 at n0 = 1024 for a pair.  Against the whole
    160 KiB the counts would be 638 and 574: there the dynamic allocation
    alone fits, but the launch, with the static arrays on top, is invalid
    (it aborted the queue before the launcher kept that reserve), so both
    sides must now refuse them."""
    skip_if_env(*XBIN_ENV)
    from nbodykit_amd.algorithms.fftpower import _xbin_lds_fits
    shape = (n0, 1, 8)
    box = xbin_box(shape)
    V = float(numpy.prod(box))
    pre = crandn(numpy.random.RandomState(64), (n0, 1, 5))
    pre2 = crandn(numpy.random.RandomState(65), pre.shape) if pair else None
    mue = numpy.linspace(-1, 1, 2)
    for nx, fits in ((nx_fit, True), (nx_fit + 1, False),
                     (nx_dyn, False), (nx_dyn + 1, False)):
        kedges = numpy.linspace(0., 1.05 * nyquist(shape, box), nx)
        args = (shape, box, 0, 0, 0, 1, V, kedges, mue, LOSES['z'], [0])
        rc, sums = run_xbin(lib, pre, pre2, *args)
        assert rc == (0 if fits else NBK_ERR_UNSUPPORTED), (nx, rc)
        assert _xbin_lds_fits(n0, nx, 2, 1, il=pair) == fits, nx
        if fits:
            # the largest launch that fits also computes the right sums
            want = xbin_reference(pre, pre2, *args)
            assert_block(unpack(host(sums), nx, 2, 1), want,
                         'xbin at the LDS limit n0=%d' % n0,
                         err_ysum=want.err_ysum)
        else:
            assert not numpy.any(host(sums))
