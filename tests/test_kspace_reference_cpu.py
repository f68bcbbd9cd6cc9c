"""
The references of tests/kspace_reference.py against the oracle, so that
they are trusted before tests/test_gpu_kspace_kernels.py lets them judge a
kernel.  CPU only.
"""
import numpy
import pytest
from numpy.testing import assert_allclose, assert_array_equal

import kspace_reference as ref
from oracle import MeshGeometry, project_to_basis
from oracle.fftpower import compensation_filter
from oracle.mesh import complex_coords, real_coords

MESHES = {'cubic': ((12, 12, 12), (30., 30., 30.)),
          'noncubic': ((10, 7, 12), (32., 30., 25.)),
          'odd_half': ((10, 7, 9), (32., 30., 25.))}
LOSES = [(0., 0., 1.), (1. / 3, 2. / 3, 2. / 3)]


def _field(shape, seed, real=False):
    rng = numpy.random.RandomState(seed)
    if real:
        return rng.normal(size=shape)
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _magnitude(values, *args, **kw):
    """per-bin sums of w |v|: bin_sums_ref of |values| at poles [0]"""
    return ref.bin_sums_ref(numpy.abs(values), *args, [0],
                            **kw).abs_ysum[0].real


def _assert_sums(got, want, poles, mag, rel=1e-13):
    """got: a bin_sums_ref namespace; want: the oracle's raw
    (xsum, musum, ysum, Nsum).  Integer counts equal; each float sum within
    ``rel`` of the bin's sum of term magnitudes.  For ysum the magnitude is
    taken with |P_l| = 1, (2l+1) times ``mag`` (the bin sums of w |v|, from
    ``_magnitude``): the oracle evaluates
    scipy's P_l as a power-basis polynomial, whose rounding error is
    absolute (a few eps times coefficients up to 35/8), not relative to a
    P_l that the recurrence resolves near its zeros."""
    xsum, musum, ysum, Nsum = want
    assert_array_equal(got.Nsum, Nsum)
    assert got.n_terms.sum() > 0
    for name, w in (('xsum', xsum), ('musum', musum)):
        g, a = getattr(got, name), getattr(got, 'abs_' + name)
        assert numpy.all(numpy.abs(g - w) <= rel * a), name
    assert poles[0] == 0
    for e, ell in enumerate(poles):
        scale = (2 * ell + 1) * mag
        assert numpy.all(numpy.abs(got.ysum[e].real - ysum[e].real)
                         <= rel * scale), ell
        assert numpy.all(numpy.abs(got.ysum[e].imag - numpy.imag(ysum[e]))
                         <= rel * scale), ell
        # a doubled mode feeds one part only: the sums are not all zero
        assert numpy.abs(got.ysum[e]).max() > 0


@pytest.mark.parametrize('mesh', ['cubic', 'noncubic', 'odd_half'])
@pytest.mark.parametrize('nmu', [1, 5])
@pytest.mark.parametrize('poles', [[0, 2, 4], [0, 1, 2, 3]])
@pytest.mark.parametrize('los', LOSES)
def test_bin_sums_ref_matches_oracle_complex(mesh, nmu, poles, los):
    nmesh, box = MESHES[mesh]
    geom = MeshGeometry(nmesh, box)
    y3d = _field(geom.cshape, 3)
    kny = numpy.pi * min(n / b for n, b in zip(nmesh, box))
    kedges = numpy.linspace(0.05, 0.8 * kny, 9)
    muedges = numpy.linspace(-1, 1, nmu + 1)
    want = project_to_basis(y3d, geom, [kedges, muedges], los=los,
                            poles=poles, _return_sums=True)
    fx, fy, fz = ref.grid_freqs(nmesh)
    args = (fx, fy, fz, nmesh, box, kedges ** 2, muedges, los)
    got = ref.bin_sums_ref(y3d, *args, poles)
    _assert_sums(got, want, poles, _magnitude(y3d, *args))
    # the overflow row and row 0 (kmin > 0) are populated: nothing dropped
    assert got.Nsum[0].sum() > 0 and got.Nsum[-1].sum() > 0
    assert got.Nsum.sum() == numpy.where(fz > 0, 2, 1).sum()


@pytest.mark.parametrize('mesh', ['cubic', 'noncubic'])
@pytest.mark.parametrize('nmu', [1, 5])
@pytest.mark.parametrize('poles', [[0, 2, 4], [0, 1, 2, 3]])
@pytest.mark.parametrize('los', LOSES)
def test_bin_sums_ref_matches_oracle_real_field(mesh, nmu, poles, los):
    nmesh, box = MESHES[mesh]
    geom = MeshGeometry(nmesh, box)
    y3d = _field(nmesh, 4, real=True)
    # the lattice spacing as bin width: most points sit ON an edge
    dr = min(box) / max(nmesh)
    redges = numpy.arange(0., 0.4 * min(box), dr)
    muedges = numpy.linspace(0, 1, nmu + 1)
    want = project_to_basis(y3d, geom, [redges, muedges], los=los,
                            poles=poles, coords=real_coords(geom),
                            hermitian=False, _return_sums=True)
    fx, fy, fz = ref.grid_freqs(nmesh, real_field=True)
    args = (fx, fy, fz, nmesh, box, redges ** 2, muedges, los)
    kw = dict(hermitian=False, real_field=True)
    got = ref.bin_sums_ref(y3d, *args, poles, **kw)
    xsum, musum, ysum, Nsum = want
    _assert_sums(got, (xsum, musum, ysum.astype('c16'), Nsum), poles,
                 _magnitude(y3d, *args, **kw))
    assert numpy.all(got.ysum.imag == 0)


def test_bin_sums_ref_on_edge_modes():
    """dk = the fundamental on a cubic mesh: every axis mode sits exactly
    on an edge, and the reference still equals the oracle bin for bin."""
    nmesh, box = (8, 8, 8), (20., 20., 20.)
    geom = MeshGeometry(nmesh, box)
    y3d = _field(geom.cshape, 5)
    kedges = numpy.arange(0, 5) * (2 * numpy.pi / 20.)
    muedges = numpy.linspace(-1, 1, 5)
    want = project_to_basis(y3d, geom, [kedges, muedges], poles=[0, 2],
                            _return_sums=True)
    fx, fy, fz = ref.grid_freqs(nmesh)
    args = (fx, fy, fz, nmesh, box, kedges ** 2, muedges, (0, 0, 1))
    got = ref.bin_sums_ref(y3d, *args, [0, 2])
    _assert_sums(got, want, [0, 2], _magnitude(y3d, *args))


def test_bin_sums_ref_is_a_sum_over_its_list():
    """any split of the element list adds up to the whole: what lets one
    reference serve every layout, slab and skipped plane."""
    nmesh, box = MESHES['noncubic']
    y3d = _field((10, 7, 7), 6)
    fx, fy, fz = ref.grid_freqs(nmesh)
    k2e = numpy.linspace(0.1, 1.2, 7) ** 2
    mue = numpy.linspace(-1, 1, 4)
    args = (nmesh, box, k2e, mue, LOSES[1], [0, 1, 2])
    full = ref.bin_sums_ref(y3d, fx, fy, fz, *args)
    sel = numpy.random.RandomState(7).uniform(size=y3d.shape) < 0.4
    a = ref.bin_sums_ref(y3d[sel], fx[sel], fy[sel], fz[sel], *args)
    b = ref.bin_sums_ref(y3d[~sel], fx[~sel], fy[~sel], fz[~sel], *args)
    assert_array_equal(a.Nsum + b.Nsum, full.Nsum)
    assert_array_equal(a.n_terms + b.n_terms, full.n_terms)
    assert numpy.all(numpy.abs(a.ysum + b.ysum - full.ysum)
                     <= 4 * ref.EPS * numpy.abs(full.abs_ysum))
    assert numpy.all(numpy.abs(a.xsum + b.xsum - full.xsum)
                     <= 4 * ref.EPS * full.abs_xsum)


def test_err_ysum_bounds_a_perturbed_power():
    """err_ysum really bounds the change of the real multipole sums when
    every |X|^2 element moves by up to delta in X."""
    nmesh, box = MESHES['noncubic']
    X = _field((10, 7, 7), 8)
    rng = numpy.random.RandomState(9)
    delta = 1e-3
    dX = delta * rng.uniform(0, 1, X.shape) \
        * numpy.exp(2j * numpy.pi * rng.uniform(size=X.shape))
    fx, fy, fz = ref.grid_freqs(nmesh)
    k2e = numpy.linspace(0., 1.2, 7) ** 2
    mue = numpy.linspace(-1, 1, 4)
    args = (nmesh, box, k2e, mue, LOSES[1], [0, 1, 2, 4])
    V = 3.5
    a = ref.bin_sums_ref(numpy.abs(X) ** 2 * V, fx, fy, fz, *args,
                         absx=numpy.abs(X), delta=delta, err_scale=V)
    b = ref.bin_sums_ref(numpy.abs(X + dX) ** 2 * V, fx, fy, fz, *args)
    diff = numpy.abs(a.ysum.real - b.ysum.real)
    assert numpy.all(diff <= a.err_ysum * (1 + 1e-12))
    assert diff.max() > 0.01 * a.err_ysum.max()      # and is not slack


@pytest.mark.parametrize('n', [8, 12, 27, 64, 4096])
@pytest.mark.parametrize('sign', [-1, 1])
def test_fft_ref_matches_numpy_f64(n, sign):
    rng = numpy.random.RandomState(n)
    x = rng.normal(size=(3, n, 2)) + 1j * rng.normal(size=(3, n, 2))
    got = ref.fft_ref(x, 1, sign)
    assert got.dtype == numpy.clongdouble
    want = numpy.fft.fft(x, axis=1) if sign < 0 \
        else numpy.fft.ifft(x, axis=1) * n
    rms = numpy.sqrt(numpy.mean(numpy.abs(want) ** 2))
    assert numpy.abs(got - want).max() <= 1e-13 * rms


@pytest.mark.parametrize('n', [8, 9, 64, 4096])
def test_rfft_irfft_ref_match_numpy_f64(n):
    rng = numpy.random.RandomState(n)
    x = rng.normal(size=(3, n))
    X = ref.rfft_ref(x)
    assert X.dtype == numpy.clongdouble
    want = numpy.fft.rfft(x, axis=-1)
    rms = numpy.sqrt(numpy.mean(numpy.abs(want) ** 2))
    assert numpy.abs(X - want).max() <= 1e-13 * rms
    # unnormalized inverse
    back = ref.irfft_ref(X, n)
    assert back.dtype == numpy.longdouble
    assert numpy.abs(back - n * x).max() <= 1e-13 * n
    # DC / Nyquist imaginary parts do not contribute
    Y = numpy.array(X)
    Y[:, 0] += 0.7j
    if n % 2 == 0:
        Y[:, -1] -= 1.3j
    assert_array_equal(ref.irfft_ref(Y, n), back)
    # ... and a non-self-conjugate entry does
    Y[:, 1] += 0.5j
    assert numpy.abs(ref.irfft_ref(Y, n) - back).max() > 0.1


def test_freqs_match_the_coordinate_arrays():
    for n in (7, 8, 9, 10, 12, 96, 100):
        assert_array_equal(ref.freq_full(numpy.arange(n), n),
                           numpy.fft.fftfreq(n) * n)
    assert_array_equal(ref.freq_half(numpy.arange(5), 8), [0, 1, 2, 3, -4])
    assert_array_equal(ref.freq_half(numpy.arange(5), 9), [0, 1, 2, 3, 4])
    assert ref.freq_full(4, 8) == -4 and ref.freq_full(4, 9) == 4
    geom = MeshGeometry((10, 7, 12), (32., 30., 25.))
    fx, fy, fz = ref.grid_freqs(geom.Nmesh)
    k = complex_coords(geom)
    k0 = 2 * numpy.pi / geom.BoxSize
    assert_array_equal(fx[:, :1, :1] * k0[0], k[0])
    assert_array_equal(fy[:1, :, :1] * k0[1], k[1])
    assert_array_equal(fz[:1, :1, :] * k0[2], k[2])


@pytest.mark.parametrize('window', ['cic', 'tsc', 'pcs'])
@pytest.mark.parametrize('interlaced', [False, True])
def test_comp_factor_matches_oracle(window, interlaced):
    nmesh = (10, 7, 12)
    fx, fy, fz = ref.grid_freqs(nmesh)
    w = ref.circular(fx, fy, fz, nmesh)
    got = ref.comp_factor({'cic': 0, 'tsc': 1, 'pcs': 2}[window],
                          interlaced, w)
    want = compensation_filter(w, window, interlaced)
    assert_allclose(got, want, rtol=1e-14, atol=0)
    assert numpy.all(ref.comp_factor(-1, interlaced, w) == 1.0)


def test_recon_factor_matches_oracle_formula():
    nmesh, box = (10, 7, 12), (32., 30., 25.)
    fx, fy, fz = ref.grid_freqs(nmesh)
    los = (1. / 3, 2. / 3, 2. / 3)
    R, bias, f = 2.5, 1.7, 0.6
    k = [fi * 2 * numpy.pi / L for fi, L in zip((fx, fy, fz), box)]
    k2 = sum(ki ** 2 for ki in k)
    k2[0, 0, 0] = 1.0
    mu = sum(ki * li for ki, li in zip(k, los)) / k2 ** 0.5
    for axis in range(3):
        want = 1j * k[axis] / k2 * numpy.exp(-0.5 * k2 * R ** 2) \
            / bias / (1 + f / bias * mu ** 2)
        want[0, 0, 0] = 0
        got = ref.recon_factor(fx, fy, fz, box, axis, R, bias, f, los)
        assert got[0, 0, 0] == 0
        assert_allclose(got.astype('c16'), want, rtol=1e-13, atol=0)
