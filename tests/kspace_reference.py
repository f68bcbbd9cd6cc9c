"""
Plain NumPy references for the FFT and k-space kernels (no torch, no GPU).

Two kinds of reference live here:

- transforms (``fft_ref``, ``rfft_ref``, ``irfft_ref``) run numpy.fft on
  long-double input -- pocketfft keeps the type, so their rounding error is
  ~2^-64 * log2 N, three orders below anything an f64 kernel is held to;
- ``bin_sums_ref`` is a brute-force restatement of the project_to_basis sums
  over an EXPLICIT element list (one frequency triple and one value per
  element).  The per-element quantities follow the kernels' documented f64
  rounding chain, so bin membership and every term are what a correct
  kernel computes, and the per-bin sums are accumulated in long double.
  Because it works on a list, any layout, offset, slab split or skipped
  plane is just a different list.

tests/test_kspace_reference_cpu.py checks these against the oracle before
tests/test_gpu_kspace_kernels.py uses them to judge a kernel.
"""
from types import SimpleNamespace

import numpy

EPS = 2.0 ** -52            # the f64 rounding unit used in every bound
LD = numpy.longdouble
CLD = numpy.clongdouble
PI_LD = 4 * numpy.arctan(LD(1))


# ---- transforms ---------------------------------------------------------

def fft_ref(x, axis, sign):
    """Unnormalized DFT (sign=-1) / inverse DFT (sign=+1) along ``axis`` in
    long double."""
    x = numpy.asarray(x, dtype=CLD)
    if sign < 0:
        return numpy.fft.fft(x, axis=axis)
    return numpy.fft.ifft(x, axis=axis) * LD(x.shape[axis])


def rfft_ref(x, axis=-1):
    """real -> half-complex along ``axis`` in long double, unnormalized."""
    return numpy.fft.rfft(numpy.asarray(x, dtype=LD), axis=axis)


def irfft_ref(X, n, axis=-1):
    """half-complex -> ``n`` reals along ``axis`` in long double,
    UNNORMALIZED (irfft_ref(rfft_ref(x)) == n * x).  The imaginary parts of
    the self-conjugate DC and (even n) Nyquist entries are zeroed
    explicitly: they do not contribute, by the c2r convention."""
    X = numpy.array(X, dtype=CLD)
    X = numpy.moveaxis(X, axis, -1)
    X[..., 0] = X[..., 0].real
    if n % 2 == 0:
        X[..., n // 2] = X[..., n // 2].real
    out = numpy.fft.irfft(X, n=n, axis=-1) * LD(n)
    return numpy.moveaxis(out, -1, axis)


# ---- frequencies (csrc/nbk_common.h) ------------------------------------

def freq_full(i, n):
    """Signed frequency of index ``i`` on a full axis of size ``n``:
    numpy's fftfreq(n) * n bit for bit, i.e. (m * fl(1/n)) * n -- Nyquist
    negative for even n, no Nyquist for odd n, and at a non-power-of-two n
    NOT always the exact integer."""
    i = numpy.asarray(i, dtype='i8')
    m = numpy.where(i < n - n // 2, i, i - n).astype('f8')
    return (m * (1.0 / float(n))) * float(n)


def freq_half(i, n):
    """Frequency of index ``i`` on the compressed axis (0..n/2): exact
    integers, the even-n Nyquist stored negative."""
    i = numpy.asarray(i, dtype='i8')
    if n % 2 == 0:
        i = numpy.where(i == n // 2, -(n // 2), i)
    return i.astype('f8')


def grid_freqs(nmesh, real_field=False):
    """(fx, fy, fz) of every element of the identity-layout field, each
    broadcast to the field's shape (a compressed last axis unless
    ``real_field``)."""
    n0, n1, n2 = (int(n) for n in nmesh)
    fx = freq_full(numpy.arange(n0), n0)
    fy = freq_full(numpy.arange(n1), n1)
    if real_field:
        fz = freq_full(numpy.arange(n2), n2)
    else:
        fz = freq_half(numpy.arange(n2 // 2 + 1), n2)
    return numpy.broadcast_arrays(fx[:, None, None], fy[None, :, None],
                                  fz[None, None, :])


# ---- elementwise factors ------------------------------------------------

def _comp_divisor1(window, interlaced, wi):
    # what one axis divides the factor by (sinc^p, or the root of the
    # aliasing sum), in the operation order csrc/nbk_common.h documents
    if interlaced:
        s = 0.5 * wi
        with numpy.errstate(invalid='ignore', divide='ignore'):
            sc = numpy.where(s == 0.0, 1.0, numpy.sin(s) / s)
        p = sc * sc
        if window >= 1:
            p = p * sc
        if window >= 2:
            p = p * sc
        return p
    s2 = numpy.sin(0.5 * wi) * numpy.sin(0.5 * wi)
    if window == 0:
        d = 1.0 - 2.0 / 3.0 * s2
    elif window == 1:
        d = 1.0 - s2 + 2.0 / 15.0 * s2 * s2
    else:
        d = (1.0 - 4.0 / 3.0 * s2 + 2.0 / 5.0 * s2 * s2
             - 4.0 / 315.0 * s2 * s2 * s2)
    return numpy.sqrt(d)


def comp_factor(window, interlaced, w):
    """Compensation factor of the elements with circular frequencies
    ``w = (wx, wy, wz)``, w_i = 2 pi f_i / N_i: window 0/1/2 = CIC/TSC/PCS,
    -1 = none; ``interlaced`` picks 1/sinc^p, otherwise the aliasing-
    corrected forms.  Sequential divides, one per axis, as
    nbk_compensate_f64 composes them (tests/test_kspace_reference_cpu.py
    pins it to oracle.compensation_filter)."""
    w = numpy.broadcast_arrays(*[numpy.asarray(wi, dtype='f8') for wi in w])
    out = numpy.ones(w[0].shape)
    if window < 0:
        return out
    for wi in w:
        out = out / _comp_divisor1(window, interlaced, wi)
    return out


def circular(fx, fy, fz, nmesh):
    """w_i = 2 pi f_i / N_i in the kernels' operation order."""
    return [2.0 * numpy.pi * f / float(n)
            for f, n in zip((fx, fy, fz), nmesh)]


def interlace_phase(fx, fy, fz, nmesh):
    """exp(i k.H / 2) = exp(i pi (fx/n0 + fy/n1 + fz/n2)) in long double."""
    ang = PI_LD * (numpy.asarray(fx, dtype=LD) / LD(int(nmesh[0]))
                   + numpy.asarray(fy, dtype=LD) / LD(int(nmesh[1]))
                   + numpy.asarray(fz, dtype=LD) / LD(int(nmesh[2])))
    return numpy.cos(ang) + 1j * numpy.sin(ang)


def recon_factor(fx, fy, fz, box, axis, R, bias, f, los):
    """The FFTRecon displacement multiplier of include/nbk_hip.h:
    i k_axis / k^2 exp(-k^2 R^2 / 2) / (bias (1 + (f / bias) mu^2)),
    exactly 0 at k = 0.  Long double; k = f * 2 pi / L as the f64 kernels
    round it."""
    k = [numpy.asarray(fi * (2.0 * numpy.pi / float(L)), dtype=LD)
         for fi, L in zip((fx, fy, fz), box)]
    k2 = k[0] * k[0] + k[1] * k[1] + k[2] * k[2]
    zero = k2 == 0
    k2s = numpy.where(zero, LD(1), k2)
    mu = (k[0] * LD(los[0]) + k[1] * LD(los[1]) + k[2] * LD(los[2])) \
        / numpy.sqrt(k2s)
    fac = k[axis] / k2s * numpy.exp(-LD(0.5) * k2s * LD(R) * LD(R)) \
        / (LD(bias) * (1 + LD(f) / LD(bias) * mu * mu))
    fac = numpy.where(zero, LD(0), fac)
    return 1j * fac.astype(CLD)


# ---- binning ------------------------------------------------------------

def _digitize(x, edges):
    # numpy.digitize(x, edges): the count of edges <= x (right-open bins)
    return numpy.digitize(x, edges)


def _ld_bin_sum(index, terms, size):
    out = numpy.zeros(size, dtype=LD)
    numpy.add.at(out, index, numpy.asarray(terms, dtype=LD))
    return out


def bin_sums_ref(values, fx, fy, fz, nmesh, box, k2edges, muedges, los,
                 ells, hermitian=True, real_field=False,
                 absx=None, delta=None, err_scale=None):
    """project_to_basis sums of an explicit element list, unfolded.

    ``values[e]`` is the (complex or real) value of element e and
    ``fx, fy, fz`` its frequency triple as freq_full / freq_half return it.
    Per element, in f64 and in this order (the kernels' documented chain):

      k   = fl(f * fl(2 pi / L));   real_field: fl(fl(f * L) / N)
      k2  = (kx*kx + ky*ky) + kz*kz
      mu  = ((kx lx + ky ly) + kz lz) / sqrt(k2),  0 at k2 == 0
      bin = (digitize(k2, k2edges), digitize(mu, muedges))
      w   = 2 where hermitian and fz > 0, else 1
      xsum += sqrt(k2) w,  musum += mu w,  Nsum += w
      ysum[l] += (2l+1) H(P_l(mu) v):  on a doubled mode H keeps twice the
                 real part for even l and twice the imaginary part for odd
                 l; P_l by the three-term recurrence

    Returns a namespace of (Nx+2, Nmu+2) arrays: ``Nsum`` (int64),
    ``xsum``, ``musum`` (f64 from long-double accumulation), ``ysum``
    (complex, (nell, Nx+2, Nmu+2)), ``n_terms`` (elements per bin) and the
    sums of the terms' magnitudes ``abs_xsum``, ``abs_musum``,
    ``abs_ysum`` (complex: its real part bounds the terms of Re ysum, its
    imaginary part those of Im ysum; both take the element's modulus |v|,
    and are 0 where H drops that part or the values are real).  Nothing is
    folded and no row is dropped.

    With ``absx``, ``delta`` and ``err_scale`` (per element) it also
    returns ``err_ysum`` (nell, ...): the sum of
    w err_scale (2l+1) |P_l| (2 absx delta + delta^2) -- how far an error
    of ``delta`` in an element of magnitude ``absx`` can move the real part
    of ysum when the element value is err_scale |X|^2 (w as H applies it:
    2 on doubled modes, where the odd-l real part is exactly 0).
    """
    values = numpy.asarray(values).ravel()
    fx = numpy.asarray(fx, dtype='f8').ravel()
    fy = numpy.asarray(fy, dtype='f8').ravel()
    fz = numpy.asarray(fz, dtype='f8').ravel()
    k2edges = numpy.asarray(k2edges, dtype='f8')
    muedges = numpy.asarray(muedges, dtype='f8')
    Nx, Nmu = len(k2edges) - 1, len(muedges) - 1
    shape = (Nx + 2, Nmu + 2)
    NB = shape[0] * shape[1]

    if real_field:
        kx = (fx * float(box[0])) / float(nmesh[0])
        ky = (fy * float(box[1])) / float(nmesh[1])
        kz = (fz * float(box[2])) / float(nmesh[2])
    else:
        kx = fx * (2.0 * numpy.pi / float(box[0]))
        ky = fy * (2.0 * numpy.pi / float(box[1]))
        kz = fz * (2.0 * numpy.pi / float(box[2]))
    k2 = (kx * kx + ky * ky) + kz * kz
    kmag = numpy.sqrt(k2)
    dot = (kx * float(los[0]) + ky * float(los[1])) + kz * float(los[2])
    with numpy.errstate(invalid='ignore', divide='ignore'):
        mu = numpy.where(kmag == 0.0, 0.0, dot / kmag)

    index = _digitize(k2, k2edges) * (Nmu + 2) + _digitize(mu, muedges)
    doubled = (fz > 0.0) if (hermitian and not real_field) \
        else numpy.zeros(fz.shape, dtype=bool)
    w = numpy.where(doubled, 2.0, 1.0)

    out = SimpleNamespace()
    out.n_terms = numpy.bincount(index, minlength=NB).reshape(shape)
    out.Nsum = numpy.bincount(index, weights=w, minlength=NB) \
        .round().astype('i8').reshape(shape)
    for name, term in (('xsum', kmag * w), ('musum', mu * w)):
        setattr(out, name,
                _ld_bin_sum(index, term, NB).astype('f8').reshape(shape))
        setattr(out, 'abs_' + name,
                _ld_bin_sum(index, numpy.abs(term), NB).astype('f8')
                .reshape(shape))

    nell = len(ells)
    out.ysum = numpy.zeros((nell,) + shape, dtype='c16')
    out.abs_ysum = numpy.zeros((nell,) + shape, dtype='c16')
    with_err = absx is not None
    if with_err:
        absx = numpy.asarray(absx, dtype='f8').ravel()
        delta = numpy.broadcast_to(
            numpy.asarray(delta, dtype='f8').ravel(), absx.shape)
        err_scale = numpy.broadcast_to(
            numpy.asarray(err_scale, dtype='f8').ravel(), absx.shape)
        verr = err_scale * (2.0 * absx * delta + delta * delta)
        out.err_ysum = numpy.zeros((nell,) + shape)

    is_complex = numpy.iscomplexobj(values)
    vre = values.real.astype('f8')
    vim = values.imag.astype('f8') if is_complex \
        else numpy.zeros(vre.shape)
    vabs = numpy.hypot(vre, vim)
    Pm1 = numpy.zeros(mu.shape)
    P = numpy.ones(mu.shape)
    e = 0
    ells = [int(l) for l in ells]
    for l in range(max(ells) + 1 if ells else 0):
        if l > 0:
            Pn = ((2 * l - 1) * mu * P - (l - 1) * Pm1) / l
            Pm1, P = P, Pn
        if e < nell and l == ells[e]:
            tre, tim = vre * P, vim * P
            if l % 2:
                tre = numpy.where(doubled, 0.0, tre)
                tim = numpy.where(doubled, 2.0 * tim, tim)
            else:
                tre = numpy.where(doubled, 2.0 * tre, tre)
                tim = numpy.where(doubled, 0.0, tim)
            tre = tre * (2.0 * l + 1.0)
            tim = tim * (2.0 * l + 1.0)
            out.ysum[e] = (
                _ld_bin_sum(index, tre, NB).astype('f8')
                + 1j * _ld_bin_sum(index, tim, NB).astype('f8')
            ).reshape(shape)
            # magnitudes by the element's MODULUS: the rounding error of
            # a product-built value is relative to |v|, not to the part
            # of it that H keeps
            tabs = numpy.where(doubled, 2.0, 1.0) * (2.0 * l + 1.0) \
                * numpy.abs(P) * vabs
            are = numpy.where(doubled & bool(l % 2), 0.0, tabs)
            aim = numpy.where(doubled & (not l % 2), 0.0, tabs) \
                if is_complex else numpy.zeros(tabs.shape)
            out.abs_ysum[e] = (
                _ld_bin_sum(index, are, NB).astype('f8')
                + 1j * _ld_bin_sum(index, aim, NB).astype('f8')
            ).reshape(shape)
            if with_err:
                wl = numpy.where(doubled, 0.0 if l % 2 else 2.0, 1.0)
                out.err_ysum[e] = _ld_bin_sum(
                    index, wl * (2.0 * l + 1.0) * numpy.abs(P) * verr,
                    NB).astype('f8').reshape(shape)
            e += 1
    if e != nell:
        raise ValueError("ells must be ascending and distinct")
    return out
