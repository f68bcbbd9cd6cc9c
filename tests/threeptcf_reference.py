"""
Host references of the isotropic 3PCF multipoles (DESIGN.md "Three-point
correlation function"), written from the formulas, in plain numpy:

(a) :func:`alm_zeta` — the a_lm algorithm: per primary, a_lm(b) = sum_j
    w_j Y_lm(d_ij / r) over the secondaries of radial bin b, then
    zeta_l(b1, b2) = 1/(4 pi) sum_i w_i sum_{m=0..l} c_m Re[a_lm(b1)
    conj(a_lm(b2))], c_0 = 1, c_m = 2.  Y_lm = N_lm Pt_l^m(z) (x + i y)^m
    with Pt_m^m = (2m - 1)!!, (l - m) Pt_l^m = (2l - 1) z Pt_(l-1)^m -
    (l + m - 1) Pt_(l-2)^m, N_lm^2 = (2l + 1)/(4 pi) (l - m)!/(l + m)!.
(b) :func:`bruteforce_zeta` — the addition theorem: (2l + 1)/(4 pi)^2
    sum_i w_i sum_{j in b1} sum_{k in b2} w_j w_k P_l(d_ij . d_ik), the
    j = k terms included, with numpy.polynomial.legendre.
(c) :func:`edge_margin` — the smallest |r / edge - 1| over all pairs and
    edges: how far the catalogue is from a binning decision that rounding
    could flip.

Bins are open below and closed above (searchsorted side='left') on
squared separations; d is the minimum image when ``box`` is given; pairs
at r = 0 are dropped.
"""
import os
from math import factorial

import numpy
from numpy.polynomial import legendre

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        'golden', 'ref_fixtures')
FIXTURE_BOX = 400.0


def load_fixture():
    """(positions in the 400 box, weights) of threeptcf_sim_data.dat"""
    data = numpy.loadtxt(os.path.join(FIXTURES, 'threeptcf_sim_data.dat'))
    return data[:, :3] * FIXTURE_BOX, data[:, 3].copy()


def load_golden():
    """truth[l, b1, b2], l = 0..10, 8 bins of linspace(0, 200, 9), as
    printed (7 digits) by the C++ code of Slepian & Eisenstein; it equals
    zeta_l (4 pi)^2 / (2l + 1)"""
    truth = numpy.full((11, 8, 8), numpy.nan)
    with open(os.path.join(FIXTURES, 'threeptcf_sim_result.dat')) as ff:
        for line in ff:
            fields = line.split()
            i, j = int(fields[0]), int(fields[1])
            truth[:, i, j] = truth[:, j, i] = [float(f) for f in fields[2:]]
    assert not numpy.isnan(truth).any()
    return truth


def golden_rescale(zeta):
    """zeta[l, ...] (4 pi)^2 / (2l + 1): the golden file's normalisation"""
    ell = numpy.arange(len(zeta)).reshape(-1, 1, 1)
    return zeta * (4 * numpy.pi) ** 2 / (2 * ell + 1)


def separations(pos, i, box):
    """d = p_j - p_i (minimum image) and r^2 = (dx^2 + dy^2) + dz^2"""
    d = pos - pos[i]
    if box is not None:
        L = numpy.ones(3) * box
        for axis in range(3):
            col = d[:, axis]
            col[col > 0.5 * L[axis]] -= L[axis]
            col[col <= -0.5 * L[axis]] += L[axis]
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return d, q


def radial_bins(q, edges):
    """(selection, bin of the selected): edges[b] < r <= edges[b+1] on
    squared values, r = 0 dropped"""
    esq = numpy.asarray(edges, dtype='f8') ** 2
    dig = numpy.searchsorted(esq, q, side='left')
    sel = (dig >= 1) & (dig <= len(esq) - 1) & (q > 0)
    return sel, dig[sel] - 1


def ylm_unnormalised(lmax, unit):
    """Pt_l^m(z) (x + i y)^m for 0 <= m <= l <= lmax: complex
    [n_lm, len(unit)], row l (l + 1) / 2 + m"""
    xy = unit[:, 0] + 1j * unit[:, 1]
    z = unit[:, 2]
    out = numpy.empty(((lmax + 1) * (lmax + 2) // 2, len(unit)), dtype='c16')
    pmm, power = 1.0, numpy.ones(len(unit), dtype='c16')
    for m in range(lmax + 1):
        if m > 0:
            pmm *= 2 * m - 1
            power = power * xy
        prev2, prev1 = numpy.zeros(len(unit)), numpy.full(len(unit), pmm)
        out[m * (m + 1) // 2 + m] = prev1 * power
        for l in range(m + 1, lmax + 1):
            cur = ((2 * l - 1) * z * prev1 - (l + m - 1) * prev2) / (l - m)
            out[l * (l + 1) // 2 + m] = cur * power
            prev2, prev1 = prev1, cur
    return out


def zeta_weights(lmax):
    """c_m N_lm^2 / (4 pi) per row of :func:`ylm_unnormalised`"""
    k = numpy.empty((lmax + 1) * (lmax + 2) // 2)
    for l in range(lmax + 1):
        for m in range(l + 1):
            n2 = (2 * l + 1) / (4 * numpy.pi) \
                * (factorial(l - m) / factorial(l + m))
            k[l * (l + 1) // 2 + m] = (1 if m == 0 else 2) * n2 \
                / (4 * numpy.pi)
    return k


def alm_zeta(pos, w, edges, lmax, box=None):
    """(a): zeta[l, b1, b2] for l <= lmax by the a_lm algorithm"""
    pos = numpy.asarray(pos, dtype='f8')
    w = numpy.asarray(w, dtype='f8')
    nbins = len(edges) - 1
    kz = zeta_weights(lmax)
    zeta = numpy.zeros((lmax + 1, nbins, nbins))
    for i in range(len(pos)):
        d, q = separations(pos, i, box)
        sel, b = radial_bins(q, edges)
        if not sel.any():
            continue
        unit = d[sel] / numpy.sqrt(q[sel])[:, None]
        onehot = numpy.zeros((len(b), nbins))
        onehot[numpy.arange(len(b)), b] = w[sel]
        alm = ylm_unnormalised(lmax, unit) @ onehot.astype('c16')
        # Re[a(b1) conj(a(b2))] weighted per (l, m), summed over m
        outer = (alm.real[:, :, None] * alm.real[:, None, :]
                 + alm.imag[:, :, None] * alm.imag[:, None, :])
        outer *= kz[:, None, None]
        for l in range(lmax + 1):
            k0 = l * (l + 1) // 2
            zeta[l] += w[i] * outer[k0:k0 + l + 1].sum(axis=0)
    return zeta


def bruteforce_zeta(pos, w, edges, lmax, box=None):
    """(b): the same by the addition theorem, O(N^3)"""
    pos = numpy.asarray(pos, dtype='f8')
    w = numpy.asarray(w, dtype='f8')
    nbins = len(edges) - 1
    zeta = numpy.zeros((lmax + 1, nbins, nbins))
    for i in range(len(pos)):
        d, q = separations(pos, i, box)
        sel, b = radial_bins(q, edges)
        if not sel.any():
            continue
        unit = d[sel] / numpy.sqrt(q[sel])[:, None]
        cosine = unit @ unit.T
        onehot = numpy.zeros((len(b), nbins))
        onehot[numpy.arange(len(b)), b] = w[sel]
        for l in range(lmax + 1):
            pl = legendre.legval(cosine, [0] * l + [1])
            zeta[l] += w[i] * (2 * l + 1) / (4 * numpy.pi) ** 2 \
                * (onehot.T @ pl @ onehot)
    return zeta


def edge_margin(pos, box, edges):
    """(c): min over pairs (r > 0) and edges (> 0) of |r / edge - 1|"""
    pos = numpy.asarray(pos, dtype='f8')
    edges = numpy.asarray(edges, dtype='f8')
    edges = edges[edges > 0]
    best = numpy.inf
    for i in range(len(pos)):
        _, q = separations(pos, i, box)
        r = numpy.sqrt(q[q > 0])
        if len(r):
            best = min(best,
                       numpy.abs(r[:, None] / edges[None, :] - 1).min())
    return best


def cauchy_schwarz_scale(zeta):
    """sqrt(zeta_l(b1, b1) zeta_l(b2, b2)): the size an entry can have"""
    diag = numpy.einsum('lbb->lb', zeta)
    assert (diag >= 0).all()
    return numpy.sqrt(diag[:, :, None] * diag[:, None, :])


def assert_zeta_close(got, want, rtol):
    """|got - want| <= rtol * the Cauchy-Schwarz scale of ``want``;
    entries whose scale is 0 must be exactly 0"""
    scale = cauchy_schwarz_scale(want)
    err = numpy.abs(got - want)
    live = scale > 0
    worst = (err[live] / scale[live]).max() if live.any() else 0.
    print('max |err| / scale = %.3g (bound %.3g)' % (worst, rtol))
    assert (got[~live] == 0).all()
    assert (err <= rtol * scale).all()
