"""
Correlation-function estimators on pair counts (reference
nbodykit/algorithms/paircount_tpcf/estimators.py): the natural estimator
DD/RR - 1 against analytic uniform randoms in a periodic box, and the
Landy-Szalay estimator against catalogue randoms.  Host-side numpy on the
few-bin results of SimulationBoxPairCount.
"""
import warnings

import numpy

from nbodykit_amd.binned_statistic import BinnedStatistic


class WedgeBinnedStatistic(BinnedStatistic):
    """A BinnedStatistic of (r, mu) wedges that converts to multipoles."""

    def to_poles(self, poles):
        r"""
        Multipoles :math:`\xi_\ell(r)` of the wedges :math:`\xi(r,\mu)`
        by the midpoint rule:
        :math:`\sum (2\ell+1) P_\ell(\mu_{mid}) \xi \Delta\mu
        / \sum \Delta\mu`.  Returns a BinnedStatistic over the first
        dimension with variables ``corr_<ell>`` and the mean separation.
        """
        x = str(self.dims[0])
        dmu = numpy.diff(self.edges['mu'])
        mu_mid = 0.5 * (self.edges['mu'][1:] + self.edges['mu'][:-1])

        dtype = [(x, 'f8')] + [('corr_%d' % ell, 'f8') for ell in poles]
        data = numpy.zeros(self.shape[0], dtype=dtype)
        for ell in poles:
            coeffs = numpy.zeros(int(ell) + 1)
            coeffs[-1] = 1.0
            kernel = (2. * ell + 1.) \
                * numpy.polynomial.legendre.legval(mu_mid, coeffs)
            data['corr_%d' % ell] = \
                numpy.sum(self['corr'] * kernel * dmu, axis=-1) \
                / numpy.sum(dmu)
        data[x] = numpy.mean(self[x], axis=-1)
        return BinnedStatistic(dims=[x], edges=[self.edges[x]], data=data,
                               poles=poles)


def filling_factor(mode, edges, BoxSize):
    """
    Fraction of the box volume each bin occupies, for uniformly
    distributed pairs: spherical shells ('1d'), spherical sectors counted
    on both sides of the line of sight ('2d', binned in |mu|), or
    cylinder shells of height 2 pi ('projected').  ``edges`` is the dict
    of bin edges of the pair counts.
    """
    volume = numpy.prod(numpy.ones(3) * BoxSize)
    if mode == '1d':
        shells = 4. / 3. * numpy.pi * numpy.asarray(edges['r']) ** 3
        return numpy.diff(shells) / volume
    if mode == '2d':
        sectors = 4. / 3. * numpy.pi * numpy.outer(
            numpy.asarray(edges['r']) ** 3, edges['mu'])
        return numpy.diff(numpy.diff(sectors, axis=0), axis=1) / volume
    if mode == 'projected':
        cylinders = numpy.pi * numpy.outer(
            numpy.asarray(edges['rp']) ** 2, 2. * numpy.asarray(edges['pi']))
        return numpy.diff(numpy.diff(cylinders, axis=0), axis=1) / volume
    raise ValueError("no analytic randoms for mode '%s'" % mode)


def analytic_randoms(mode, dims, edges, BoxSize, N1, N2=None):
    """Expected pair counts of uniform randoms: a WedgeBinnedStatistic
    with ``npairs`` = ``wnpairs`` = N1 N2 (or N1^2) x filling factor and
    ``attrs['total_wnpairs']`` = N1 (N1 - 1) / 2 (or N1 N2 / 2)."""
    fill = filling_factor(mode, edges, BoxSize)
    if N2 is None:
        RR = float(N1) ** 2 * fill
        total = 0.5 * N1 * (N1 - 1)
    else:
        RR = float(N1) * float(N2) * fill
        total = 0.5 * N1 * N2
    data = numpy.empty(RR.shape, dtype=[('npairs', 'f8'),
                                        ('wnpairs', 'f8')])
    data['npairs'] = RR
    data['wnpairs'] = RR
    pairs = WedgeBinnedStatistic(dims, [edges[d] for d in dims], data)
    pairs.attrs['total_wnpairs'] = total
    return pairs


def natural_corr(DD, DD_total, RR, RR_total):
    """DD (RR_total / DD_total) / RR - 1 on weighted counts."""
    return (DD * (RR_total / DD_total)) / RR - 1.


def landy_szalay_corr(DD, DR, RD, RR, DD_total, DR_total, RD_total,
                      RR_total, RR_npairs):
    """(fDD DD - fDR DR - fRD RD) / RR + 1 with f = RR_total / total;
    NaN where the randoms have no pairs."""
    fDD = RR_total / DD_total
    fDR = RR_total / DR_total
    fRD = RR_total / RD_total
    corr = numpy.full(numpy.shape(DD), numpy.nan)
    ok = numpy.asarray(RR_npairs) > 0
    corr[ok] = (fDD * DD[ok] - fDR * DR[ok] - fRD * RD[ok]) / RR[ok] + 1
    return corr


def make_corr(pairs, corr):
    """The result container: ``corr`` and the mean separation of the
    data-data counts."""
    x = pairs.dims[0]
    data = numpy.empty(corr.shape, dtype=[('corr', 'f8'), (x, 'f8')])
    data['corr'] = corr
    data[x] = pairs[x]
    return WedgeBinnedStatistic(pairs.dims,
                                [pairs.edges[d] for d in pairs.dims], data)


def NaturalEstimator(D1D2):
    """(R1R2 pairs, corr) of a finished periodic data-data pair count
    using analytic randoms."""
    attrs = D1D2.attrs
    N2 = attrs['N2'] if attrs['is_cross'] else None
    R1R2 = analytic_randoms(attrs['mode'], D1D2.pairs.dims,
                            D1D2.pairs.edges, attrs['BoxSize'],
                            attrs['N1'], N2)
    corr = natural_corr(D1D2.pairs['wnpairs'], attrs['total_wnpairs'],
                        R1R2['wnpairs'], R1R2.attrs['total_wnpairs'])
    return R1R2, make_corr(D1D2.pairs, corr)


def LandySzalayEstimator(pair_counter, data1, data2, randoms1, randoms2,
                         R1R2=None, logger=None, **kwargs):
    """Run the pair counts of the Landy-Szalay estimator (four, or three
    for an auto-correlation; a supplied ``R1R2`` is reused) and return
    (D1D2, D1R2, D2R1, R1R2, corr)."""
    if randoms1 is None:
        raise ValueError("the Landy-Szalay estimator needs randoms")
    if randoms2 is None:
        randoms2 = randoms1

    def count(name, first, second):
        if logger is not None and data1.comm.rank == 0:
            logger.info("computing %s pair counts" % name)
        return pair_counter(first=first, second=second, **kwargs)

    if R1R2 is None:
        R1R2 = count('randoms1 - randoms2', randoms1, randoms2)
    D1D2 = count('data1 - data2', data1, data2)
    D1R2 = count('data1 - randoms2', data1, randoms2)
    D2R1 = D1R2
    if data2 is not None:
        D2R1 = count('data2 - randoms1', data2, randoms1)

    corr = landy_szalay_corr(
        D1D2.pairs['wnpairs'], D1R2.pairs['wnpairs'], D2R1.pairs['wnpairs'],
        R1R2.pairs['wnpairs'], D1D2.attrs['total_wnpairs'],
        D1R2.attrs['total_wnpairs'], D2R1.attrs['total_wnpairs'],
        R1R2.attrs['total_wnpairs'], R1R2.pairs['npairs'])
    if data1.comm.rank == 0 and numpy.isnan(corr).any():
        warnings.warn("the randoms-randoms counts of the Landy-Szalay "
                      "estimator have empty separation bins; the "
                      "correlation function is NaN there.  Use more "
                      "randoms or broader bins.")
    return (D1D2.pairs, D1R2.pairs, D2R1.pairs, R1R2.pairs,
            make_corr(D1D2.pairs, corr))
