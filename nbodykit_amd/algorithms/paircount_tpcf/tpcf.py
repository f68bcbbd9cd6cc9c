"""
SimulationBox2PCF and SurveyData2PCF — the two-point correlation function
by pair counting (reference nbodykit/algorithms/paircount_tpcf/tpcf.py).
In a simulation box: natural estimator with analytic randoms for a
periodic box without randoms, Landy-Szalay otherwise.  For survey data:
always Landy-Szalay.  ``wp(rp)`` in projected mode.
"""
import logging

import numpy

from nbodykit_amd import CurrentMPIComm
from ..pair_counters import SimulationBoxPairCount, SurveyDataPairCount
from .estimators import (LandySzalayEstimator, NaturalEstimator,
                         WedgeBinnedStatistic)

PAIR_COUNTS = ['D1D2', 'D1R2', 'D2R1', 'R1R2']


def compute_wp(corr):
    """wp(rp) = sum over pi of 2 xi(rp, pi) dpi, as a WedgeBinnedStatistic
    over rp with ``corr`` and the pi-averaged ``rp``."""
    x = corr.dims[0]
    dpi = numpy.diff(corr.edges[corr.dims[1]])
    data = numpy.empty(corr.shape[0], dtype=[('corr', 'f8'), (x, 'f8')])
    data['corr'] = (2 * corr['corr'] * dpi).sum(axis=-1)
    data[x] = numpy.mean(corr[x], axis=-1)
    return WedgeBinnedStatistic([x], [corr.edges[x]], data)


class BasePairCount2PCF(object):
    """State, save and load of a finished correlation function."""

    def __getstate__(self):
        state = {'corr': self.corr.data, 'dims': self.corr.dims,
                 'edges': [self.corr.edges[d] for d in self.corr.dims]}
        for name in PAIR_COUNTS + ['wp']:
            value = getattr(self, name, None)
            state[name] = value.data if value is not None else None
        state['attrs'] = self.attrs
        return state

    def __setstate__(self, state):
        dims, edges = list(state['dims']), state['edges']
        self.attrs = state['attrs']
        self.corr = WedgeBinnedStatistic(dims, edges, state['corr'])
        self.wp = None
        if state.get('wp') is not None:
            # the second dimension was summed over
            self.wp = WedgeBinnedStatistic(dims[:1], edges[:1],
                                           state['wp'])
        for name in PAIR_COUNTS:
            value = state.get(name)
            if value is not None:
                value = WedgeBinnedStatistic(dims, edges, value)
            setattr(self, name, value)

    def save(self, output):
        """Save the result as a JSON file ``output``."""
        import json
        from nbodykit_amd.utils import JSONEncoder
        if self.comm.rank == 0:
            self.logger.info('measurement done; saving result to %s'
                             % output)
            with open(output, 'w') as ff:
                json.dump(self.__getstate__(), ff, cls=JSONEncoder)

    @classmethod
    @CurrentMPIComm.enable
    def load(cls, output, comm=None):
        """Load a result saved with :func:`save`."""
        import json
        from nbodykit_amd.utils import JSONDecoder
        if comm.rank == 0:
            with open(output, 'r') as ff:
                state = json.load(ff, cls=JSONDecoder)
        else:
            state = None
        state = comm.bcast(state)
        self = object.__new__(cls)
        self.__setstate__(state)
        self.comm = comm
        return self


class SimulationBox2PCF(BasePairCount2PCF):
    """
    Two-point correlation function of data in a simulation box as a
    function of r, (r, mu) or (rp, pi).

    Parameters follow ``nbodykit.algorithms.SimulationBox2PCF``.  Without
    ``randoms1`` a periodic box uses the natural estimator against
    analytic (unweighted) uniform randoms; with randoms the Landy-Szalay
    estimator runs (``randoms2`` defaults to ``randoms1``; a supplied
    ``R1R2`` pair count is reused).  Results: :attr:`D1D2`, :attr:`D1R2`,
    :attr:`D2R1`, :attr:`R1R2` (pair counts), :attr:`corr` and, for
    ``mode='projected'``, :attr:`wp`.
    """
    logger = logging.getLogger('SimulationBox2PCF')

    def __init__(self, mode, data1, edges, Nmu=None, pimax=None,
                 data2=None, randoms1=None, randoms2=None, R1R2=None,
                 periodic=True, BoxSize=None, los='z', weight='Weight',
                 position='Position', show_progress=False, **config):
        if mode == 'angular':
            raise NotImplementedError(
                "mode='angular' is not implemented in nbodykit_amd")
        self.comm = data1.comm
        self.attrs = {'mode': mode, 'edges': numpy.array(edges),
                      'Nmu': Nmu, 'pimax': pimax, 'periodic': periodic,
                      'BoxSize': BoxSize, 'los': los, 'weight': weight,
                      'position': position, 'show_progress': show_progress,
                      'config': config}
        self.data1 = data1
        self.data2 = data2
        self.randoms1 = randoms1
        self.randoms2 = randoms2
        self.R1R2 = R1R2
        self.run()

    def run(self):
        """Count the pairs and evaluate the estimator."""
        kws = self.attrs.copy()
        kws.update(kws.pop('config'))

        if kws['periodic'] and self.randoms1 is None:
            DD = SimulationBoxPairCount(first=self.data1,
                                        second=self.data2, **kws)
            self.R1R2, self.corr = NaturalEstimator(DD)
            self.D1D2 = DD.pairs
            self.D1R2 = self.D2R1 = None
        else:
            if self.randoms1 is None:
                raise ValueError(
                    "a catalog of randoms must be specified as the "
                    "``randoms1`` keyword when the data is not in a "
                    "simulation box with periodic boundary conditions")
            if self.data2 is not None and self.randoms2 is None:
                self.randoms2 = self.randoms1
            (self.D1D2, self.D1R2, self.D2R1, self.R1R2,
             self.corr) = LandySzalayEstimator(
                SimulationBoxPairCount, self.data1, self.data2,
                self.randoms1, self.randoms2, R1R2=self.R1R2,
                logger=self.logger, **kws)

        self.wp = None
        if self.attrs['mode'] == 'projected':
            self.wp = compute_wp(self.corr)


class SurveyData2PCF(BasePairCount2PCF):
    """
    Two-point correlation function of survey data (RA, DEC, redshift) as
    a function of r, (r, mu), (rp, pi) or theta, by the Landy-Szalay
    estimator.

    Parameters follow ``nbodykit.algorithms.SurveyData2PCF``:
    ``randoms1`` is required, ``randoms2`` defaults to ``randoms1`` in a
    cross-correlation, and a supplied ``R1R2`` pair count is reused.
    Results: :attr:`D1D2`, :attr:`D1R2`, :attr:`D2R1`, :attr:`R1R2` (pair
    counts), :attr:`corr` and, for ``mode='projected'``, :attr:`wp`.
    """
    logger = logging.getLogger('SurveyData2PCF')

    def __init__(self, mode, data1, randoms1, edges, cosmo=None, Nmu=None,
                 pimax=None, data2=None, randoms2=None, R1R2=None,
                 ra='RA', dec='DEC', redshift='Redshift', weight='Weight',
                 show_progress=False, **config):
        self.comm = data1.comm
        self.attrs = {'mode': mode, 'edges': numpy.array(edges),
                      'cosmo': cosmo, 'Nmu': Nmu, 'pimax': pimax,
                      'ra': ra, 'dec': dec, 'redshift': redshift,
                      'weight': weight, 'show_progress': show_progress,
                      'config': config}
        self.data1 = data1
        self.data2 = data2
        self.randoms1 = randoms1
        self.randoms2 = randoms2
        self.R1R2 = R1R2
        self.run()

    def run(self):
        """Count the pairs and evaluate the estimator."""
        kws = self.attrs.copy()
        kws.update(kws.pop('config'))
        if self.data2 is not None and self.randoms2 is None:
            self.randoms2 = self.randoms1
        (self.D1D2, self.D1R2, self.D2R1, self.R1R2,
         self.corr) = LandySzalayEstimator(
            SurveyDataPairCount, self.data1, self.data2, self.randoms1,
            self.randoms2, R1R2=self.R1R2, logger=self.logger, **kws)

        self.wp = None
        if self.attrs['mode'] == 'projected':
            self.wp = compute_wp(self.corr)
