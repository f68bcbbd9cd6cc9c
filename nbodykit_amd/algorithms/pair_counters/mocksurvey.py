"""
SurveyDataPairCount — pair counts of a sky catalogue (RA, DEC, redshift)
as a function of r, (r, mu), (rp, pi) or theta (reference
nbodykit/algorithms/pair_counters/mocksurvey.py and base.py).  The
reference hands the arithmetic to Corrfunc.mocks; here it is the sky
modes of the cell-list HIP kernel of csrc/nbk_pairs.hip, driven by
:mod:`.kernel`.

Semantics (DESIGN.md "Survey pair counting"): the observer is at the
origin, the line of sight of a pair is its midpoint direction p1 + p2,
the grid is never periodic, first-dimension bins are closed below and
open above on squared separations (squared chords in angular mode),
``npairs`` counts ordered pairs, ``wnpairs`` sums w1 w2 and the first
variable is the mean separation (or angle in degrees) of the bin, 0 when
it is empty.
"""
import logging

import numpy

from nbodykit_amd import CurrentMPIComm, transform
from nbodykit_amd.binned_statistic import BinnedStatistic
from . import simbox
from .simbox import VALID_MODES, _column_sum, pairs_data


def second_dim(mode, Nmu, pimax):
    """(dims, second-dimension edges or None) of a mode; the simulation
    box's, plus ``theta``."""
    if mode == 'angular':
        return ['theta'], None
    return simbox.second_dim(mode, Nmu, pimax)


def make_pairs(mode, edges, Nmu, pimax, data):
    """The ``pairs`` BinnedStatistic of a result array."""
    if mode == 'angular':
        return BinnedStatistic(['theta'], [numpy.asarray(edges, dtype='f8')],
                               data, fields_to_sum=['npairs', 'wnpairs'])
    return simbox.make_pairs(mode, edges, Nmu, pimax, data)


def prepare_attrs(mode, first, edges, cosmo=None, second=None, Nmu=None,
                  pimax=None, ra='RA', dec='DEC', redshift='Redshift',
                  weight='Weight', show_progress=False, domain_factor=4,
                  config=None):
    """Validate the arguments of SurveyDataPairCount and return its
    ``attrs`` (everything known before the GPU is needed)."""
    config = {} if config is None else config
    if mode not in VALID_MODES:
        raise ValueError("allowed 'mode' values are: %s" % VALID_MODES)

    # sources: columns (no redshift on the unit sphere)
    required = [ra, dec, weight]
    if mode != 'angular':
        required.append(redshift)
    other = first if second is None else second
    for source in (first, other):
        for col in required:
            if col not in source:
                raise ValueError("the column '%s' is missing from input "
                                 "source; cannot do pair count" % col)
    if mode != 'angular' and cosmo is None:
        raise ValueError("'cosmo' keyword is required when 'mode' is not "
                         "'angular'")

    # binning arguments
    edges = numpy.array(edges, dtype='f8')
    if edges.ndim != 1 or len(edges) < 2 \
            or not numpy.all(numpy.diff(edges) > 0):
        raise ValueError("'edges' must be an increasing sequence of at "
                         "least two bin edges")
    if numpy.min(edges) <= 0.:
        raise ValueError("the lower edge of the 1st separation bin must "
                         "greater than zero (no self-pairs)")
    if mode == 'angular' and numpy.max(edges) > 180.:
        raise ValueError("angular 'edges' are in degrees and must "
                         "satisfy 0 < theta <= 180")
    if mode == '2d' and Nmu is None:
        raise ValueError("'Nmu' keyword is required when 'mode' is '2d'")
    if Nmu is not None and mode != '2d':
        raise ValueError("mode should be '2d' if 'Nmu' is specified")
    if mode == 'projected' and pimax is None:
        raise ValueError("'pimax' keyword is required when 'mode' is "
                         "'projected'")
    if pimax is not None and mode != 'projected':
        raise ValueError("mode should be 'projected' if 'pimax' is "
                         "specified")
    if mode == 'projected' and pimax < 1.0:
        raise ValueError("'pimax' must be at least 1.0 when 'mode' is "
                         "'projected'")
    if mode == '2d' and int(Nmu) < 1:
        raise ValueError("'Nmu' must be at least 1")

    comm = first.comm
    is_cross = not (second is None or second is first)
    attrs = {}
    attrs['mode'] = mode
    attrs['edges'] = edges
    attrs['Nmu'] = Nmu
    attrs['pimax'] = pimax
    attrs['show_progress'] = show_progress
    attrs['N1'] = first.csize
    attrs['N2'] = second.csize if second is not None else None

    # the total weighted pair count, as in the simulation box
    W1 = comm.allreduce(_column_sum(first[weight]))
    if is_cross:
        W2 = comm.allreduce(_column_sum(second[weight]))
        attrs['total_wnpairs'] = 0.5 * W1 * W2
    else:
        W1sq = comm.allreduce(_column_sum(first[weight], 2))
        attrs['total_wnpairs'] = 0.5 * (W1 ** 2 - W1sq)
    attrs['is_cross'] = is_cross

    attrs['cosmo'] = cosmo
    attrs['ra'] = ra
    attrs['dec'] = dec
    attrs['redshift'] = redshift
    attrs['weight'] = weight
    attrs['domain_factor'] = domain_factor
    attrs['config'] = config

    if comm.size > 1:
        raise NotImplementedError(
            "SurveyDataPairCount runs on a single rank")
    return attrs


def _host_column(col):
    """a column as a native f64 numpy array (device columns are copied to
    the host: the distance-redshift relation is a host table)"""
    if hasattr(col, 'detach'):            # torch tensor
        col = col.detach().cpu().numpy()
    col = numpy.asarray(col)
    return numpy.ascontiguousarray(col, dtype='f8')


def sky_positions(source, attrs):
    """(n, 3) host positions: Cartesian Mpc/h from the origin, or unit
    vectors in angular mode."""
    ra = _host_column(source[attrs['ra']])
    dec = _host_column(source[attrs['dec']])
    if attrs['mode'] == 'angular':
        return transform.SkyToUnitSphere(ra, dec)
    z = _host_column(source[attrs['redshift']])
    return transform.SkyToCartesian(ra, dec, z, attrs['cosmo'])


class SurveyDataPairCount(object):
    """
    Count (weighted) pairs of objects of a survey catalogue, seen from
    the origin.

    Parameters follow ``nbodykit.algorithms.SurveyDataPairCount``:
    ``mode`` is '1d', '2d' (needs ``Nmu``), 'projected' (needs ``pimax``)
    or 'angular' (``edges`` in degrees, no redshift and no ``cosmo``
    needed); ``cosmo`` turns redshifts into comoving distances;
    ``second`` selects a cross-correlation.  ``show_progress``,
    ``domain_factor`` and ``**config`` are accepted and recorded only.
    Columns may be numpy arrays or device tensors.

    The result is :attr:`pairs`, a BinnedStatistic with the variables
    ``r`` (``rp``, ``theta``), ``npairs`` and ``wnpairs``.
    """
    logger = logging.getLogger('SurveyDataPairCount')

    def __init__(self, mode, first, edges, cosmo=None, second=None,
                 Nmu=None, pimax=None, ra='RA', dec='DEC',
                 redshift='Redshift', weight='Weight', show_progress=False,
                 domain_factor=4, **config):
        self.attrs = prepare_attrs(mode, first, edges, cosmo, second, Nmu,
                                   pimax, ra, dec, redshift, weight,
                                   show_progress, domain_factor, config)
        self.first = first
        self.second = second
        self.comm = first.comm
        self.run()

    def run(self):
        """Count the pairs on the GPU; sets :attr:`pairs`."""
        from . import kernel
        from nbodykit_amd import hiplib
        hiplib.require()

        attrs = self.attrs
        mode = attrs['mode']
        dims, edges2 = second_dim(mode, attrs['Nmu'], attrs['pimax'])

        def load(source):
            return kernel.to_device_columns(
                sky_positions(source, attrs), source[attrs['weight']],
                [0, 1, 2])

        pos1, w1 = load(self.first)
        pos2 = w2 = None
        if attrs['is_cross']:
            pos2, w2 = load(self.second)
        if attrs['show_progress']:
            self.logger.info("counting %s pairs of %d x %d objects"
                             % (mode, attrs['N1'],
                                attrs['N2'] or attrs['N1']))

        npairs, wsum, xsum = kernel.count_pairs(
            mode, pos1, w1, pos2, w2, attrs['edges'], edges2, None, False,
            pimax=attrs['pimax'], sky=True)

        self.pairs = make_pairs(mode, attrs['edges'], attrs['Nmu'],
                                attrs['pimax'],
                                pairs_data(dims[0], npairs, wsum, xsum))
        self.pairs.attrs['total_wnpairs'] = attrs['total_wnpairs']

    def __getstate__(self):
        return {'pairs': self.pairs.data, 'attrs': self.attrs}

    def __setstate__(self, state):
        self.attrs = state['attrs']
        self.pairs = make_pairs(self.attrs['mode'], self.attrs['edges'],
                                self.attrs['Nmu'], self.attrs['pimax'],
                                state['pairs'])
        if 'total_wnpairs' in self.attrs:
            self.pairs.attrs['total_wnpairs'] = self.attrs['total_wnpairs']

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
