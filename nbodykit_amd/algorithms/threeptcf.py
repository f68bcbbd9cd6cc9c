"""
SimulationBox3PCF and SurveyData3PCF — multipoles of the isotropic
three-point correlation function in configuration space (reference
nbodykit/algorithms/threeptcf.py; Slepian & Eisenstein, MNRAS 454, 4142,
2015).  The reference loops over primaries in Python with a kd-tree and
sympy-generated spherical harmonics; here it is the cell-list a_lm kernel
of csrc/nbk_3pcf.hip, driven by
:func:`.pair_counters.kernel.zeta_multipoles`.

Semantics (DESIGN.md "Three-point correlation function"): the catalogue
is correlated with itself, separations are minimum-image when periodic,
radial bins are open below and closed above (``edges[b] < r <=
edges[b+1]``, binned on squared separations), a pair at r = 0 is dropped,
and ``corr_<ell>`` is normalised as eq. 15 of the paper, which is
(2 ell + 1) / (4 pi)^2 times the sum over triplets of w1 w2 w3 P_ell.
"""
import logging
import numbers

import numpy

from nbodykit_amd import CurrentMPIComm, transform
from nbodykit_amd.binned_statistic import BinnedStatistic


def validate_binning(poles, edges):
    """(poles as a list of ints, edges as f8) or ValueError; the limits
    are the kernel's and need no GPU."""
    from .pair_counters import kernel
    poles = list(numpy.atleast_1d(numpy.asarray(poles, dtype=object)))
    if len(poles) == 0:
        raise ValueError("'poles' must name at least one multipole")
    for ell in poles:
        if isinstance(ell, bool) \
                or not isinstance(ell, (numbers.Integral, numpy.integer)):
            raise ValueError("'poles' must be non-negative integers, got %r"
                             % (ell,))
        if ell < 0:
            raise ValueError("'poles' must be non-negative integers, got %r"
                             % (ell,))
    poles = [int(ell) for ell in poles]
    max_ell, _ = kernel.threeptcf_limits()
    if max(poles) > max_ell:
        raise ValueError("multipoles above %d are not supported" % max_ell)

    edges = numpy.array(edges, dtype='f8')
    if edges.ndim != 1 or len(edges) < 2 \
            or not numpy.all(numpy.diff(edges) > 0):
        raise ValueError("'edges' must be an increasing sequence of at "
                         "least two bin edges")
    if numpy.min(edges) < 0.:
        raise ValueError("'edges' must not be negative")
    cap = kernel.threeptcf_limits(max(poles))[1]
    if len(edges) - 1 > cap:
        raise ValueError("at most %d separation bins at multipoles up to "
                         "%d" % (cap, max(poles)))
    return poles, edges


def make_poles(poles, edges, zeta):
    """The ``poles`` BinnedStatistic from zeta[l] for l <= max(poles)."""
    nbins = len(edges) - 1
    dtype = numpy.dtype([('corr_%d' % ell, 'f8') for ell in poles])
    data = numpy.empty((nbins, nbins), dtype=dtype)
    for ell in poles:
        data['corr_%d' % ell] = zeta[ell]
    return BinnedStatistic(['r1', 'r2'], [edges, edges], data)


class Base3PCF(object):
    """
    What the two 3PCF classes share: validation, the launch, the result
    and its (de)serialisation.  Use :class:`SimulationBox3PCF` or
    :class:`SurveyData3PCF`.
    """

    def __init__(self, source, poles, edges, required_cols, BoxSize=None,
                 periodic=None):
        for col in required_cols:
            if col not in source:
                raise ValueError("the column '%s' is missing from input "
                                 "source; cannot compute the 3PCF" % col)
        poles, edges = validate_binning(poles, edges)
        self.source = source
        self.comm = source.comm
        self.attrs = {}
        self.attrs['poles'] = poles
        self.attrs['edges'] = edges

        # the box of a simulation (periodic is None for survey data)
        if periodic is not None:
            box = numpy.zeros(3)
            if source.attrs.get('BoxSize', None) is not None:
                box[:] = source.attrs['BoxSize']
            if BoxSize is not None:
                box[:] = BoxSize
            if periodic and not (box > 0.).all():
                raise ValueError("BoxSize must be supplied in the source "
                                 "``attrs`` or via the ``BoxSize`` keyword")
            self.attrs['BoxSize'] = box
            self.attrs['periodic'] = bool(periodic)
            if periodic and numpy.amax(edges) > 0.5 * box.min():
                raise ValueError("periodic pair counts cannot be computed "
                                 "for Rmax > BoxSize/2")
        if self.comm.size > 1:
            raise NotImplementedError(
                "%s runs on a single rank" % type(self).__name__)

    def _run(self, pos, w, box, periodic):
        """zeta on the GPU from device columns -> the BinnedStatistic"""
        from .pair_counters import kernel
        poles, edges = self.attrs['poles'], self.attrs['edges']
        zeta = kernel.zeta_multipoles(pos, w, edges, max(poles), box,
                                      periodic)
        return make_poles(poles, edges, zeta)

    def __getstate__(self):
        return {'poles': self.poles.data, 'attrs': self.attrs}

    def __setstate__(self, state):
        self.attrs = state['attrs']
        edges = numpy.asarray(self.attrs['edges'], dtype='f8')
        self.poles = BinnedStatistic(['r1', 'r2'], [edges, edges],
                                     state['poles'])

    def save(self, output):
        """Save the :attr:`poles` result as a JSON file ``output``."""
        import json
        from nbodykit_amd.utils import JSONEncoder
        if self.comm.rank == 0:
            self.logger.info('measurement done; saving result to %s'
                             % output)
            with open(output, 'w') as ff:
                json.dump(self.__getstate__(), ff, cls=JSONEncoder)

    @classmethod
    @CurrentMPIComm.enable
    def load(cls, filename, comm=None):
        """Load a result saved with :func:`save`."""
        import json
        from nbodykit_amd.utils import JSONDecoder
        if comm.rank == 0:
            with open(filename, 'r') as ff:
                state = json.load(ff, cls=JSONDecoder)
        else:
            state = None
        state = comm.bcast(state)
        self = object.__new__(cls)
        self.__setstate__(state)
        self.comm = comm
        return self


class SimulationBox3PCF(Base3PCF):
    """
    Multipoles of the isotropic 3PCF of objects in a simulation box.

    Parameters follow ``nbodykit.algorithms.SimulationBox3PCF``: ``poles``
    is the list of multipole numbers, ``edges`` the separation bin edges
    (``edges[0] = 0`` is allowed); ``BoxSize`` is needed when ``periodic``
    and may have three different sides.  Columns may be numpy arrays or
    device tensors.

    The result is :attr:`poles`, a BinnedStatistic over (``r1``, ``r2``)
    with one variable ``corr_<ell>`` per requested multipole.
    """
    logger = logging.getLogger('SimulationBox3PCF')

    def __init__(self, source, poles, edges, BoxSize=None, periodic=True,
                 weight='Weight', position='Position'):
        Base3PCF.__init__(self, source, poles, edges, [position, weight],
                          BoxSize=BoxSize, periodic=periodic)
        self.attrs['weight'] = weight
        self.attrs['position'] = position
        self.poles = self.run()

    def run(self, pedantic=False):
        """Compute and return :attr:`poles` on the GPU.  ``pedantic``
        (one pair per callback in the reference) changes nothing here."""
        from .pair_counters import kernel
        from nbodykit_amd import hiplib
        hiplib.require()
        attrs = self.attrs
        pos, w = kernel.to_device_columns(self.source[attrs['position']],
                                          self.source[attrs['weight']],
                                          [0, 1, 2])
        if attrs['periodic']:
            pos = kernel.wrap_periodic(pos, attrs['BoxSize'])
        return self._run(pos, w, attrs['BoxSize'], attrs['periodic'])


class SurveyData3PCF(Base3PCF):
    """
    Multipoles of the isotropic 3PCF of a survey catalogue (RA and DEC in
    degrees, redshift).

    Parameters follow ``nbodykit.algorithms.SurveyData3PCF``: ``cosmo``
    turns redshifts into comoving distances; ``domain_factor`` is accepted
    and recorded only.  The run is never periodic.
    """
    logger = logging.getLogger('SurveyData3PCF')

    def __init__(self, source, poles, edges, cosmo, domain_factor=4,
                 ra='RA', dec='DEC', redshift='Redshift', weight='Weight'):
        Base3PCF.__init__(self, source, poles, edges,
                          [ra, dec, redshift, weight])
        if cosmo is None:
            raise ValueError("'cosmo' is required to convert redshifts "
                             "into distances")
        self.attrs['cosmo'] = cosmo
        self.attrs['weight'] = weight
        self.attrs['ra'] = ra
        self.attrs['dec'] = dec
        self.attrs['redshift'] = redshift
        self.attrs['domain_factor'] = domain_factor
        self.poles = self.run()

    def run(self, pedantic=False):
        """Compute and return :attr:`poles` on the GPU."""
        from .pair_counters import kernel
        from .pair_counters.mocksurvey import _host_column
        from nbodykit_amd import hiplib
        hiplib.require()
        attrs = self.attrs
        xyz = transform.SkyToCartesian(
            _host_column(self.source[attrs['ra']]),
            _host_column(self.source[attrs['dec']]),
            _host_column(self.source[attrs['redshift']]), attrs['cosmo'])
        pos, w = kernel.to_device_columns(xyz, self.source[attrs['weight']],
                                          [0, 1, 2])
        return self._run(pos, w, None, False)
