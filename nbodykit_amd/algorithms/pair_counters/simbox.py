"""
SimulationBoxPairCount — pair counts of objects in a simulation box as
a function of r, (r, mu) or (rp, pi) (reference
nbodykit/algorithms/pair_counters/simbox.py and base.py).  The reference
hands the arithmetic to Corrfunc; here it is the cell-list HIP kernel of
csrc/nbk_pairs.hip, driven by :mod:`.kernel`.

Semantics (DESIGN.md "Pair counting"): axes are permuted so the line of
sight is last, periodic positions are wrapped into [0, L), separations
are minimum-image, first-dimension bins are closed below and open above
on squared separations, ``npairs`` counts ordered pairs (auto-correlation
excludes i == j and counts both orderings), ``wnpairs`` sums w1 w2 and
the first variable is the mean separation of the bin (0 when empty).
"""
import logging
import numbers

import numpy

from nbodykit_amd import CurrentMPIComm
from nbodykit_amd.binned_statistic import BinnedStatistic

VALID_MODES = ['1d', '2d', 'projected', 'angular']


def second_dim(mode, Nmu, pimax):
    """(dims, second-dimension edges or None) of a mode."""
    if mode == '1d':
        return ['r'], None
    if mode == '2d':
        return ['r', 'mu'], numpy.linspace(0, 1., Nmu + 1)
    if mode == 'projected':
        return ['rp', 'pi'], numpy.linspace(0, pimax, int(pimax + 1))
    raise ValueError("mode = '%s' should be one of %s"
                     % (mode, VALID_MODES[:3]))


def make_pairs(mode, edges, Nmu, pimax, data):
    """The ``pairs`` BinnedStatistic of a result array."""
    dims, edges2 = second_dim(mode, Nmu, pimax)
    all_edges = [numpy.asarray(edges, dtype='f8')]
    if edges2 is not None:
        all_edges.append(edges2)
    return BinnedStatistic(dims, all_edges, data,
                           fields_to_sum=['npairs', 'wnpairs'])


def pairs_data(dim0, npairs, wsum, xsum):
    """Structured result: mean separation, npairs, wnpairs."""
    data = numpy.zeros(npairs.shape, dtype=[(dim0, 'f8'), ('npairs', 'u8'),
                                            ('wnpairs', 'f8')])
    filled = npairs > 0
    data[dim0][filled] = xsum[filled] / npairs[filled]
    data['npairs'] = npairs
    data['wnpairs'] = wsum
    return data


def _column_sum(col, power=1):
    """Sum of a host or device column in f64 (a python float)."""
    if hasattr(col, 'detach'):            # torch tensor
        import torch
        col = col.to(torch.float64)
        return float((col ** power).sum().item())
    return float((numpy.asarray(col, dtype='f8') ** power).sum())


def verify_box(first, second, BoxSize):
    """The 3-vector box of the run; ValueError when it is absent or the
    sources and the keyword disagree."""
    box = numpy.zeros(3)
    box1 = first.attrs.get('BoxSize', None)
    box2 = second.attrs.get('BoxSize', None)
    if box1 is not None:
        box[:] = box1
    elif box2 is not None:
        box[:] = box2
    if BoxSize is not None:
        box[:] = BoxSize
    if (box == 0.).all():
        raise ValueError("BoxSize must be supplied in the source ``attrs`` "
                         "or via the ``BoxSize`` keyword")
    if box1 is not None and box2 is not None \
            and not numpy.all(numpy.asarray(box1) == numpy.asarray(box2)):
        raise ValueError("BoxSize mismatch between pair count "
                         "cross-correlation sources")
    for b in (box1, box2):
        if b is not None and not numpy.all(numpy.asarray(b) == box):
            raise ValueError("BoxSize mismatch between sources and the "
                             "pair count algorithm")
    return box


def prepare_attrs(mode, first, edges, BoxSize=None, periodic=True,
                  second=None, los='z', Nmu=None, pimax=None,
                  weight='Weight', position='Position',
                  show_progress=False, config=None):
    """Validate the arguments of SimulationBoxPairCount and return its
    ``attrs`` (everything known before the GPU is needed)."""
    config = {} if config is None else config
    # line of sight: an axis name or index, never a vector
    if isinstance(los, str):
        if len(los) != 1 or los not in 'xyz':
            raise ValueError("``los`` should be one of 'x', 'y', 'z'")
        los = 'xyz'.index(los)
    elif isinstance(los, numbers.Integral) \
            and not isinstance(los, bool):
        los = int(los)
        if los < 0:
            los += 3
    else:
        raise ValueError("``los`` should be either ['x', 'y', 'z'] or "
                         "[0,1,2]")
    if los not in [0, 1, 2]:
        raise ValueError("``los`` should be either ['x', 'y', 'z'] or "
                         "[0,1,2]")

    # sources: columns and box
    other = first if second is None else second
    for source in (first, other):
        for col in (position, weight):
            if col not in source:
                raise ValueError("the column '%s' is missing from input "
                                 "source; cannot do pair count" % col)
    BoxSize = verify_box(first, other, BoxSize)

    # binning arguments
    if mode not in VALID_MODES:
        raise ValueError("allowed 'mode' values are: %s" % VALID_MODES)
    if mode == 'angular':
        raise NotImplementedError(
            "mode='angular' is not implemented in nbodykit_amd")
    edges = numpy.array(edges, dtype='f8')
    if edges.ndim != 1 or len(edges) < 2 \
            or not numpy.all(numpy.diff(edges) > 0):
        raise ValueError("'edges' must be an increasing sequence of at "
                         "least two bin edges")
    if numpy.min(edges) <= 0.:
        raise ValueError("the lower edge of the 1st separation bin must "
                         "greater than zero (no self-pairs)")
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

    # the total weighted pair count; auto-correlations exclude the
    # self pairs, and the factor 0.5 is a convention that cancels in
    # the estimators
    W1 = comm.allreduce(_column_sum(first[weight]))
    if is_cross:
        W2 = comm.allreduce(_column_sum(second[weight]))
        attrs['total_wnpairs'] = 0.5 * W1 * W2
    else:
        W1sq = comm.allreduce(_column_sum(first[weight], 2))
        attrs['total_wnpairs'] = 0.5 * (W1 ** 2 - W1sq)
    attrs['is_cross'] = is_cross

    attrs['BoxSize'] = BoxSize
    attrs['periodic'] = periodic
    attrs['weight'] = weight
    attrs['position'] = position
    attrs['config'] = config
    attrs['los'] = los

    if periodic:
        half = 0.5 * BoxSize.min()
        if numpy.amax(edges) > half \
                or (mode == 'projected' and pimax > half):
            raise ValueError("periodic pair counts cannot be computed "
                             "for Rmax > BoxSize/2")
        if not numpy.all(BoxSize == BoxSize[0]):
            raise NotImplementedError(
                "periodic pair counts require a cubic box")
    if comm.size > 1:
        raise NotImplementedError(
            "SimulationBoxPairCount runs on a single rank")

    return attrs


class SimulationBoxPairCount(object):
    """
    Count (weighted) pairs of objects in a simulation box.

    Parameters follow ``nbodykit.algorithms.SimulationBoxPairCount``:
    ``mode`` is '1d', '2d' (needs ``Nmu``) or 'projected' (needs
    ``pimax``); ``edges`` are the r (or rp) bin edges; ``second`` selects
    a cross-correlation; ``los`` is 'x', 'y', 'z' or 0, 1, 2.
    ``show_progress`` and ``**config`` (Corrfunc options in the
    reference) are accepted and recorded only.  Columns may be numpy
    arrays or device tensors.

    The result is :attr:`pairs`, a BinnedStatistic with the variables
    ``r`` (or ``rp``), ``npairs`` and ``wnpairs``.
    """
    logger = logging.getLogger('SimulationBoxPairCount')

    def __init__(self, mode, first, edges, BoxSize=None, periodic=True,
                 second=None, los='z', Nmu=None, pimax=None,
                 weight='Weight', position='Position',
                 show_progress=False, **config):
        self.attrs = prepare_attrs(mode, first, edges, BoxSize, periodic,
                                   second, los, Nmu, pimax, weight,
                                   position, show_progress, config)
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
        mode, los = attrs['mode'], attrs['los']
        axes_order = [i for i in [0, 1, 2] if i != los] + [los]
        box = attrs['BoxSize'][axes_order]
        dims, edges2 = second_dim(mode, attrs['Nmu'], attrs['pimax'])

        def load(source):
            pos, w = kernel.to_device_columns(
                source[attrs['position']], source[attrs['weight']],
                axes_order)
            if attrs['periodic']:
                pos = kernel.wrap_periodic(pos, box)
            return pos, w

        pos1, w1 = load(self.first)
        pos2 = w2 = None
        if attrs['is_cross']:
            pos2, w2 = load(self.second)
        if attrs['show_progress']:
            self.logger.info("counting %s pairs of %d x %d objects"
                             % (mode, attrs['N1'],
                                attrs['N2'] or attrs['N1']))

        npairs, wsum, xsum = kernel.count_pairs(
            mode, pos1, w1, pos2, w2, attrs['edges'], edges2, box,
            attrs['periodic'], pimax=attrs['pimax'])

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
