"""
CylindricalGroups — the cylinder-grouping method of Okumura et al. 2016
(reference nbodykit/algorithms/cgm.py).  The reference enumerates the pairs
of a kd-tree into a pandas dataframe and selects the centrals with a Python
``groupby.apply``; here the pairs are walked on the two-level cell list of
the FOF finder and the greedy selection runs as data-parallel sweeps,
csrc/nbk_cgm.hip.

Semantics (DESIGN.md "Cylindrical groups"): objects get a strict priority
order from ``rankby`` (ascending sort, first column most significant, the
LAST object has the highest priority; ties fall to input order).  Two
objects are neighbours iff the pair lies in the cylinder, evaluated in the
reference's order of operations.  From the highest priority down, an object
is a central iff none of its higher-priority neighbours is a central, else
a satellite of the highest-priority central among its neighbours.

:func:`rank_priority` and :func:`cgm_grid` are host-or-device code without
a GPU-only call inside.
"""
import logging
import warnings

import numpy

from nbodykit_amd import hiplib, profiling
from .fof import (LEVEL_CELLS_PER_AXIS, _as_tensor, cells_along,
                  two_level_sort)

# particles per cell of a sparse catalogue (DESIGN.md "Cylindrical groups",
# the per_cell table)
PER_CELL = 0.5
# resolve sweeps per read-back of the flags (DESIGN.md "Cylindrical
# groups", sweeps per read-back); the sweeps after the fixpoint are no-ops
SWEEP_BATCH = 4

# the padding of the cylinder in cgm_grid, relative to rmax^2
_PAD = 2. ** -48


# ---- the grid -----------------------------------------------------------

def cylinder_extent(rperp, rpar, los):
    """
    Per axis, a half-extent that covers every pair the FLOATING-POINT
    predicate of the kernel accepts.

    Exact arithmetic, fixed line of sight l, lam = |l|, u = l / lam: an
    accepted pair has (d.l)^2 <= rpar^2, so |d.u| <= rpar / lam =: p, and
    |d.d - (d.l)^2| <= rperp^2, so the part of d across u has
    d.d - (d.u)^2 = (d.d - (d.l)^2) + (d.u)^2 (lam^2 - 1)
                 <= rperp^2 + p^2 max(0, lam^2 - 1) =: q^2
    (the constructor admits lam within 1e-5 of 1).  A cylinder of radius q
    and half-height p about u reaches q sqrt(1 - u_a^2) + p |u_a| along
    axis a.  For the observer line of sight, d.d <= rperp^2 + rpar^2 = rmax^2
    bounds every axis.

    Rounding, eps = 2^-53: the separation components carry a relative
    error of at most 2 eps (one subtraction, one wrap), so
    fl(d.d) = d.d (1 + t), |t| <= 8 eps (two roundings of each square on
    top, two additions).  fl(d.l) misses d.l by at most 5 eps |d| |l|, and
    rlos2 = fl(fl(d.l)^2) misses (d.l)^2 by at most 11 eps d.d |l|^2.  The
    observer form, dot^2 / c.c, stays within 16 eps d.d of its value.  The
    subtraction d.d - rlos2 cancels, so these ABSOLUTE errors, below
    28 eps d.d, are what the comparison with rperp^2 sees, with
    d.d <= rmax^2 (1 + 1e-4).  Hence an accepted pair has
      across^2 <= q^2 + 32 eps rmax^2 = q^2 + 2^-48 rmax^2,
      |d.u| <= p (1 + 2^-48) + 2^-48 rmax
    (the second term is the 5 eps |d| of fl(d.l): it matters for a flat
    disc, rperp >> rpar, as the first does for a thin cylinder,
    rpar >> rperp).  Both paddings are applied before the extent is formed.
    """
    rperp, rpar = float(rperp), float(rpar)
    rmax2 = rperp * rperp + rpar * rpar
    rmax = numpy.sqrt(rmax2)
    if los is None:
        q2 = rperp * rperp + _PAD * rmax2
        p = rpar * (1 + _PAD) + _PAD * rmax
        return numpy.ones(3) * numpy.sqrt(q2 + p * p)
    l = numpy.asarray(los, dtype='f8')
    lam = numpy.sqrt((l * l).sum())
    u = numpy.abs(l) / lam
    p = rpar / lam
    q2 = rperp * rperp + p * p * max(0., lam * lam - 1.)
    # the same bounds with rmax taken for the stretched cylinder
    rmax2 = q2 + p * p
    q = numpy.sqrt(q2 + _PAD * rmax2)
    p = p * (1 + _PAD) + _PAD * numpy.sqrt(rmax2)
    return q * numpy.sqrt(numpy.maximum(0., 1. - u * u)) + p * u


def cgm_grid(periodic, box, rperp, rpar, los, n, lo=None, hi=None,
             per_cell=PER_CELL):
    """(origin, inv_cell, ncoarse, fine) of the two-level grid of a
    cylinder search: over [0, L) for a periodic run, over the bounding box
    [lo, hi] otherwise.

    The cell side on axis a is max(e_a, (per_cell V / n)^(1/3)), e_a the
    padded half-extent of :func:`cylinder_extent`: a neighbour is at most
    one cell away, and a sparse catalogue gets about ``per_cell`` objects
    per cell.  The split into two levels is fof_grid's: per axis
    ncell = ncoarse * fine with fine = ceil(ncell / 34), rounded down to a
    multiple of fine, so sides only grow.  A flat axis gets one cell."""
    if periodic:
        origin = numpy.zeros(3)
        extent = numpy.asarray(box, dtype='f8') * numpy.ones(3)
    else:
        origin = numpy.asarray(lo, dtype='f8')
        extent = numpy.asarray(hi, dtype='f8') - origin
    reach = cylinder_extent(rperp, rpar, los)
    volume = float(numpy.prod(extent))
    sparse = (per_cell * volume / max(int(n), 1)) ** (1. / 3)
    grow = 1.
    while True:
        side = numpy.maximum(reach, sparse) * grow
        # (a side of 0: no radius and no volume, one cell)
        ncell = [cells_along(e, s) if s > 0 else 1
                 for e, s in zip(extent, side)]
        fine = [-(-c // LEVEL_CELLS_PER_AXIS) for c in ncell]
        ncoarse = [c // f for c, f in zip(ncell, fine)]
        if numpy.prod(fine, dtype='i8') <= hiplib.SORT_LDS_INTS:
            break
        # (only a bounding box with a flat or very thin axis gets here)
        grow *= 1.25
    ncell = [c * f for c, f in zip(ncoarse, fine)]
    inv_cell = [c / e if e > 0 else 0.0 for c, e in zip(ncell, extent)]
    return origin, numpy.asarray(inv_cell), ncoarse, fine


# ---- the priority order ---------------------------------------------------

def rank_priority(columns, n):
    """
    The int32 priority of every row, a permutation of 0..n-1: the position
    of the row in the ascending sort by ``columns`` (tensors or arrays of
    n values on any device; the first one most significant), so the last
    row of that order has the highest priority.  The sorts are stable and
    run from the last key to the first: ties fall to input order, and no
    columns at all give the input order.  Keys are compared by value;
    non-finite keys raise ValueError.
    """
    import torch
    n = int(n)
    keys = [_as_tensor(c) for c in columns]
    device = keys[0].device if keys else torch.device('cpu')
    order = torch.arange(n, dtype=torch.int64, device=device)
    for key in reversed(keys):
        if key.shape != (n,):
            raise ValueError("a rank column must have shape (%d,), got %r"
                             % (n, tuple(key.shape)))
        if key.is_floating_point() and not bool(torch.isfinite(key).all()):
            raise ValueError("a rank column holds non-finite values")
        key = key.to(device)
        order = order[torch.sort(key[order], stable=True).indices]
    prio = torch.empty(n, dtype=torch.int32, device=device)
    prio[order] = torch.arange(n, dtype=torch.int32, device=device)
    return prio


# ---- the device pipeline -------------------------------------------------

def _resolve(lib, common, state, n, batch, stream):
    """Resolve sweeps over ``state`` (zeroed) to the fixpoint; returns the
    number of sweeps after which nothing was undecided.  Sweeps run in
    batches of ``batch``, every sweep with its own (decided, undecided)
    pair of flags, read back once per batch: the sweeps after the fixpoint
    are no-ops."""
    import torch
    done = 0
    while True:
        flags = torch.zeros((batch, 2), dtype=torch.int32,
                            device=state.device)
        for k in range(batch):
            hiplib.check(lib.nbk_cgm_resolve_f64(
                *common, hiplib.dptr(state), hiplib.dptr(flags[k]), stream),
                'nbk_cgm_resolve_f64')
        for decided, undecided in flags.tolist():
            done += 1
            if not undecided:
                return done
            if not decided or done > n + 1:
                # (the highest-priority undecided object can always
                # decide: only priorities that are no permutation, or a
                # corrupt table, get here)
                raise RuntimeError(
                    "the cylinder grouping did not converge after %d "
                    "sweeps over %d objects" % (done, n))


def cylindrical_groups(pos, prio, rperp, rpar, los=None, box=None,
                       periodic=False, per_cell=PER_CELL,
                       batch=SWEEP_BATCH, info=None):
    """
    (cgm_type, cgm_haloid, num_cgm_sats) of device positions, in input
    order: int32 (0 central, 1 satellite), int64 and int64 CUDA tensors.

    pos: (n, 3) f64 CUDA rows (wrapped into ``box``, 3 values, here when
    periodic); prio: n distinct integers in 0..n-1 on the device, a higher
    value is a higher priority (:func:`rank_priority`); los: a 3-vector, or
    None for the observer at the origin.  ``batch`` sweeps run per
    read-back of the flags; it does not change the result.  ``info``, if a
    dict, receives the grid and the number of sweeps.
    """
    import torch
    from .pair_counters import kernel
    lib = hiplib.require()
    n = int(pos.shape[0])
    dev = torch.device('cuda')
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1, got %r" % (batch,))
    if not per_cell > 0:
        raise ValueError("per_cell must be positive, got %r" % (per_cell,))
    if n == 0:
        if info is not None:
            info.update(sweeps=0)
        return (torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    if periodic:
        pos = kernel.wrap_periodic(pos, box)

    lo = hi = None
    if not periodic:
        lo, hi = pos.amin(dim=0).tolist(), pos.amax(dim=0).tolist()
    grid = cgm_grid(periodic, box, rperp, rpar, los, n, lo, hi,
                    per_cell=float(per_cell))
    origin, inv_cell, ncoarse, fine = grid
    spos, sindex, fine_start = two_level_sort(pos, grid, stage='cgm')
    sindex = sindex.to(torch.int64)
    sprio = prio.to(device=dev, dtype=torch.int32)[sindex].contiguous()

    stream = hiplib.cur_stream()
    common = (hiplib.dptr(spos), hiplib.dptr(fine_start), hiplib.dptr(sprio),
              n, hiplib.int_arr(ncoarse), hiplib.int_arr(fine),
              hiplib.f64_arr(box if periodic else [0.0, 0.0, 0.0]),
              1 if periodic else 0, 0 if los is not None else 1,
              hiplib.f64_arr(los if los is not None else [0.0, 0.0, 0.0]),
              float(rperp) * float(rperp), float(rpar) * float(rpar))

    state = torch.zeros(n, dtype=torch.int32, device=dev)
    with profiling.collect('cgm_resolve', units=n):
        sweeps = _resolve(lib, common, state, n, batch, stream)

    host = torch.empty(n, dtype=torch.int32, device=dev)
    with profiling.collect('cgm_host', units=n):
        hiplib.check(lib.nbk_cgm_host_f64(
            *common, hiplib.dptr(state), hiplib.dptr(host), stream),
            'nbk_cgm_host_f64')
    nsat = torch.empty(n, dtype=torch.int32, device=dev)
    with profiling.collect('cgm_count', units=n):
        hiplib.check(lib.nbk_cgm_count_f64(
            *common, hiplib.dptr(state), hiplib.dptr(host),
            hiplib.dptr(nsat), stream), 'nbk_cgm_count_f64')

    with profiling.collect('cgm_labels', units=n):
        haloid = halo_ids(state, host, sprio)
        cgm_type = torch.empty(n, dtype=torch.int32, device=dev)
        cgm_type[sindex] = (state == 2).to(torch.int32)
        cgm_haloid = torch.empty(n, dtype=torch.int64, device=dev)
        cgm_haloid[sindex] = haloid
        num_sats = torch.empty(n, dtype=torch.int64, device=dev)
        num_sats[sindex] = nsat.to(torch.int64)
    if info is not None:
        info.update(ncoarse=ncoarse, fine=fine, origin=origin,
                    inv_cell=inv_cell, fine_start=fine_start, sweeps=sweeps)
    return cgm_type, cgm_haloid, num_sats


def halo_ids(state, host, prio):
    """``cgm_haloid`` (int64) of every slot from the final state, the host
    slot and the priority of every slot (tensors of any device): centrals
    are numbered from 0 by decreasing priority, a satellite carries its
    central's number."""
    import torch
    n = state.shape[0]
    prio = prio.to(torch.int64)
    central = torch.zeros(n, dtype=torch.int64, device=state.device)
    central[prio] = (state == 1).to(torch.int64)
    # centrals of the same or a higher priority, less the central itself
    above = torch.flip(torch.cumsum(torch.flip(central, dims=[0]), 0),
                       dims=[0]) - 1
    return above[prio[host.to(torch.int64)]]


# ---- the algorithm --------------------------------------------------------

class CylindricalGroups(object):
    """
    Groups of objects by the cylindrical grouping method: all satellites
    within a cylinder around a central object (Okumura et al. 2016,
    arXiv:1611.04165).

    Parameters follow ``nbodykit.algorithms.CylindricalGroups``: ``rperp``
    is the radius of the cylinder across the line of sight and ``rpar``
    half its height along it; ``rankby`` is a column name, a list of them
    or None (input order), and objects ranked LAST are the first to be
    centrals; ``flat_sky_los`` is a unit 3-vector, or None for the line of
    sight of every pair as seen from the origin; ``BoxSize`` in the
    source's attrs wins over the keyword and is needed when ``periodic``.
    Columns may be numpy arrays or device tensors; nothing is added to
    ``source``.

    The result is :attr:`groups`, an ArrayCatalog of the input's length
    with ``cgm_type`` (u4: 0 central, 1 satellite), ``cgm_haloid`` (i8: the
    number of the group, 0 for the group of the highest-priority central)
    and ``num_cgm_sats`` (i8: the satellites of a central, 0 for a
    satellite).
    """
    logger = logging.getLogger('CylindricalGroups')

    def __init__(self, source, rankby, rperp, rpar, flat_sky_los=None,
                 periodic=False, BoxSize=None):
        if 'Position' not in source:
            raise ValueError("the 'Position' column must be defined in the "
                             "input source")
        if rankby is None:
            rankby = []
        if isinstance(rankby, str):
            rankby = [rankby]
        for col in rankby:
            if col not in source:
                raise ValueError("cannot rank by column '%s'; no such "
                                 "column" % col)

        self.source = source
        self.comm = source.comm
        self.attrs = {}

        self.attrs['BoxSize'] = numpy.empty(3)
        BoxSize = source.attrs.get('BoxSize', BoxSize)
        if periodic and BoxSize is None:
            raise ValueError("please specify a BoxSize if using periodic "
                             "boundary conditions")
        # (a non-periodic run needs none: NaN, as numpy makes of None)
        self.attrs['BoxSize'][:] = numpy.nan if BoxSize is None else BoxSize
        if periodic and not (numpy.isfinite(self.attrs['BoxSize']).all()
                             and (self.attrs['BoxSize'] > 0).all()):
            raise ValueError("a periodic BoxSize must be positive and "
                             "finite, got %r" % (BoxSize,))

        if flat_sky_los is not None:
            if numpy.isscalar(flat_sky_los) or len(flat_sky_los) != 3:
                raise ValueError("line-of-sight ``flat_sky_los`` should be "
                                 "vector with length 3")
            if not numpy.allclose(numpy.einsum('i,i', flat_sky_los,
                                               flat_sky_los), 1.0,
                                  rtol=1e-5):
                raise ValueError("line-of-sight ``flat_sky_los`` must be a "
                                 "unit vector")

        if flat_sky_los is None and periodic:
            warnings.warn("CylindricalGroups using periodic boundary "
                          "conditions with line-of-sight computed from "
                          "origin (0,0,0); maybe specify a line-of-sight?")

        for name, value in (('rperp', rperp), ('rpar', rpar)):
            if not (numpy.isscalar(value) and numpy.isfinite(value)
                    and value >= 0):
                raise ValueError("%s must be a finite number >= 0, got %r"
                                 % (name, value))

        self.attrs['rpar'] = rpar
        self.attrs['rperp'] = rperp
        self.attrs['periodic'] = periodic
        self.attrs['rankby'] = rankby
        self.attrs['flat_sky_los'] = flat_sky_los

        position = source['Position']
        if len(position.shape) != 2 or position.shape[1] != 3:
            raise ValueError("the 'Position' column must have shape (N, 3)")
        if source.csize >= 2 ** 31:
            raise ValueError("CylindricalGroups handles fewer than 2^31 "
                             "objects")
        import torch
        if not bool(torch.isfinite(_as_tensor(position)).all()):
            raise ValueError("'Position' holds non-finite values")

        if self.comm.size > 1:
            raise NotImplementedError("CylindricalGroups runs on a single "
                                      "rank")

        if self.comm.rank == 0:
            self.logger.info("finding groups with rperp=%s and rpar=%s "
                             % (str(rperp), str(rpar)))
        self.run()

    def run(self):
        """Compute the groups on the GPU; sets :attr:`groups`."""
        import torch
        from .pair_counters import kernel
        from nbodykit_amd.source.catalog.array import ArrayCatalog
        source = self.source
        n = len(source['Position'])
        # (non-finite rank keys are refused before any GPU call)
        prio = rank_priority([source[col] for col in self.attrs['rankby']],
                             n)
        hiplib.require()
        dtype = numpy.dtype([('cgm_type', 'u4'), ('cgm_haloid', 'i8'),
                             ('num_cgm_sats', 'i8')])
        groups = numpy.zeros(n, dtype=dtype)
        # the grid and the number of sweeps of the run
        self.info = {'sweeps': 0}
        if n > 0:
            pos, _ = kernel.to_device_columns(source['Position'], None,
                                              [0, 1, 2])
            los = self.attrs['flat_sky_los']
            if los is not None:
                los = [float(v) for v in los]
            periodic = bool(self.attrs['periodic'])
            cgm_type, haloid, nsat = cylindrical_groups(
                pos, prio, float(self.attrs['rperp']),
                float(self.attrs['rpar']), los=los,
                box=self.attrs['BoxSize'] if periodic else None,
                periodic=periodic, info=self.info)
            groups['cgm_type'] = cgm_type.cpu().numpy()
            groups['cgm_haloid'] = haloid.cpu().numpy()
            groups['num_cgm_sats'] = nsat.cpu().numpy()
        self.groups = ArrayCatalog(groups, comm=self.comm, **self.attrs)

        centrals = groups['cgm_type'] == 0
        if self.comm.rank == 0:
            self.logger.info("found %d CGM centrals total" % centrals.sum())
            self.logger.info(
                "%d/%d are isolated centrals (no satellites)"
                % ((centrals & (groups['num_cgm_sats'] == 0)).sum(),
                   centrals.sum()))
