"""
FOF — the friends-of-friends halo finder (reference
nbodykit/algorithms/fof.py).  The reference hands the clustering to
``kdcount.cluster.fof`` (a kd-tree); here it is a two-level cell list and
a lock-free union-find, csrc/nbk_fof.hip.

Semantics (DESIGN.md "Friends-of-friends"): two particles are friends iff
``(dx^2 + dy^2) + dz^2 <= ll^2`` with the minimum-image separation of a
periodic run; a group is a connected component.  ``minid`` is the
smallest input index of a particle's group, which makes the result
independent of the sort's arbitrary in-cell order.  Labels follow the
reference's ``_assign_labels``: groups with ``Length <= nmin`` (``<=``,
as the reference computes, although its docstring says "fewer") get
label 0, the others 1..Nhalo by decreasing Length; among equal Lengths
the group with the LARGER minid gets the smaller label (the reference's
order there is numpy's unstable argsort, reversed; ours is the stable
sort, reversed).

The label rule and the group catalogue (:func:`assign_labels`,
:func:`centerofmass`, :func:`group_catalog`) are torch code for tensors of
any device, with no GPU-only call inside.
"""
import logging

import numpy

from nbodykit_amd import hiplib, profiling

# cells per axis of one sort level (pair_counters.kernel: the largest
# cube that fits one LDS histogram)
LEVEL_CELLS_PER_AXIS = 34
assert LEVEL_CELLS_PER_AXIS ** 3 <= hiplib.SORT_LDS_INTS


# ---- the grid -----------------------------------------------------------

def cells_along(length, side):
    """Number of cells of side >= ``side`` along an axis of ``length``:
    the rule of pair_counters.kernel.cells_along without its cap."""
    if not length > 0:
        return 1
    n = max(1, int(numpy.floor(length / side)))
    # a cell side within rounding of ``side`` could put an in-range pair
    # two cells apart; with fewer than 3 cells every cell is visited anyway
    if n >= 3 and length / n < side * (1 + 1e-12):
        n -= 1
    return n


def fof_grid(periodic, box, ll, n, lo=None, hi=None, per_cell=2.):
    """(origin, inv_cell, ncoarse, fine) of the two-level grid: over
    [0, L) for a periodic run, over the bounding box [lo, hi] otherwise.

    The cell side is max(ll, (per_cell V / n)^(1/3)), about ``per_cell``
    particles per cell (FOF's two unless told otherwise); per axis
    ncell = ncoarse * fine with fine = ceil(ncell / 34),
    rounded down to a multiple of fine, so sides only grow and never fall
    below ``ll``.  A flat axis gets one cell."""
    if periodic:
        origin = numpy.zeros(3)
        extent = numpy.asarray(box, dtype='f8') * numpy.ones(3)
    else:
        origin = numpy.asarray(lo, dtype='f8')
        extent = numpy.asarray(hi, dtype='f8') - origin
    volume = float(numpy.prod(extent))
    side = max(float(ll), (per_cell * volume / max(int(n), 1)) ** (1. / 3))
    while True:
        ncell = [cells_along(e, side) for e in extent]
        fine = [-(-c // LEVEL_CELLS_PER_AXIS) for c in ncell]
        ncoarse = [c // f for c, f in zip(ncell, fine)]
        if numpy.prod(fine, dtype='i8') <= hiplib.SORT_LDS_INTS:
            break
        # (only a bounding box with a flat or very thin axis gets here:
        # its volume says nothing about the spacing of the particles)
        side *= 1.25
    ncell = [c * f for c, f in zip(ncoarse, fine)]
    inv_cell = [c / e if e > 0 else 0.0 for c, e in zip(ncell, extent)]
    return origin, numpy.asarray(inv_cell), ncoarse, fine


def block_major_to_grid(per_cell, ncoarse, fine):
    """a per-cell tensor in the kernels' block-major order (coarse_id *
    nfine + sub_id) as a (ncell[0], ncell[1], ncell[2]) array"""
    c, f = list(ncoarse), list(fine)
    a = per_cell.reshape(c[0], c[1], c[2], f[0], f[1], f[2])
    return a.permute(0, 3, 1, 4, 2, 5).reshape(c[0] * f[0], c[1] * f[1],
                                               c[2] * f[2])


def candidate_pairs(fine_start, ncoarse, fine, periodic):
    """Separations the link kernel evaluates: for every particle the
    lower-indexed particles of its neighbour (cell, shift)s."""
    import torch
    occ = block_major_to_grid(torch.diff(fine_start).to(torch.int64),
                              ncoarse, fine)
    reach = occ
    for axis in range(3):
        n = occ.shape[axis]
        total = torch.zeros_like(reach)
        for d in (-1, 0, 1):
            if periodic:
                total = total + torch.roll(reach, d, dims=axis)
            else:
                sl_to = [slice(None)] * 3
                sl_from = [slice(None)] * 3
                sl_to[axis] = slice(max(0, d), n + min(0, d))
                sl_from[axis] = slice(max(0, -d), n + min(0, -d))
                total[tuple(sl_to)] += reach[tuple(sl_from)]
        reach = total
    ordered = int((occ * reach).sum().item())
    return (ordered - int(occ.sum().item())) // 2


# ---- the device pipeline -----------------------------------------------

def two_level_sort(pos, grid, stage='fof'):
    """
    The coarse sort and the fine pass of device positions over a grid of
    :func:`fof_grid`: (spos, sindex, fine_start), the cell-sorted SoA
    planes [3n] f64, the input index of every sorted slot [n] int32 and
    the fine start table [ncells + 1] int32, in block-major cell order.
    The two profiling stages are named ``<stage>_coarse_sort`` and
    ``<stage>_fine_sort``.  pos: (n, 3) f64 CUDA rows, n > 0.
    """
    import torch
    from .pair_counters import kernel
    lib = hiplib.require()
    n = int(pos.shape[0])
    dev = torch.device('cuda')
    origin, inv_cell, ncoarse, fine = grid
    ncoarse_all = int(numpy.prod(ncoarse))
    ncells = ncoarse_all * int(numpy.prod(fine))
    stream = hiplib.cur_stream()
    grid_c = (hiplib.f64_arr(origin), hiplib.f64_arr(inv_cell),
              hiplib.int_arr(ncoarse), hiplib.int_arr(fine))

    with profiling.collect(stage + '_coarse_sort', units=n):
        index = torch.arange(n, dtype=torch.float64, device=dev)
        chunk = kernel._sort_chunk(n, ncoarse_all)
        nchunks = -(-n // chunk)
        mat = torch.empty(nchunks * ncoarse_all, dtype=torch.int32,
                          device=dev)
        hiplib.check(lib.nbk_fof_cell_count_f64(
            hiplib.dptr(pos), n, chunk, *grid_c, hiplib.dptr(mat), stream),
            'nbk_fof_cell_count_f64')
        bases, coarse_start = hiplib.scan_count_matrix(
            lib, mat, nchunks, ncoarse_all, stream)
        cpos = torch.empty(3 * n, dtype=torch.float64, device=dev)
        cindex = torch.empty(n, dtype=torch.float64, device=dev)
        hiplib.check(lib.nbk_fof_cell_scatter_f64(
            hiplib.dptr(pos), hiplib.dptr(index), n, chunk, *grid_c,
            hiplib.dptr(bases), hiplib.dptr(cpos), hiplib.dptr(cindex),
            stream), 'nbk_fof_cell_scatter_f64')

    with profiling.collect(stage + '_fine_sort', units=n):
        spos = torch.empty(3 * n, dtype=torch.float64, device=dev)
        sindex = torch.empty(n, dtype=torch.int32, device=dev)
        fine_start = torch.empty(ncells + 1, dtype=torch.int32, device=dev)
        hiplib.check(lib.nbk_fof_fine_sort_f64(
            hiplib.dptr(cpos), hiplib.dptr(cindex), n, *grid_c,
            hiplib.dptr(coarse_start), hiplib.dptr(spos),
            hiplib.dptr(sindex), hiplib.dptr(fine_start), stream),
            'nbk_fof_fine_sort_f64')
    return spos, sindex, fine_start


def fof_minid(pos, ll, box, periodic, info=None, per_cell=2.):
    """
    ``minid`` of device positions: an int64 CUDA tensor that gives every
    particle, in input order, the smallest input index of its group.

    pos: (n, 3) f64 CUDA rows, already wrapped into the box for a periodic
    run.  ``info``, if a dict, receives the grid and the start table.
    ``per_cell`` is fof_grid's: it changes the cells, never the result.
    """
    import torch
    lib = hiplib.require()
    n = int(pos.shape[0])
    dev = torch.device('cuda')
    if n == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)

    lo = hi = None
    if not periodic:
        lo, hi = pos.amin(dim=0).tolist(), pos.amax(dim=0).tolist()
    origin, inv_cell, ncoarse, fine = fof_grid(periodic, box, ll, n, lo, hi,
                                               per_cell=float(per_cell))
    stream = hiplib.cur_stream()
    ncoarse_c = hiplib.int_arr(ncoarse)
    fine_c = hiplib.int_arr(fine)
    spos, sindex, fine_start = two_level_sort(
        pos, (origin, inv_cell, ncoarse, fine))

    parent = torch.arange(n, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    with profiling.collect('fof_link', units=n):
        hiplib.check(lib.nbk_fof_link_f64(
            hiplib.dptr(spos), hiplib.dptr(fine_start), n, ncoarse_c,
            fine_c, hiplib.f64_arr(box if periodic else [0.0, 0.0, 0.0]),
            1 if periodic else 0, float(ll) * float(ll),
            hiplib.dptr(parent), hiplib.dptr(err), stream),
            'nbk_fof_link_f64')
    root = torch.empty(n, dtype=torch.int32, device=dev)
    with profiling.collect('fof_flatten', units=n):
        hiplib.check(lib.nbk_fof_flatten_i32(
            hiplib.dptr(parent), n, hiplib.dptr(root), hiplib.dptr(err),
            stream), 'nbk_fof_flatten_i32')

    with profiling.collect('fof_minid', units=n):
        minid = minid_from_roots(root, sindex)
    if info is not None:
        info.update(ncoarse=ncoarse, fine=fine, origin=origin,
                    inv_cell=inv_cell, fine_start=fine_start)
    return minid


def minid_from_roots(root, sindex):
    """``minid`` in input order from the root of every sorted slot and the
    input index of every sorted slot (integer min: bitwise reproducible)"""
    import torch
    n = root.shape[0]
    root = root.to(torch.int64)
    sindex = sindex.to(torch.int64)
    smallest = torch.full((n,), n, dtype=torch.int64, device=root.device)
    smallest.scatter_reduce_(0, root, sindex, 'amin', include_self=True)
    minid = torch.empty(n, dtype=torch.int64, device=root.device)
    minid[sindex] = smallest[root]
    return minid


# ---- labels and the group catalogue (tensors of any device) -------------

def assign_labels(minid, nmin):
    """
    Labels from ``minid`` (reference ``_assign_labels``, one rank): groups
    with ``Length <= nmin`` get 0, the others 1..Nhalo by decreasing
    Length, ties by decreasing minid.  int32, or int64 above 2^31 groups.
    """
    import torch
    minid = torch.as_tensor(minid)
    if minid.numel() == 0:
        return torch.empty(0, dtype=torch.int32, device=minid.device)
    _, inverse, length = torch.unique(minid, return_inverse=True,
                                      return_counts=True)
    # groups are in increasing minid here; the reference reverses an
    # ascending sort of Length
    order = torch.flip(torch.argsort(length, stable=True), dims=[0])
    dtype = torch.int64 if length.numel() + 1 > 2 ** 31 else torch.int32
    rank = torch.arange(1, length.numel() + 1, dtype=dtype,
                        device=minid.device)
    rank = torch.where(length[order] > int(nmin), rank,
                       torch.zeros_like(rank))
    label_of_group = torch.empty_like(rank)
    label_of_group[order] = rank
    return label_of_group[inverse]


def centerofmass(label, pos, boxsize, nhalo0):
    """
    Mean of ``pos`` (n, d) per label, (nhalo0, d) in f64 (reference
    ``centerofmass``).  With a ``boxsize`` it is periodic-aware: the
    differences from the per-label component-wise minimum are wrapped into
    [-L/2, L/2), averaged, added back and reduced modulo L.  A label
    without particles gives NaN.
    """
    import torch
    label = torch.as_tensor(label).to(torch.int64)
    pos = torch.as_tensor(pos).to(device=label.device, dtype=torch.float64)
    d = pos.shape[1]
    count = torch.bincount(label, minlength=nhalo0).to(torch.float64)
    index = label[:, None].expand(-1, d)
    if boxsize is not None:
        box = torch.as_tensor(numpy.ones(d) * numpy.asarray(
            boxsize, dtype='f8')).to(label.device)
        posmin = torch.full((nhalo0, d), float('inf'), dtype=torch.float64,
                            device=label.device)
        posmin.scatter_reduce_(0, index, pos, 'amin', include_self=True)
        dpos = pos - posmin[label]
        half = box * 0.5
        dpos = torch.where(dpos < -half, dpos + box, dpos)
        dpos = torch.where(dpos >= half, dpos - box, dpos)
    else:
        dpos = pos
    total = torch.zeros((nhalo0, d), dtype=torch.float64,
                        device=label.device)
    total.index_add_(0, label, dpos)
    mean = total / count[:, None]
    if boxsize is None:
        return mean
    return torch.remainder(posmin + mean, box)


def group_catalog(label, position, velocity, boxsize, initposition=None,
                  peak=None):
    """
    The group catalogue of ``label`` (reference ``fof_catalog``): a
    structured numpy array of max(label) + 1 rows with CMPosition,
    CMVelocity (f4, 3) and Length (i4, row 0 set to 0), InitialPosition
    with ``initposition``, PeakPosition / PeakVelocity with the column
    ``peak`` (the particles at the largest value of it per group).
    Row 0 stands for no group.
    """
    import torch
    label = torch.as_tensor(label).to(torch.int64)
    nhalo0 = int(label.max().item()) + 1 if label.numel() else 1
    dtype = [('CMPosition', ('f4', 3)), ('CMVelocity', ('f4', 3)),
             ('Length', 'i4')]
    columns = {
        'CMPosition': centerofmass(label, position, boxsize, nhalo0),
        'CMVelocity': centerofmass(label, velocity, None, nhalo0)}
    if initposition is not None:
        dtype.append(('InitialPosition', ('f4', 3)))
        columns['InitialPosition'] = centerofmass(label, initposition,
                                                  boxsize, nhalo0)
    if peak is not None:
        dtype.append(('PeakPosition', ('f4', 3)))
        dtype.append(('PeakVelocity', ('f4', 3)))
        peak = torch.as_tensor(peak).to(device=label.device,
                                        dtype=torch.float64)
        dmax = torch.full((nhalo0,), -float('inf'), dtype=torch.float64,
                          device=label.device)
        dmax.scatter_reduce_(0, label, peak, 'amax', include_self=True)
        # every particle that is not at its group's peak moves to label 0
        label1 = label * (peak >= dmax[label]).to(torch.int64)
        columns['PeakPosition'] = centerofmass(label1, position, boxsize,
                                               nhalo0)
        columns['PeakVelocity'] = centerofmass(label1, velocity, None,
                                               nhalo0)
    catalog = numpy.empty(nhalo0, dtype=numpy.dtype(dtype))
    for name, value in columns.items():
        catalog[name] = value.cpu().numpy()
    catalog['Length'] = torch.bincount(label, minlength=nhalo0).cpu().numpy()
    catalog['Length'][0] = 0
    return catalog


def _as_tensor(col):
    """a host or device column as a torch tensor (native byte order)"""
    import torch
    if isinstance(col, torch.Tensor):
        return col
    arr = numpy.asarray(col)
    return torch.from_numpy(numpy.ascontiguousarray(
        arr, dtype=arr.dtype.newbyteorder('=')))


# ---- the algorithm ------------------------------------------------------

class FOF(object):
    """
    A friends-of-friends halo finder: the label of the halo each particle
    belongs to.

    Parameters follow ``nbodykit.algorithms.FOF``: ``linking_length`` is
    relative to the mean particle separation unless ``absolute``; halos of
    ``nmin`` particles or fewer are ignored (label 0); ``domain_factor``
    (the reference's domain decomposition) is accepted and recorded only.
    ``BoxSize`` in the source's attrs may be a scalar or three values.
    Columns may be numpy arrays or device tensors.

    The results are :attr:`labels` (a numpy array in input order) and
    :attr:`max_label`; see :func:`find_features` for the halo catalogue.
    ``to_halos`` is not part of this package.
    """
    logger = logging.getLogger('FOF')

    def __init__(self, source, linking_length, nmin, absolute=False,
                 periodic=True, domain_factor=1):
        self.comm = source.comm
        self._source = source

        if 'Position' not in source:
            raise ValueError("cannot compute FOF without 'Position' column")

        self.attrs = {}
        self.attrs['linking_length'] = linking_length
        self.attrs['nmin'] = nmin
        self.attrs['absolute'] = absolute
        self.attrs['periodic'] = periodic
        self.attrs['domain_factor'] = domain_factor

        if periodic and 'BoxSize' not in source.attrs:
            raise ValueError("Periodic FOF requires BoxSize in "
                             ".attrs['BoxSize']")

        position = source['Position']
        if len(position.shape) != 2 or position.shape[1] != 3:
            raise ValueError("the 'Position' column must have shape (N, 3)")
        if source.csize >= 2 ** 31:
            raise ValueError("FOF handles fewer than 2^31 particles")

        # linking length relative to mean separation
        if not absolute:
            if 'Nmesh' in source.attrs:
                ndim = len(numpy.atleast_1d(source.attrs['Nmesh']))
            else:
                ndim = position.shape[1]
            if 'BoxSize' not in source.attrs:
                raise ValueError("a relative linking length requires "
                                 "BoxSize in .attrs['BoxSize']")
            # (a scalar BoxSize is the side of every axis)
            volume = numpy.prod(numpy.ones(ndim) * numpy.asarray(
                source.attrs['BoxSize'], dtype='f8'))
            mean_separation = pow(volume / max(source.csize, 1),
                                  1.0 / ndim)
            linking_length = linking_length * mean_separation
        self._linking_length = float(linking_length)
        if not (numpy.isfinite(self._linking_length)
                and self._linking_length > 0):
            raise ValueError("the linking length must be positive and "
                             "finite, got %r" % (linking_length,))

        self._box = None
        if periodic:
            self._box = numpy.ones(3) * numpy.asarray(
                source.attrs['BoxSize'], dtype='f8')
            if self._linking_length > self._box.min():
                raise ValueError("the linking length of a periodic FOF "
                                 "cannot exceed the smallest BoxSize")

        import torch
        if not bool(torch.isfinite(_as_tensor(position)).all()):
            raise ValueError("'Position' holds non-finite values")

        if self.comm.size > 1:
            raise NotImplementedError("FOF runs on a single rank")

        # and run
        self.run()

    def run(self):
        """Run the finder on the GPU; sets :attr:`labels` (the label of
        every particle, in input order) and :attr:`max_label`."""
        from .pair_counters import kernel
        hiplib.require()
        periodic = self.attrs['periodic']
        n = len(self._source['Position'])
        if n == 0:
            # no kernel is launched
            self.labels = numpy.zeros(0, dtype='i4')
            self.max_label = self.comm.allgather(0)
            return
        pos, _ = kernel.to_device_columns(self._source['Position'], None,
                                          [0, 1, 2])
        if periodic:
            pos = kernel.wrap_periodic(pos, self._box)
        minid = fof_minid(pos, self._linking_length, self._box, periodic)
        with profiling.collect('fof_labels', units=n):
            labels = assign_labels(minid, self.attrs['nmin'])
        self.labels = labels.cpu().numpy()
        self.max_label = self.comm.allgather(self.labels.max())

    def find_features(self, peakcolumn=None):
        """
        The groups of :attr:`labels` as an ArrayCatalog of max_label + 1
        rows: the centre of mass ``CMPosition`` and ``CMVelocity``,
        ``Length`` (row 0 stands for no group and has Length 0),
        ``InitialPosition`` if the source has that column, and
        ``PeakPosition`` / ``PeakVelocity`` of the particle at the peak of
        ``peakcolumn`` if one is given.  Evaluated on the host; device
        columns are copied there.
        """
        import torch
        from nbodykit_amd.source.catalog.array import ArrayCatalog
        source = self._source
        for col in ['Position', 'Velocity']:
            if col not in source:
                raise ValueError("the column '%s' is missing from parent "
                                 "source; cannot compute halos" % col)
        if peakcolumn is not None and peakcolumn not in source:
            raise ValueError("the column '%s' is missing from parent "
                             "source" % peakcolumn)

        # the group catalogue is one pass of reductions over the columns:
        # it runs on the host, like the reference's (DESIGN.md
        # "Friends-of-friends", group catalogue)
        def column(name):
            return _as_tensor(source[name]).cpu()

        halos = group_catalog(
            torch.from_numpy(self.labels), column('Position'),
            column('Velocity'), self._box,
            initposition=(column('InitialPosition')
                          if 'InitialPosition' in source else None),
            peak=None if peakcolumn is None else column(peakcolumn))
        attrs = dict(source.attrs)
        attrs.update(self.attrs)
        return ArrayCatalog(halos, comm=self.comm, **attrs)
