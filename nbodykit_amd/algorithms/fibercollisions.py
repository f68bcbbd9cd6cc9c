"""
FiberCollisions — fibre collision groups and the fibre assignment inside
them (reference nbodykit/algorithms/fibercollisions.py).  The reference
runs its FOF with a periodic kd-tree on the unit sphere and assigns fibres
in a Python loop over groups with a scipy ``pdist`` per round; here the
groups come from the cell-list union-find of :mod:`.fof` and the assignment
is one wave or one block per group, csrc/nbk_fibers.hip.

Semantics (DESIGN.md "Fiber collisions"): positions are
``SkyToUnitSphere(ra, dec) + 1.1`` in f64; with ``ll`` the collision radius
in radians two objects collide iff ``(dx^2 + dy^2) + dz^2 <= ll^2``, the
predicate of the FOF link, so a collision group is a connected component of
the collision graph.  Inside a group, while any two active members collide,
the member with the most collisions, then the smallest sum of its
neighbours' collisions, then the smallest :func:`fiber_key`, then the
smallest input index is marked collided and set aside.  ``NeighborID`` of a
collided object is the nearest object of its group that is not collided.

:func:`fiber_key` and :func:`collision_groups` are host-or-device code
without a GPU-only call inside.
"""
import logging

import numpy

from nbodykit_amd import hiplib, profiling
from .fof import _as_tensor, assign_labels, fof_minid

# particles per cell of the FOF grid over the bounding box of a sphere
# (DESIGN.md "Fiber collisions", the per_cell table)
PER_CELL = 0.25
# the positions sit on a unit sphere inside a box of 2.2: the largest
# linking length for which the reference's periodic FOF cannot link through
# the boundary
MAX_RADIUS_RAD = 0.2
# groups of up to this many members take the one-wave kernel
WAVE_GROUP = 64

_MASK64 = (1 << 64) - 1


def fiber_key(seed, index):
    """
    The priority of the object with input index ``index`` under ``seed``
    (Python integers): the splitmix64 finaliser of
    ``seed + (index + 1) * 0x9E3779B97F4A7C15``, modulo 2^64.  Among members
    tied in their collision counts the SMALLEST key is collided.
    """
    z = (int(seed) + (int(index) + 1) * 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def collision_groups(label):
    """
    (midx, gstart, nbig) of a label tensor of any device: the input indices
    of the objects with a label > 0, group after group (label 1 first) and
    ascending inside a group (int32); the start table of max(label) + 1
    entries into it (int32); and the number of leading groups up to the last
    one with more than 64 members.  Labels by decreasing size, as
    :func:`.fof.assign_labels` gives them, make those a prefix.
    """
    import torch
    label = torch.as_tensor(label).to(torch.int64)
    member = torch.nonzero(label > 0).flatten()
    mlabel = label[member]
    # (stable: members keep their ascending input order inside a group)
    order = torch.sort(mlabel, stable=True).indices
    midx = member[order].to(torch.int32)
    ngroup = int(mlabel.max().item()) if mlabel.numel() else 0
    size = torch.bincount(mlabel - 1, minlength=ngroup)
    gstart = torch.zeros(ngroup + 1, dtype=torch.int64, device=label.device)
    gstart[1:] = torch.cumsum(size, 0)
    big = torch.nonzero(size > WAVE_GROUP).flatten()
    nbig = int(big.max().item()) + 1 if big.numel() else 0
    return midx, gstart.to(torch.int32), nbig


def assign_fibers(pos, label, ll, seed):
    """
    (Collided, NeighborID) of device positions and their collision group
    labels, in input order: int32 CUDA tensors.

    pos: (n, 3) f64 CUDA rows; label: n integers on the device, 0 for an
    object in no group; ll: the collision radius as a chord; seed: an
    integer, taken modulo 2^64.
    """
    import torch
    lib = hiplib.require()
    if not (pos.is_cuda and pos.dtype == torch.float64 and pos.ndim == 2
            and pos.shape[1] == 3 and pos.is_contiguous()):
        raise ValueError("pos must be contiguous (n, 3) f64 CUDA rows")
    n = int(pos.shape[0])
    dev = torch.device('cuda')
    collided = torch.zeros(n, dtype=torch.int32, device=dev)
    neighbor = torch.full((n,), -1, dtype=torch.int32, device=dev)
    if n == 0:
        return collided, neighbor
    with profiling.collect('fibers_groups', units=n):
        midx, gstart, nbig = collision_groups(label.to(dev))
    nmember = int(midx.shape[0])
    ngroup = int(gstart.shape[0]) - 1
    if nmember == 0:
        return collided, neighbor
    cap = lib.nbk_fibers_max_group()
    largest = int(torch.diff(gstart).max().item())
    if largest > cap:
        raise ValueError(
            "the largest collision group has %d members; the fibre "
            "assignment handles groups of up to %d" % (largest, cap))

    with profiling.collect('fibers_assign', units=nmember):
        mcollided = torch.zeros(nmember, dtype=torch.int32, device=dev)
        mneighbor = torch.full((nmember,), -1, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        hiplib.check(lib.nbk_fibers_assign_f64(
            hiplib.dptr(pos), n, hiplib.dptr(midx), nmember,
            hiplib.dptr(gstart), ngroup, nbig, float(ll) * float(ll),
            int(seed) & _MASK64, hiplib.dptr(mcollided),
            hiplib.dptr(mneighbor), hiplib.dptr(err),
            hiplib.cur_stream()), 'nbk_fibers_assign_f64')
        # (midx is a slice of a permutation: a plain indexed store)
        where = midx.to(torch.int64)
        collided[where] = mcollided
        neighbor[where] = mneighbor
    if int(err.item()):
        raise RuntimeError("nbk_fibers_assign_f64 met a group table it "
                           "cannot handle")
    return collided, neighbor


def sky_to_position(ra, dec, degrees):
    """``SkyToUnitSphere(ra, dec, degrees) + 1.1`` as f64 (n, 3) rows: a
    numpy array for host columns, a tensor of their device when both are
    tensors (the same formulas)."""
    import torch
    from nbodykit_amd import transform
    if isinstance(ra, torch.Tensor) and isinstance(dec, torch.Tensor):
        ra = ra.to(torch.float64)
        dec = dec.to(device=ra.device, dtype=torch.float64)
        if degrees:
            ra = torch.deg2rad(ra)
            dec = torch.deg2rad(dec)
        x = torch.cos(dec) * torch.cos(ra)
        y = torch.cos(dec) * torch.sin(ra)
        z = torch.sin(dec)
        return (torch.stack([x, y, z], dim=1) + 1.1).contiguous()

    def host(col):
        if isinstance(col, torch.Tensor):
            return col.cpu().numpy()
        return numpy.asarray(col)
    # (C order: SkyToUnitSphere gives the transpose of its three rows)
    return numpy.ascontiguousarray(
        transform.SkyToUnitSphere(host(ra), host(dec), degrees=degrees)
        + 1.1)


class FiberCollisions(object):
    """
    Run an angular FOF algorithm to determine fiber collision groups from
    an input catalog, and then assign fibers inside every group.

    This determines two populations: the "clean" objects, no two of which
    collide, and the collided objects, each of which collides with some
    object.  As in the reference, the greedy assignment does not promise the
    LARGEST clean sample, and a collided object's colliding neighbour may
    have been collided later itself.

    Parameters follow ``nbodykit.algorithms.FiberCollisions``: ``ra`` and
    ``dec`` are the coordinate columns (numpy arrays or device tensors), in
    degrees when ``degrees``; ``collision_radius`` is ALWAYS in degrees, 62
    arcseconds by default, and must stay below 0.2 rad; ``seed`` fixes the
    choice among tied objects (drawn and recorded when None).

    The result is :attr:`labels`, an ArrayCatalog of the input's length with
    ``Label`` (the collision group, 0 for none), ``Collided`` and
    ``NeighborID`` (the input index of the nearest object of the group that
    is not collided, -1 for an object that is not collided), all i4.
    """
    logger = logging.getLogger('FiberCollisions')

    def __init__(self, ra, dec, collision_radius=62 / 60. / 60., seed=None,
                 degrees=True, comm=None):
        import torch
        from nbodykit_amd import CurrentMPIComm
        from nbodykit_amd.source.catalog.array import ArrayCatalog
        if comm is None:
            comm = CurrentMPIComm.get()

        if len(ra) != len(dec):
            raise ValueError("ra and dec must have the same length, got %d "
                             "and %d" % (len(ra), len(dec)))
        for name, col in (('ra', ra), ('dec', dec)):
            col = _as_tensor(col)
            if col.ndim != 1:
                raise ValueError("%s must be a 1d column" % name)
            if not bool(torch.isfinite(col.to(torch.float64)).all()):
                raise ValueError("%s holds non-finite values" % name)
        if not (numpy.isscalar(collision_radius)
                and numpy.isfinite(collision_radius)
                and collision_radius > 0):
            raise ValueError("the collision radius must be positive and "
                             "finite, got %r" % (collision_radius,))
        # store collision radius in radians
        self._collision_radius_rad = float(numpy.deg2rad(collision_radius))
        if self._collision_radius_rad >= MAX_RADIUS_RAD:
            raise ValueError(
                "the collision radius of %r degrees is %.4f rad; it must "
                "stay below %.1f rad (about 11.46 degrees): the positions "
                "lie on a unit sphere inside a box of 2.2, and beyond that "
                "the reference's periodic FOF links through the boundary, "
                "which the non-periodic FOF used here does not"
                % (collision_radius, self._collision_radius_rad,
                   MAX_RADIUS_RAD))
        if len(ra) >= 2 ** 31:
            raise ValueError("FiberCollisions handles fewer than 2^31 "
                             "objects")
        if comm.size > 1:
            raise NotImplementedError("FiberCollisions runs on a single "
                                      "rank")

        # the one array FOF and the assignment read
        self._position = sky_to_position(ra, dec, degrees)
        pos = self._position
        if isinstance(pos, torch.Tensor):
            pos = pos.cpu().numpy()
        self.source = ArrayCatalog({'Position': pos},
                                   BoxSize=numpy.array([2.2, 2.2, 2.2]),
                                   comm=comm)
        self.comm = self.source.comm

        # set the seed randomly if it is None
        if seed is None:
            if self.comm.rank == 0:
                seed = numpy.random.randint(0, 4294967295)
            seed = self.comm.bcast(seed)

        self.attrs = {}
        self.attrs['collision_radius'] = collision_radius
        self.attrs['seed'] = seed
        self.attrs['degrees'] = degrees

        if self.comm.rank == 0:
            self.logger.info("collision radius in degrees = %.4f"
                             % collision_radius)
        self.run()

    def run(self):
        """Find the groups and assign the fibres on the GPU; sets
        :attr:`labels`."""
        import torch
        from .pair_counters import kernel
        from nbodykit_amd.source.catalog.array import ArrayCatalog
        n = int(self._position.shape[0])
        dtype = numpy.dtype([('Label', 'i4'), ('Collided', 'i4'),
                             ('NeighborID', 'i4')])
        result = numpy.zeros(n, dtype=dtype)
        result['NeighborID'] = -1
        if n > 1:
            # (fewer than two objects: no group, nothing is launched)
            hiplib.require()
            ll = self._collision_radius_rad
            pos, _ = kernel.to_device_columns(self._position, None,
                                              [0, 1, 2])
            minid = fof_minid(pos, ll, None, False, per_cell=PER_CELL)
            with profiling.collect('fof_labels', units=n):
                label = assign_labels(minid, 1)
            collided, neighbor = assign_fibers(pos, label, ll,
                                               self.attrs['seed'])
            result['Label'] = label.cpu().numpy()
            result['Collided'] = collided.cpu().numpy()
            result['NeighborID'] = neighbor.cpu().numpy()

        N_pop2 = int(self.comm.allreduce(result['Collided'].sum()))
        N_pop1 = int(self.comm.allreduce(n)) - N_pop2
        f = N_pop2 * 1. / max(N_pop1 + N_pop2, 1)
        if self.comm.rank == 0:
            self.logger.info("population 1 (clean) size = %d" % N_pop1)
            self.logger.info("population 2 (collided) size = %d" % N_pop2)
            self.logger.info("collision fraction = %.4f" % f)

        self.labels = ArrayCatalog(result, comm=self.comm,
                                   **self.source.attrs)
