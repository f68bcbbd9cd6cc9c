"""
Device driver of the pair counter: cell grid, cell sort and the count
passes over ``nbk_pairs_*`` (csrc/nbk_pairs.hip).  Replaces the
Corrfunc.theory.DD / DDsmu / DDrppi calls of the reference's
pair_counters/corrfunc/theory.py, and with ``sky=True`` the
DDsmu_mocks / DDrppi_mocks / DDtheta_mocks calls of corrfunc/mocks.py
(SurveyDataPairCount).  ``zeta_multipoles`` drives the 3PCF kernel
``nbk_3pcf_zeta_f64`` (csrc/nbk_3pcf.hip) on the same grid and cell
sort.  Everything here runs on the GPU; the
only host transfers are the bounding box (non-periodic runs) and the
finished histograms.
"""
import numpy

from nbodykit_amd import hiplib, profiling

MODE_IDS = {'1d': 0, '2d': 1, 'projected': 2}
# the modes of nbk_pairs_count_sky_f64: the line of sight of a pair is
# its midpoint direction from the origin ('1d' has no line of sight and
# stays mode 0 on a non-periodic grid)
SKY_MODE_IDS = {'2d': 3, 'projected': 4, 'angular': 5}

# cells per axis: the largest cube that fits the LDS histogram of the
# cell sort
MAX_CELLS_PER_AXIS = 34
assert MAX_CELLS_PER_AXIS ** 3 <= hiplib.SORT_LDS_INTS \
    < (MAX_CELLS_PER_AXIS + 1) ** 3


def chord_edges_sq(theta_edges):
    """Squared chords of the unit sphere at angular edges in degrees."""
    theta_edges = numpy.asarray(theta_edges, dtype='f8')
    return (2 * numpy.sin(0.5 * numpy.deg2rad(theta_edges))) ** 2


def max_3d_separation(mode, edges, pimax):
    """The largest 3-D separation a counted pair can have."""
    if mode == 'angular':
        return float(numpy.sqrt(numpy.max(chord_edges_sq(edges))))
    rmax = float(numpy.max(edges))
    if mode == 'projected':
        rmax = float(numpy.sqrt(rmax ** 2 + float(pimax) ** 2))
    return rmax


def cells_along(length, rmax):
    """Number of cells of side >= rmax along an axis of ``length``."""
    if not length > 0:
        return 1
    n = int(numpy.floor(length / rmax))
    n = max(1, min(n, MAX_CELLS_PER_AXIS))
    # a cell side within rounding of rmax could put an in-range pair two
    # cells apart; with fewer than 3 cells every cell is visited anyway
    if n >= 3 and length / n < rmax * (1 + 1e-12):
        n -= 1
    return n


def make_grid(periodic, box, rmax, lo=None, hi=None):
    """(origin, inv_cell, ncell) of the cell grid: over [0, L) for a
    periodic run, over the joint bounding box [lo, hi] otherwise."""
    if periodic:
        origin = numpy.zeros(3)
        extent = numpy.asarray(box, dtype='f8')
    else:
        origin = numpy.asarray(lo, dtype='f8')
        extent = numpy.asarray(hi, dtype='f8') - origin
    ncell = [cells_along(e, rmax) for e in extent]
    inv_cell = [n / e if e > 0 else 0.0 for n, e in zip(ncell, extent)]
    return origin, numpy.asarray(inv_cell), ncell


def candidate_pairs(start1, start2, ncell, periodic):
    """Candidate pair evaluations of one count pass, from the cell
    occupancies: sum over first-catalogue cells of n1(cell) times the
    n2 of every visited (neighbour cell, shift)."""
    n1 = numpy.diff(numpy.asarray(start1)).reshape(ncell).astype('i8')
    n2 = numpy.diff(numpy.asarray(start2)).reshape(ncell).astype('i8')
    reach = n2
    for axis, n in enumerate(ncell):
        if periodic:
            reach = sum(numpy.roll(reach, d, axis=axis)
                        for d in (-1, 0, 1))
        else:
            pad = [(1, 1) if a == axis else (0, 0) for a in range(3)]
            p = numpy.pad(reach, pad)
            sl = [slice(None)] * 3
            total = 0
            for d in (0, 1, 2):
                sl[axis] = slice(d, d + n)
                total = total + p[tuple(sl)]
            reach = total
    return int((n1 * reach).sum())


def to_device_columns(position, weight, axes_order):
    """numpy (any float width / byte order) or torch columns -> f64 CUDA
    tensors, position as contiguous (n, 3) rows with the line of sight
    last.  Device columns stay on the device.  ``weight`` may be None
    (positions only): the second result is then None."""
    import torch

    def as_tensor(col):
        if isinstance(col, torch.Tensor):
            return col
        arr = numpy.asarray(col)
        arr = numpy.ascontiguousarray(
            arr, dtype=arr.dtype.newbyteorder('='))
        return torch.from_numpy(arr)

    pos = as_tensor(position).to(device='cuda', dtype=torch.float64)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("position column must have shape (N, 3)")
    pos = pos[:, list(axes_order)].contiguous()
    if weight is None:
        return pos, None
    w = as_tensor(weight).to(device='cuda', dtype=torch.float64)
    w = w.contiguous()
    if w.shape != (pos.shape[0],):
        raise ValueError("weight column must have shape (N,)")
    return pos, w


def wrap_periodic(pos, box):
    """positions into [0, L) per axis"""
    import torch
    L = torch.as_tensor(numpy.asarray(box, dtype='f8')).to(pos.device)
    pos = torch.remainder(pos, L)
    return torch.where(pos >= L, pos - L, pos).contiguous()


def _sort_chunk(n, ncells):
    return max(4096, 4 * ncells, -(-n // 512))


def cell_sort(lib, pos, w, origin, inv_cell, ncell):
    """Counting sort by cell: (SoA positions [3n], weights [n], cell-start
    table [ncells + 1] int32)."""
    import torch
    n = int(pos.shape[0])
    ncells = int(numpy.prod(ncell))
    start = torch.zeros(ncells + 1, dtype=torch.int32, device='cuda')
    out = torch.empty(3 * n, dtype=torch.float64, device='cuda')
    out_w = torch.empty(n, dtype=torch.float64, device='cuda')
    if n == 0:
        return out, out_w, start
    stream = hiplib.cur_stream()
    chunk = _sort_chunk(n, ncells)
    nchunks = -(-n // chunk)
    origin_c = hiplib.f64_arr(origin)
    inv_c = hiplib.f64_arr(inv_cell)
    ncell_c = hiplib.int_arr(ncell)
    mat = torch.empty(nchunks * ncells, dtype=torch.int32, device='cuda')
    hiplib.check(lib.nbk_pairs_cell_count_f64(
        hiplib.dptr(pos), n, chunk, origin_c, inv_c, ncell_c,
        hiplib.dptr(mat), stream), 'nbk_pairs_cell_count_f64')
    bases, _ = hiplib.scan_count_matrix(lib, mat, nchunks, ncells, stream,
                                        bucket_bases=start)
    hiplib.check(lib.nbk_pairs_cell_scatter_f64(
        hiplib.dptr(pos), hiplib.dptr(w), n, chunk, origin_c, inv_c,
        ncell_c, hiplib.dptr(bases), hiplib.dptr(out), hiplib.dptr(out_w),
        stream), 'nbk_pairs_cell_scatter_f64')
    return out, out_w, start


def single_pass_capacity():
    """Total bins one count pass holds (NBK_PAIRS_MAX_BINS)."""
    return int(hiplib.load().nbk_pairs_max_bins())


def threeptcf_limits(lmax=None):
    """(largest multipole, bins that fit at ``lmax``) of nbk_3pcf_zeta_f64;
    the bin capacity is None without ``lmax``.  Needs no GPU."""
    lib = hiplib.load()
    max_ell = int(lib.nbk_3pcf_max_ell())
    if lmax is None:
        return max_ell, None
    return max_ell, int(lib.nbk_3pcf_max_bins(int(lmax)))


def zeta_multipoles(pos, w, edges, lmax, box, periodic, info=None):
    """
    3PCF multipoles zeta_l(r1, r2), l = 0..lmax, of a device catalogue
    with itself (csrc/nbk_3pcf.hip): a host array (lmax + 1, nbins, nbins).

    pos: (n, 3) f64 CUDA rows, already wrapped into the box for a periodic
    run; bins are open below and closed above.  The grid covers the box
    (periodic) or the bounding box, its cells at least max(edges) wide.
    ``info``, if a dict, receives the grid and the launch shape.
    """
    import torch
    lib = hiplib.require()
    edges = numpy.asarray(edges, dtype='f8')
    nbins = len(edges) - 1
    lmax = int(lmax)
    max_ell, _ = threeptcf_limits()
    if lmax < 0 or lmax > max_ell:
        raise ValueError("multipoles must lie in [0, %d]" % max_ell)
    cap = threeptcf_limits(lmax)[1]
    if nbins < 1 or nbins > cap:
        raise ValueError("at most %d bins at lmax = %d" % (cap, lmax))
    rmax = float(numpy.max(edges))
    n = int(pos.shape[0])

    lo = hi = None
    if not periodic:
        if n:
            lo, hi = pos.amin(dim=0).tolist(), pos.amax(dim=0).tolist()
        else:
            lo = hi = [0.0, 0.0, 0.0]
    origin, inv_cell, ncell = make_grid(periodic, box, rmax, lo, hi)

    with profiling.collect('3pcf_sort', units=n):
        spos, sw, start = cell_sort(lib, pos, w, origin, inv_cell, ncell)

    dev = torch.device('cuda')
    esq = torch.as_tensor(edges * edges).to(dev)
    # a persistent grid: the blocks a CU holds by their LDS (64 bytes per
    # bin and (l, m) per wave, up to 4 waves) and by their registers (4-
    # wave blocks at 4, 3, 2 waves per SIMD for lmax < 8, < 12, <= 15:
    # DESIGN.md "Three-point correlation function")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    nlm = (lmax + 1) * (lmax + 2) // 2
    by_regs = 4 if lmax < 8 else 3 if lmax < 12 else 2
    per_cu = max(1, min(by_regs,
                        (150 * 1024) // (4 * 64 * nbins * nlm + 8192)))
    nblocks = ncu * per_cu
    nent = (lmax + 1) * nbins * (nbins + 1) // 2
    partials = torch.empty(nblocks * nent, dtype=torch.float64, device=dev)
    zeta = torch.empty((lmax + 1) * nbins * nbins, dtype=torch.float64,
                       device=dev)
    with profiling.collect('3pcf_zeta', units=n):
        hiplib.check(lib.nbk_3pcf_zeta_f64(
            hiplib.dptr(spos), hiplib.dptr(sw), hiplib.dptr(start), n,
            hiplib.int_arr(ncell),
            hiplib.f64_arr(box if periodic else [0.0, 0.0, 0.0]),
            1 if periodic else 0, hiplib.dptr(esq), nbins, lmax, nblocks,
            hiplib.dptr(partials), hiplib.dptr(zeta),
            hiplib.cur_stream()), 'nbk_3pcf_zeta_f64')
    if info is not None:
        info.update(ncell=ncell, nblocks=nblocks,
                    start=start.cpu().numpy())
    return zeta.cpu().numpy().reshape(lmax + 1, nbins, nbins)


def count_pairs(mode, pos1, w1, pos2, w2, edges, edges2, box, periodic,
                pimax=None, info=None, sky=False):
    """
    Pair counts of device catalogues (``pos2 is None``: auto-correlation).

    pos*: (n, 3) f64 CUDA rows, line of sight last, already wrapped into
    the box for a periodic run; edges2: the second-dimension edges, or
    None in '1d'.  Returns host arrays (npairs u8, wsum f8, xsum f8) of
    shape (nb0,) or (nb0, nb1).  ``info``, if a dict, receives the grid
    and the cell-start tables.

    ``sky``: positions seen from the origin, never periodic; '2d' and
    'projected' use the midpoint line of sight of every pair, 'angular'
    takes unit vectors and ``edges`` in degrees, and xsum sums degrees.
    """
    import torch
    lib = hiplib.require()
    if sky:
        periodic = False
    elif mode == 'angular':
        raise ValueError("mode 'angular' needs sky=True")
    auto = pos2 is None
    edges = numpy.asarray(edges, dtype='f8')
    nb0 = len(edges) - 1
    nb1 = 1 if edges2 is None else len(edges2) - 1
    cap = single_pass_capacity()
    if nb0 > cap:
        raise ValueError("at most %d bins along the first dimension"
                         % cap)
    rmax = max_3d_separation(mode, edges, pimax)

    lo = hi = None
    if not periodic:
        both = [p for p in (pos1, pos2) if p is not None and len(p)]
        if both:
            lo = torch.stack([p.amin(dim=0) for p in both]).amin(dim=0)
            hi = torch.stack([p.amax(dim=0) for p in both]).amax(dim=0)
            lo, hi = lo.tolist(), hi.tolist()
        else:
            lo = hi = [0.0, 0.0, 0.0]
    origin, inv_cell, ncell = make_grid(periodic, box, rmax, lo, hi)
    ncells = int(numpy.prod(ncell))

    with profiling.collect('pairs_sort', units=len(pos1)):
        s1, sw1, start1 = cell_sort(lib, pos1, w1, origin, inv_cell, ncell)
        if auto:
            s2, sw2, start2 = s1, sw1, start1
        else:
            s2, sw2, start2 = cell_sort(lib, pos2, w2, origin, inv_cell,
                                        ncell)
    n1 = int(pos1.shape[0])
    n2 = n1 if auto else int(pos2.shape[0])

    dev = torch.device('cuda')
    if mode == 'angular':
        e0sq = torch.as_tensor(chord_edges_sq(edges)).to(dev)
    else:
        e0sq = torch.as_tensor(edges * edges).to(dev)
    e1 = None
    if edges2 is not None:
        e1 = torch.as_tensor(numpy.asarray(edges2, dtype='f8')).to(dev)

    npairs = torch.zeros(nb0 * nb1, dtype=torch.int64, device=dev)
    wsum = torch.zeros(nb0 * nb1, dtype=torch.float64, device=dev)
    xsum = torch.zeros(nb0 * nb1, dtype=torch.float64, device=dev)

    # second-dimension bins per pass, and a persistent grid of a few
    # blocks per CU (one when the histograms fill most of the LDS)
    per_pass = max(1, cap // nb0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    stream = hiplib.cur_stream()
    box_c = hiplib.f64_arr(box if periodic else [0.0, 0.0, 0.0])
    ncell_c = hiplib.int_arr(ncell)
    npasses = 0
    with profiling.collect('pairs_count', units=n1):
        for j0 in range(0, nb1, per_pass):
            j1 = min(nb1, j0 + per_pass)
            nb = nb0 * (j1 - j0)
            nblocks = ncu * (2 if nb <= 2048 else 1)
            partials = torch.empty(3 * nblocks * nb, dtype=torch.float64,
                                   device=dev)
            cats = (hiplib.dptr(s1), hiplib.dptr(sw1), hiplib.dptr(start1),
                    n1, hiplib.dptr(s2), hiplib.dptr(sw2),
                    hiplib.dptr(start2), n2, 1 if auto else 0, ncell_c)
            bins = (hiplib.dptr(e0sq), nb0, hiplib.dptr(e1), nb1, j0, j1,
                    nblocks, hiplib.dptr(partials), hiplib.dptr(npairs),
                    hiplib.dptr(wsum), hiplib.dptr(xsum), stream)
            if sky and mode in SKY_MODE_IDS:
                hiplib.check(lib.nbk_pairs_count_sky_f64(
                    *cats, SKY_MODE_IDS[mode], *bins),
                    'nbk_pairs_count_sky_f64')
            else:
                hiplib.check(lib.nbk_pairs_count_f64(
                    *cats, box_c, 1 if periodic else 0, MODE_IDS[mode],
                    *bins), 'nbk_pairs_count_f64')
            npasses += 1

    if info is not None:
        info.update(ncell=ncell, npasses=npasses,
                    start1=start1.cpu().numpy(),
                    start2=start2.cpu().numpy())

    shape = (nb0,) if edges2 is None else (nb0, nb1)
    return (npairs.cpu().numpy().astype('u8').reshape(shape),
            wsum.cpu().numpy().reshape(shape),
            xsum.cpu().numpy().reshape(shape))
