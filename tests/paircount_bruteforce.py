"""
Brute-force O(N1 N2) numpy oracle of the pair-counting contract
(DESIGN.md "Pair counting"): every operation in f64, rounded separately,
exactly as the expressions are written below.  Shared by
test_paircount_cpu.py, test_gpu_paircount.py and
test_gpu_pairs_kernels.py.
"""
import numpy


def second_edges(mode, Nmu=None, pimax=None):
    if mode == '2d':
        return numpy.linspace(0, 1., Nmu + 1)
    if mode == 'projected':
        return numpy.linspace(0, pimax, int(pimax + 1))
    return None


def _digitize(v, e):
    """bin j with e[j] <= v < e[j+1]; -1 / len(e)-1 outside"""
    return numpy.searchsorted(e, v, side='right') - 1


def _margin(v, e, j, relative):
    """distance of each v to its nearest edge of e (j = _digitize)"""
    lo = e[numpy.clip(j, 0, len(e) - 1)]
    hi = e[numpy.clip(j + 1, 0, len(e) - 1)]
    if relative:
        dlo = numpy.abs(v - lo) / lo
        dhi = numpy.abs(hi - v) / hi
    else:
        dlo = numpy.abs(v - lo)
        dhi = numpy.abs(hi - v)
    return numpy.minimum(dlo, dhi)


def bruteforce_paircount(mode, pos1, edges, BoxSize, w1=None, pos2=None,
                         w2=None, periodic=True, los=2, Nmu=None,
                         pimax=None, chunk=256):
    """
    Returns a dict:
      npairs (u8), wnpairs (f8), mean (f8; r or rp, 0 where empty) of
      shape (nb0,) or (nb0, nb1);
      margin0: the smallest relative distance of any pair's q = r^2 (or
      rp^2) to a squared first-dimension edge;
      margin1: the smallest absolute distance of any first-dimension
      in-range pair's mu (or pi) to a second-dimension edge (inf in 1d);
      n_mu1: number of counted pairs with mu exactly 1.
    ``pos2 is None`` is the auto-correlation (pairs i == j excluded, both
    orderings counted).
    """
    auto = pos2 is None
    axes = [i for i in [0, 1, 2] if i != los] + [los]
    L = (numpy.ones(3) * BoxSize)[axes]

    def prepare(pos):
        p = numpy.asarray(pos).astype('f8')[:, axes]
        if periodic:
            p = numpy.mod(p, L)
            p = numpy.where(p >= L, p - L, p)
        return p

    p1 = prepare(pos1)
    p2 = p1 if auto else prepare(pos2)
    w1 = numpy.ones(len(p1)) if w1 is None else numpy.asarray(w1, 'f8')
    if auto:
        w2 = w1
    else:
        w2 = numpy.ones(len(p2)) if w2 is None else numpy.asarray(w2, 'f8')

    edges = numpy.asarray(edges, dtype='f8')
    esq = edges * edges
    e2 = second_edges(mode, Nmu, pimax)
    nb0 = len(edges) - 1
    nb1 = 1 if e2 is None else len(e2) - 1

    npairs = numpy.zeros(nb0 * nb1, dtype='u8')
    wsum = numpy.zeros(nb0 * nb1)
    xsum = numpy.zeros(nb0 * nb1)
    margin0 = numpy.inf
    margin1 = numpy.inf
    n_mu1 = 0

    for i0 in range(0, len(p1), chunk):
        a = p1[i0:i0 + chunk]
        d = a[:, None, :] - p2[None, :, :]
        if periodic:
            d = numpy.where(d > L / 2, d - L,
                            numpy.where(d < -L / 2, d + L, d))
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        rp2 = dx * dx + dy * dy
        q = rp2 if mode == 'projected' else rp2 + dz * dz
        keep = numpy.ones(q.shape, dtype=bool)
        if auto:
            ii = numpy.arange(i0, i0 + len(a))
            keep[numpy.arange(len(a)), ii] = False

        k = _digitize(q, esq)
        margin0 = min(margin0, _margin(q, esq, k, True)[keep].min())
        keep &= (k >= 0) & (k < nb0)

        x = numpy.sqrt(q)
        j = numpy.zeros(q.shape, dtype='i8')
        if e2 is not None:
            with numpy.errstate(invalid='ignore', divide='ignore'):
                v = numpy.abs(dz) / x if mode == '2d' else numpy.abs(dz)
            j = _digitize(v, e2)
            if keep.any():
                margin1 = min(margin1,
                              _margin(v, e2, j, False)[keep].min())
            if mode == '2d':
                top = keep & (v == e2[-1])
                n_mu1 += int(top.sum())
                j = numpy.where(top, nb1 - 1, j)
            keep &= (j >= 0) & (j < nb1)

        flat = (k * nb1 + j)[keep]
        ww = (w1[i0:i0 + chunk, None] * w2[None, :])[keep]
        npairs += numpy.bincount(flat, minlength=nb0 * nb1).astype('u8')
        wsum += numpy.bincount(flat, weights=ww, minlength=nb0 * nb1)
        xsum += numpy.bincount(flat, weights=x[keep], minlength=nb0 * nb1)

    shape = (nb0,) if e2 is None else (nb0, nb1)
    mean = numpy.zeros(nb0 * nb1)
    filled = npairs > 0
    mean[filled] = xsum[filled] / npairs[filled]
    return dict(npairs=npairs.reshape(shape), wnpairs=wsum.reshape(shape),
                mean=mean.reshape(shape), margin0=float(margin0),
                margin1=float(margin1), n_mu1=n_mu1)


def lattice_positions(n=8, spacing=8.0):
    """n^3 lattice points (0, spacing, ...) as (n^3, 3) f8"""
    g = numpy.arange(n) * spacing
    return numpy.stack(numpy.meshgrid(g, g, g, indexing='ij'),
                       axis=-1).reshape(-1, 3).astype('f8')
