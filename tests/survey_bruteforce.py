"""
Brute-force O(N1 N2) numpy oracle of the survey pair-counting contract
(DESIGN.md "Survey pair counting"): the observer at the origin, every
operation in f64, rounded separately, sums associated exactly as the
expressions are written below.  Shared by test_survey_paircount_cpu.py,
test_gpu_survey_pairs_kernels.py and test_gpu_survey_paircount.py.

Positions are Cartesian rows (unit vectors in 'angular' mode); the sky
conversion is not part of the contract and is done by the caller.
"""
import numpy

from paircount_bruteforce import _digitize, _margin, second_edges


def chord_edges_sq(theta_edges):
    """squared chord of the angular edges (degrees)"""
    theta_edges = numpy.asarray(theta_edges, dtype='f8')
    return (2 * numpy.sin(0.5 * numpy.deg2rad(theta_edges))) ** 2


def chord_to_degrees(q):
    """the angle of a squared chord q of the unit sphere, in degrees"""
    return (2 * numpy.arcsin(numpy.minimum(1, 0.5 * numpy.sqrt(q)))) \
        * (180 / numpy.pi)


def bruteforce_survey_paircount(mode, pos1, edges, w1=None, pos2=None,
                                w2=None, Nmu=None, pimax=None, chunk=256):
    """
    Returns a dict:
      npairs (u8), wnpairs (f8), mean (f8; s, rp or theta in degrees, 0
      where empty) of shape (nb0,) or (nb0, nb1);
      margin0: the smallest relative distance of any pair's q to a
      squared first-dimension edge (in 'projected' mode over the pairs
      that have a q, i.e. l^2 > 0);
      margin1: the smallest absolute distance of any first-dimension
      in-range pair's mu (or pi) to a second-dimension edge (inf in '1d'
      and 'angular'); mu >= 1 is exempt, that edge is closed;
      n_top: counted pairs with mu >= 1; n_nan: in-range pairs dropped
      for a NaN mu or pi.
    ``pos2 is None`` is the auto-correlation (pairs i == j excluded, both
    orderings counted).
    """
    auto = pos2 is None
    p1 = numpy.asarray(pos1).astype('f8')
    p2 = p1 if auto else numpy.asarray(pos2).astype('f8')
    w1 = numpy.ones(len(p1)) if w1 is None else numpy.asarray(w1, 'f8')
    if auto:
        w2 = w1
    else:
        w2 = numpy.ones(len(p2)) if w2 is None else numpy.asarray(w2, 'f8')

    edges = numpy.asarray(edges, dtype='f8')
    esq = chord_edges_sq(edges) if mode == 'angular' else edges * edges
    e2 = second_edges(mode, Nmu, pimax)
    nb0 = len(edges) - 1
    nb1 = 1 if e2 is None else len(e2) - 1

    npairs = numpy.zeros(nb0 * nb1, dtype='u8')
    wsum = numpy.zeros(nb0 * nb1)
    xsum = numpy.zeros(nb0 * nb1)
    margin0 = numpy.inf
    margin1 = numpy.inf
    n_top = n_nan = 0

    for i0 in range(0, len(p1), chunk):
        a = p1[i0:i0 + chunk]
        d = a[:, None, :] - p2[None, :, :]
        el = a[:, None, :] + p2[None, :, :]
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        lx, ly, lz = el[..., 0], el[..., 1], el[..., 2]
        s2 = (dx * dx + dy * dy) + dz * dz
        l2 = (lx * lx + ly * ly) + lz * lz
        dl = (dx * lx + dy * ly) + dz * lz
        keep = numpy.ones(s2.shape, dtype=bool)
        if auto:
            ii = numpy.arange(i0, i0 + len(a))
            keep[numpy.arange(len(a)), ii] = False
        if not keep.any() or p2.shape[0] == 0:
            continue

        v = None
        with numpy.errstate(invalid='ignore', divide='ignore'):
            if mode == '2d':
                q = s2
                v = numpy.abs(dl) / numpy.sqrt(l2 * s2)
            elif mode == 'projected':
                pi2 = (dl * dl) / l2
                v = numpy.sqrt(pi2)
                q = s2 - pi2
            else:
                q = s2

        has_q = keep & ~numpy.isnan(q)
        k = _digitize(q, esq)
        if has_q.any():
            with numpy.errstate(invalid='ignore', divide='ignore'):
                margin0 = min(margin0,
                              _margin(q, esq, k, True)[has_q].min())
        keep = has_q & (k >= 0) & (k < nb0)

        x = chord_to_degrees(q) if mode == 'angular' \
            else numpy.sqrt(numpy.where(keep, q, 0.))
        j = numpy.zeros(q.shape, dtype='i8')
        if e2 is not None:
            nan = keep & numpy.isnan(v)
            n_nan += int(nan.sum())
            keep &= ~nan
            j = _digitize(numpy.where(keep, v, 0.), e2)
            if mode == '2d':
                top = keep & (v >= e2[-1])
                n_top += int(top.sum())
                j = numpy.where(top, nb1 - 1, j)
                inner = keep & ~top
            else:
                inner = keep
            if inner.any():
                margin1 = min(margin1,
                              _margin(v, e2, j, False)[inner].min())
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
                margin1=float(margin1), n_top=n_top, n_nan=n_nan)


# ---- the fixtures of the survey tests ------------------------------------

def sky_survey(seed, n):
    """z ~ N(0.5, 0.1), RA in [110, 260], DEC in [-3.6, 60], drawn in
    that order"""
    rng = numpy.random.RandomState(seed)
    z = rng.normal(0.5, 0.1, size=n)
    ra = rng.uniform(110., 260., size=n)
    dec = rng.uniform(-3.6, 60., size=n)
    return ra, dec, z


def sky_clump(seed, n):
    """RA in [178.5, 181.5], DEC in [28.5, 31.5], z in [0.49, 0.51],
    drawn in that order: about 70 Mpc/h across"""
    rng = numpy.random.RandomState(seed)
    ra = rng.uniform(178.5, 181.5, size=n)
    dec = rng.uniform(28.5, 31.5, size=n)
    z = rng.uniform(0.49, 0.51, size=n)
    return ra, dec, z


def sky_patch(seed, n):
    """a 12 x 10 degree patch straddling RA = 0 / 360"""
    rng = numpy.random.RandomState(seed)
    ra = numpy.mod(rng.uniform(-6., 6., size=n), 360.)
    dec = rng.uniform(-5., 5., size=n)
    return ra, dec


def sky_cap(seed, n):
    """a 4 degree polar cap, uniform in area to first order"""
    rng = numpy.random.RandomState(seed)
    ra = rng.uniform(0., 360., size=n)
    dec = 90. - 4. * numpy.sqrt(rng.uniform(size=n))
    return ra, dec


def sky_sphere(seed, n):
    """the whole sphere, uniform in area"""
    rng = numpy.random.RandomState(seed)
    ra = rng.uniform(0., 360., size=n)
    dec = numpy.rad2deg(numpy.arcsin(rng.uniform(-1., 1., size=n)))
    return ra, dec


def sky_weights(seed, n):
    return numpy.random.RandomState(1000 + seed).uniform(0.5, 1.5, size=n)
