"""
Plain numpy references for the cylinder-grouping tests (test_cgm_cpu.py,
test_gpu_cgm_kernels.py, test_gpu_cgm.py), written from the definition in
DESIGN.md "Cylindrical groups": the O(n^2) neighbour relation, the
sequential greedy selection, the Jacobi sweeps and the labels.  Nothing
here runs on the GPU.

The neighbour relation rounds like the kernel (the library is built with
-ffp-contract=off): d = r1 - r2 per axis, wrapped when periodic by
``d[d > L/2] -= L`` and then ``d[d <= -L/2] += L``;
flat sky: rlos = (dx lx + dy ly) + dz lz, rlos2 = rlos rlos; observer:
c = 0.5 (r1 + r2), dot = (dx cx + dy cy) + dz cz,
rlos2 = (dot dot) / ((cx cx + cy cy) + cz cz);
rsky2 = |((dx dx + dy dy) + dz dz) - rlos2|; neighbours iff
rsky2 <= rperp rperp and rlos2 <= rpar rpar.  NaN compares false.
"""
import numpy


def neighbours(pos, box, rperp, rpar, los, periodic):
    """(n, n) bool: adj[i, j] is the predicate of the pair (r1 = pos[i],
    r2 = pos[j]), False on the diagonal.  ``los``: 3 values, or None for
    the observer at the origin; ``box``: 3 values, read when periodic."""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    n = len(pos)
    adj = numpy.zeros((n, n), dtype=bool)
    # (in blocks of rows: the temporaries of 5000 x 5000 pairs at once
    # would take gigabytes)
    for i0 in range(0, n, 512):
        adj[i0:i0 + 512] = _neighbour_rows(pos[i0:i0 + 512], pos, box, rperp,
                                           rpar, los, periodic)
    adj[numpy.arange(n), numpy.arange(n)] = False
    return adj


def _neighbour_rows(first, second, box, rperp, rpar, los, periodic):
    d = []
    for a in range(3):
        da = first[:, None, a] - second[None, :, a]
        if periodic:
            L = float(box[a])
            da[da > L * 0.5] -= L
            da[da <= -L * 0.5] += L
        d.append(da)
    with numpy.errstate(invalid='ignore', divide='ignore'):
        if los is not None:
            l = [float(v) for v in los]
            rlos = (d[0] * l[0] + d[1] * l[1]) + d[2] * l[2]
            rlos2 = rlos * rlos
        else:
            c = [0.5 * (first[:, None, a] + second[None, :, a])
                 for a in range(3)]
            dot = (d[0] * c[0] + d[1] * c[1]) + d[2] * c[2]
            c2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]
            rlos2 = (dot * dot) / c2
        dr2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        rsky2 = numpy.abs(dr2 - rlos2)
        return (rsky2 <= float(rperp) * float(rperp)) \
            & (rlos2 <= float(rpar) * float(rpar))


def greedy(adj, prio):
    """(state, host) of the sequential selection, highest priority first:
    state 1 central / 2 satellite; host[i] = i for a central, the
    highest-priority central among the neighbours of a satellite"""
    prio = numpy.asarray(prio)
    n = len(prio)
    state = numpy.zeros(n, dtype='i4')
    host = numpy.full(n, -1, dtype='i8')
    for i in numpy.argsort(-prio, kind='stable'):
        centrals = numpy.flatnonzero(adj[i] & (state == 1)
                                     & (prio > prio[i]))
        if len(centrals) == 0:
            state[i] = 1
            host[i] = i
        else:
            state[i] = 2
            host[i] = centrals[numpy.argmax(prio[centrals])]
    return state, host


def sweeps(adj, prio):
    """(state, count) of the Jacobi fixpoint: every sweep reads the state
    of the sweep before only; ``count`` is the number of sweeps after which
    nothing was undecided"""
    prio = numpy.asarray(prio)
    n = len(prio)
    higher = adj & (prio[None, :] > prio[:, None])
    state = numpy.zeros(n, dtype='i4')
    count = 0
    while (state == 0).any():
        undecided = state == 0
        central_above = (higher & (state == 1)[None, :]).any(axis=1)
        blocked = (higher & undecided[None, :]).any(axis=1)
        new = state.copy()
        new[undecided & central_above] = 2
        new[undecided & ~central_above & ~blocked] = 1
        assert (new != state).any()
        state = new
        count += 1
    return state, count


def labels(state, host, prio):
    """(cgm_type u4, cgm_haloid i8, num_cgm_sats i8): centrals numbered
    from 0 by decreasing priority"""
    state = numpy.asarray(state)
    host = numpy.asarray(host)
    prio = numpy.asarray(prio)
    n = len(state)
    centrals = numpy.flatnonzero(state == 1)
    centrals = centrals[numpy.argsort(-prio[centrals], kind='stable')]
    number = numpy.full(n, -1, dtype='i8')
    number[centrals] = numpy.arange(len(centrals))
    nsat = numpy.bincount(host[state == 2], minlength=n).astype('i8')
    return (state == 2).astype('u4'), number[host], nsat


def groups(pos, prio, box, rperp, rpar, los, periodic):
    """the three columns of a catalogue by brute force"""
    adj = neighbours(pos, box, rperp, rpar, los, periodic)
    state, host = greedy(adj, prio)
    return labels(state, host, prio)


def rank(columns, n):
    """priority from rank columns: ascending lexsort, first column most
    significant, ties to input order, the last has the highest priority"""
    keys = [numpy.asarray(c) for c in columns]
    order = numpy.lexsort(keys[::-1]) if keys else numpy.arange(n)
    prio = numpy.empty(n, dtype='i8')
    prio[order] = numpy.arange(n)
    return prio


def line(n=200, spacing=1.0):
    """(pos, prio) of the adversarial case: n points on the x axis,
    priority falling along the line; with rperp = 1.5 across a z line of
    sight every point neighbours the next only, so the selection is
    central, satellite, central, ... and every Jacobi sweep decides one
    point"""
    pos = numpy.zeros((n, 3))
    pos[:, 0] = numpy.arange(n) * spacing + 0.5
    return pos, numpy.arange(n)[::-1].copy()
