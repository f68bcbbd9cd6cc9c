"""
Brute force of the fibre collision definition (DESIGN.md "Fiber
collisions"), pure numpy with Python integers for the key.  Every operation
is rounded on its own, as in the kernels (the library is built with
-ffp-contract=off), so comparisons with it are exact integer equality.

Not a test module: the tests import it.
"""
import numpy

MASK64 = (1 << 64) - 1


def key(seed, index):
    """the tie-break priority of an input index (Python integers)"""
    z = (int(seed) + (int(index) + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def positions(ra, dec, degrees=True):
    """the f64 positions of the definition, from host columns"""
    ra = numpy.asarray(ra, dtype='f8')
    dec = numpy.asarray(dec, dtype='f8')
    if degrees:
        ra = numpy.deg2rad(ra)
        dec = numpy.deg2rad(dec)
    x = numpy.cos(dec) * numpy.cos(ra)
    y = numpy.cos(dec) * numpy.sin(ra)
    z = numpy.sin(dec)
    return numpy.vstack([x, y, z]).T + 1.1


def dist2(a, b):
    """(dx*dx + dy*dy) + dz*dz of every row of a against every row of b"""
    a = numpy.asarray(a, dtype='f8').reshape(-1, 3)
    b = numpy.asarray(b, dtype='f8').reshape(-1, 3)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def collision_pairs(pos, r2, rows=500):
    """all (i, j), i < j, that collide: O(n^2), a slab of rows at a time"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    out = []
    for lo in range(0, len(pos), rows):
        d2 = dist2(pos[lo:lo + rows], pos)
        i, j = numpy.nonzero(d2 <= r2)
        i += lo
        keep = i < j
        out.append(numpy.stack([i[keep], j[keep]], axis=1))
    if not out:
        return numpy.zeros((0, 2), dtype='i8')
    return numpy.concatenate(out).astype('i8')


def components(n, pairs):
    """minid[n]: the smallest index of every object's connected component"""
    parent = list(range(n))

    def find(k):
        while parent[k] != k:
            parent[k] = parent[parent[k]]
            k = parent[k]
        return k

    for i, j in pairs:
        ri, rj = find(int(i)), find(int(j))
        if ri != rj:
            parent[max(ri, rj)] = min(ri, rj)
    return numpy.array([find(k) for k in range(n)], dtype='i8')


def labels(minid):
    """FOF labels with nmin = 1: 0 for a lone object, else 1..G by
    decreasing size, ties to the LARGER minid first"""
    minid = numpy.asarray(minid, dtype='i8')
    roots, size = numpy.unique(minid, return_counts=True)
    order = sorted(range(len(roots)), key=lambda g: (-size[g], -roots[g]))
    label_of_root = {}
    for rank, g in enumerate(order):
        label_of_root[int(roots[g])] = rank + 1 if size[g] > 1 else 0
    return numpy.array([label_of_root[int(m)] for m in minid], dtype='i4')


def groups_of(label):
    """the member indices (ascending) of label 1, 2, ..."""
    label = numpy.asarray(label)
    return [numpy.flatnonzero(label == g)
            for g in range(1, int(label.max()) + 1 if len(label) else 1)]


def greedy(pos, members, r2, seed):
    """(collided, neighbour) of one group: booleans and input indices (-1
    where not collided), in the order of ``members`` (ascending input
    indices)"""
    members = numpy.asarray(members, dtype='i8')
    m = len(members)
    d2 = dist2(pos[members], pos[members])
    adj = (d2 <= r2)
    adj[numpy.arange(m), numpy.arange(m)] = False
    # (0/1 in f64: the sums below are exact)
    A = adj.astype('f8')
    keys = [key(seed, i) for i in members]
    active = numpy.ones(m, dtype=bool)
    collided = numpy.zeros(m, dtype=bool)
    for _ in range(m):
        n_coll = A.sum(axis=1)
        if n_coll.max() == 0:
            break
        n_other = A @ n_coll
        cand = numpy.flatnonzero(active & (n_coll == n_coll.max()))
        cand = cand[n_other[cand] == n_other[cand].min()]
        pick = min(cand, key=lambda c: (keys[c], c))
        collided[pick] = True
        active[pick] = False
        A[pick, :] = 0
        A[:, pick] = 0
    neighbour = numpy.full(m, -1, dtype='i8')
    clean = numpy.flatnonzero(~collided)
    for i in numpy.flatnonzero(collided):
        # (argmin: the first of equal distances)
        neighbour[i] = members[clean[numpy.argmin(d2[i, clean])]]
    return collided, neighbour


def assign(pos, groups, r2, seed):
    """(Collided, NeighborID), int32 in input order, over explicit groups
    (lists of ascending input indices; not assumed connected)"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    collided = numpy.zeros(len(pos), dtype='i4')
    neighbour = numpy.full(len(pos), -1, dtype='i4')
    for members in groups:
        if len(members) == 0:
            continue
        c, nb = greedy(pos, members, r2, seed)
        collided[members] = c
        neighbour[members] = nb
    return collided, neighbour


def run(pos, ll, seed):
    """(Label, Collided, NeighborID) of positions, collision radius ``ll``
    (the chord, compared as ll*ll) and seed: the whole definition"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    r2 = float(ll) * float(ll)
    label = labels(components(len(pos), collision_pairs(pos, r2)))
    collided, neighbour = assign(pos, groups_of(label), r2, seed)
    return label, collided, neighbour


def invariants(pos, ll, collided):
    """the reference test's two properties: (clean pairs that collide,
    collided objects that collide with nobody)"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    collided = numpy.asarray(collided).astype(bool)
    pairs = collision_pairs(pos, float(ll) * float(ll))
    clean_pairs = int((~collided[pairs[:, 0]] & ~collided[pairs[:, 1]]).sum())
    touched = numpy.zeros(len(pos), dtype=bool)
    touched[pairs.ravel()] = True
    return clean_pairs, int((collided & ~touched).sum())
