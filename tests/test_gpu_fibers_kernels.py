"""
Kernel-level tests of nbk_fibers_assign_f64 (csrc/nbk_fibers.hip), called
through the C ABI with explicit group tables and compared with the brute
force of fibers_reference.py — never with another GPU kernel.

Every comparison is exact equality of integers: the brute force rounds every
operation like the kernel (the library is built with -ffp-contract=off).
The outputs are filled with a sentinel and have a margin on both sides that
must come back untouched.
"""
import numpy
import pytest
from numpy.testing import assert_array_equal

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
if not torch.cuda.is_available():
    pytest.skip('no GPU', allow_module_level=True)

import fibers_reference as fref                                 # noqa: E402
from nbodykit_amd import hiplib                                 # noqa: E402

DEVICE = 'cuda'
NBK_OK = 0
NBK_ERR_ARG = -2
SENTINEL = -7
MARGIN = 64
SEEDS = [0, 42, 2 ** 32 - 1, 2 ** 63 + 5]


@pytest.fixture(scope='module')
def lib():
    return hiplib.require()


@pytest.fixture(scope='module')
def cap(lib):
    cap = lib.nbk_fibers_max_group()
    assert cap >= 1024
    return cap


def dev(arr, dtype):
    return torch.as_tensor(numpy.ascontiguousarray(arr, dtype=dtype)).to(
        DEVICE)


def tables(groups):
    """(midx, gstart, nbig) of explicit groups"""
    sizes = numpy.array([len(g) for g in groups], dtype='i8')
    midx = (numpy.concatenate([numpy.asarray(g, dtype='i4') for g in groups])
            if len(groups) else numpy.zeros(0, dtype='i4'))
    gstart = numpy.concatenate([[0], numpy.cumsum(sizes)]).astype('i4')
    big = numpy.flatnonzero(sizes > 64)
    return midx.astype('i4'), gstart, int(big.max()) + 1 if len(big) else 0


class Call(object):
    """one call over fresh sentinel-filled outputs; ``replace`` overrides
    arguments by name (a pointer by None)"""

    def __init__(self, lib, pos, groups, r2, seed, replace=None):
        pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
        midx, gstart, nbig = tables(groups)
        self.midx, self.gstart = midx, gstart
        self.nmember = len(midx)
        t = dict(pos=dev(pos, 'f8'), midx=dev(midx, 'i4'),
                 gstart=dev(gstart, 'i4'))
        self.out = {
            name: torch.full((2 * MARGIN + self.nmember,), SENTINEL,
                             dtype=torch.int32, device=DEVICE)
            for name in ('collided', 'neighbor')}
        self.err_t = torch.full((2 * MARGIN + 1,), SENTINEL,
                                dtype=torch.int32, device=DEVICE)
        self.err_t[MARGIN] = 0
        a = dict(pos=hiplib.dptr(t['pos']), n=len(pos),
                 midx=hiplib.dptr(t['midx']), nmember=self.nmember,
                 gstart=hiplib.dptr(t['gstart']), ngroup=len(groups),
                 nbig=nbig, r2=float(r2), seed=int(seed),
                 collided=hiplib.dptr(self.out['collided'][MARGIN:]),
                 neighbor=hiplib.dptr(self.out['neighbor'][MARGIN:]),
                 err=hiplib.dptr(self.err_t[MARGIN:]))
        a.update(replace or {})
        self.rc = lib.nbk_fibers_assign_f64(
            a['pos'], a['n'], a['midx'], a['nmember'], a['gstart'],
            a['ngroup'], a['nbig'], a['r2'], a['seed'], a['collided'],
            a['neighbor'], a['err'], None)
        torch.cuda.synchronize()
        self._keep = t
        err = self.err_t.cpu().numpy()
        assert (err[:MARGIN] == SENTINEL).all()
        assert (err[MARGIN + 1:] == SENTINEL).all()
        self.err = int(err[MARGIN])

    def member(self, name):
        """an output in member order, its margins checked"""
        full = self.out[name].cpu().numpy()
        assert (full[:MARGIN] == SENTINEL).all()
        assert (full[MARGIN + self.nmember:] == SENTINEL).all()
        return full[MARGIN:MARGIN + self.nmember]

    def untouched(self):
        return all((self.out[name].cpu().numpy() == SENTINEL).all()
                   for name in self.out)


def compare(lib, pos, groups, r2, seed):
    """the call against the brute force; returns the brute force's
    (Collided, NeighborID) in input order"""
    pos = numpy.asarray(pos, dtype='f8').reshape(-1, 3)
    want_c, want_n = fref.assign(pos, groups, r2, seed)
    c = Call(lib, pos, groups, r2, seed)
    assert c.rc == NBK_OK, lib.nbk_last_error_string().decode()
    assert c.err == 0
    assert_array_equal(c.member('collided'), want_c[c.midx])
    assert_array_equal(c.member('neighbor'), want_n[c.midx])
    return want_c, want_n


def line(m, step=1.):
    """m points along x"""
    pos = numpy.zeros((m, 3))
    pos[:, 0] = step * numpy.arange(m)
    return pos


# ---- small groups ----------------------------------------------------------

@pytest.mark.parametrize('seed', SEEDS)
def test_separate_pairs(lib, seed):
    pos = numpy.zeros((400, 3))
    pos[0::2, 0] = 10. * numpy.arange(200)
    pos[1::2, 0] = 10. * numpy.arange(200) + 1.
    groups = [[2 * k, 2 * k + 1] for k in range(200)]
    want_c, want_n = compare(lib, pos, groups, 1., seed)
    # one of each pair, the first of it sometimes and the second sometimes
    assert_array_equal(want_c[0::2] + want_c[1::2], numpy.ones(200))
    assert 50 < want_c[0::2].sum() < 150


def test_pair_at_the_radius(lib):
    pos = [[0., 0., 0.], [3., 4., 0.]]
    want_c, want_n = compare(lib, pos, [[0, 1]], 25., 42)
    assert want_c.sum() == 1
    # one ulp less: no collision, both clean, no neighbour
    want_c, want_n = compare(lib, pos, [[0, 1]],
                             numpy.nextafter(25., 0.), 42)
    assert_array_equal(want_c, [0, 0])
    assert_array_equal(want_n, [-1, -1])


STAR = [[0, 0, 0], [5, 0, 0], [-5, 0, 0], [0, 5, 0], [0, -5, 0], [0, 0, 5]]
TRIANGLE_PENDANT = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0]]


@pytest.mark.parametrize('seed', SEEDS)
def test_small_graphs(lib, seed):
    for m in (3, 4, 5):
        want_c, _ = compare(lib, line(m), [list(range(m))], 1., seed)
        assert want_c.sum() == m // 2
    want_c, want_n = compare(lib, STAR, [list(range(6))], 25., seed)
    assert_array_equal(want_c, [1, 0, 0, 0, 0, 0])
    assert want_n[0] == 1           # five leaves at one distance: the first
    want_c, _ = compare(lib, TRIANGLE_PENDANT, [[0, 1, 2, 3]], 2., seed)
    # (1 has three collisions and goes first; 0 and 2 are left as a pair)
    assert want_c[1] == 1 and want_c[3] == 0 and want_c.sum() == 2
    # all of them in one call, one group each
    pos = numpy.concatenate([line(3), 100. + line(4), 200. + line(5),
                             300. + numpy.array(STAR, dtype='f8'),
                             400. + numpy.array(TRIANGLE_PENDANT,
                                                dtype='f8')])
    edges = numpy.cumsum([0, 3, 4, 5, 6, 4])
    compare(lib, pos, [list(range(a, b))
                       for a, b in zip(edges[:-1], edges[1:])], 1., seed)


@pytest.mark.parametrize('seed', SEEDS)
def test_coincident_points(lib, seed):
    # three coincident points and one at the radius: a clique whose
    # neighbour distances tie at 0
    pos = [[0., 0., 0.], [0., 0., 0.], [0., 0., 0.], [1., 0., 0.]]
    want_c, want_n = compare(lib, pos, [[0, 1, 2, 3]], 1., seed)
    assert want_c.sum() == 3
    # two clean points at one distance from the collided one
    pos = [[1., 0., 0.], [0., 0., 0.], [1., 0., 0.], [-1., 0., 0.]]
    want_c, want_n = compare(lib, pos, [[0, 1, 2, 3]], 1., seed)
    # 70 coincident points: the block tier
    compare(lib, numpy.ones((70, 3)), [list(range(70))], 0., seed)


def test_groups_of_one_and_unconnected_groups(lib):
    pos = numpy.concatenate([line(6), 50. + line(70, step=3.)])
    # single members, a "group" without a collision, two components in one
    # group, and the same in the block tier
    groups = [[0], [2, 4], [1, 3, 5], list(range(6, 76))]
    want_c, want_n = compare(lib, pos, groups, 1., 42)
    assert want_c.sum() == 0 and (want_n == -1).all()
    groups = [list(range(6, 76)), [0, 1, 3, 4], [5]]
    want_c, _ = compare(lib, pos, groups, 1., 42)
    assert want_c.sum() == 2
    pos = numpy.concatenate([line(40), 100. + line(40)])
    want_c, _ = compare(lib, pos, [list(range(80))], 1., 42)
    assert want_c.sum() == 40


# ---- the two tiers at their edges ------------------------------------------

def edge_sizes(cap):
    return [63, 64, 65, cap - 1, cap]


@pytest.mark.parametrize('which', range(5))
@pytest.mark.parametrize('kind', ['clique', 'path'])
def test_tier_edges(lib, cap, kind, which):
    m = edge_sizes(cap)[which]
    # the group between two pairs, its members away from the front of pos
    pos = numpy.concatenate([line(2), 1e4 + line(m), 1e6 + line(2)])
    big = list(range(2, m + 2))
    groups = [big, [0, 1], [m + 2, m + 3]]
    r2 = float(m) * m if kind == 'clique' else 1.
    for seed in (SEEDS if m <= 65 else [42]):
        want_c, _ = compare(lib, pos, groups, r2, seed)
        assert want_c[big].sum() == (m - 1 if kind == 'clique' else m // 2)


def test_group_above_the_cap(lib, cap):
    m = cap + 1
    pos = numpy.concatenate([line(m), 1e6 + line(2)])
    groups = [list(range(m)), [m, m + 1]]
    c = Call(lib, pos, groups, 1., 42)
    assert c.rc == NBK_OK and c.err == 1
    assert (c.member('collided')[:m] == SENTINEL).all()
    assert (c.member('neighbor')[:m] == SENTINEL).all()
    # the pair behind it is served all the same
    want_c, want_n = fref.assign(pos, groups[1:], 1., 42)
    assert_array_equal(c.member('collided')[m:], want_c[m:])
    assert_array_equal(c.member('neighbor')[m:], want_n[m:])


def test_large_group_beyond_nbig(lib):
    pos = numpy.concatenate([line(2), 100. + line(65)])
    groups = [[0, 1], list(range(2, 67))]
    c = Call(lib, pos, groups, 1., 42, dict(nbig=0))
    assert c.rc == NBK_OK and c.err == 1
    assert (c.member('collided')[2:] == SENTINEL).all()
    assert (c.member('neighbor')[2:] == SENTINEL).all()
    assert c.member('collided')[:2].sum() == 1
    # with the promise kept it is served
    want_c, _ = compare(lib, pos, groups, 1., 42)
    assert want_c.sum() == 1 + 32


def test_member_index_out_of_range(lib):
    pos = line(4)
    for bad in (-1, 4):
        c = Call(lib, pos, [[0, 1], [2, bad]], 1., 42)
        assert c.rc == NBK_OK and c.err == 1
        assert c.member('collided')[:2].sum() == 1
        assert (c.member('collided')[2:] == SENTINEL).all()


def test_no_groups(lib):
    c = Call(lib, line(5), [], 1., 42)
    assert c.rc == NBK_OK and c.err == 0 and c.untouched()
    # nothing is read: no tables are needed
    c = Call(lib, line(5), [], 1., 42,
             dict(gstart=None, midx=None, err=None))
    assert c.rc == NBK_OK and c.untouched()
    c = Call(lib, numpy.zeros((0, 3)), [], 1., 42, dict(pos=None))
    assert c.rc == NBK_OK and c.untouched()


@pytest.mark.parametrize('replace', [
    dict(r2=-1.), dict(r2=float('nan')), dict(r2=float('inf')),
    dict(r2=-float('inf')),
    dict(n=-1), dict(n=2 ** 31), dict(nmember=-1), dict(nmember=2 ** 31),
    dict(ngroup=-1), dict(ngroup=2 ** 31), dict(nbig=-1), dict(nbig=3),
    dict(pos=None), dict(midx=None), dict(gstart=None), dict(collided=None),
    dict(neighbor=None), dict(err=None)],
    ids=lambda r: '%s=%r' % list(r.items())[0])
def test_bad_arguments(lib, replace):
    c = Call(lib, line(4), [[0, 1], [2, 3]], 1., 42, replace)
    assert c.rc == NBK_ERR_ARG
    assert 'nbk_fibers_assign_f64' in lib.nbk_last_error_string().decode()
    assert c.err == 0 and c.untouched()


def test_rows_outside_the_groups_are_not_read(lib):
    # NaN in every row that midx does not name
    rng = numpy.random.RandomState(11)
    n = 1000
    pos = numpy.full((n, 3), numpy.nan)
    named = numpy.sort(rng.choice(n, 330, replace=False))
    pos[named[:200:2], 0] = 10. * numpy.arange(100)
    pos[named[1:200:2], 0] = 10. * numpy.arange(100) + 1.
    pos[named[:200], 1:] = 0.
    pos[named[200:]] = 5000. + line(130)
    groups = [named[200:].tolist()] + [named[2 * k:2 * k + 2].tolist()
                                       for k in range(100)]
    for seed in SEEDS:
        want_c, _ = compare(lib, pos, groups, 1., seed)
        assert want_c.sum() == 65 + 100


# ---- larger inputs ---------------------------------------------------------

def test_lattice(lib):
    pos = numpy.array([(0.9 * i, 0.9 * j, 0.) for i in range(20)
                       for j in range(20)])
    label = fref.labels(fref.components(400, fref.collision_pairs(pos, 1.)))
    assert (label == 1).all()
    assert len(fref.collision_pairs(pos, 1.)) == 760
    want_c, _ = compare(lib, pos, [list(range(400))], 1., 42)
    assert want_c.sum() == 200


@pytest.mark.parametrize('s,radius,largest', [
    (1, 0.025, 289), (2, 0.025, 458), (3, 0.025, 182), (3, 0.0218, 64)])
def test_dense_patch(lib, cap, s, radius, largest):
    rng = numpy.random.RandomState(s)
    ra = rng.uniform(0, 1, 2000)
    dec = rng.uniform(-0.5, 0.5, 2000)
    pos = fref.positions(ra, dec)
    ll = numpy.deg2rad(radius)
    r2 = ll * ll
    label = fref.labels(fref.components(2000,
                                        fref.collision_pairs(pos, r2)))
    groups = fref.groups_of(label)
    size = numpy.array([len(g) for g in groups])
    # a drift of the input fails here, it does not quietly lose coverage
    if radius == 0.0218:
        assert size.max() == 64
    else:
        assert 64 < size.max() <= cap
        assert 6 <= (size > 64).sum() <= 8
    assert size.max() == largest
    for seed in (42, 2 ** 63 + 5):
        compare(lib, pos, [g.tolist() for g in groups], r2, seed)
