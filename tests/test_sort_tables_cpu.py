"""
Host-side tables the locality sorts and the gather paint trust
(_PAIR_GHOST, _GHOST_RANGE, _two_level_ys, _pair_gs, _sort_chunk), and
a brute-force self-check of the numpy references that
test_gpu_sort_kernels.py compares the kernels with.  No GPU needed.
"""
import math
from types import SimpleNamespace

import numpy
import pytest

import sort_reference as ref
from nbodykit_amd.source.mesh.catalog import (
    _PAIR_GHOST, _GHOST_RANGE, _two_level_ys, _pair_gs, _sort_chunk)

# (N, L) of every axis of the GPU file's meshes and boxes
AXES = [(32, 10.0), (32, 100.0 / 3), (32, 7.3), (4, 10.0), (8, 10.0),
        (2, 10.0), (6, 10.0), (64, 100.0 / 3), (48, 7.3)]

LDS_INTS = 40960


# ---- ghost tables vs the oracle stencil --------------------------------

def _axis_samples(N, L):
    return numpy.concatenate([
        ref.edge_pool(N, L),
        numpy.random.RandomState(N).uniform(-L, 2 * L, size=2000)])


@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('interlaced', [False, True])
def test_ghost_tables_cover_oracle_stencil(window, interlaced):
    """Every row the oracle stencil deposits to lies within the [lo, hi]
    the pair sort duplicates for and the router ships ghosts for, up to
    a weight of 1e-15 of the particle's mass.  Interlaced tables feed
    one sorted array to both paints, so they must hold at shift 0.0 and
    0.5.  The stencil is evaluated at u = x*(N/L) + shift, the same
    product the row index floor(x*(N/L)) is taken from: the tables are
    statements about the stencil's reach from that row."""
    plo, phi = _PAIR_GHOST[(window, interlaced)]
    glo, ghi = _GHOST_RANGE[(window, interlaced)]
    lo, hi = max(plo, glo), min(phi, ghi)       # both must cover
    worst = 0.0
    for N, L in AXES:
        x = _axis_samples(N, L)
        for shift in ((0.0, 0.5) if interlaced else (0.0,)):
            offsets, w, _ = ref.axis_deposits(x, N, L, window, shift)
            outside = (offsets < lo) | (offsets > hi)
            worst = max(worst, w[outside].max())
            # the in-range rows carry the whole (unit) mass
            numpy.testing.assert_allclose(w[~outside].sum(axis=0), 1.0,
                                          rtol=0, atol=1e-14)
    # Observed maximum over these samples: exactly 0.0 for every
    # (window, interlaced).  A row that the rounding of u + shift or
    # u + 0.5 pushes outside the table sits at the far end of the
    # window's support, where the B-spline weight is exactly 0.
    assert worst <= 1e-15, worst


@pytest.mark.parametrize('window', ref.WINDOWS)
@pytest.mark.parametrize('interlaced', [False, True])
def test_ghost_tables_vs_oracle_coordinates(window, interlaced):
    """The same check with the stencil evaluated where oracle.paint
    evaluates it, u' = x/H + shift.  u' and x*(N/L) are two roundings of
    one real number (relative error <= 2 * 2^-53 each), so next to a
    cell boundary the oracle can start its stencil one row away from
    floor(x*(N/L)) and leave a row outside the table.  The coordinate
    gap is <= 4 * 2^-53 * |u| (+ half an ulp from adding the shift) and
    no window's slope exceeds 1, which bounds that row's weight — the
    amount by which a kernel that honours the tables may differ from the
    oracle, far inside the 1e-12 paint bar.  Observed maxima: CIC
    7.1e-15 (1 ulp of u in [32, 64)), TSC 0.0, PCS 6e-44 (their tails
    are quadratic / cubic in the gap)."""
    plo, phi = _PAIR_GHOST[(window, interlaced)]
    glo, ghi = _GHOST_RANGE[(window, interlaced)]
    lo, hi = max(plo, glo), min(phi, ghi)
    for N, L in AXES:
        x = _axis_samples(N, L)
        for shift in ((0.0, 0.5) if interlaced else (0.0,)):
            offsets, w, u = ref.axis_deposits(x, N, L, window, shift,
                                              coords='oracle')
            outside = (offsets < lo) | (offsets > hi)
            bound = 5 * 2.0 ** -53 * numpy.maximum(numpy.abs(u), 1.0)
            assert (w[outside].max(axis=0) <= bound).all()


def test_pair_ghost_matches_ghost_range():
    # both describe the same stencil span, one for y groups and one for
    # x slabs
    assert _PAIR_GHOST == _GHOST_RANGE


# ---- LDS-budget helpers obey the launchers' guards ---------------------

SWEEP = [(n0, n1, n2)
         for n0 in (2, 3, 4, 6, 8, 32, 256, 1024, 4096)
         for n1 in (4, 32, 48, 64, 96, 512, 2048, 4096)
         for n2 in (8, 32, 48, 64, 512, 1024, 4096, 20480, 32768)]


def _ys_ok(n0, n1, n2, ys):
    # the guards of nbk_xsort_count_f64 / nbk_bucket_fine_f64 (cell mode)
    win = (1 << ys) * n2
    return ((1 << ys) <= n1 and n1 % (1 << ys) == 0
            and n0 * (n1 >> ys) <= LDS_INTS
            and win <= LDS_INTS and win % 1024 == 0)


def _gs_ok(n0, n1, n2, gs):
    # the guards of nbk_psort_count_f64 and of both gather launchers in
    # pair mode (the fused one pads rows by 4 doubles)
    rg = 1 << gs
    return (n0 % 2 == 0 and rg <= n1 and n1 % rg == 0
            and (n0 >> 1) * (n1 >> gs) <= LDS_INTS
            and rg * (n2 + 4) * 8 <= 160 * 1024)


def test_two_level_ys_satisfies_launcher_guards():
    some = 0
    for n0, n1, n2 in SWEEP:
        ys = _two_level_ys(SimpleNamespace(Nmesh=[n0, n1, n2]))
        valid = [s for s in range(0, 16) if _ys_ok(n0, n1, n2, s)]
        if ys is None:
            assert not valid, (n0, n1, n2, valid)
        else:
            some += 1
            assert _ys_ok(n0, n1, n2, ys), (n0, n1, n2, ys)
    assert some > 50


def test_pair_gs_satisfies_launcher_guards():
    some = 0
    for n0, n1, n2 in SWEEP:
        gs = _pair_gs([n0, n1, n2])
        valid = [s for s in range(1, 16) if _gs_ok(n0, n1, n2, s)]
        if gs is None:
            assert not valid, (n0, n1, n2, valid)
        else:
            some += 1
            assert _gs_ok(n0, n1, n2, gs), (n0, n1, n2, gs)
            assert gs == max(valid)     # largest tile = fewest copies
    assert some > 50


def test_gpu_test_meshes_reach_both_pipelines():
    for nmesh in ([32, 32, 32], [4, 32, 32], [8, 64, 32], [2, 32, 32],
                  [6, 64, 48]):
        assert _two_level_ys(SimpleNamespace(Nmesh=nmesh)) is not None
        gs = _pair_gs(nmesh)
        assert gs is not None
        # every _PAIR_GHOST span fits one group, also at the 8-row
        # groups the GPU tests use to get more than one group
        for dlo, dhi in _PAIR_GHOST.values():
            assert dhi - dlo < (1 << 3) <= (1 << gs)


def test_sort_chunk_clamp(monkeypatch):
    monkeypatch.delenv('NBK_SORT_CHUNK', raising=False)
    for n in (1, 1000, 10 ** 6, 10 ** 8, 2 ** 31 - 1):
        for nbuck in (1, 1024, 40960):
            ch = _sort_chunk(n, nbuck)
            assert ch >= 16384 and ch >= 4 * nbuck
            assert ch <= max(16384, 4 * nbuck, 1 << 21)
            if max(16384, 4 * nbuck) < ch < (1 << 21):
                assert -(-n // ch) <= 512       # ~512 blocks target
    for env, want in (('1', 4096), ('4096', 4096), ('100000', 100000),
                      ('99999999999', 1 << 22)):
        monkeypatch.setenv('NBK_SORT_CHUNK', env)
        assert _sort_chunk(10 ** 6, 1024) == want
    monkeypatch.setenv('NBK_SORT_CHUNK', 'junk')
    assert _sort_chunk(10 ** 6, 1024) == 16384  # falls back to default


# ---- the numpy references vs brute-force loops -------------------------

NMESH, BOX = [6, 8, 4], (10.0, 100.0 / 3, 7.3)


def _loop_index(p, nmesh, box):
    out = []
    for ax in range(3):
        i = math.floor(float(p[ax]) * (nmesh[ax] / box[ax]))
        out.append(i)
    return out


def test_reference_keys_match_loops():
    pos = ref.edge_positions(NMESH, BOX, 400, 5)
    n0, n1, n2 = NMESH
    cid = ref.cell_ids(pos, NMESH, BOX)
    rid = ref.row_ids(pos, NMESH, BOX)
    ck = ref.coarse_keys(pos, NMESH, BOX, 2)
    k1, k2 = ref.pair_keys(pos, NMESH, BOX, 2, -1, 2)
    ncopy = 0
    for j, p in enumerate(pos):
        ux, uy, uz = _loop_index(p, NMESH, BOX)
        ix, iy, iz = ux % n0, uy % n1, uz % n2      # Python % is floored
        assert cid[j] == (ix * n1 + iy) * n2 + iz
        assert rid[j] == ix * n1 + iy
        assert ck[j] == ix * (n1 // 4) + iy // 4
        g1 = ((uy - 1) % n1) // 4
        g2 = ((uy + 2) % n1) // 4
        assert k1[j] == (ix // 2) * (n1 // 4) + g1
        assert k2[j] == (-1 if g1 == g2 else (ix // 2) * (n1 // 4) + g2)
        ncopy += 1 + (g1 != g2)
    assert ncopy == len(pos) + (k2 >= 0).sum()
    # the catalogue really sits on the edges: wrapped and boundary cases
    u = ref.floor_index(pos, NMESH, BOX)
    assert (u < 0).any() and (u >= numpy.array(NMESH)).any()
    assert (k2 >= 0).any() and (k2 < 0).any()


def test_reference_histograms_and_scan_match_loops():
    rng = numpy.random.RandomState(3)
    keys = rng.randint(0, 7, size=53)
    keys2 = numpy.where(rng.uniform(size=53) < 0.3,
                        rng.randint(0, 7, size=53), -1)
    mat = ref.chunk_histograms((keys, keys2), 7, 10)
    assert mat.shape == (6, 7)
    want = numpy.zeros((6, 7), dtype='i8')
    for i in range(53):
        want[i // 10, keys[i]] += 1
        if keys2[i] >= 0:
            want[i // 10, keys2[i]] += 1
    assert (mat == want).all()

    bases, bucket_bases = ref.scan_matrix(mat)
    for b in range(7):
        before = sum(int(want[c, bb]) for c in range(6) for bb in range(b))
        assert bucket_bases[b] == before
        for c in range(6):
            assert bases[c, b] == before + sum(int(want[cc, b])
                                               for cc in range(c))
    assert bucket_bases[7] == want.sum()


def test_reference_row_table_and_canonical_rows():
    rows = numpy.array([0, 0, 2, 2, 2, 5])
    tab = ref.row_table(rows, 7)
    for r in range(7):
        assert tab[r] == sum(1 for v in rows if v < r)
    a = numpy.array([[0.0, 1.0, 2.0], [-0.0, 1.0, 2.0], [3.0, 1.0, 2.0]])
    m = numpy.array([1.0, 2.0, 3.0])
    perm = [2, 0, 1]
    assert (ref.canonical_rows(a, m) ==
            ref.canonical_rows(a[perm], m[perm])).all()
    # a mass swapped between two particles, or a sign-of-zero change,
    # is a different multiset
    assert (ref.canonical_rows(a, m) !=
            ref.canonical_rows(a, m[[1, 0, 2]])).any()
    b = a.copy()
    b[1, 0] = 0.0
    assert (ref.canonical_rows(a, m) != ref.canonical_rows(b, m)).any()


def test_edge_catalogues_hit_what_they_claim():
    nmesh, box = [8, 64, 32], BOX
    pos = ref.edge_positions(nmesh, box, 20011, 101)
    assert numpy.isfinite(pos).all()
    assert (numpy.abs(pos) <= 3 * numpy.array(box)).all()
    H = numpy.array(box) / nmesh
    for ax in range(3):
        x = pos[:, ax]
        assert (x == box[ax]).any() and (x < 0).any() \
            and (x > box[ax]).any()
        assert (numpy.signbit(x) & (x == 0)).any()      # -0.0
        assert (x == (nmesh[ax] - 1) * H[ax]).any()
    c = ref.clustered_positions(nmesh, box, 10000, 102)
    assert len(numpy.unique(ref.cell_ids(c, nmesh, box))) == 1
    r = ref.last_row_positions(nmesh, box, 20011, 103)
    assert (ref.row_ids(r, nmesh, box) == 8 * 64 - 1).all()
    assert len(numpy.unique(ref.cell_ids(r, nmesh, box))) == 32
