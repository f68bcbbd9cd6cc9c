"""
CylindricalGroups, the cylinder-grouping method of Okumura et al. 2016, on
a LogNormalCatalog ranked by a mock mass.

    python examples/cgm_demo.py
    python examples/cgm_demo.py --timing --sizes 1e6 1e7

It prints the HIP-event time of every stage of one call, the number of
resolve sweeps and the group statistics, and checks the first 2000 rows,
grouped on their own, against an O(n^2) brute force of the definition
(DESIGN.md "Cylindrical groups").

With ``--timing`` it also prints, per size, the stage times (the median of
``--repeats`` runs after a warm-up) for 0.5 to 8 objects per cell, the
resolve stage for 1, 2, 4 and 8 sweeps per read-back of the flags, the time
of every single sweep, and for scale the ``fof_link`` stage of FOF at
b = 0.2 on the same catalogue, which is NOT the code under test: one fixed
walk over 27 cells with a distance test.

Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))

import numpy

from nbodykit_amd import hiplib, profiling
from nbodykit_amd.algorithms import cgm
from nbodykit_amd.algorithms import fof as fofmod
from nbodykit_amd.lab import (ArrayCatalog, CylindricalGroups, LinearPower,
                              LogNormalCatalog, Planck15)

T0 = time.perf_counter()
PER_CELL = (0.5, 1., 2., 4., 8.)
BATCH = (1, 2, 4, 8)
LOS = [0., 0., 1.]


def progress(what):
    """a timestamped line on stderr, so that a long run shows where it is"""
    sys.stderr.write('[%7.1f s] %s\n' % (time.perf_counter() - T0, what))
    sys.stderr.flush()


def report(record):
    print(json.dumps(record), flush=True)


def make_catalog(n, box, nmesh):
    """a lognormal catalogue with a mock mass, log-uniform in [1e12, 1e15)"""
    Plin = LinearPower(Planck15, redshift=0.55, transfer='EisensteinHu')
    cat = LogNormalCatalog(Plin=Plin, nbar=n / box ** 3, BoxSize=box,
                           Nmesh=nmesh, seed=42)
    rng = numpy.random.RandomState(7)
    cat['Mass'] = 10 ** rng.uniform(12, 15, cat.csize)
    return cat


def brute_force(pos, mass, box, rperp, rpar):
    """(cgm_type, cgm_haloid, num_cgm_sats) of a periodic box with the z
    line of sight, straight from the definition"""
    n = len(pos)
    d = pos[:, None, :] - pos[None, :, :]
    d[d > 0.5 * box] -= box
    d[d <= -0.5 * box] += box
    rlos2 = d[..., 2] * d[..., 2]
    dr2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + rlos2
    adj = (numpy.abs(dr2 - rlos2) <= rperp * rperp) & (rlos2 <= rpar * rpar)
    cgm_type = numpy.zeros(n, dtype='u4')
    haloid = numpy.full(n, -1, dtype='i8')
    nsat = numpy.zeros(n, dtype='i8')
    central = numpy.zeros(n, dtype=bool)
    ncen = 0
    # ascending stable sort, the last first
    for i in numpy.argsort(mass, kind='stable')[::-1]:
        hosts = numpy.flatnonzero(adj[i] & central)
        if len(hosts) == 0:
            central[i] = True
            haloid[i] = ncen
            ncen += 1
        else:
            host = hosts[numpy.argmax(mass[hosts])]
            cgm_type[i] = 1
            haloid[i] = haloid[host]
            nsat[host] += 1
    return cgm_type, haloid, nsat


def stage_medians(run, repeats):
    """{stage: median ms} over ``repeats`` runs after one warm-up"""
    import torch
    run()
    torch.cuda.synchronize()
    samples = {}
    for _ in range(repeats):
        profiling.enable()
        run()
        for name, rec in profiling.summary().items():
            samples.setdefault(name, []).append(rec['ms'])
        profiling.disable()
    return {name: round(float(numpy.median(ms)), 3)
            for name, ms in samples.items()}


def workflow(n, box, nmesh, rperp, rpar):
    cat = make_catalog(n, box, nmesh)
    progress('lognormal catalogue of %d objects' % cat.csize)
    CylindricalGroups(cat, 'Mass', rperp, rpar, flat_sky_los=LOS,
                      periodic=True)             # warm-up
    profiling.enable()
    r = CylindricalGroups(cat, 'Mass', rperp, rpar, flat_sky_los=LOS,
                          periodic=True)
    stages = {name: round(rec['ms'], 3)
              for name, rec in profiling.summary().items()}
    profiling.disable()
    cgm_type = numpy.asarray(r.groups['cgm_type'])
    nsat = numpy.asarray(r.groups['num_cgm_sats'])
    report({'run': 'CylindricalGroups', 'N': cat.csize, 'BoxSize': box,
            'rperp': rperp, 'rpar': rpar, 'stages_ms': stages,
            'sweeps': r.info['sweeps'], 'ncoarse': r.info['ncoarse'],
            'fine': r.info['fine'],
            'centrals': int((cgm_type == 0).sum()),
            'isolated_centrals': int(((cgm_type == 0) & (nsat == 0)).sum()),
            'largest_num_cgm_sats': int(nsat.max())})

    m = min(2000, cat.csize)
    pos = numpy.asarray(cat['Position'], dtype='f8')[:m]
    mass = numpy.asarray(cat['Mass'])[:m]
    # (wider cylinders, so that the thinned sample still has satellites)
    wide = (cat.csize / m) ** (1. / 3)
    sub = CylindricalGroups(ArrayCatalog({'Position': pos, 'Mass': mass},
                                         BoxSize=box), 'Mass', rperp * wide,
                            rpar * wide, flat_sky_los=LOS, periodic=True)
    want = brute_force(numpy.remainder(pos, box), mass, box, rperp * wide,
                       rpar * wide)
    names = ['cgm_type', 'cgm_haloid', 'num_cgm_sats']
    same = all(numpy.array_equal(numpy.asarray(sub.groups[c]), w)
               for c, w in zip(names, want))
    report({'run': 'subsample against the brute force', 'N': m,
            'satellites': int(want[0].sum()), 'identical': bool(same)})
    if not same:
        raise SystemExit('the subsample differs from the brute force')


def sweep_times(pos, prio, box3, rperp, rpar, per_cell):
    """ms of every single resolve sweep to the fixpoint, and the objects
    still undecided before each"""
    import torch
    lib = hiplib.require()
    n = int(pos.shape[0])
    grid = cgm.cgm_grid(True, box3, rperp, rpar, LOS, n, per_cell=per_cell)
    spos, sindex, fine_start = fofmod.two_level_sort(pos, grid, stage='cgm')
    sprio = prio.cuda()[sindex.long()].contiguous()
    common = (hiplib.dptr(spos), hiplib.dptr(fine_start), hiplib.dptr(sprio),
              n, hiplib.int_arr(grid[2]), hiplib.int_arr(grid[3]),
              hiplib.f64_arr(box3), 1, 0, hiplib.f64_arr(LOS), rperp * rperp,
              rpar * rpar)
    state = torch.zeros(n, dtype=torch.int32, device='cuda')
    times, undecided = [], []
    for _ in range(n + 1):
        left = int((state == 0).sum().item())
        if left == 0:
            break
        undecided.append(left)
        flags = torch.zeros(2, dtype=torch.int32, device='cuda')
        start, stop = (torch.cuda.Event(enable_timing=True),
                       torch.cuda.Event(enable_timing=True))
        start.record()
        hiplib.check(lib.nbk_cgm_resolve_f64(
            *common, hiplib.dptr(state), hiplib.dptr(flags),
            hiplib.cur_stream()), 'nbk_cgm_resolve_f64')
        stop.record()
        stop.synchronize()
        times.append(round(start.elapsed_time(stop), 3))
    return times, undecided


def timing(n, box, nmesh, rperp, rpar, repeats):
    from nbodykit_amd.algorithms.pair_counters import kernel
    cat = make_catalog(n, box, nmesh)
    n = cat.csize
    progress('lognormal catalogue of %d objects' % n)
    pos, _ = kernel.to_device_columns(cat['Position'], None, [0, 1, 2])
    box3 = [box] * 3
    pos = kernel.wrap_periodic(pos, box3)
    prio = cgm.rank_priority([cat['Mass']], n)

    def run(per_cell, batch=cgm.SWEEP_BATCH, info=None):
        return cgm.cylindrical_groups(pos, prio, rperp, rpar, los=LOS,
                                      box=box3, periodic=True,
                                      per_cell=per_cell, batch=batch,
                                      info=info)

    by_per_cell = {}
    for per_cell in PER_CELL:
        info = {}
        stages = stage_medians(lambda: run(per_cell, info=info), repeats)
        stages.update(sweeps=info['sweeps'], ncoarse=info['ncoarse'],
                      fine=info['fine'])
        by_per_cell['per_cell=%g' % per_cell] = stages
        progress('per_cell = %g' % per_cell)
    best = min(PER_CELL, key=lambda m: sum(
        by_per_cell['per_cell=%g' % m][s]
        for s in ('cgm_coarse_sort', 'cgm_fine_sort', 'cgm_resolve',
                  'cgm_host', 'cgm_count')))
    by_batch = {}
    for batch in BATCH:
        info = {}
        stages = stage_medians(lambda: run(best, batch, info), repeats)
        by_batch['batch=%d' % batch] = dict(cgm_resolve=stages['cgm_resolve'],
                                            sweeps=info['sweeps'])
        progress('batch = %d' % batch)
    times, undecided = sweep_times(pos, prio, box3, rperp, rpar, best)

    ll = 0.2 * (box ** 3 / n) ** (1. / 3)
    link = stage_medians(lambda: fofmod.fof_minid(pos, ll, box3, True),
                         repeats)
    cgm_type, _, nsat = run(best)
    report({'run': 'cgm timing', 'N': n, 'BoxSize': box, 'rperp': rperp,
            'rpar': rpar, 'repeats': repeats,
            'satellites_per_object': round(float(cgm_type.sum().item()) / n,
                                           3),
            'stages_ms_by_per_cell': by_per_cell, 'fastest_per_cell': best,
            'resolve_ms_by_batch': by_batch,
            'ms_of_every_sweep': times, 'undecided_before_sweep': undecided,
            'fof_link_ms_b0.2': link['fof_link']})


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=float, default=2e5)
    ap.add_argument('--box', type=float, default=250.)
    ap.add_argument('--nmesh', type=int, default=64)
    ap.add_argument('--rperp', type=float, default=None,
                    help='default: 0.5 mean separations')
    ap.add_argument('--rpar', type=float, default=None,
                    help='default: 1.5 mean separations')
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--skip-workflow', action='store_true')
    ap.add_argument('--sizes', type=float, nargs='+', default=[1e6, 1e7])
    ap.add_argument('--timing-box', type=float, default=1000.)
    ap.add_argument('--timing-nmesh', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()

    def radii(n, box):
        sep = box / n ** (1. / 3)
        return (args.rperp if args.rperp is not None else 0.5 * sep,
                args.rpar if args.rpar is not None else 1.5 * sep)

    if not args.skip_workflow:
        workflow(int(args.n), args.box, args.nmesh,
                 *radii(int(args.n), args.box))
    if args.timing:
        for size in args.sizes:
            timing(int(size), args.timing_box, args.timing_nmesh,
                   *radii(int(size), args.timing_box), args.repeats)
