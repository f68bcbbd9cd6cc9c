"""
KDDensity, the 7th-nearest-neighbour density proxy, and the workflow it is
the other half of: the density of a LogNormalCatalog becomes the peak
column of FOF.find_features.

    python examples/kddensity_demo.py
    python examples/kddensity_demo.py --timing --sizes 1e6 1e7

With ``--timing`` it also prints, per catalogue (uniform and lognormal at
every size), the HIP-event time of the three stages of the search
(``knn_coarse_sort``, ``knn_fine_sort``, ``knn_search``; the median of
``--repeats`` runs after a warm-up) for 1, 2, 4 and 8 particles per cell,
and for scale two runs that are NOT the code under test:

  - the ``fof_link`` stage of FOF at b = 0.2 on the same catalogue: one
    fixed walk over 27 cells, the natural floor of a cell-list search;
  - scipy's ``cKDTree(pos, boxsize).query(pos, k=[8], workers=16)`` on the
    host, which is what the reference runs.

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

from nbodykit_amd import profiling
from nbodykit_amd.algorithms import fof as fofmod
from nbodykit_amd.algorithms import kdtree
from nbodykit_amd.lab import (FOF, KDDensity, LinearPower, LogNormalCatalog,
                              Planck15, UniformCatalog)

T0 = time.perf_counter()
PER_CELL = (1., 2., 4., 8.)


def progress(what):
    """a timestamped line on stderr, so that a long run shows where it is"""
    sys.stderr.write('[%7.1f s] %s\n' % (time.perf_counter() - T0, what))
    sys.stderr.flush()


def report(record):
    print(json.dumps(record), flush=True)


def make_catalog(kind, n, box, nmesh):
    nbar = n / box ** 3
    if kind == 'uniform':
        return UniformCatalog(nbar=nbar, BoxSize=box, seed=42)
    Plin = LinearPower(Planck15, redshift=0.55, transfer='EisensteinHu')
    return LogNormalCatalog(Plin=Plin, nbar=nbar, BoxSize=box, Nmesh=nmesh,
                            seed=42)


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


def workflow(n, box, nmesh):
    """density -> peak column of the FOF group catalogue"""
    source = make_catalog('lognormal', n, box, nmesh)
    progress('lognormal catalogue of %d points' % source.csize)
    t0 = time.perf_counter()
    kd = KDDensity(source)
    wall = time.perf_counter() - t0
    source['Density'] = kd.density
    fof = FOF(source, linking_length=0.2, nmin=20)
    halos = fof.find_features(peakcolumn='Density')
    length = numpy.asarray(halos['Length'])
    # in units of the mean density: n(<d) = 8 at d, the point included
    mean = source.csize / box ** 3
    unit = 8. / (4. / 3 * numpy.pi) / mean
    report({
        'run': 'KDDensity -> FOF.find_features(peakcolumn)',
        'N': source.csize, 'BoxSize': box,
        'meansep_attr': kd.attrs['meansep'],
        'wall_s_first_call': round(wall, 3),
        'density_over_mean_percentiles_1_50_99': [
            round(float(v), 3) for v in
            numpy.percentile(kd.density * unit, [1, 50, 99])],
        'halos_above_nmin': int(halos.csize - 1),
        'largest_halo': int(length.max()),
        'peak_of_largest_halo': [
            round(float(v), 3) for v in
            numpy.asarray(halos['PeakPosition'])[int(length.argmax())]]})


def timing(kind, n, box, nmesh, repeats, workers):
    import torch
    from nbodykit_amd.algorithms.pair_counters import kernel
    cat = make_catalog(kind, n, box, nmesh)
    n = cat.csize
    progress('%s catalogue of %d points' % (kind, n))
    host = numpy.remainder(numpy.asarray(cat['Position'], dtype='f8'), box)
    pos, _ = kernel.to_device_columns(host, None, [0, 1, 2])
    pos = kernel.wrap_periodic(pos, [box] * 3)
    box3 = [box] * 3

    table = {}
    for per_cell in PER_CELL:
        info = {}
        stages = stage_medians(
            lambda: kdtree.knn(pos, 7, box=box3, per_cell=per_cell,
                               info=info), repeats)
        occ = torch.diff(info['fine_start'])
        stages.update(ncoarse=info['ncoarse'], fine=info['fine'],
                      max_cell_occupancy=int(occ.max().item()))
        table['per_cell=%g' % per_cell] = stages
        progress('per_cell = %g' % per_cell)
    r2, _ = kdtree.knn(pos, 7, box=box3)
    d_gpu = r2.sqrt().cpu().numpy()

    ll = 0.2 * (box ** 3 / n) ** (1. / 3)
    link = stage_medians(lambda: fofmod.fof_minid(pos, ll, box3, True),
                         repeats)
    progress('fof_link')

    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(host, boxsize=box)
    t1 = time.perf_counter()
    d, _ = tree.query(host, k=[8], workers=workers)
    t2 = time.perf_counter()
    progress('scipy')
    best = min(PER_CELL, key=lambda m: table['per_cell=%g' % m]['knn_search'])
    gpu_ms = sum(table['per_cell=%g' % best][s] for s in
                 ('knn_coarse_sort', 'knn_fine_sort', 'knn_search'))
    report({
        'run': 'knn k=7 timing', 'kind': kind, 'N': n, 'BoxSize': box,
        'repeats': repeats, 'stages_ms': table,
        'fof_link_ms_b0.2': link['fof_link'],
        'scipy_build_s': round(t1 - t0, 2),
        'scipy_query_s_workers%d' % workers: round(t2 - t1, 2),
        'fastest_per_cell': best,
        'gpu_three_stages_ms_at_fastest': round(gpu_ms, 3),
        'speedup_over_scipy_build_plus_query':
        round((t2 - t0) / (1e-3 * gpu_ms), 1),
        'max_rel_diff_of_d_to_scipy':
        float(numpy.max(numpy.abs(d_gpu - d[:, 0]) / d[:, 0]))})


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=float, default=2e5)
    ap.add_argument('--box', type=float, default=250.)
    ap.add_argument('--nmesh', type=int, default=64)
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--skip-workflow', action='store_true')
    ap.add_argument('--sizes', type=float, nargs='+', default=[1e6, 1e7])
    ap.add_argument('--kinds', nargs='+', default=['uniform', 'lognormal'],
                    choices=['uniform', 'lognormal'])
    ap.add_argument('--timing-box', type=float, default=1000.)
    ap.add_argument('--timing-nmesh', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--workers', type=int, default=16)
    args = ap.parse_args()
    if not args.skip_workflow:
        workflow(int(args.n), args.box, args.nmesh)
    if args.timing:
        for size in args.sizes:
            for kind in args.kinds:
                timing(kind, int(size), args.timing_box, args.timing_nmesh,
                       args.repeats, args.workers)
