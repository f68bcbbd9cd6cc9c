"""
Friends-of-friends halos of a uniform or a lognormal catalogue in a
periodic box: FOF at b = 0.2 with find_features.  Prints the time per
stage of the GPU run (HIP events of the timed run after a warm-up), the
number of groups and the candidate pairs per second of the link kernel,
and for scale two runs that are NOT the code under test:

  - the ``pairs_count`` stage of SimulationBoxPairCount('1d',
    edges=[ll/2, ll]) on the same catalogue: the same neighbour walk
    without the union-find, on the single-level grid of at most 34 cells
    per axis (what the finer two-level grid buys);
  - a host FOF, scipy's cKDTree.query_pairs + connected_components, on a
    subsample at the same b.

    python examples/fof_demo.py
    python examples/fof_demo.py --kind lognormal --n 1e7 --subsample 1e6

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
from nbodykit_amd.lab import (FOF, ArrayCatalog, LinearPower,
                              LogNormalCatalog, Planck15,
                              SimulationBoxPairCount, UniformCatalog)


T0 = time.perf_counter()


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


def profiled(run):
    """stage times {name: ms} and the result of one run after a warm-up"""
    import torch
    run()
    torch.cuda.synchronize()
    profiling.enable()
    t0 = time.perf_counter()
    result = run()
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    stages = {k: round(v['ms'], 3) for k, v in profiling.summary().items()}
    profiling.disable()
    return stages, wall, result


def host_fof(pos, ll, box):
    """number of groups by cKDTree.query_pairs + connected_components"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(pos)
    tree = cKDTree(numpy.remainder(pos, box), boxsize=box)
    pairs = tree.query_pairs(ll, output_type='ndarray')
    graph = coo_matrix((numpy.ones(len(pairs), dtype='i1'),
                        (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    return connected_components(graph, directed=False)[0]


def main(kind, n, box, b, nmin, nmesh, subsample):
    import torch
    from nbodykit_amd.algorithms.pair_counters import kernel
    cat = make_catalog(kind, n, box, nmesh)
    n = cat.csize
    progress('%s catalogue of %d points' % (kind, n))
    ll = b * (box ** 3 / n) ** (1. / 3)
    # positions on the device once: the stages time kernels, not PCIe
    pos, _ = kernel.to_device_columns(cat['Position'], None, [0, 1, 2])
    dcat = ArrayCatalog({'Position': numpy.asarray(cat['Position']),
                         'Velocity': numpy.asarray(cat['Velocity'])
                         if 'Velocity' in cat
                         else numpy.zeros((n, 3), dtype='f4')}, BoxSize=box)

    progress('columns on the device')
    stages, wall, f = profiled(lambda: FOF(dcat, b, nmin))
    progress('FOF twice')
    info = {}
    wrapped = kernel.wrap_periodic(pos, [box] * 3)
    fofmod.fof_minid(wrapped, ll, [box] * 3, True, info=info)
    cand = fofmod.candidate_pairs(info['fine_start'], info['ncoarse'],
                                  info['fine'], True)
    occ = torch.diff(info['fine_start'])
    ngroups = len(numpy.unique(f.labels)) - 1
    progress('candidate pairs')
    halos = f.find_features()
    progress('find_features')
    report({
        'run': 'FOF b=%g nmin=%d' % (b, nmin), 'kind': kind, 'N': n,
        'BoxSize': box, 'll': round(ll, 5),
        'ncoarse': info['ncoarse'], 'fine': info['fine'],
        'max_cell_occupancy': int(occ.max().item()),
        'stages_ms': stages, 'wall_ms': round(wall, 1),
        'halos_above_nmin': ngroups,
        'largest_halo': int(numpy.asarray(halos['Length']).max()),
        'particles_in_halos': int((f.labels > 0).sum()),
        'candidate_pairs': cand,
        'candidate_pairs_per_s':
        round(cand / (1e-3 * stages['fof_link']))})
    all_groups = FOF(dcat, b, 0)
    report({'run': 'FOF b=%g nmin=0' % b,
            'groups': int(all_groups.labels.max())})
    del all_groups, wrapped, info, occ
    progress('FOF at nmin = 0')

    # for scale 1: the pair counter's neighbour walk on its 34-cell grid
    edges = [0.5 * ll, ll]
    stages, wall, r = profiled(
        lambda: SimulationBoxPairCount('1d', dcat, edges))
    report({
        'run': "SimulationBoxPairCount('1d', [ll/2, ll])", 'N': n,
        'stages_ms': stages, 'wall_ms': round(wall, 1),
        'npairs': int(r.pairs['npairs'][0])})

    progress('pair count')

    # for scale 2: a host FOF on a random subsample, at the same b (the
    # rows of a lognormal catalogue are in mesh-cell order)
    m = min(int(subsample), n)
    rows = numpy.sort(numpy.random.RandomState(1).choice(n, m,
                                                         replace=False))
    sub = numpy.asarray(cat['Position'], dtype='f8')[rows]
    ll_sub = b * (box ** 3 / m) ** (1. / 3)
    t0 = time.perf_counter()
    host_groups = host_fof(sub, ll_sub, box)
    host_s = time.perf_counter() - t0
    progress('host FOF')
    scat = ArrayCatalog({'Position': sub}, BoxSize=box)
    stages, wall, fs = profiled(lambda: FOF(scat, b, 0))
    report({
        'run': 'host cKDTree FOF on a subsample', 'N': m,
        'll': round(ll_sub, 5), 'host_s': round(host_s, 2),
        'host_groups': int(host_groups),
        'gpu_groups': int(fs.labels.max()),
        'gpu_wall_ms': round(wall, 1), 'gpu_stages_ms': stages})


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--kind', choices=['uniform', 'lognormal'],
                    default='uniform')
    ap.add_argument('--n', type=float, default=1e6)
    ap.add_argument('--box', type=float, default=1000.)
    ap.add_argument('--b', type=float, default=0.2)
    ap.add_argument('--nmin', type=int, default=20)
    ap.add_argument('--nmesh', type=int, default=256)
    ap.add_argument('--subsample', type=float, default=1e6)
    args = ap.parse_args()
    main(args.kind, int(args.n), args.box, args.b, args.nmin, args.nmesh,
         args.subsample)
