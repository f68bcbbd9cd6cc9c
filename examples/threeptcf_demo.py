"""
Multipoles of the isotropic three-point correlation function of a
uniform catalogue in a periodic box: SimulationBox3PCF with poles 0..10
and 10 separation bins.  Prints the wall-clock time and the primaries per
second of the GPU run (median of the timed runs after a warm-up), and for
scale the time of the numpy restatement of the same algorithm
(tests/threeptcf_reference.py) on a subsample of at most 2000 points,
beside the GPU on that same subsample.

    python examples/threeptcf_demo.py
    python examples/threeptcf_demo.py --nbar 1e-3 --repeats 5

Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', 'tests'))

import numpy

from nbodykit_amd.lab import ArrayCatalog, SimulationBox3PCF, UniformCatalog


def timed(run, repeats):
    """wall ms of each of ``repeats`` runs after one warm-up, last result"""
    import torch
    run()
    torch.cuda.synchronize()
    walls = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        walls.append(1e3 * (time.perf_counter() - t0))
    return walls, r


def main(nbar, box, rmax, repeats, subsample):
    import threeptcf_reference as ref
    poles = list(range(11))
    edges = numpy.linspace(0., rmax, 11)
    cat = UniformCatalog(nbar=nbar, BoxSize=box, seed=42)
    n = cat.csize
    # mean number of secondaries within rmax of a primary
    nsec = nbar * 4. / 3 * numpy.pi * rmax ** 3

    walls, r = timed(lambda: SimulationBox3PCF(cat, poles, edges), repeats)
    med = float(numpy.median(walls))
    print(json.dumps({
        'run': 'SimulationBox3PCF poles 0..10, 10 bins', 'N': n,
        'BoxSize': box, 'rmax': rmax, 'secondaries_per_primary':
        round(nsec, 1), 'wall_ms': [round(w, 2) for w in walls],
        'median_ms': round(med, 2),
        'primaries_per_s': round(n / (1e-3 * med))}))
    print('%6s %14s %14s %14s' % ('r', 'zeta_0(r, r)', 'zeta_1(r, r)',
                                  'zeta_2(r, r)'))
    for i in range(len(edges) - 1):
        print('%6.1f %14.6e %14.6e %14.6e'
              % (0.5 * (edges[i] + edges[i + 1]),
                 r.poles['corr_0'][i, i], r.poles['corr_1'][i, i],
                 r.poles['corr_2'][i, i]))

    # for scale: the numpy restatement, and the GPU, on a subsample
    pos = numpy.asarray(cat['Position'])[:subsample]
    w = numpy.ones(len(pos))
    t0 = time.perf_counter()
    want = ref.alm_zeta(pos, w, edges, 10, box=box)
    host_s = time.perf_counter() - t0
    sub = ArrayCatalog({'Position': pos}, BoxSize=box)
    walls, rs = timed(lambda: SimulationBox3PCF(sub, poles, edges), repeats)
    got = numpy.array([rs.poles['corr_%d' % ell] for ell in poles])
    scale = ref.cauchy_schwarz_scale(want)
    live = scale > 0
    print(json.dumps({
        'run': 'subsample', 'N': len(pos),
        'numpy_restatement_s': round(host_s, 3),
        'gpu_median_ms': round(float(numpy.median(walls)), 2),
        'max_err_over_scale':
        float((numpy.abs(got - want)[live] / scale[live]).max())}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--nbar', type=float, default=1e-4)
    ap.add_argument('--box', type=float, default=1000.)
    ap.add_argument('--rmax', type=float, default=100.)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--subsample', type=int, default=2000)
    args = ap.parse_args()
    main(args.nbar, args.box, args.rmax, args.repeats,
         min(args.subsample, 2000))
