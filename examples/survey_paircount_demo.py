"""
Configuration-space clustering of survey data (the reference's
SurveyData2PCF flow): mock data and randoms on the sky -> xi(s, mu) with
the pair line of sight -> multipoles, and the angular correlation
function w(theta) of the same catalogues.  Prints wall times.

    python examples/survey_paircount_demo.py            # the flow
    python examples/survey_paircount_demo.py --timing   # BASELINE.md timings

--timing times SurveyDataPairCount('2d') on a mock catalogue and
SimulationBoxPairCount('2d', periodic=False) on the same Cartesian
positions (warm-up runs first, device events around each timed run).
Needs an MI355X.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))

import numpy

from nbodykit_amd.lab import (ArrayCatalog, SimulationBoxPairCount,
                              SurveyData2PCF, SurveyDataPairCount,
                              transform)
from nbodykit_amd.cosmology import Planck15


def make_survey(n, seed):
    """uniform in RA, sin(DEC) and redshift over a 30 x 30 degree patch"""
    rng = numpy.random.RandomState(seed)
    ra = rng.uniform(120., 150., n)
    lo, hi = numpy.sin(numpy.deg2rad([-5., 25.]))
    dec = numpy.rad2deg(numpy.arcsin(rng.uniform(lo, hi, n)))
    z = rng.uniform(0.4, 0.7, n)
    return ArrayCatalog({'RA': ra, 'DEC': dec, 'Redshift': z})


def flow():
    data = make_survey(50000, 42)
    randoms = make_survey(150000, 84)
    edges = numpy.linspace(10., 110., 11)

    t0 = time.time()
    r = SurveyData2PCF('2d', data, randoms, edges, cosmo=Planck15, Nmu=20)
    t1 = time.time()
    poles = r.corr.to_poles([0, 2])
    print('%d data, %d randoms: xi(s, mu) in %.2f s (%d data pairs, '
          '%d random pairs)' % (data.csize, randoms.csize, t1 - t0,
                                r.D1D2['npairs'].sum(),
                                r.R1R2['npairs'].sum()))
    print('%8s %12s %12s' % ('s', 'xi0', 'xi2'))
    for i in range(len(edges) - 1):
        print('%8.2f %12.5f %12.5f' % (poles['r'][i], poles['corr_0'][i],
                                       poles['corr_2'][i]))

    theta = numpy.geomspace(0.01, 5., 11)
    t0 = time.time()
    w = SurveyData2PCF('angular', data, randoms, theta)
    t1 = time.time()
    print('w(theta) in %.2f s' % (t1 - t0))
    print('%10s %12s' % ('theta', 'w'))
    for i in range(len(theta) - 1):
        print('%10.4f %12.5f' % (w.corr['theta'][i], w.corr['corr'][i]))

    r.save('survey_paircount_demo.json')
    print('saved survey_paircount_demo.json')


def timed(run, repeats):
    """(wall ms of each run, count + reduce ms per run, last result)"""
    import torch
    from nbodykit_amd import profiling
    run()
    run()                                       # two warm-up runs
    torch.cuda.synchronize()
    profiling.enable()
    walls = []
    for _ in range(repeats):
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        r = run()
        end.record()
        torch.cuda.synchronize()
        walls.append(start.elapsed_time(end))
    split = profiling.summary()
    profiling.disable()
    return walls, split['pairs_count']['ms'] / repeats, r


def timing(repeats, n=200000):
    sky = make_survey(n, 42)
    edges = numpy.linspace(1., 100., 21)
    pos = transform.SkyToCartesian(sky['RA'], sky['DEC'], sky['Redshift'],
                                   Planck15)
    # the same points as a box catalogue: only the line of sight differs
    box = ArrayCatalog({'Position': pos - pos.min(axis=0)},
                       BoxSize=float((pos.max(axis=0)
                                      - pos.min(axis=0)).max()) + 1.)
    runs = [
        ('SurveyDataPairCount 2d',
         lambda: SurveyDataPairCount('2d', sky, edges, cosmo=Planck15,
                                     Nmu=20)),
        ('SimulationBoxPairCount 2d periodic=False',
         lambda: SimulationBoxPairCount('2d', box, edges, Nmu=20,
                                        periodic=False)),
    ]
    for label, run in runs:
        walls, count_ms, r = timed(run, repeats)
        print(json.dumps({
            'run': label, 'N': n, 'wall_ms': [round(w, 2) for w in walls],
            'count_ms': round(count_ms, 3),
            'npairs': int(r.pairs['npairs'].sum())}))
        sys.stdout.flush()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if args.timing:
        timing(args.repeats)
    else:
        flow()
