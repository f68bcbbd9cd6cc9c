"""
Pair-counting correlation function next to the FFT estimator: a
LogNormal box through SimulationBox2PCF('2d') and to_poles([0, 2]),
printed beside FFTCorr's multipoles of the same catalogue.

    python examples/paircount_demo.py            # the comparison
    python examples/paircount_demo.py --timing   # BASELINE.md timings

--timing times SimulationBoxPairCount on UniformCatalog-sized boxes held
in a DeviceArrayCatalog (warm-up runs first, device events around each
timed run) and reports the candidate pair evaluations per second, with
the candidate count computed from the cell occupancy.  Needs an MI355X.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..'))

import numpy

from nbodykit_amd.lab import (LogNormalCatalog, LinearPower, FFTCorr,
                              SimulationBox2PCF, SimulationBoxPairCount)
from nbodykit_amd.cosmology import Planck15

# f64 work per candidate pair in the count kernel's inner loop: three
# subtractions of the pair, three of the image shift, three squares and
# two adds; the two range compares and the (rare) binning of an in-range
# pair are not counted
FLOPS_PER_CANDIDATE = 11
# MI355X f64 vector peak: half the 157.3 TFLOPS f32 vector peak, and
# that figure counts an FMA as two flops; the library is built with
# contraction off, so multiplies and adds issue separately and the
# reachable rate is half of it again
F64_VECTOR_PEAK = 78.6e12


def comparison():
    Plin = LinearPower(Planck15, redshift=0.55, transfer='EisensteinHu')
    cat = LogNormalCatalog(Plin=Plin, nbar=3e-4, BoxSize=500., Nmesh=128,
                           bias=2.0, seed=42)
    edges = numpy.linspace(10., 110., 11)

    pc = SimulationBox2PCF('2d', cat, edges, Nmu=20)
    poles = pc.corr.to_poles([0, 2])

    fft = FFTCorr(cat, mode='1d', Nmesh=128, dr=10., rmin=10., rmax=115.,
                  poles=[0, 2])

    print('%d objects, %d pairs counted'
          % (cat.csize, pc.D1D2['npairs'].sum()))
    print('%8s %12s %12s %12s %12s' % ('r', 'xi0 pairs', 'xi0 FFT',
                                       'xi2 pairs', 'xi2 FFT'))
    for i in range(len(edges) - 1):
        print('%8.2f %12.5f %12.5f %12.5f %12.5f'
              % (poles['r'][i], poles['corr_0'][i],
                 numpy.real(fft.poles['corr_0'][i]), poles['corr_2'][i],
                 numpy.real(fft.poles['corr_2'][i])))
    pc.save('paircount_demo.json')
    print('saved paircount_demo.json')


def candidate_evaluations(cat, mode, edges, **kw):
    """Candidate pairs one count pass of this run evaluates, from the
    occupancy of its cell grid, and the number of passes."""
    from nbodykit_amd.algorithms.pair_counters import kernel
    info = {}
    orig = kernel.count_pairs
    kernel.count_pairs = lambda *a, **k: orig(*a, info=info, **k)
    try:
        SimulationBoxPairCount(mode, cat, edges, **kw)
    finally:
        kernel.count_pairs = orig
    return kernel.candidate_pairs(info['start1'], info['start2'],
                                  info['ncell'], True), info['npasses']


def timing(repeats):
    import torch
    from nbodykit_amd import profiling
    from nbodykit_amd.source.catalog.device import DeviceArrayCatalog

    BoxSize = 1000.
    edges = numpy.linspace(1, 50, 26)
    runs = [('1d 1e6', 1e-3, '1d', {}),
            ('2d Nmu=100 1e6', 1e-3, '2d', dict(Nmu=100)),
            ('1d 1e7', 1e-2, '1d', {})]
    for label, nbar, mode, kw in runs:
        N = int(nbar * BoxSize ** 3)
        gen = torch.Generator(device='cuda').manual_seed(42)
        pos = torch.rand(N, 3, dtype=torch.float64, device='cuda',
                         generator=gen) * BoxSize
        weight = torch.ones(N, dtype=torch.float64, device='cuda')
        cat = DeviceArrayCatalog({'Position': pos, 'Weight': weight},
                                 BoxSize=BoxSize)

        candidates, npasses = candidate_evaluations(cat, mode, edges,
                                                    **kw)   # warm-up 1
        SimulationBoxPairCount(mode, cat, edges, **kw)      # warm-up 2
        torch.cuda.synchronize()

        profiling.enable()
        walls = []
        for _ in range(repeats):
            start = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            start.record()
            r = SimulationBoxPairCount(mode, cat, edges, **kw)
            end.record()
            torch.cuda.synchronize()
            walls.append(start.elapsed_time(end))
        split = profiling.summary()
        profiling.disable()

        count_ms = split['pairs_count']['ms'] / repeats
        rate = candidates * npasses / (count_ms * 1e-3)
        print(json.dumps({
            'run': label, 'N': N, 'wall_ms': [round(w, 2) for w in walls],
            'sort_ms': round(split['pairs_sort']['ms'] / repeats, 3),
            'count_ms': round(count_ms, 3),
            'passes': npasses,
            'candidates_per_pass': candidates,
            'npairs': int(r.pairs['npairs'].sum()),
            'candidates_per_s': rate,
            'share_of_f64_vector_peak':
                rate * FLOPS_PER_CANDIDATE / F64_VECTOR_PEAK}))
        sys.stdout.flush()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if args.timing:
        timing(args.repeats)
    else:
        comparison()
