"""
FiberCollisions, the fibre collision groups of a survey and the fibre
assignment inside them, on a random patch of sky.

    python examples/fibercollisions_demo.py
    python examples/fibercollisions_demo.py --timing --sizes 1e6 1e7

It prints the HIP-event time of every stage of one call and the sizes of the
two populations, and checks the two properties the reference's test asks for
by brute force: no two clean objects collide, and every collided object
collides with some object.

With ``--timing`` it also prints, per size, the stage times (the median of
``--repeats`` runs after a warm-up) of the whole pipeline on a uniform
full-sky catalogue at 62 arcseconds for 2, 0.5, 0.25 and 0.125 objects per
cell of the FOF grid, and the same on a 10 x 5 degree patch of
``--patch-size`` objects.

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
from nbodykit_amd.algorithms import fibercollisions as fc
from nbodykit_amd.algorithms import fof as fofmod
from nbodykit_amd.lab import FiberCollisions

T0 = time.perf_counter()
PER_CELL = (2., 0.5, 0.25, 0.125)
RADIUS = 62 / 60. / 60.
STAGES = ('fof_coarse_sort', 'fof_fine_sort', 'fof_link', 'fof_flatten',
          'fof_minid', 'fof_labels', 'fibers_groups', 'fibers_assign')


def progress(what):
    """a timestamped line on stderr, so that a long run shows where it is"""
    sys.stderr.write('[%7.1f s] %s\n' % (time.perf_counter() - T0, what))
    sys.stderr.flush()


def report(record):
    print(json.dumps(record), flush=True)


def patch(n, seed=42):
    """n objects uniform in ra over [0, 10) and in dec over [-5, 0) degrees
    (the input of the reference's test)"""
    rng = numpy.random.RandomState(seed)
    return 10. * rng.random_sample(n), 5. * rng.random_sample(n) - 5.


def full_sky(n, seed=42):
    """n objects uniform on the sphere, in degrees"""
    rng = numpy.random.RandomState(seed)
    ra = 360. * rng.random_sample(n)
    dec = numpy.rad2deg(numpy.arcsin(2. * rng.random_sample(n) - 1.))
    return ra, dec


def brute_force_properties(pos, ll, collided, rows=500):
    """(clean pairs within the radius, collided objects that collide with
    nothing), O(n^2) a slab of rows at a time"""
    collided = collided.astype(bool)
    clean_pairs, touched = 0, numpy.zeros(len(pos), dtype=bool)
    for lo in range(0, len(pos), rows):
        d = pos[lo:lo + rows, None, :] - pos[None, :, :]
        hit = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])
               + d[..., 2] * d[..., 2]) <= ll * ll
        hit[numpy.arange(len(hit)), lo + numpy.arange(len(hit))] = False
        touched[lo:lo + rows] = hit.any(axis=1)
        clean = ~collided[lo:lo + rows, None] & ~collided[None, :]
        clean_pairs += int((hit & clean).sum())
    return clean_pairs // 2, int((collided & ~touched).sum())


def workflow(n):
    ra, dec = patch(n)
    FiberCollisions(ra, dec, seed=42)                # warm-up
    profiling.enable()
    r = FiberCollisions(ra, dec, seed=42)
    stages = {name: round(rec['ms'], 3)
              for name, rec in profiling.summary().items()}
    profiling.disable()
    label = numpy.asarray(r.labels['Label'])
    collided = numpy.asarray(r.labels['Collided'])
    size = numpy.bincount(label)[1:]
    report({'run': 'FiberCollisions', 'N': n, 'collision_radius': RADIUS,
            'seed': r.attrs['seed'], 'stages_ms': stages,
            'groups': int(len(size)),
            'largest_group': int(size.max()) if len(size) else 0,
            'objects_in_groups': int((label > 0).sum()),
            'collided': int(collided.sum()),
            'collision_fraction': round(float(collided.mean()), 4)})
    clean_pairs, lonely = brute_force_properties(
        numpy.asarray(r.source['Position']), r._collision_radius_rad,
        collided)
    report({'run': 'the two properties by brute force', 'N': n,
            'clean_pairs_within_the_radius': clean_pairs,
            'collided_that_collide_with_nothing': lonely})
    if clean_pairs or lonely:
        raise SystemExit('the assignment breaks one of the two properties')


def pipeline(pos, ll, seed, per_cell):
    """what FiberCollisions.run launches, with the FOF grid's per_cell"""
    minid = fofmod.fof_minid(pos, ll, None, False, per_cell=per_cell)
    with profiling.collect('fof_labels', units=int(pos.shape[0])):
        label = fofmod.assign_labels(minid, 1)
    collided, _ = fc.assign_fibers(pos, label, ll, seed)
    return label, collided


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


def timing(what, ra, dec, repeats):
    import torch
    n = len(ra)
    pos = torch.from_numpy(fc.sky_to_position(ra, dec, True)).cuda()
    pos = pos.contiguous()
    ll = float(numpy.deg2rad(RADIUS))
    by_per_cell = {}
    for per_cell in PER_CELL:
        info = {}

        def run():
            info['label'], info['collided'] = pipeline(pos, ll, 42, per_cell)
        stages = stage_medians(run, repeats)
        stages['total'] = round(sum(stages.get(s, 0.) for s in STAGES), 3)
        by_per_cell['per_cell=%g' % per_cell] = stages
        progress('%s, n = %d, per_cell = %g' % (what, n, per_cell))
    size = torch.bincount(info['label'].to(torch.int64))[1:]
    report({'run': 'fiber collisions timing', 'catalogue': what, 'N': n,
            'collision_radius': RADIUS, 'repeats': repeats,
            'groups': int(size.numel()),
            'largest_group': int(size.max().item()) if size.numel() else 0,
            'collided': int(info['collided'].sum().item()),
            'stages_ms_by_per_cell': by_per_cell,
            'fastest_per_cell': min(
                PER_CELL,
                key=lambda m: by_per_cell['per_cell=%g' % m]['total'])})


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=float, default=1e4)
    ap.add_argument('--timing', action='store_true')
    ap.add_argument('--skip-workflow', action='store_true')
    ap.add_argument('--sizes', type=float, nargs='+', default=[1e6, 1e7])
    ap.add_argument('--patch-size', type=float, default=1e5)
    ap.add_argument('--repeats', type=int, default=5)
    args = ap.parse_args()

    if not args.skip_workflow:
        workflow(int(args.n))
    if args.timing:
        timing('10 x 5 degree patch', *patch(int(args.patch_size)),
               repeats=args.repeats)
        for size in args.sizes:
            timing('full sky', *full_sky(int(size)), repeats=args.repeats)
