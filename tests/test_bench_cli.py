"""
bench.py command line: a plain run prints the headline line only,
`--full` adds the roofline / CPU-baseline legs, `--dump-outputs` writes
the last timed step's result as float64 .npy files.
"""
import json
import os
import subprocess
import sys
import types

import numpy
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = {'metric', 'value', 'unit', 'higher_is_better', 'dtype',
            'ms_per_step', 'steps', 'warmup', 'n_gpus'}


def run_bench(*argv):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')]
                          + list(argv), cwd=ROOT, capture_output=True,
                          text=True, timeout=240)


def test_dump_outputs_layout(tmp_path):
    import bench
    from nbodykit_amd.binned_statistic import BinnedStatistic
    data = numpy.zeros(4, dtype=[('k', 'f8'), ('power', 'c16'),
                                 ('modes', 'i8')])
    data['k'] = [0.1, 0.2, numpy.nan, 0.4]
    data['power'] = [1 + 2j, 3, 4, 5 - 1j]
    data['modes'] = [6, 8, 0, 12]
    power = BinnedStatistic(['k'], [numpy.arange(5.)], data)
    result = types.SimpleNamespace(
        power=power, poles=None,
        attrs={'shotnoise': 125., 'N1': 7, 'N2': 7})
    out = str(tmp_path / 'dump')
    bench.dump_outputs(result, out)
    assert sorted(os.listdir(out)) == [
        'attrs_N1.npy', 'attrs_N2.npy', 'attrs_shotnoise.npy',
        'power_k.npy', 'power_modes.npy', 'power_power_imag.npy',
        'power_power_real.npy']
    for fn in os.listdir(out):
        assert numpy.load(os.path.join(out, fn)).dtype == numpy.float64
    numpy.testing.assert_array_equal(
        numpy.load(os.path.join(out, 'power_power_real.npy')),
        data['power'].real)
    numpy.testing.assert_array_equal(
        numpy.load(os.path.join(out, 'power_power_imag.npy')),
        data['power'].imag)
    numpy.testing.assert_array_equal(
        numpy.load(os.path.join(out, 'power_modes.npy')), data['modes'])
    numpy.testing.assert_array_equal(
        numpy.load(os.path.join(out, 'power_k.npy')), data['k'])


def test_steps_must_be_positive():
    p = run_bench('--steps', '0')
    assert p.returncode == 2
    assert '--steps must be at least 1' in p.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps(tmp_path):
    out = str(tmp_path / 'dump')
    p = run_bench('--gpus', '1', '--steps', '3', '--warmup', '1',
                  '--workload', 'c2', '--particles', '200000',
                  '--nmesh', '64', '--dump-outputs', out)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert HEADLINE <= set(line)
    assert 'roofline' not in line and 'cpu_baseline' not in line
    assert line['steps'] == 3 and line['warmup'] == 1
    assert line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(
        line['config']['particles'] / (line['ms_per_step'] * 1e-3))
    modes = numpy.load(os.path.join(out, 'power_modes.npy'))
    power = numpy.load(os.path.join(out, 'power_power_real.npy'))
    assert modes.dtype == power.dtype == numpy.float64
    assert modes.shape == power.shape and modes.sum() > 0
    assert numpy.isfinite(power[modes > 0]).all()


@pytest.mark.gpu
def test_full_run_reports_roofline_and_cpu_baseline():
    p = run_bench('--gpus', '1', '--steps', '2', '--warmup', '1',
                  '--workload', 'c2', '--particles', '200000',
                  '--nmesh', '64', '--full')
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert HEADLINE <= set(line)
    assert line['roofline']['paint_ms_per_launch'] > 0
    assert line['cpu_baseline']['value'] > 0
