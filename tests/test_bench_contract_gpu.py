"""GPU: bench.py's contract with the driver -- one JSON line with the agreed keys, at N = 1 directly and under torchrun with one rank (RCCL
initialised, barriers, the optional gather), plain and with --full, and the outputs --dump-outputs writes -- on a small batch so that the
test takes seconds."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config', 'roofline'}


def run(cmd):
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [line for line in res.stdout.splitlines() if line.startswith('{')]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def check(line, steps, warmup):
    assert KEYS <= set(line), KEYS - set(line)
    assert line['steps'] == steps and line['warmup'] == warmup and line['n_gpus'] == 1 and line['higher_is_better'] is True
    assert line['dtype'] == 'f64' and line['data'] == 'synthetic' and line['vs_baseline'] is None and 'workload' in line['config']
    assert line['value'] > 0 and line['ms_per_step'] > 0
    roof = line['roofline']
    assert {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'} <= set(roof) and roof['bound'] == 'hbm' and roof['peak'] == 8000.
    assert abs(roof['frac'] - roof['achieved'] / roof['peak']) < 1e-12
    assert line['parity_spot_check_tilted_err'] < 1e-13


def test_single_process_line():
    line = run([sys.executable, 'bench.py', '--rows', '4000', '--steps', '3', '--warmup', '1', '--ramp-ms', '20', '--no-cpu-baseline', '--no-secondary', '--full'])
    check(line, 3, 1)
    assert line['scaling'] == 'weak' and line['config']['rccl_ranks'] == 0 and line['value_api'] > 0


def test_one_rank_under_torchrun():
    base = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr', '127.0.0.1']
    line = run(base + ['--master-port', '29541', 'bench.py', '--gpus', '1', '--rows', '4000', '--steps', '3', '--warmup', '1', '--ramp-ms', '20',
                       '--no-cpu-baseline', '--no-secondary', '--gather', '--full'])
    check(line, 3, 1)
    assert line['config']['rccl_ranks'] == 1 and line['gather_ms'] > 0 and line['value_with_gather'] > 0
    split = run(base + ['--master-port', '29542', 'bench.py', '--gpus', '1', '--config', '5', '--rows', '200000', '--steps', '2', '--warmup', '1', '--gather'])
    assert split['scaling'] == 'strong' and split['config']['rccl_ranks'] == 1 and split['value'] > 0 and split['unit'] == 'samples/s'
    assert split['parity_spot_check']['max_rel_err'] < 1e-10 and split['ms_per_step_rank_min'] <= split['ms_per_step_rank_max'] <= split['ms_per_step'] * 1.01
    # config 4 under the launcher: both filters on the rank's block of cosmologies, each with its oracle spot check on the line
    filt = run(base + ['--master-port', '29543', 'bench.py', '--gpus', '1', '--config', '4', '--rows', '3000', '--steps', '2', '--warmup', '1', '--gather'])
    assert filt['scaling'] == 'strong' and filt['config']['rccl_ranks'] == 1 and filt['unit'] == 'filtered vectors/s' and filt['value'] > 0
    assert filt['config']['per_gpu'] == 3000 and len(filt['ms_per_step_by_rank']) == 1 and filt['gather_ms'] > 0
    for engine in ('wallish2018', 'brieden2022'):
        assert filt['parity_spot_check'][engine]['max_rel_err'] < 1e-9
    assert line['ms_per_step_rank_min'] <= line['ms_per_step_rank_max'] and len(line['ms_per_step_by_rank']) == 1
    # what a multi-GPU --full run prints by default (here forced on one rank): the gather timed, the strong splits of configs 4 and 5 on the same line
    multi = run(base + ['--master-port', '29544', 'bench.py', '--gpus', '1', '--rows', '3000', '--steps', '2', '--warmup', '1', '--ramp-ms', '20',
                        '--no-cpu-baseline', '--no-secondary', '--split-configs', '--gather', '--full'])
    check(multi, 2, 1)
    assert multi['gather_ms'] > 0 and set(multi['split_configs']) == {'config4', 'config5'}
    for name, unit in (('config4', 'filtered vectors/s'), ('config5', 'samples/s')):
        sub = multi['split_configs'][name]
        assert sub['unit'] == unit and sub['value'] > 0 and sub['scaling'] == 'strong' and sub['config']['rccl_ranks'] == 1 and sub['value_with_gather'] > 0


def test_self_launch():
    """`python bench.py --gpus N` without a launcher starts its own ranks: with --launcher also for N = 1 (RCCL then initialised); asking for more
    GPUs than the node has, or a launcher whose world size is not --gpus, exits non-zero instead of printing a line."""
    import torch
    small = ['--rows', '4000', '--steps', '3', '--warmup', '1', '--ramp-ms', '20', '--no-cpu-baseline', '--no-secondary', '--full']
    line = run([sys.executable, 'bench.py', '--gpus', '1', '--launcher'] + small)
    check(line, 3, 1)
    assert line['config']['rccl_ranks'] == 1
    too_many = torch.cuda.device_count() + 1
    res = subprocess.run([sys.executable, 'bench.py', '--gpus', str(too_many)] + small, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=600)
    assert res.returncode != 0 and not any(ln.startswith('{') for ln in res.stdout.splitlines()) and 'GPU(s) visible' in res.stderr
    env = dict(os.environ, RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
    res = subprocess.run([sys.executable, 'bench.py', '--gpus', '2'] + small, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=600)
    assert res.returncode != 0 and not any(ln.startswith('{') for ln in res.stdout.splitlines()) and 'WORLD_SIZE' in res.stderr


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline keys and nothing that needs a measurement of its own; --dump-outputs writes the output grid
    and the sampled rows of the last timed step, which are the transforms of the bench's input rows (numpy oracle)."""
    import numpy as np
    import bench
    from oracle import fftlog as ofl
    from oracle.workloads import pk_eh_default, config2_rows
    nb, dump = 4000, tmp_path / 'out'
    line = run([sys.executable, 'bench.py', '--rows', str(nb), '--steps', '3', '--warmup', '1', '--ramp-ms', '20', '--dump-outputs', str(dump)])
    assert KEYS <= set(line), KEYS - set(line)
    assert line['steps'] == 3 and line['warmup'] == 1 and line['n_gpus'] == 1 and line['higher_is_better'] is True and line['dtype'] == 'f64'
    assert line['value'] > 0 and line['ms_per_step'] > 0 and abs(line['value'] - nb / (line['ms_per_step'] * 1e-3)) < 1e-6 * line['value']
    assert abs(line['roofline']['frac'] - line['roofline']['achieved'] / line['roofline']['peak']) < 1e-12
    assert not {'cpu_baseline', 'secondary', 'value_api', 'parity_spot_check_tilted_err', 'split_configs', 'gather_ms'} & set(line)
    s, xi = np.load(dump / 's.npy'), np.load(dump / 'xi.npy')
    idx = bench.dump_rows(nb)
    assert s.dtype == xi.dtype == np.float64 and s.shape == (bench.N_K,) and xi.shape == (bench.DUMP_ROWS, bench.N_K) == (idx.size, bench.N_K)
    k, pk = pk_eh_default(bench.N_K)
    t = ofl.power_to_correlation(k, ell=0)
    assert np.allclose(s, t.y[0], rtol=1e-14, atol=0.)
    rows = config2_rows(k, pk, 0, nb, seed=0, nbatch=nb)[idx]
    ref = ofl.apply(t, rows[:, None, :])[:, 0]
    w = t.y[0] ** 1.5
    assert np.abs((xi - ref) * w).max() / np.abs(ref * w).max() < 1e-12
