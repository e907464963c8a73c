"""The benchmark's commands, end to end on the GPU (runs LAST: the file name sorts behind the parity tests):
`python bench.py --full --gpus 1 --steps 20 --warmup 5` prints exactly one JSON line with the contract's keys, the roofline
of the dominant kernel with its HBM-side traffic (measured in the run when rocprofv3 is there) and the CPU baseline;
the same command without --full prints the headline alone and spends at most 30 s outside its steps."""
import json
import os
import signal
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONTRACT = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
            'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline')


def test_the_drivers_bench_command_prints_one_complete_line():
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    p = subprocess.Popen([sys.executable, os.path.join(ROOT, 'bench.py'), '--full', '--gpus', '1', '--steps', '20', '--warmup', '5'],
                         cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=420)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)            # the process group started here (bench.py and its rocprofv3 passes)
        out, err = p.communicate()
        pytest.fail('bench.py did not finish within 420 s:\n' + (err or '')[-1500:])
    assert p.returncode == 0, err[-2000:]
    lines = [ln for ln in out.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out[-1000:]
    d = json.loads(lines[0])
    for k in CONTRACT:
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 20 and d['warmup'] == 5 and d['higher_is_better'] is True
    assert d['unit'] == 'frames/s' and d['value'] > 1000 and d['vs_baseline'] is None
    assert d['full'] is True
    # fp32 results: the linear steps of the batched launches take two-plane f16 operands on the matrix cores
    assert d['dtype'].startswith('f32') and 'f16x2' in d['dtype']
    assert abs(d['ms_per_step'] * d['value'] - 1e3) < 1.0                  # one frame per step
    assert 'configs[1]' in d['config']['workload'] and 'model' not in d['config']
    r = d['roofline']
    assert r['bound'] == 'mfma' and r['unit'] == 'TFLOP/s' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9
    # priced against the f16 matrix-core peak / 3 products (838.9 TFLOP/s); the f32-MFMA (vector pipe) figure beside it
    assert r['peak'] > 800 and 'peak_definition' in r and 0.05 < r['frac'] < 1.0 and r['frac_of_f32_mfma_peak'] > 0.5
    assert r['traffic'] and r['traffic'] > 1e8                              # ~200 MB per launch of nine frames
    # the plain-f32 path, configs[4] (VoVNet levels) and configs[2] (a training iteration) ride in the same line
    assert d['f32_path']['matrix_path'] == 'f32' and 1000 < d['f32_path']['value'] < d['value'] * 1.05
    assert 'configs[4]' in d['vovnet']['workload'] and d['vovnet']['value'] > 1000
    assert 'configs[2]' in d['train']['workload'] and 0.1 < d['train']['ms_per_iteration'] < 5.0
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['cores'] >= 1 and c['value'] > 0 and c['sample']


#: what a plain run leaves to --full: keys of the side measurements in the line
SIDE_KEYS = ('roofline', 'cpu_baseline', 'single_lane', 'latency_ms_per_frame', 'pipeline_latency_ms', 'dropin_forward',
             'with_input_delivery', 'end_to_end', 'with_handoff', 'frames_per_launch_sweep', 'f32_path', 'vovnet', 'train')
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')


def test_a_plain_run_prints_the_headline_alone_within_30_s_outside_its_steps():
    """`bench.py --gpus 1 --steps N --warmup W` without --full: set-up, warm-up, the N timed steps, the line -- none of
    the side measurements, and at most 30 s outside the steps: the whole run in a fresh process, from start to exit,
    less (N + W) x ms_per_step."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup',
                        str(warmup)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-1000:]
    d = json.loads(lines[0])
    for k in HEADLINE:
        assert k in d, k
    assert d['full'] is False and not [k for k in SIDE_KEYS if d.get(k) is not None]
    assert d['steps'] == steps and d['warmup'] == warmup and d['timing']['timed_steps'] == steps
    assert d['unit'] == 'frames/s' and d['value'] > 1000 and d['higher_is_better'] is True
    assert d['dtype'].startswith('f32') and 'f16x2' in d['dtype']
    assert abs(d['ms_per_step'] * d['value'] - 1e3) < 1.0                  # one frame per step
    outside = wall - (steps + warmup) * d['ms_per_step'] * 1e-3
    print('plain run: %.1f s in all, %.1f s outside its steps' % (wall, outside))
    assert outside <= 30.0, outside


def test_dump_outputs_of_the_last_timed_step_are_the_same_every_run(tmp_path):
    """`bench.py ... --dump-outputs DIR`: what the timed path's last step computed (the head's outputs and the decoded
    boxes of that step's frame) as float32 .npy files -- the same arrays in two runs with the same arguments, and the
    decode belongs to the same frame as the head outputs (its best score is the sigmoid of their largest logit)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '20', '--warmup', '5',
                            '--main-only', '--dump-outputs', str(d)], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=420)
        assert p.returncode == 0, p.stderr[-2000:]
        assert len([ln for ln in p.stdout.splitlines() if ln.startswith('{')]) == 1
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == ['all_bbox_preds', 'all_cls_scores', 'boxes', 'labels', 'scores', 'valid']
    layers = a['all_cls_scores'].shape[0]
    assert a['all_cls_scores'].shape == a['all_bbox_preds'].shape == (layers, 1, 900, 10)
    assert a['boxes'].shape == (1, 300, 9) and a['scores'].shape == a['labels'].shape == a['valid'].shape == (1, 300)
    assert sum(v.nbytes for v in a.values()) <= 64e6
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k
    best = 1.0 / (1.0 + np.exp(-a['all_cls_scores'][-1, 0].astype(np.float64).max()))
    assert abs(a['scores'][0, 0] - best) < 1e-5
