#!/usr/bin/env python3
"""The Hungarian assignment alone, device route against the host route it replaces: python tools/lsa_time.py
  device: tc_lsa_assign_ws (transposing pre-pass + solve where the shape needs them), HIP events around back-to-back calls
  host:   cost.cpu() + scipy.optimize.linear_sum_assignment per (output, sample) + the upload of the result, wall clock
  --shape Q,G     (repeatable) instead of 900,24 (the small kernel: the anchor) 900,129 900,300 1300,150 4096,512
  --calls N       device calls per timed window (host: N // 4, at least 3)
  --train-tree LABEL=DIR     (repeatable, in run order; a label may repeat) runs `bench.py --train` of the checkout DIR
                  in a child process before anything else and records its ms per iteration with the command: the same
                  session's comparison of this commit with its parent, e.g.
                  --train-tree parent@<rev>=../parent --train-tree this@<rev>=. --train-tree parent@<rev>=../parent
  --out FILE      the JSON record (default profiles/lsa_large_bench.json)
3 outputs, B = 1, structured costs (a few cheap queries per box).  Not a gate: the device route is chosen for the
absence of a host synchronisation, not for its latency."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transcar_amd import _lib as L                         # noqa: E402

LYR, B = 3, 1
SHAPES = [(900, 24), (900, 129), (900, 300), (1300, 150), (4096, 512)]


def _shape(text):
    q, g = (int(v) for v in text.split(','))
    return q, g


TRAIN_CMD = ['bench.py', '--gpus', '1', '--train', '--steps', '400', '--warmup', '40', '--no-roofline', '--main-only']


def _train_tree(text):
    label, tree = text.split('=', 1)
    return label, os.path.abspath(tree)


def train_ms(tree):
    """ms per training iteration (`ms_per_step` of bench.py --train's line) of the checkout `tree`, in a child process"""
    out = subprocess.run([sys.executable] + TRAIN_CMD, cwd=tree, check=True, stdout=subprocess.PIPE, timeout=170).stdout
    line = [l for l in out.decode().splitlines() if l.startswith('{')][-1]
    return float(json.loads(line)['ms_per_step'])


def make_costs(Q, G):
    rng = np.random.RandomState(Q * 131 + G)
    cost = rng.rand(LYR, B, Q, G).astype(np.float32) * 4.0
    for g in range(G):
        cost[:, :, (7 * g) % Q, g] *= 0.05
        cost[1, :, (7 * g + 3) % Q, g] *= 0.02
    return cost


def host_route(cost_d, G):
    cost_h = cost_d.cpu().numpy()
    assigned = np.full(cost_h.shape[:3], -1, dtype=np.int32)
    for l in range(LYR):
        for b in range(B):
            rows, cols = linear_sum_assignment(cost_h[l, b, :, :G])
            assigned[l, b, rows] = cols
    up = torch.from_numpy(assigned).to(cost_d.device)
    torch.cuda.synchronize()
    return up


def time_shape(Q, G, n):
    dev = torch.device('cuda:0')
    lib = L.lib()
    cost = torch.from_numpy(make_costs(Q, G)).to(dev)
    counts = torch.full((B,), G, dtype=torch.int32, device=dev)
    asg = torch.empty((LYR, B, Q), dtype=torch.int32, device=dev)
    z = torch.zeros(4 * LYR + 1, dtype=torch.float32, device=dev)
    need = lib.tc_lsa_workspace_bytes(LYR, B, Q, G)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def device_route():
        L.check(lib.tc_lsa_assign_ws(cost.data_ptr(), counts.data_ptr(), LYR, B, Q, G, asg.data_ptr(), z.data_ptr(),
                                     z[4 * LYR:].data_ptr(), z[2 * LYR:].data_ptr(), ws.data_ptr(), need, L.TC_LSA_AUTO,
                                     st), 'tc_lsa_assign_ws')
    for _ in range(3):
        device_route()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        device_route()
    e1.record()
    torch.cuda.synchronize()
    dev_us = e0.elapsed_time(e1) / n * 1e3
    want = host_route(cost, G)
    assert int(z[4 * LYR:].view(torch.int32).item()) == 0 and torch.equal(asg, want), 'device and scipy disagree'
    m = max(3, n // 4)
    t0 = time.perf_counter()
    for _ in range(m):
        host_route(cost, G)
    host_us = (time.perf_counter() - t0) / m * 1e6
    kernel = 'large (transposed workspace, %d bytes)' % need if need else 'small (costs in LDS or strided)'
    print('Q=%d G=%d [%s]: device %.1f us, host round trip %.1f us' % (Q, G, kernel, dev_us, host_us))
    return {'Q': Q, 'G': G, 'outputs': LYR, 'B': B, 'kernel': 'large' if need else 'small', 'workspace_bytes': need,
            'device_us': dev_us, 'host_us': host_us, 'device_over_host': dev_us / host_us}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shape', type=_shape, action='append', metavar='Q,G')
    ap.add_argument('--calls', type=int, default=40)
    ap.add_argument('--train-tree', type=_train_tree, action='append', default=[], metavar='LABEL=DIR')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lsa_large_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/lsa_time.py times the GPU'
    runs = []
    for label, tree in args.train_tree:                # (before this process opens the GPU: one user at a time)
        runs.append({'label': label, 'ms_per_iteration': train_ms(tree)})
        print('bench.py --train [%s]: %.4f ms per iteration' % (label, runs[-1]['ms_per_iteration']))
    if not runs:
        print('WARNING: no --train-tree: the record lacks the bench.py --train comparison with the parent commit',
              file=sys.stderr)
    rec = {'what': 'Hungarian assignment, 3 outputs x 1 sample: tc_lsa_assign_ws (events, back-to-back calls) against '
                   'D2H + scipy per problem + H2D (wall clock); 256 threads x 16 columns per problem on the large '
                   'kernel (the 1024-thread x 4-column split was not built)',
           'device': torch.cuda.get_device_name(0),
           'shapes': [time_shape(Q, G, args.calls) for Q, G in args.shape or SHAPES]}
    rec['bench_train'] = {'command': 'python ' + ' '.join(TRAIN_CMD) + '  (ms_per_step of its line; one child process '
                                     'per run, in this order, before the shapes above)', 'runs': runs} if runs else None
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print('wrote %s' % args.out)


if __name__ == '__main__':
    main()
