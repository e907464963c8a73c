#!/usr/bin/env python3
"""What Detr3DCrossAtten.num_points costs: frames/s of the bench's res101 head (bench.build_head's seeded weights,
configs.head_cfg() with num_points overridden) through the same FramePipeline measurement as bench.py's headline
(bench._pipeline_rate: its lanes, the resident frames per launch, whole launches per window), interleaved P = 1 / P.
    python tools/num_points_bench.py [--points 1 5] [--rounds 3] [--steps 20]        (one JSON line)"""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import transcar_amd as T  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402


def build_head(dev, num_points):
    sd = synth.make_state_dict(seed=3, num_points=num_points)
    head = T.build_head(configs.head_cfg(num_points=num_points))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, nargs='+', default=[1, 5])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {p: build_head(dev, p) for p in a.points}
    fpl = bench.auto_frames_per_launch(heads[a.points[0]], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {p: [] for p in a.points}
    for _ in range(a.rounds):
        for p in a.points:
            r, pipe, lanes = bench._pipeline_rate(heads[p], dev, args, 'res101', fpl, None)
            rates[p].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'shapes': 'res101', 'frames_per_launch': fpl, 'lanes': a.lanes,
           'rounds': a.rounds, 'rates': {str(p): rates[p] for p in a.points},
           'median': {str(p): float(np.median(rates[p])) for p in a.points}}
    base = res['median'][str(a.points[0])]
    res['relative_to_first'] = {str(p): res['median'][str(p)] / base for p in a.points}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
