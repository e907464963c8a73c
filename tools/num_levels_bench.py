#!/usr/bin/env python3
"""What Detr3DCrossAtten.num_levels costs: frames/s of the bench's res101 head (seeded weights, configs.head_cfg() with
num_levels overridden) fed the FIRST L res101 levels, through the same FramePipeline measurement as bench.py's headline
(bench._pipeline_rate: its lanes, the resident frames per launch, whole launches per window), interleaved over L.
L = 4 is the headline configuration; L < 4 runs the generic chain kernels (DESIGN.md "num_levels < 4").
    python tools/num_levels_bench.py [--levels 4 3 2 1] [--rounds 3] [--steps 20]        (one JSON line)"""
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


def build_head(dev, num_levels):
    sd = synth.make_state_dict(seed=3, num_levels=num_levels)
    head = T.build_head(configs.head_cfg(num_levels=num_levels))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def shapes_of(num_levels):
    """a LEVEL_SHAPES key for the first num_levels res101 levels (bench.make_inputs looks the shapes up by name)"""
    if num_levels == 4:
        return 'res101'
    key = 'res101_first%d' % num_levels
    configs.LEVEL_SHAPES[key] = configs.LEVEL_SHAPES['res101'][:num_levels]
    return key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--levels', type=int, nargs='+', default=[4, 3, 2, 1])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {n: build_head(dev, n) for n in a.levels}
    fpl = bench.auto_frames_per_launch(heads[a.levels[0]], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {n: [] for n in a.levels}
    for _ in range(a.rounds):
        for n in a.levels:
            r, pipe, lanes = bench._pipeline_rate(heads[n], dev, args, shapes_of(n), fpl, None)
            rates[n].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'shapes': 'res101, first L levels', 'frames_per_launch': fpl, 'lanes': a.lanes,
           'rounds': a.rounds, 'rates': {str(n): rates[n] for n in a.levels},
           'median': {str(n): float(np.median(rates[n])) for n in a.levels}}
    base = res['median'][str(a.levels[0])]
    res['relative_to_first'] = {str(n): res['median'][str(n)] / base for n in a.levels}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
