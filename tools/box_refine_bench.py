#!/usr/bin/env python3
"""What box refinement costs the decoder: frames/s of the bench's res101 head (configs.head_cfg() with with_box_refine
overridden, synth.make_state_dict(with_box_refine=False)'s shared branches in both heads) through the same FramePipeline
measurement as bench.py's headline (bench._pipeline_rate), interleaved refine / no refine.
    python tools/box_refine_bench.py [--rounds 3] [--steps 20]        (one JSON line)"""
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


def build_head(dev, refine):
    sd = synth.make_state_dict(seed=3, with_box_refine=False)
    head = T.build_head(configs.head_cfg(with_box_refine=refine))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    modes = ('refine', 'norefine')
    heads = {m: build_head(dev, m == 'refine') for m in modes}
    fpl = bench.auto_frames_per_launch(heads['refine'], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            r, pipe, lanes = bench._pipeline_rate(heads[m], dev, args, 'res101', fpl, None)
            rates[m].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'shapes': 'res101', 'frames_per_launch': fpl, 'lanes': a.lanes,
           'rounds': a.rounds, 'rates': rates, 'median': {m: float(np.median(rates[m])) for m in modes}}
    res['norefine_over_refine'] = res['median']['norefine'] / res['median']['refine']
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
