#!/usr/bin/env python3
"""What the decoder self-attention's head count costs: frames/s of the bench's res101 head (seeded weights,
configs.head_cfg() with attn_cfgs[0].num_heads overridden) through the same FramePipeline measurement as bench.py's
headline (bench._pipeline_rate: its lanes, the resident frames per launch, whole launches per window), interleaved over
H.  H = 8 is the headline configuration (head dimension 32); 4 and 16 run the attention cores' D = 64 and D = 16
instantiations (DESIGN.md "Decoder self-attention with 4 or 16 heads").
    python tools/num_heads_bench.py [--heads 8 4 16] [--rounds 3] [--steps 20]        (one JSON line)"""
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


def build_head(dev, num_heads):
    sd = synth.make_state_dict(seed=3)                # (the state dict does not depend on the head count)
    head = T.build_head(configs.head_cfg(num_heads=num_heads))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--heads', type=int, nargs='+', default=[8, 4, 16])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {n: build_head(dev, n) for n in a.heads}
    fpl = bench.auto_frames_per_launch(heads[a.heads[0]], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {n: [] for n in a.heads}
    for _ in range(a.rounds):
        for n in a.heads:
            r, pipe, lanes = bench._pipeline_rate(heads[n], dev, args, 'res101', fpl, None)
            rates[n].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'shapes': 'res101', 'frames_per_launch': fpl, 'lanes': a.lanes,
           'rounds': a.rounds, 'rates': {str(n): rates[n] for n in a.heads},
           'median': {str(n): float(np.median(rates[n])) for n in a.heads}}
    base = res['median'][str(a.heads[0])]
    res['relative_to_first'] = {str(n): res['median'][str(n)] / base for n in a.heads}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
