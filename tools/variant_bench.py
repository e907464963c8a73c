#!/usr/bin/env python3
"""What one keyword of the head's configuration costs: frames/s of the bench's res101 head (seeded weights,
configs.head_cfg() with that keyword overridden) through the same FramePipeline measurement as bench.py's headline
(bench._pipeline_rate: its lanes, the resident frames per launch, whole launches per window), interleaved over the
values.  The first value is the base of `relative_to_first`.
    python tools/variant_bench.py --vary num_points 1 5 [--rounds 3] [--steps 20]        (one JSON line)
    python tools/variant_bench.py --vary num_levels 4 3 2 1
    python tools/variant_bench.py --vary num_heads 8 4 16
    python tools/variant_bench.py --vary radar_num_heads 8 4 16
    python tools/variant_bench.py --vary with_box_refine 1 0

num_points       Detr3DCrossAtten.num_points (DESIGN.md "num_points").
num_levels       the head is fed the FIRST L res101 levels; L = 4 is the headline configuration, L < 4 runs the generic
                 chain kernels (DESIGN.md "num_levels < 4").
num_heads        the decoder self-attention's head count: 8 is the headline (head dimension 32); 4 and 16 run the
                 attention cores' D = 64 and D = 16 instantiations.  The state dict does not depend on it.
radar_num_heads  the radar fusion attention's head count (8 is the headline): the same kernels with 16 / 8 / 4 lanes per
                 head.  The state dict does not depend on it either.
with_box_refine  both heads carry synth.make_state_dict(with_box_refine=False)'s shared branches; the results are keyed
                 'refine' / 'norefine' and `norefine_over_refine` is reported, as profiles/box_refine_bench.json has it."""
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

KEYWORDS = ('num_points', 'num_levels', 'num_heads', 'radar_num_heads', 'with_box_refine')


def build_head(dev, keyword, value):
    sd_kw = {'num_heads': {}, 'radar_num_heads': {}, 'with_box_refine': dict(with_box_refine=False)}.get(keyword, {keyword: value})
    head = T.build_head(configs.head_cfg(**{keyword: bool(value) if keyword == 'with_box_refine' else value}))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=3, **sd_kw).items()}, strict=True)
    return head.to(dev).eval()


def shapes_of(keyword, value):
    """a LEVEL_SHAPES key: res101, or its first num_levels levels (bench.make_inputs looks the shapes up by name)"""
    if keyword != 'num_levels' or value == 4:
        return 'res101'
    key = 'res101_first%d' % value
    configs.LEVEL_SHAPES[key] = configs.LEVEL_SHAPES['res101'][:value]
    return key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vary', nargs='+', required=True, metavar=('KEYWORD', 'VALUE'))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    keyword, values = a.vary[0], [int(v) for v in a.vary[1:]]
    if keyword not in KEYWORDS or not values:
        ap.error('--vary takes one of %s and at least one value' % ', '.join(KEYWORDS))
    refine = keyword == 'with_box_refine'
    label = {v: (('norefine', 'refine')[bool(v)] if refine else str(v)) for v in values}
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {v: build_head(dev, keyword, v) for v in values}
    fpl = bench.auto_frames_per_launch(heads[values[0]], dev)
    args = types.SimpleNamespace(lanes=a.lanes, warmup_s=0.5, steps=a.steps)
    rates = {v: [] for v in values}
    for _ in range(a.rounds):
        for v in values:
            r, pipe, lanes = bench._pipeline_rate(heads[v], dev, args, shapes_of(keyword, v), fpl, None)
            rates[v].append(r)
            del pipe, lanes
            torch.cuda.synchronize()
    res = {'metric': 'frames_per_s', 'vary': keyword,
           'shapes': 'res101, first L levels' if keyword == 'num_levels' else 'res101', 'frames_per_launch': fpl,
           'lanes': a.lanes, 'rounds': a.rounds, 'rates': {label[v]: rates[v] for v in values},
           'median': {label[v]: float(np.median(rates[v])) for v in values}}
    base = res['median'][label[values[0]]]
    res['relative_to_first'] = {label[v]: res['median'][label[v]] / base for v in values}
    if refine and set(label.values()) == {'refine', 'norefine'}:
        res['norefine_over_refine'] = res['median']['norefine'] / res['median']['refine']
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
