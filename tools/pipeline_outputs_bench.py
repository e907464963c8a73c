#!/usr/bin/env python3
"""Frames/s of a FramePipeline in each output mode (DESIGN.md "Pipeline outputs"), res101 shapes, seeded weights, nine
frames per launch, three lanes -- the bench's headline geometry:
  * the default pipeline (outputs='fusion');
  * outputs='camera' with the heads of every decoder level, and with decoder_levels='last';
  * outputs='all';
  * for scale, the eager outputs='camera' call one frame at a time (plugin graphs off), and the same call replayed from
    the plugin entry's graph.
The four pipelines share lanes (static inputs) and streams and are timed in alternation over `--rounds` rounds, a host
clock around `--window` seconds of whole launches that end in a device synchronise; the figures are medians.
    python tools/pipeline_outputs_bench.py [--rounds 5] [--window 0.5] [--lanes 3] [--frames 9]
One JSON line, also written to profiles/pipeline_outputs_bench.json."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402
from transcar_amd.detr3d_head import head_options  # noqa: E402
from transcar_amd.pipeline import FramePipeline  # noqa: E402

#: name -> (Detr3DHead.outputs, decoder_levels)
PIPELINES = {'fusion': ('fusion', 'all'), 'camera': ('camera', 'all'), 'camera_last': ('camera', 'last'), 'all': ('all', 'all')}


def window_rate(head, pipe, seconds):
    """frames/s over whole launches of every lane for at least `seconds`"""
    head.outputs = pipe.mode
    per_round = pipe.frames_per_launch * pipe.lanes
    torch.cuda.synchronize()
    frames, t0 = 0, time.perf_counter()
    while True:
        for _ in range(4 * per_round):
            pipe.submit()
        frames += 4 * per_round
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return frames / dt


def eager_ms(head, feats, metas, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        head(feats, metas)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.5)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--frames', type=int, default=9)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--shapes', default='res101')
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    head, _ = bench.build_head(dev)
    lanes = [bench.make_inputs(head, dev, a.shapes, a.frames, seed=41 + 5 * i, host_feats=False) for i in range(a.lanes)]
    pipes, streams = {}, None
    rates = {name: [] for name in PIPELINES}
    eager = {'eager': [], 'plugin_graph': []}
    try:
        for name, (mode, levels) in PIPELINES.items():
            head.outputs = mode
            kw = {} if mode == 'fusion' else dict(outputs=mode, decoder_levels=levels)
            pipes[name] = FramePipeline(head, lanes, streams=streams, options=head_options(), **kw)
            streams = pipes[name].streams
            window_rate(head, pipes[name], 0.3)                   # warm-up: code objects, allocator
        g = torch.Generator(device=dev)
        g.manual_seed(5)
        feats = [torch.randn((1, 6, 256, h, w), device=dev, generator=g) for (h, w) in configs.LEVEL_SHAPES[a.shapes]]
        metas = synth.make_img_metas(1, synth.make_lidar2img())
        head.outputs = 'camera'
        for graphs in (False, True):
            head.plugin_graphs = graphs
            eager_ms(head, feats, metas, 10)
        for _ in range(a.rounds):
            for name in PIPELINES:
                rates[name].append(window_rate(head, pipes[name], a.window))
            head.outputs = 'camera'
            for graphs, key in ((False, 'eager'), (True, 'plugin_graph')):
                head.plugin_graphs = graphs
                eager[key].append(eager_ms(head, feats, metas, a.steps))
    finally:
        head.outputs, head.plugin_graphs = 'fusion', True
    med = {name: float(np.median(v)) for name, v in rates.items()}
    res = {'metric': 'frames_per_s', 'shapes': a.shapes, 'lanes': a.lanes, 'frames_per_launch': a.frames,
           'rounds': a.rounds, 'window_s': a.window,
           'tile_rows': {name: p.tile_rows_of() for name, p in pipes.items()},
           'frames_per_s': rates, 'frames_per_s_median': med,
           'relative_to_fusion': {name: med[name] / med['fusion'] for name in med},
           'camera_one_frame_ms': eager,
           'camera_one_frame_ms_median': {k: float(np.median(v)) for k, v in eager.items()}}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'pipeline_outputs_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
