#!/usr/bin/env python3
"""What the depth of the radar fusion stack costs (Detr3DHead(num_fusion_layers=N), DESIGN.md "Fusion depth"), bench.py's
default geometry (res101 shapes, 900 queries, 255 radar points), seeded weights -- the N-layer head carries the first N
layers of the three-layer head's weights:
  * frames/s of a FramePipeline of three lanes, nine frames per launch (bench.py's default line), for N = 1, 2, 3;
  * ms of one training iteration (bench.py's train side run: the fused path with the decoder look-ahead) for each.
The depths are interleaved over `--rounds` rounds; the medians are reported beside every round's value.
    python tools/fusion_depth_bench.py [--rounds 3] [--skip-train]
One JSON line, also written to profiles/fusion_depth_bench.json."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

DEPTHS = (1, 2, 3)


def build_head(dev, depth, train=False):
    from transcar_amd import configs, synth
    import transcar_amd as T
    cfg = configs.head_cfg(num_fusion_layers=depth)
    if train:
        cfg['train_cfg'] = configs.train_cfg_pts
    head = T.build_head(cfg)
    sd = synth.make_state_dict(seed=3, num_fusion_layers=depth)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def inference_rate(head, dev, args):
    from transcar_amd.detr3d_head import head_options
    rate, pipe, lanes = bench._pipeline_rate(head, dev, args, args.shapes, args.frames, head_options())
    del pipe, lanes
    torch.cuda.empty_cache()
    return rate


class Trainer:
    """bench.train_side_run's loop for a head of any depth, kept alive across the rounds."""

    def __init__(self, head, dev, depth, args):
        from transcar_amd import synth
        from transcar_amd.trainer import FusionTrainer
        self.P = args.frames
        self.thead = build_head(dev, depth, train=True)
        boxes, labels = synth.make_gt(seed=7, n=24)
        gt = torch.from_numpy(boxes).clone()
        gt[:, 2] += gt[:, 5] * 0.5
        self.gts, self.lbs = [gt.to(dev)], [torch.from_numpy(labels).to(dev)]
        with torch.enable_grad():
            self.tr = FusionTrainer(self.thead, prefetch_depth=self.P)
        self.loader = bench.LookAheadFrames(head, dev, args.shapes, self.P, 1, seed=3)

    def step(self):
        f = self.loader.next()
        self.tr.step_fused_nhwc(f['nhwc'], f['l2i'], f['hw'], f['tokens'], f['pad_mult'], self.gts, self.lbs,
                                prefetch=self.loader.prefetch)

    def ms_per_iteration(self):
        with torch.enable_grad():
            for _ in range(2 * self.P):
                self.step()
            torch.cuda.synchronize()
            return bench._replay_rate(self.step, torch.cuda.synchronize, 6 * self.P, min_s=0.8) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--frames', type=int, default=9, help='frames per launch (bench.py: --pair, automatic = 9)')
    ap.add_argument('--shapes', default='res101')
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup-s', dest='warmup_s', type=float, default=0.5)
    ap.add_argument('--skip-train', action='store_true')
    a = ap.parse_args()
    bench._imports()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {n: build_head(dev, n) for n in DEPTHS}
    res = {'metric': 'frames/s of FramePipeline(%d lanes x %d frames per launch); ms per training iteration' % (a.lanes, a.frames),
           'shapes': a.shapes, 'rounds': a.rounds, 'frames_per_s': {n: [] for n in DEPTHS}, 'train_ms': {n: [] for n in DEPTHS}}
    trainers = {} if a.skip_train else {n: Trainer(heads[n], dev, n, a) for n in DEPTHS}
    for _ in range(a.rounds):
        for n in DEPTHS:
            res['frames_per_s'][n].append(inference_rate(heads[n], dev, a))
        for n, t in trainers.items():
            res['train_ms'][n].append(t.ms_per_iteration())
    res['frames_per_s_median'] = {n: float(np.median(v)) for n, v in res['frames_per_s'].items()}
    res['train_ms_median'] = {n: float(np.median(v)) for n, v in res['train_ms'].items() if v}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'fusion_depth_bench.json'), 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
