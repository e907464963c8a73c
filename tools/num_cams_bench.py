#!/usr/bin/env python3
"""What a camera count costs: frames/s of the res101 head built with Detr3DCrossAtten(num_cams=N) (seeded weights) on a
ring rig of N cameras (synth.ring_yaws), through the FramePipeline measurement of bench.py's headline
(bench._pipeline_rate's lanes, warm-up and timing window; tools/variant_bench.py does not take the key, bench.make_inputs
draws the configs' six cameras), interleaved over the counts, with the visible (query, camera) pairs per frame -- the
sampling step's cost scales with those.  Up to 8 cameras run the fixed-level kernels (and, with one lane, the camera
pre-gather); more cameras the generic ones.
    python tools/num_cams_bench.py 6 9 12 16 [--rounds 3] [--steps 20] [--lanes 3]        (one JSON line)"""
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
import transcar_amd as T  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402


def build_head(dev, N):
    head = T.build_head(configs.head_cfg(num_cams=N))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=3, num_cams=N).items()}, strict=True)
    return head.to(dev).eval()


def lane(head, dev, N, fpl, seed):
    """bench.make_inputs(host_feats=False) on N cameras: iid N(0,1) res101 maps drawn on the device, the ring rig's
    lidar2img, radar points near the boxes a first pass predicts.  -> (lane inputs, visible pairs per frame)"""
    from transcar_amd import radar as R
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + seed)
    nhwc = [torch.randn((fpl * N, h, w, 256), device=dev, generator=g) for (h, w) in configs.LEVEL_SHAPES['res101']]
    l2i_np = synth.make_lidar2img(yaws_deg=synth.ring_yaws(N))
    l2i = torch.from_numpy(np.stack([l2i_np] * fpl).astype(np.float32)).to(dev)
    hw = configs.IMG_SHAPE[:2]
    tok0, pm0 = R.pack_tokens([R.build_radar_features(synth.make_radar_frame(seed=2 + b)) for b in range(fpl)])
    o = head.forward_nhwc(nhwc, l2i, hw, torch.from_numpy(tok0).to(dev), pm0, aux=True)
    r = o['aux']['inter_references'][-1].cpu().numpy().astype(np.float64)
    pcr, fl = configs.point_cloud_range, []
    for b in range(fpl):
        c = np.round(np.stack([r[b, :, 0] * (pcr[3] - pcr[0]) + pcr[0], r[b, :, 1] * (pcr[4] - pcr[1]) + pcr[1]], 1), 2)
        fl.append(R.build_radar_features(synth.make_radar_frame(seed=2 + b, centres=c)))
    tok, pm = R.pack_tokens(fl)
    inp = dict(feats_np=None, nhwc=nhwc, l2i=l2i, l2i_np=l2i_np, hw=hw, tokens=torch.from_numpy(tok).to(dev), pad_mult=pm,
               radar_feats=fl)
    return inp, int(o['aux']['sample_pairs'].item()) / fpl


def rate(head, dev, N, fpl, a):
    """bench._pipeline_rate on the N-camera lanes"""
    from transcar_amd.pipeline import FramePipeline
    built = [lane(head, dev, N, fpl, 41 + 5 * i) for i in range(max(1, a.lanes))]
    pipe = FramePipeline(head, [b[0] for b in built])
    step = (lambda: pipe.launch()) if fpl == 1 else pipe.submit

    def sync():
        if fpl > 1:
            pipe.flush()
        torch.cuda.synchronize()
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:
        for _ in range(fpl * pipe.lanes):
            step()
        sync()
    rounds = max(2, -(-max(20, a.steps) // (fpl * pipe.lanes)))
    t = bench._replay_rate(step, sync, rounds * fpl * pipe.lanes, min_s=0.6)
    pairs = float(np.mean([b[1] for b in built]))
    del pipe, built
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return 1.0 / t, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('counts', type=int, nargs='+')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--lanes', type=int, default=3)
    a = ap.parse_args()
    bench._imports()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    heads = {N: build_head(dev, N) for N in a.counts}
    fpl = bench.auto_frames_per_launch(heads[a.counts[0]], dev)
    rates, pairs = {N: [] for N in a.counts}, {}
    for _ in range(a.rounds):
        for N in a.counts:
            r, pairs[N] = rate(heads[N], dev, N, fpl, a)
            rates[N].append(r)
    res = {'metric': 'frames_per_s', 'vary': 'num_cams', 'shapes': 'res101', 'rig': 'synth.ring_yaws(N)', 'frames_per_launch': fpl,
           'lanes': a.lanes, 'rounds': a.rounds, 'rates': {str(N): rates[N] for N in a.counts},
           'median': {str(N): float(np.median(rates[N])) for N in a.counts},
           'visible_pairs_per_frame': {str(N): pairs[N] for N in a.counts},
           'kernels': {str(N): 'fixed-level' if N <= 8 else 'generic' for N in a.counts}}
    base = res['median'][str(a.counts[0])]
    res['relative_to_first'] = {str(N): res['median'][str(N)] / base for N in a.counts}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
