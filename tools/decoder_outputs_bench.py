#!/usr/bin/env python3
"""What the decoder levels' own outputs cost (Detr3DHead.outputs, DESIGN.md "Decoder heads"), res101 shapes, seeded
weights:
  * the new launch alone (tc_decoder_outputs_fwd on kept decoder states) for one and for nine frames, device events
    around `--iters` back-to-back launches;
  * a frame through the eager plugin entry `head(mlvl_feats, img_metas)` (plugin graphs off) with outputs =
    'camera', 'all' and 'fusion', interleaved over `--rounds` rounds, host clock around `--steps` forwards that end in a
    device synchronise.
    python tools/decoder_outputs_bench.py [--rounds 3] [--steps 30] [--iters 200]
One JSON line, also written to profiles/decoder_outputs_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from transcar_amd import _lib as L  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402
from transcar_amd import detr3d_head as D  # noqa: E402

MODES = ('camera', 'all', 'fusion')


def launch_us(head, dev, B, iters):
    inp = bench.make_inputs(head, dev, 'res101', B, seed=3, host_feats=False)
    aux = head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], aux=True,
                            decoder_only=True)['aux']
    cls, box = head.decoder_outputs(aux)
    # the C entry itself in the timed loop: no allocation, no struct building on the host between the launches
    view, opt = head.decoder_heads(), D.head_options()
    opt.range_status = head.status_buffer(dev).data_ptr()
    args = (C.byref(view), aux['inter_states'].data_ptr(), aux['init_reference'].data_ptr(),
            aux['inter_references'].data_ptr(), B, head.num_query, cls.data_ptr(), box.data_ptr(), C.byref(opt),
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    fwd = L.lib().tc_decoder_outputs_fwd
    for _ in range(10):
        L.check(fwd(*args), 'tc_decoder_outputs_fwd')
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fwd(*args)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    head, _ = bench.build_head(dev)
    head.plugin_graphs = False
    res = {'metric': 'microseconds', 'shapes': 'res101',
           'launch_us': {str(B): launch_us(head, dev, B, a.iters) for B in (1, 9)}}
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    feats = [torch.randn((1, 6, 256, h, w), device=dev, generator=g) for (h, w) in configs.LEVEL_SHAPES['res101']]
    l2i = synth.make_lidar2img()
    metas = {True: synth.make_img_metas(1, l2i, radar=synth.make_radar_frame(seed=2, n_per_radar=51)),
             False: synth.make_img_metas(1, l2i)}
    frame_us = {m: [] for m in MODES}
    try:
        for m in MODES:                                   # warm-up: packing, workspaces, code objects
            head.outputs = m
            for _ in range(5):
                head(feats, metas[m != 'camera'])
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for m in MODES:
                head.outputs = m
                torch.cuda.synchronize()
                t = time.perf_counter()
                for _ in range(a.steps):
                    head(feats, metas[m != 'camera'])
                torch.cuda.synchronize()
                frame_us[m].append((time.perf_counter() - t) * 1e6 / a.steps)
    finally:
        head.outputs = 'fusion'
    res['frame_us'] = frame_us
    res['frame_us_median'] = {m: float(np.median(v)) for m, v in frame_us.items()}
    res['all_minus_fusion_us'] = res['frame_us_median']['all'] - res['frame_us_median']['fusion']
    res['rounds'], res['steps'], res['iters'] = a.rounds, a.steps, a.iters
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'decoder_outputs_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
