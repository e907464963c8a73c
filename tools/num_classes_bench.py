#!/usr/bin/env python3
"""What the second 16-column pass of the fusion layers' class head costs (DESIGN.md "Class counts above 16"): the radar
part of the head (tc_radar_fusion_fwd: encoders, row order, the three fusion layers in one chain launch) on the decoder
states of nine frames, res101 shapes, seeded weights, at 16, 23 and 32 classes -- one sub-tile against two.  Device
events around `--iters` back-to-back calls, the class counts interleaved over `--rounds` rounds, per tile height.
    python tools/num_classes_bench.py [--rounds 3] [--iters 200]
One JSON line, also written to profiles/num_classes_bench.json."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from transcar_amd import _lib as L  # noqa: E402
from transcar_amd import configs, synth  # noqa: E402
from transcar_amd import detr3d_head as D  # noqa: E402

CLASSES = (16, 23, 32)
TILES = {'auto': {}, 'f16x2-32': dict(tile_rows=32, matrix_path='f16x2'), 'f16x2-16': dict(tile_rows=16, matrix_path='f16x2')}
FRAMES = 9


def build(dev, ncls):
    """A head of `ncls` classes whose weights are those of the 32-class head, the last layer of every class branch cut to
    its first `ncls` rows: the decoder, the boxes, hence the radar gates' hits and the attention's work are the same at
    every class count (synth draws a state dict in one stream: heads of different counts differ in EVERY weight, and
    the fusion layers' time follows the hit counts)."""
    import re
    import transcar_amd as T
    sd = synth.make_state_dict(seed=3, num_classes=max(CLASSES))
    last = re.compile(r'^(cls_branches\.\d+|final_cls\d?)\.6\.(weight|bias)$')
    sd = {k: (v[:ncls].copy() if last.match(k) else v) for k, v in sd.items()}
    assert sum(1 for k in sd if last.match(k)) == 18
    head = T.build_head(configs.head_cfg(num_classes=ncls))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return head.to(dev).eval()


def radar_call(head, dev, tiles):
    """-> a closure that enqueues one tc_radar_fusion_fwd on the nine frames' decoder states, and what it keeps alive"""
    inp = bench.make_inputs(head, dev, 'res101', FRAMES, seed=3, host_feats=False)
    aux = head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'], aux=True,
                            decoder_only=True)['aux']
    pv = head._packed_view
    B, Q, T = FRAMES, head.num_query, inp['tokens'].shape[1]
    hs, ref, box = aux['inter_states'][-1].contiguous(), aux['inter_references'][-1].contiguous(), aux['last_box']
    ws = torch.empty(L.lib().tc_head_workspace_bytes(C.byref(pv), B, T), dtype=torch.uint8, device=dev)
    cls = torch.empty((3, B, Q, head.cls_out_channels), dtype=torch.float32, device=dev)
    out = torch.empty((3, B, Q, head.code_size), dtype=torch.float32, device=dev)
    hits = torch.empty((3, B, Q), dtype=torch.int32, device=dev)
    calls = {}
    for name, kw in tiles.items():
        opt = D.head_options(**kw)
        args = (C.byref(pv), hs.data_ptr(), ref.data_ptr(), box.data_ptr(), inp['tokens'].data_ptr(), B, T,
                int(inp['pad_mult']), 0, 3, cls.data_ptr(), out.data_ptr(), hits.data_ptr(), C.byref(opt), ws.data_ptr(),
                ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        calls[name] = (args, opt)
    return calls, (head, inp, aux, hs, ref, box, ws, cls, out, hits, pv)      # (the view points into the head's parameters)


def timed(args, iters):
    fwd = L.lib().tc_radar_fusion_fwd
    for _ in range(10):
        L.check(fwd(*args), 'tc_radar_fusion_fwd')
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
    ap.add_argument('--iters', type=int, default=200)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    dev = torch.device('cuda:0')
    rigs = {n: radar_call(build(dev, n), dev, TILES) for n in CLASSES}
    us = {t: {str(n): [] for n in CLASSES} for t in TILES}
    for _ in range(a.rounds):
        for t in TILES:
            for n in CLASSES:
                us[t][str(n)].append(timed(rigs[n][0][t][0], a.iters))
    med = {t: {n: float(np.median(v)) for n, v in d.items()} for t, d in us.items()}
    res = {'metric': 'microseconds per tc_radar_fusion_fwd, nine frames', 'shapes': 'res101', 'frames': FRAMES,
           'radar_us': us, 'radar_us_median': med,
           'second_pass_us': {t: {'23_minus_16': m['23'] - m['16'], '32_minus_16': m['32'] - m['16']} for t, m in med.items()},
           'rounds': a.rounds, 'iters': a.iters}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    with open(os.path.join(ROOT, 'profiles', 'num_classes_bench.json'), 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
