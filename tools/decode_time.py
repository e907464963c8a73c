#!/usr/bin/env python3
"""The box decode alone, HIP-event timed: python tools/decode_time.py  (B = 1 and 9, 900 x 10 scores, top 300)
  --shape Q,C,K   (repeatable) num_query, num_classes, max_num instead of 900,10,300
  --path P[,P]    the kernel: 0 the one the shape asks for, 1 keys in registers, 2 streaming; several: one after the other
  --rounds R      the whole sweep R times (an A/B of two paths alternates them); --calls N: calls per timed window"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transcar_amd import configs, ops                      # noqa: E402


def _shape(text):
    q, c, k = (int(v) for v in text.split(','))
    return q, c, k


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shape', type=_shape, action='append', metavar='Q,C,K')
    ap.add_argument('--path', type=lambda t: [int(v) for v in t.split(',')], default=[0], metavar='P[,P]')
    ap.add_argument('--rounds', type=int, default=1)
    ap.add_argument('--calls', type=int, default=200)
    args = ap.parse_args()
    assert all(p in (0, 1, 2) for p in args.path), args.path
    for _ in range(args.rounds):
        for Q, C, K in args.shape or [(900, 10, 300)]:
            for path in args.path:
                if args.shape or args.path != [0]:
                    print('%d x %d scores, top %d, path %d' % (Q, C, K, path))
                time_shape(Q, C, K, path, args.calls)


def time_shape(Q, C, K, path, n):
    dev = torch.device('cuda:0')
    rng = np.random.RandomState(3)
    pcr = configs.pts_bbox_head['bbox_coder']['post_center_range']
    for B in (1, 9):
        cls = torch.from_numpy(rng.standard_normal((B, Q, C)).astype(np.float32) - 2.0).to(dev)
        box = torch.from_numpy(rng.standard_normal((B, Q, 10)).astype(np.float32) * 0.3).to(dev)
        for _ in range(5):
            ops.box_decode_topk(cls, box, pcr, K, path=path)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            ops.box_decode_topk(cls, box, pcr, K, path=path)
        e1.record()
        torch.cuda.synchronize()
        print('B=%d: %.2f us per call (back to back, launch included)' % (B, e0.elapsed_time(e1) / n * 1e3))
        from transcar_amd import _lib as L
        dll = L.lib()
        if hasattr(dll, 'tc_debug_decode_stamps'):        # STAMPS=1 build: s_memtime per phase, workgroup 0 thread 0
            import ctypes
            buf = np.zeros(16, dtype=np.int64)
            dll.tc_debug_decode_stamps.argtypes = [ctypes.c_void_p]
            assert dll.tc_debug_decode_stamps(buf.ctypes.data) == 0
            names = ['entry', 'keys+zero', 'bucket hist', 'bucket chosen', 'filed', 'byte pass 1', 'byte pass 2', 'byte pass 3', 'byte pass 4',
                     'byte pass 5', 'byte pass 6', 'selected', 'compacted', 'ranked', 'written']
            print('  stamps (ticks since entry):', ', '.join('%s %d' % (nm, buf[i] - buf[0]) for i, nm in enumerate(names) if buf[i] >= buf[0] and buf[i] > 0))


if __name__ == '__main__':
    main()
