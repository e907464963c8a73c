#!/usr/bin/env python3
"""Fixtures of Detr3DHead(with_box_refine=False), from the REFERENCE's own code (oracle/ref_harness.py), as
make_golden_points.py makes the num_points > 1 ones.  Run only in the authoring container:
    python tests/golden/make_golden_norefine.py

Without box refinement the head shares one cls and one reg branch across the decoder layers (HEAD:223-231) and hands
the decoder reg_branches=None (HEAD:271).  The weights are synth.make_state_dict(with_box_refine=False): the seeded
branch .0 under every index, which is what such a head's state_dict holds.  Written:
  g5_head_{tiny,res101}_norefine.npz   Detr3DHead.forward (G5's rig: two passes, radar near the pass-1 centres)
  g5_head_tiny_p5_norefine.npz         ... at num_points 5
  g8_train_grads_norefine.npz          one training iteration's gradients, tiny shapes (G8's rig)
  g9_norefine_state_dict.json          the reference head's state_dict keys and shapes"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_golden as MG                                 # noqa: E402
from oracle import ref_harness as RH                     # noqa: E402
from transcar_amd import configs, synth                  # noqa: E402


def ref_head(num_points=None, train=False):
    head = RH.build_reference_head(configs.head_cfg(num_points=num_points, with_box_refine=False),
                                   configs.train_cfg_pts if train else None)
    assert not head.with_box_refine
    assert head.reg_branches[0] is head.reg_branches[5] and head.cls_branches[0] is head.cls_branches[5]
    sd = synth.make_state_dict(seed=3, num_points=num_points or 1, with_box_refine=False)
    ref_keys = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert ref_keys == {k: tuple(v.shape) for k, v in sd.items()}
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    head.eval()
    return head


def g9_state_dict(head):
    keys = {k: list(v.shape) for k, v in head.state_dict().items()}
    path = os.path.join(HERE, 'g9_norefine_state_dict.json')
    with open(path, 'w') as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote g9_norefine_state_dict.json (%d keys)' % len(keys))


def g8_train_grads():
    """make_golden.g8_train_grads without box refinement (tiny shapes)."""
    head = ref_head(train=True)
    MG.freeze_like_train_py(head)
    g5 = np.load(os.path.join(HERE, 'g5_head_tiny_norefine.npz'))
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    with torch.enable_grad():
        outs, cap, _ = MG.run_head(head, feats, l2i, frame)
        d = np.abs(outs['all_cls_scores'].detach().numpy() - g5['all_cls_scores']).max()
        assert d < 5e-4, d
        losses = head.loss([RH.GtBoxes(torch.from_numpy(boxes))], [torch.from_numpy(labels)], outs)
        total = sum(v for k, v in losses.items() if 'loss' in k)
        total.backward()
    out = {'total_loss': float(total),
           'all_cls_scores': outs['all_cls_scores'].detach().numpy(),
           'all_bbox_preds': outs['all_bbox_preds'].detach().numpy(),
           'Lq': np.array([cap['Lq%d' % i] for i in range(3)])}
    out.update({'loss__' + k.replace('.', '_'): float(v) for k, v in losses.items()})
    for k, p in head.named_parameters():
        if not p.requires_grad:
            continue
        key = k.replace('.', '__')
        if p.grad is None:
            out[key + '__none'] = np.zeros(1)
            continue
        g = p.grad.detach().double().flatten()
        out[key + '__stats'] = np.array([g.sum(), g.abs().sum(), g.norm()], np.float64)
        out[key + '__head'] = g[:16].float().numpy()
    MG.save('g8_train_grads_norefine.npz', **out)


def main():
    torch.set_grad_enabled(False)
    ref = RH.load_reference()
    h = ref_head()
    g9_state_dict(h)
    MG.g345_head(h, ref, 'tiny', 'tiny_norefine')
    MG.g345_head(h, ref, 'res101', 'res101_norefine')
    MG.g345_head(ref_head(5), ref, 'tiny', 'tiny_p5_norefine')
    g8_train_grads()


if __name__ == '__main__':
    main()
