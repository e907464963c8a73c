#!/usr/bin/env python3
"""Fixtures of Detr3DCrossAtten with num_levels < 4, from the REFERENCE's own code (oracle/ref_harness.py), as
make_golden.py makes the 4-level ones.  Run only in the authoring container:
    python tests/golden/make_golden_levels.py          (`... g8`: the gradient fixture only)

The reference initialises attention_weights to zero (XFMR:297-300): every sigmoid is then 0.5 and a wrong (camera,
level) order of the logits would go unseen.  The weights here are synth.make_state_dict's seeded ones (non-zero
attention_weights, checked below).  Every fixture stores its level shapes (`level_shapes`).  Written:
  g2_cross_atten_l{1,3}.npz            Detr3DCrossAtten.forward on tiny level 0 / levels 0-2 (G2's inputs)
  g5_head_tiny_l1.npz                  Detr3DHead.forward on ONE level that is not level 0: (2, 3)
  g5_head_tiny_l{2,3}.npz              ... on the first two / three tiny levels (G5's rig)
  g5_head_res101_l2.npz                ... on the first two res101 levels (the large maps)
  g5_head_tiny_l3_p5_norefine.npz      ... three levels, num_points = 5, with_box_refine=False
  g8_train_grads_l2.npz                one training iteration's gradients, tiny shapes, two levels (G8's rig with the
                                       radar frame of seed G8_RADAR_SEED)

A radar gate decision that sits next to its radius flips between two fp32 evaluation orders, and a flipped row of the
third fusion layer moves its attention's gradients by ~1 % (G5-L2's radar frame, seed 2: query 880, 2.1e-4 m from the
radius).  The gradient fixture takes the radar frame whose closest gate decision, in all three fusion layers, is the
farthest from its radius among seeds 3 .. 39 (seed 13: 8.9e-4 m, measured with the oracle)."""
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

TINY, RES101 = configs.LEVEL_SHAPES['tiny'], configs.LEVEL_SHAPES['res101']
G8_RADAR_SEED = 13


def ref_head(num_levels, num_points=1, refine=True, train=False):
    head = RH.build_reference_head(configs.head_cfg(num_levels=num_levels, num_points=num_points,
                                                    with_box_refine=refine),
                                   configs.train_cfg_pts if train else None)
    assert head.transformer.decoder.layers[0].attentions[1].num_levels == num_levels
    sd = synth.make_state_dict(seed=3, num_levels=num_levels, num_points=num_points, with_box_refine=refine)
    ref_keys = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    assert ref_keys == {k: tuple(v.shape) for k, v in sd.items()}
    for i in range(6):
        w = sd['transformer.decoder.layers.%d.attentions.1.attention_weights.weight' % i]
        assert w.shape[0] == 6 * num_points * num_levels and np.abs(w).min() > 0 and w.std() > 0.01
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    head.eval()
    return head


def add_shapes(name, shapes):
    """store the level shapes in a written fixture"""
    path = os.path.join(HERE, name)
    d = dict(np.load(path))
    d['level_shapes'] = np.asarray(shapes, np.int64)
    MG.save(name, **d)


def g2_cross_atten(head, shapes, tag):
    """make_golden.g2_cross_atten's inputs and rows, on the given levels."""
    rng = np.random.RandomState(21)
    feats = synth.make_feats(shapes, seed=22)
    metas = synth.make_img_metas(1, synth.make_lidar2img())
    Q = 900
    query = rng.standard_normal((Q, 1, 256)).astype(np.float32)
    qpos = rng.standard_normal((Q, 1, 256)).astype(np.float32)
    refp = rng.uniform(0.02, 0.98, (1, Q, 3)).astype(np.float32)
    attn = head.transformer.decoder.layers[2].attentions[1]
    with torch.no_grad():
        out = attn(torch.from_numpy(query), None, [torch.from_numpy(f) for f in feats],
                   query_pos=torch.from_numpy(qpos), reference_points=torch.from_numpy(refp), img_metas=metas)
    MG.save('g2_cross_atten_%s.npz' % tag, out=out.numpy()[::4], level_shapes=np.asarray(shapes, np.int64))


def g5_head(head, ref, shapes, tag):
    MG.g345_head(head, ref, shapes, tag)
    add_shapes('g5_head_%s.npz' % tag, shapes)


def g8_train_grads(num_levels, shapes, tag):
    """make_golden.g8_train_grads on the given levels (tiny shapes)."""
    head = ref_head(num_levels, train=True)
    MG.freeze_like_train_py(head)
    g5 = np.load(os.path.join(HERE, 'g5_head_tiny_%s.npz' % tag))
    feats = synth.make_feats(shapes, seed=1, smooth=MG.SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=G8_RADAR_SEED, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    with torch.enable_grad():
        outs, cap, _ = MG.run_head(head, feats, l2i, frame)
        losses = head.loss([RH.GtBoxes(torch.from_numpy(boxes))], [torch.from_numpy(labels)], outs)
        total = sum(v for k, v in losses.items() if 'loss' in k)
        total.backward()
    out = {'total_loss': float(total),
           'all_cls_scores': outs['all_cls_scores'].detach().numpy(),
           'all_bbox_preds': outs['all_bbox_preds'].detach().numpy(),
           'Lq': np.array([cap['Lq%d' % i] for i in range(3)]),
           'level_shapes': np.asarray(shapes, np.int64), 'radar_seed': G8_RADAR_SEED}
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
    MG.save('g8_train_grads_%s.npz' % tag, **out)


def main():
    torch.set_grad_enabled(False)
    ref = RH.load_reference()
    h1, h2, h3 = ref_head(1), ref_head(2), ref_head(3)
    g2_cross_atten(h1, TINY[:1], 'l1')
    g2_cross_atten(h3, TINY[:3], 'l3')
    if sys.argv[1:] != ['g8']:
        g5_head(h1, ref, [TINY[2]], 'tiny_l1')
        g5_head(h2, ref, TINY[:2], 'tiny_l2')
        g5_head(h3, ref, TINY[:3], 'tiny_l3')
        g5_head(h2, ref, RES101[:2], 'res101_l2')
        g5_head(ref_head(3, num_points=5, refine=False), ref, TINY[:3], 'tiny_l3_p5_norefine')
    g8_train_grads(2, TINY[:2], 'l2')


if __name__ == '__main__':
    main()
