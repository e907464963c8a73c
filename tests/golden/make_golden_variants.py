#!/usr/bin/env python3
"""Fixtures of the head's variants beside the TransCAR configs' (4 levels, num_points 1, box refinement), from the
REFERENCE's own code (oracle/ref_harness.py) with make_golden.py's functions and rigs (G2's inputs; G5's two passes,
radar near the predicted centres; G8's iteration).  Run only in the authoring container:
    python tests/golden/make_golden_variants.py [points] [levels] [norefine]          (none named: all three)

points -- Detr3DCrossAtten(num_points > 1):
  g2_cross_atten_p5.npz                Detr3DCrossAtten.forward at P = 5
  g5_head_{tiny,res101}_p5.npz         Detr3DHead.forward at P = 5
  g5_head_tiny_p3.npz                  ... at P = 3
  g8_train_grads_p5.npz                one training iteration's gradients, tiny shapes, P = 5
levels -- num_levels < 4; every fixture stores its level shapes (`level_shapes`):
  g2_cross_atten_l{1,3}.npz            Detr3DCrossAtten.forward on tiny level 0 / levels 0-2
  g5_head_tiny_l1.npz                  Detr3DHead.forward on ONE level that is not level 0: (2, 3)
  g5_head_tiny_l{2,3}.npz              ... on the first two / three tiny levels
  g5_head_res101_l2.npz                ... on the first two res101 levels (the large maps)
  g5_head_tiny_l3_p5_norefine.npz      ... three levels, num_points = 5, with_box_refine=False
  g8_train_grads_l2.npz                one training iteration's gradients, two tiny levels, the radar frame of seed
                                       G8_L2_RADAR_SEED
norefine -- Detr3DHead(with_box_refine=False): one cls and one reg branch shared across the decoder layers
(HEAD:223-231), reg_branches=None handed to the decoder (HEAD:271):
  g5_head_{tiny,res101}_norefine.npz   Detr3DHead.forward
  g5_head_tiny_p5_norefine.npz         ... at num_points 5
  g8_train_grads_norefine.npz          one training iteration's gradients, tiny shapes
  g9_norefine_state_dict.json          the reference head's state_dict keys and shapes

A radar gate decision that sits next to its radius flips between two fp32 evaluation orders, and a flipped row of the
third fusion layer moves its attention's gradients by ~1 % (G5-L2's radar frame, seed 2: query 880, 2.1e-4 m from the
radius).  The two-level gradient fixture takes the radar frame whose closest gate decision, in all three fusion layers,
is the farthest from its radius among seeds 3 .. 39 (seed 13: 8.9e-4 m, measured with the oracle)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                                 # noqa: E402
from make_golden import g2_cross_atten, g345_head, g8_train_grads, ref_head      # noqa: E402

TINY, RES101 = MG.configs.LEVEL_SHAPES['tiny'], MG.configs.LEVEL_SHAPES['res101']
G8_L2_RADAR_SEED = 13


def points(ref):
    h5 = ref_head(num_points=5)
    g2_cross_atten(h5, tag='_p5')
    g345_head(h5, ref, 'tiny', 'tiny_p5')
    g345_head(h5, ref, 'res101', 'res101_p5')
    g345_head(ref_head(num_points=3), ref, 'tiny', 'tiny_p3')
    g8_train_grads(suffix='_p5', num_points=5)


def levels(ref):
    h1, h2, h3 = ref_head(1), ref_head(2), ref_head(3)
    g2_cross_atten(h1, TINY[:1], '_l1')
    g2_cross_atten(h3, TINY[:3], '_l3')
    g345_head(h1, ref, [TINY[2]], 'tiny_l1')
    g345_head(h2, ref, TINY[:2], 'tiny_l2')
    g345_head(h3, ref, TINY[:3], 'tiny_l3')
    g345_head(h2, ref, RES101[:2], 'res101_l2')
    g345_head(ref_head(3, num_points=5, with_box_refine=False), ref, TINY[:3], 'tiny_l3_p5_norefine')
    g8_train_grads(suffix='_l2', shapes=TINY[:2], radar_seed=G8_L2_RADAR_SEED, num_levels=2)


def norefine(ref):
    h = ref_head(with_box_refine=False)
    keys = {k: list(v.shape) for k, v in h.state_dict().items()}
    with open(os.path.join(HERE, 'g9_norefine_state_dict.json'), 'w') as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write('\n')
    print('wrote g9_norefine_state_dict.json (%d keys)' % len(keys))
    g345_head(h, ref, 'tiny', 'tiny_norefine')
    g345_head(h, ref, 'res101', 'res101_norefine')
    g345_head(ref_head(num_points=5, with_box_refine=False), ref, 'tiny', 'tiny_p5_norefine')
    g8_train_grads(suffix='_norefine', with_box_refine=False)


def main():
    ref = MG.RH.load_reference()
    for make in (points, levels, norefine):
        if make.__name__ in sys.argv[1:] or not sys.argv[1:]:
            make(ref)


if __name__ == '__main__':
    main()
