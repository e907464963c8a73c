#!/usr/bin/env python3
"""Fixtures of heads whose decoder self-attention has 4 or 16 heads (attn_cfgs[0].num_heads; the TransCAR configs: 8),
from the REFERENCE's own code (oracle/ref_harness.py) with make_golden.py's rigs (G5's two passes, radar near the
predicted centres; G8's iteration).  Run only in the authoring container:
    python tests/golden/make_golden_heads.py

  g5_head_tiny_h{4,16}.npz             Detr3DHead.forward, tiny maps (self-attention never sees the maps), 900 queries
  g8_train_grads_h4.npz                one training iteration's gradients, tiny shapes, 4 heads

The state dict does not depend on the head count (same keys, same shapes: loaded strictly), and the radar fusion
attention keeps the 8 heads the reference builds it with (HEAD:129-171) -- asserted below."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                                 # noqa: E402
from make_golden import g345_head, g8_train_grads       # noqa: E402


def ref_head_with(num_heads):
    """make_golden.ref_head for a decoder MultiheadAttention of `num_heads` heads (the other variants: the configs')."""
    def ref_head(train=False, **variant):
        assert not variant, variant
        head = MG.RH.build_reference_head(MG.configs.head_cfg(num_heads=num_heads),
                                          MG.configs.train_cfg_pts if train else None)
        for ly in head.transformer.decoder.layers:
            assert ly.attentions[0].attn.num_heads == num_heads
        for m in (head.rf_multihead_attn, head.rf_multihead_attn2, head.rf_multihead_attn3):
            assert m.num_heads == 8
        sd = MG.synth.make_state_dict(seed=3)
        assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
        head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        head.eval()
        return head
    return ref_head


def main():
    ref = MG.RH.load_reference()
    for H in (4, 16):
        g345_head(ref_head_with(H)(), ref, 'tiny', 'tiny_h%d' % H)
    keep = MG.ref_head
    MG.ref_head = ref_head_with(4)          # g8_train_grads builds its head through make_golden's module-level name
    try:
        g8_train_grads(suffix='_h4')
    finally:
        MG.ref_head = keep


if __name__ == '__main__':
    main()
