#!/usr/bin/env python3
"""Fixtures of a radar fusion attention with 4 and with 16 heads from the REFERENCE's own head, imported unmodified through
oracle/ref_harness.py and run on G5's tiny rig and G8's training rig (make_golden.py's functions, weights and maps).

The reference builds rf_multihead_attn{,2,3} as nn.MultiheadAttention(256, 8) (HEAD:129-171) and offers no argument for
the count.  The count adds no parameter, and torch's module reads it from two attributes at every call: after
`m.num_heads, m.head_dim = H, 256 // H` an nn.MultiheadAttention(256, 8) computes, bit for bit, what a freshly built
nn.MultiheadAttention(256, H) with the same weights computes (asserted below, with a mask).  So the reference's file stays
as it is and the three attributes are set on the built head.

Run only in the authoring container:   python tests/golden/make_golden_radar_heads.py

  g5_head_tiny_rh{4,16}.npz       outputs, reference points, per-layer hit counts (of the selected rows), fill_in, the
                                  radar seed and its gate margin
  g8_train_grads_rh{4,16}.npz     make_golden.write_g8's layout, the radar seed, its gate margin and tie sensitivity

The radar seed of the forward fixtures is chosen as make_golden_radar_gate chooses one: seeds 2 .. 39 are scanned on the
CPU oracle with its fusion attention at H heads (head_variant_rig.gate_margin) and the one whose closest gate decision is
farthest from its radius is kept; that margin is stored.

The gradient fixtures need more of their frame.  A gradient is discontinuous where a ReLU input of the trainable stack
crosses zero, as it is where a gate decision flips: two fp32 evaluation orders of a LayerNorm or a 256-term product part
by about 256 * 2^-24 = 1.5e-5 on operands of order one, so an input nearer to zero than that can be taken on either side,
and the gradients then differ by a rank-one term.  On the forward fixtures' frame (seed 5) one such input, 6.8e-6 from zero
in a matched row of the 4-head stack, moves radar_position_encoder.0.bias by 2.05e-3 of check_grads_against_g8's unit
where its caller allows 2e-3 -- taken on the other side in the ORACLE it reproduces, figure by figure, what the kernels
give on that frame.  So the gradient fixtures' seed is chosen by radar_heads_rig.tie_sensitivity too: the largest
deviation, in the figures check_grads_against_g8 compares, between the oracle's gradients and its gradients with EVERY ReLU
input of the trainable stack within TIE_TAU = 3e-5 (twice the estimate above) of zero taken on the other side at once.
Among the seeds on which that stays below half of the 2e-3 the tests allow, at 4 and at 16 heads, the one with the
largest gate margin is kept (one seed for both counts); margin and sensitivity are stored."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG                                 # noqa: E402
import head_variant_rig as R                             # noqa: E402
import radar_heads_rig as RR                             # noqa: E402
from oracle import ref_harness as RH                     # noqa: E402
from oracle import transcar_oracle as O                  # noqa: E402
from transcar_amd import synth                           # noqa: E402

SEEDS = range(2, 40)


def check_the_attribute_route(H):
    """nn.MultiheadAttention(256, 8) with num_heads / head_dim set to H equals nn.MultiheadAttention(256, H), bit for bit"""
    g = torch.Generator().manual_seed(H)
    a, b = torch.nn.MultiheadAttention(256, 8), torch.nn.MultiheadAttention(256, H)
    b.load_state_dict(a.state_dict())
    a.num_heads, a.head_dim = H, 256 // H
    q, kv = torch.randn((40, 1, 256), generator=g), torch.randn((70, 1, 256), generator=g)
    mask = torch.rand((40, 70), generator=g) < 0.8
    mask[:, 0] = False
    assert torch.equal(a(q, kv, kv, attn_mask=mask)[0], b(q, kv, kv, attn_mask=mask)[0])


def ref_head(H, train=False):
    head = MG.ref_head(train=train)
    for m in (head.rf_multihead_attn, head.rf_multihead_attn2, head.rf_multihead_attn3):
        m.num_heads, m.head_dim = H, 256 // H
    return head


def choose_seed(H, centres):
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    sd = O.to_torch_sd(synth.make_state_dict(seed=3))
    best = None
    for seed in SEEDS:
        frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=centres)
        m = R.gate_margin(sd, feats, frame, radar_num_heads=H)
        print('H %d seed %d: margin %.3g m' % (H, seed, m))
        if best is None or m > best[1]:
            best = (seed, m)
    return best


def choose_grad_seed(centres):
    """-> (seed, {H: (gate margin, tie sensitivity)}): see the module's docstring"""
    sd = O.to_torch_sd(synth.make_state_dict(seed=3))
    best = None
    for seed in SEEDS:
        host = R.g8_frame('g5_head_tiny.npz', radar_seed=seed, centres=centres)
        figs = {H: (R.gate_margin(sd, host['feats_np'], host['frame'], radar_num_heads=H), RR.tie_sensitivity(host, H))
                for H in RR.HEADS}
        print('seed %d:' % seed, {H: '%.3g m, %.3g' % f for H, f in figs.items()})
        margin = min(f[0] for f in figs.values())
        if max(f[1] for f in figs.values()) < RR.TIE_BOUND and (best is None or margin > best[2]):
            best = (seed, figs, margin)
    return best[0], best[1]


def make(H, grad_seed, grad_figs):
    check_the_attribute_route(H)
    centres = np.load(os.path.join(HERE, 'g5_head_tiny.npz'))['radar_centres']
    seed, margin = choose_seed(H, centres)
    print('H %d: radar seed %d, margin %.3g m' % (H, seed, margin))
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=centres)
    outs, cap, tcap = MG.run_head(ref_head(H), feats, l2i, frame)
    tokens = cap['tokens'][0].numpy()
    fill_in = int((tokens[:, 0] != 500.0).sum())
    hits = [(~cap['mask%d' % i].numpy()).sum(1).astype(np.int32) for i in range(3)]
    MG.save(RR.g5_name(H), all_cls_scores=outs['all_cls_scores'].numpy(),
            all_bbox_preds=outs['all_bbox_preds'].numpy(), inter_refs=tcap['inter_refs'].numpy(),
            Lq=np.array([cap['Lq%d' % i] for i in range(3)]), hit_counts0=hits[0], hit_counts1=hits[1], hit_counts2=hits[2],
            fill_in=fill_in, radar_seed=seed, gate_margin=margin, radar_num_heads=H)
    print('H %d: Lq' % H, [cap['Lq%d' % i] for i in range(3)])
    seed = grad_seed
    frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=centres)
    head = ref_head(H, train=True)
    MG.freeze_like_train_py(head)
    boxes, labels = synth.make_gt(seed=7, n=24)
    with torch.enable_grad():
        outs, cap, _ = MG.run_head(head, feats, l2i, frame)
        losses = head.loss([RH.GtBoxes(torch.from_numpy(boxes))], [torch.from_numpy(labels)], outs)
        total = sum(v for k, v in losses.items() if 'loss' in k)
        total.backward()
    MG.write_g8(RR.g8_name(H), head, outs, cap, losses, total, radar_seed=seed, radar_num_heads=H,
                gate_margin=grad_figs[H][0], tie_sensitivity=grad_figs[H][1])


def main():
    RH.load_reference()
    centres = np.load(os.path.join(HERE, 'g5_head_tiny.npz'))['radar_centres']
    grad_seed, grad_figs = choose_grad_seed(centres)
    print('gradient fixtures: radar seed %d' % grad_seed, grad_figs)
    for H in RR.HEADS:
        make(H, grad_seed, grad_figs)


if __name__ == '__main__':
    main()
