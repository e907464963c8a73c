#!/usr/bin/env python3
"""Fixtures of a head with 23 classes (the raw nuScenes annotation categories; the TransCAR configs: the benchmark's 10
merged ones), from the REFERENCE's own code (oracle/ref_harness.py) with make_golden.py's rigs (G5's two passes, radar
near the predicted centres; G8's iteration).  Run only in the authoring container:
    python tests/golden/make_golden_classes.py [seeds]

  g5_head_tiny_c23.npz                 Detr3DHead.forward, tiny maps, 900 queries; decoded with NMSFreeCoder(num_classes=23)
  g8_train_grads_c23.npz               one training iteration's gradients, tiny shapes, ground-truth labels 0 .. 22, the
                                       radar frame of seed G8_C23_RADAR_SEED

23 classes put seven columns of every class head into the second 16-column sub-tile of the row chains' narrow step, and
the ground truth (synth.make_gt(seed=7, n=24, num_classes=23)) matches labels above 15 (asserted below).

make_golden.g345_head builds its coder from the configs' 10 classes and g8_train_grads draws the configs' ground truth,
so both rigs are restated here with the class count passed on; run_head, write_g8 and the freezing are make_golden's.
hs_rows keeps every 32nd query (the other G5 fixtures: every 16th): with 23 logits a row the file would otherwise pass
the largest fixture committed so far.

`seeds` prints, per radar seed 2 .. 39, the distance of the closest gate decision of the three fusion layers from its
radius, measured with the oracle at 23 classes on G5-C23's centres (make_golden_variants.py: a decision next to its
radius flips between two fp32 evaluation orders and moves the attention's gradients by ~1 %).  Seed 2, G5's frame, has
one 3.8e-5 m from its radius; G8_C23_RADAR_SEED is the seed with the largest such distance (seed 14: 8.9e-4 m)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                                 # noqa: E402
from make_golden import configs, synth                   # noqa: E402
from oracle import transcar_oracle as O                  # noqa: E402

NC = 23
HS_STRIDE = 32
G8_C23_RADAR_SEED = 14      # `seeds`: 8.9e-4 m, the largest of seeds 2 .. 39


def ref_head(train=False):
    """The REFERENCE's head at NC classes with synth's seeded weights, loaded strictly."""
    cfg = configs.head_cfg(num_classes=NC)
    assert cfg['num_classes'] == NC and cfg['bbox_coder']['num_classes'] == NC
    head = MG.RH.build_reference_head(cfg, configs.train_cfg_pts if train else None)
    assert head.num_classes == NC and head.cls_out_channels == NC
    sd = synth.make_state_dict(seed=3, num_classes=NC)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert sd['final_cls3.6.weight'].shape == (NC, 256) and sd['cls_branches.5.6.bias'].shape == (NC,)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    head.eval()
    return head


def g5_head(ref):
    """make_golden.g345_head on the tiny maps with the coder at NC classes."""
    head = ref_head()
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    l2i = synth.make_lidar2img()
    _, _, tcap = MG.run_head(head, feats, l2i, synth.make_radar_frame(seed=2, n_per_radar=51))
    r = tcap['inter_refs'][-1][0].numpy().astype(np.float64)
    pcr = configs.point_cloud_range
    centres = np.round(np.stack([r[:, 0] * (pcr[3] - pcr[0]) + pcr[0], r[:, 1] * (pcr[4] - pcr[1]) + pcr[1]], 1), 2)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=centres)
    outs, cap, tcap = MG.run_head(head, feats, l2i, frame)
    tokens = cap['tokens'][0].numpy()
    fill_in = int((tokens[:, 0] != 500.0).sum())
    hit_counts = [(~cap['mask%d' % i].numpy()).sum(1).astype(np.int32) for i in range(3)]
    coder = dict(configs.head_cfg(num_classes=NC)['bbox_coder'])
    coder.pop('type')
    dec = ref.CODER.NMSFreeCoder(**coder)
    assert dec.num_classes == NC
    preds = dec.decode({'all_cls_scores': outs['all_cls_scores'], 'all_bbox_preds': outs['all_bbox_preds']})[0]
    assert int(preds['labels'].max()) > 15
    bb = preds['bboxes'].clone()
    bb[:, 2] = bb[:, 2] - bb[:, 5] * 0.5                    # HEAD:1018
    hs = tcap['hs'].numpy()                                  # [6,Q,1,C]
    MG.save('g5_head_tiny_c%d.npz' % NC,
            all_cls_scores=outs['all_cls_scores'].numpy(), all_bbox_preds=outs['all_bbox_preds'].numpy(),
            inter_refs=tcap['inter_refs'].numpy(), init_ref=tcap['init_ref'].numpy(),
            hs_rows=hs[:, ::HS_STRIDE, 0, :], hs_stride=HS_STRIDE, hs_sum=hs.astype(np.float64).sum(axis=(1, 2, 3)),
            radar_centres=centres, radar_tokens=tokens[:fill_in], fill_in=fill_in,
            Lq=np.array([cap['Lq%d' % i] for i in range(3)]),
            hit_counts0=hit_counts[0], hit_counts1=hit_counts[1], hit_counts2=hit_counts[2],
            dec_boxes=bb.numpy(), dec_scores=preds['scores'].numpy(), dec_labels=preds['labels'].numpy())
    print('c%d' % NC, 'fill_in', fill_in, 'Lq', [cap['Lq%d' % i] for i in range(3)],
          'labels > 15 among the decoded:', int((preds['labels'] > 15).sum()))


def gate_margins(seeds):
    """Per radar seed: min over the three fusion layers, the queries, the three circles and the tokens of
    |distance - radius| (metres), from the oracle at NC classes on G5-C23's centres."""
    g5 = np.load(os.path.join(HERE, 'g5_head_tiny_c%d.npz' % NC))
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_classes=NC))
    feats = [torch.from_numpy(f) for f in synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    keep, seen = O.circle_mask, []

    def circle_mask(centre_xy, length_log, rot_sin, rot_cos, radar_xy, rmin, rmax):
        length = length_log.exp()
        radii = torch.clamp((length / 2.0).reshape(-1, 1), min=rmin, max=rmax)
        live = radar_xy[0, :, 0] != 500.0                  # the padding tokens sit far outside every circle
        for sign in (0.0, 0.25, -0.25):
            c = centre_xy.clone()
            c[..., 0] = c[..., 0] + sign * length * -rot_sin
            c[..., 1] = c[..., 1] + sign * length * -rot_cos
            seen.append(float((torch.cdist(c, radar_xy, p=2.0)[0][:, live] - radii).abs().min()))
        return keep(centre_xy, length_log, rot_sin, rot_cos, radar_xy, rmin, rmax)

    out = {}
    O.circle_mask = circle_mask
    try:
        for seed in seeds:
            del seen[:]
            frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=g5['radar_centres'])
            O.head_forward(sd, feats, l2i, configs.IMG_SHAPE[:2], O.build_radar_features(frame), configs.point_cloud_range)
            assert len(seen) == 9
            out[seed] = min(seen)
            print('radar seed %2d: closest gate decision %.2e m from its radius' % (seed, out[seed]))
    finally:
        O.circle_mask = keep
    return out


def g8_train_grads():
    """make_golden.g8_train_grads with the ground truth drawn from NC classes and the frame of G8_C23_RADAR_SEED."""
    head = ref_head(train=True)
    MG.freeze_like_train_py(head)
    g5 = np.load(os.path.join(HERE, 'g5_head_tiny_c%d.npz' % NC))
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=G8_C23_RADAR_SEED, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24, num_classes=NC)
    assert labels.max() > 15 and labels.max() < NC
    with torch.enable_grad():
        outs, cap, _ = MG.run_head(head, feats, l2i, frame)
        losses = head.loss([MG.RH.GtBoxes(torch.from_numpy(boxes))], [torch.from_numpy(labels)], outs)
        total = sum(v for k, v in losses.items() if 'loss' in k)
        total.backward()
    # labels above 15 are matched in every fusion level: their columns of the class head see a positive target
    gt = MG.RH.GtBoxes(torch.from_numpy(boxes))
    gc = torch.cat((gt.gravity_center, gt.tensor[:, 3:]), 1)
    for i in range(3):
        inds = head.assigner.assign(outs['all_bbox_preds'][i, 0].detach(), outs['all_cls_scores'][i, 0].detach(), gc,
                                    torch.from_numpy(labels)).gt_inds.numpy()
        assert (labels[inds[inds > 0] - 1] > 15).sum() >= 1
    MG.write_g8('g8_train_grads_c%d.npz' % NC, head, outs, cap, losses, total, radar_seed=G8_C23_RADAR_SEED)


def main():
    if 'seeds' in sys.argv[1:]:
        m = gate_margins(range(2, 40))
        best = max(m, key=m.get)
        print('largest: seed %d, %.2e m' % (best, m[best]))
        return
    g5_head(MG.RH.load_reference())
    g8_train_grads()


if __name__ == '__main__':
    main()
