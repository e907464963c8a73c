#!/usr/bin/env python3
"""The reference's fixtures of a head with another camera count than the configs' six (Detr3DCrossAtten.num_cams; the
reference reads the count off lidar2img in feature_sampling and sizes attention_weights as Linear(C, N * P * L),
XFMR:280-292, 381-422), made as make_golden.py makes G5 and G8 and with its functions (run_head, the two-pass centre
scheme of g345_head, freeze_like_train_py, write_g8); this script supplies the 12-camera maps and cameras.

Run only in the authoring container:   python tests/golden/make_golden_num_cams.py

  g5_head_tiny_cams12.npz      Detr3DHead.forward of the reference head built with num_cams=12 (72 queries, tiny maps of
                               twelve cameras, the ring rig of tests/num_cams_rig.py) in g345_head's two passes -- the
                               second pass's radar frame of the seed chosen as below, stored with its distance: at
                               g345_head's seed 2 a gate decision of fusion layer 3 sits 4.9e-4 m from its radius, and
                               torch.cdist's |x|^2 + |y|^2 - 2 x.y form cancels to about that at 50 m, so another CPU's
                               matrix product takes it the other way (seen: 44 rows hit here, 43 there) -- plus the
                               keys and shapes of the reference head's own state dict (sd_keys, sd_shapes): at 12
                               cameras attention_weights is [48, 256] and the unused attention_weights2/3 stay [24, 256]
                               (HEAD:191-192 writes 6 * 4)
  g8_train_grads_cams12.npz    one training iteration's gradients of the same head, the radar frame of the seed chosen
                               as make_golden_variants chooses one: of seeds 2 .. 39 on G5-cams12's centres the one whose
                               closest gate decision (head_variant_rig.gate_margin, on the CPU oracle at the ring's
                               count) is farthest from its radius; seed and distance are stored (`seeds` prints them all)"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))               # tests/: the rigs

import make_golden as MG                                 # noqa: E402
import head_variant_rig as R                             # noqa: E402
import num_cams_rig as NR                                # noqa: E402
from oracle import ref_harness as RH                     # noqa: E402
from oracle import transcar_oracle as O                  # noqa: E402
from transcar_amd import configs, synth                  # noqa: E402

N = 12
TAG = 'tiny_cams%d' % N


def ref_head(train=False):
    """The reference's head at N cameras and NR.NQ queries with synth's seeded weights (strict load: same keys, same
    shapes).  -> (head, {key: shape} of the reference head's own state dict)"""
    cfg = configs.head_cfg(num_query=NR.NQ, num_cams=N)
    head = RH.build_reference_head(cfg, configs.train_cfg_pts if train else None)
    for ly in head.transformer.decoder.layers:
        assert ly.attentions[1].num_cams == N and ly.attentions[1].attention_weights.out_features == N * 4
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
    sd = NR.state_dict(N)
    assert shapes == {k: tuple(v.shape) for k, v in sd.items()}
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    head.eval()
    return head, shapes


class _rig_inputs:
    """make_golden's functions on the N-camera rig: they ask synth for the maps and `cameras` for lidar2img"""

    def __enter__(self):
        self.saved = (MG.synth.make_feats, MG.cameras)
        make_feats = self.saved[0]
        MG.synth.make_feats = functools.partial(make_feats, num_cams=N)
        MG.cameras = lambda geometry: (NR.Ring(N).lidar2img(), configs.IMG_SHAPE)
        make_frame = MG.synth.make_radar_frame
        self.saved += (make_frame,)

        def frame(seed=2, centres=None, **kw):          # pass 2 (the one near the centres): the chosen seed
            return make_frame(seed=seed if centres is None else NR.G8_CAMS12_RADAR_SEED, centres=centres, **kw)
        MG.synth.make_radar_frame = frame

    def __exit__(self, *exc):
        MG.synth.make_feats, MG.cameras, MG.synth.make_radar_frame = self.saved


def g5():
    head, shapes = ref_head()
    with _rig_inputs():
        MG.g345_head(head, RH.load_reference(), 'tiny', TAG)
    path = os.path.join(HERE, NR.G5_CAMS12)
    g = dict(np.load(path))
    keys = sorted(shapes)
    margins = g8_margins()
    seed = max(margins, key=margins.get)
    assert seed == NR.G8_CAMS12_RADAR_SEED, (seed, margins[seed])      # (the search runs on the centres pass 1 just stored)
    MG.save(NR.G5_CAMS12, radar_seed=seed, gate_margin=margins[seed], sd_keys=np.array(keys), sd_shapes=np.array([list(shapes[k]) + [0] * (2 - len(shapes[k])) for k in keys], np.int64),
            sd_ndim=np.array([len(shapes[k]) for k in keys], np.int64), **g)


def g8_margins():
    """{seed: gate margin} of the oracle at N cameras on G5-cams12's centres"""
    sd, feats = O.to_torch_sd(NR.state_dict(N)), NR.feats(N)
    cen = R.gold(NR.G5_CAMS12)['radar_centres']
    return {s: R.gate_margin(sd, feats, synth.make_radar_frame(seed=s, n_per_radar=51, centres=cen), **NR.variant(N))
            for s in NR.SEED_RANGE}


def g8():
    margins = g8_margins()
    seed = max(margins, key=margins.get)
    assert seed == NR.G8_CAMS12_RADAR_SEED, (seed, margins[seed])
    head, _ = ref_head(train=True)
    MG.freeze_like_train_py(head)
    g5_ = R.gold(NR.G5_CAMS12)
    frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=g5_['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    with torch.enable_grad():
        outs, cap, _ = MG.run_head(head, NR.feats(N), NR.Ring(N).lidar2img(), frame)
        losses = head.loss([RH.GtBoxes(torch.from_numpy(boxes))], [torch.from_numpy(labels)], outs)
        total = sum(v for k, v in losses.items() if 'loss' in k)
        total.backward()
    MG.write_g8(NR.G8_CAMS12, head, outs, cap, losses, total, radar_seed=seed, gate_margin=margins[seed])


if __name__ == '__main__':
    if sys.argv[1:] == ['seeds']:
        for s, m in sorted(g8_margins().items()):
            print('seed %2d: %.3e m' % (s, m))
    else:
        g5()
        g8()
