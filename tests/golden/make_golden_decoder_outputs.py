#!/usr/bin/env python3
"""Generate g10_decoder_outputs_tiny{,_norefine}.npz: the class scores and boxes of the six DETR3D decoder levels
(HEAD:277-298) from the REFERENCE's own arithmetic.

The reference computes these outputs and drops them (HEAD:607-608 reset the lists), so its return value cannot be
recorded.  Forward hooks on each distinct module of head.cls_branches / head.reg_branches keep the OUTPUT TENSORS
THEMSELVES (no clone): HEAD:287-293 edits `tmp` in place after the module returned, so after the forward a kept
reg-branch output IS outputs_coord of its level.  With box refinement the decoder calls every reg branch once more
(XFMR:191); the head's calls are the last six recorded.

Same rig as g5_head_tiny: feature maps seed 1 with SMOOTH, state dict seed 3 (the decoder reads no radar).  The
generator asserts that its inter_references equal the g5 fixture's bit for bit: the fixtures describe the same run.

Run only in the authoring container:   python tests/golden/make_golden_decoder_outputs.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG                                 # noqa: E402
from transcar_amd import synth                           # noqa: E402

torch.set_grad_enabled(False)


def decoder_outputs(with_box_refine, g5_name, out_name):
    head = MG.ref_head(with_box_refine=with_box_refine)
    calls = {'cls': [], 'reg': []}
    hooks = []
    for kind, branches in (('cls', head.cls_branches), ('reg', head.reg_branches)):
        seen = set()
        for m in branches:
            if id(m) in seen:                            # without refinement: one module under every index
                continue
            seen.add(id(m))
            hooks.append(m.register_forward_hook(lambda mod, inp, out, kind=kind: calls[kind].append(out)))
    feats = synth.make_feats('tiny', seed=1, smooth=MG.SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    _, _, tcap = MG.run_head(head, feats, synth.make_lidar2img(), frame)
    for h in hooks:
        h.remove()
    L = 6
    assert len(calls['cls']) == L and len(calls['reg']) == (2 * L if with_box_refine else L), \
        (len(calls['cls']), len(calls['reg']))
    g5 = np.load(os.path.join(HERE, g5_name))
    assert np.array_equal(tcap['inter_refs'].numpy(), g5['inter_refs']), 'not the run of ' + g5_name
    dec_cls = torch.stack(calls['cls']).numpy()
    dec_box = torch.stack(calls['reg'][-L:]).numpy()
    assert dec_cls.shape == (L, 1, 900, 10) and dec_box.shape == (L, 1, 900, 10), (dec_cls.shape, dec_box.shape)
    assert dec_cls.dtype == np.float32 and dec_box.dtype == np.float32
    print(out_name, 'box x', dec_box[..., 0].min(), dec_box[..., 0].max())
    MG.save(out_name, dec_cls=dec_cls, dec_box=dec_box)


if __name__ == '__main__':
    decoder_outputs(True, 'g5_head_tiny.npz', 'g10_decoder_outputs_tiny.npz')
    decoder_outputs(False, 'g5_head_tiny_norefine.npz', 'g10_decoder_outputs_tiny_norefine.npz')
