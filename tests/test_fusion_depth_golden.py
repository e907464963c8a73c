"""The gradient fixtures of the one- and two-layer fusion heads (tests/golden/make_golden_fusion_depth.py: the reference's
forward cut to levels [:N], its own loss() and backward) against the CPU oracle: the oracle's forward, its levels [:N],
oracle.loss, backward -- losses and gradients within the 2e-3 of test_training's oracle-versus-reference check.  No GPU."""
import os

import numpy as np
import pytest
import torch

import fusion_depth_rig as F
from oracle import transcar_oracle as O
from test_training import g8_inputs, trainable
from transcar_amd import configs, synth


@pytest.fixture(scope='module')
def oracle_run(golden_dir):
    """The oracle's three-layer forward on G8's tiny frame with the trainable weights as leaves, once."""
    feats, l2i, frame, boxes, labels = g8_inputs(golden_dir)
    sd = O.to_torch_sd(synth.make_state_dict(3))
    for k, v in sd.items():
        if trainable(k):
            v.requires_grad_(True)
    with torch.enable_grad():
        outs = O.head_forward(sd, [torch.from_numpy(f) for f in feats], torch.from_numpy(l2i).float()[None],
                              configs.IMG_SHAPE[:2], O.build_radar_features(frame), configs.point_cloud_range)
    return sd, outs, torch.from_numpy(boxes), torch.from_numpy(labels)


@pytest.mark.parametrize('depth', F.DEPTHS)
def test_oracle_backward_of_the_first_levels_matches_reference(golden_dir, oracle_run, depth):
    g8 = np.load(os.path.join(golden_dir, 'g8_train_grads_f%d.npz' % depth))
    sd, outs, boxes, labels = oracle_run
    assert int(g8['num_fusion_layers']) == depth and g8['all_cls_scores'].shape[0] == depth
    cut = {k: outs[k][:depth] for k in ('all_cls_scores', 'all_bbox_preds')}
    for k, v in cut.items():
        assert np.abs(v.detach().numpy() - g8[k]).max() < 5e-4, k
    for v in sd.values():
        v.grad = None
    with torch.enable_grad():
        res, _ = O.loss(cut, boxes, labels, sd['code_weights'])
        assert sorted('loss__' + k.replace('.', '_') for k in res) == sorted(k for k in g8.files if k.startswith('loss__'))
        for k, v in res.items():
            ref = float(g8['loss__' + k.replace('.', '_')])
            assert abs(float(v) - ref) < 2e-3 * max(1.0, abs(ref)), (k, float(v), ref)
        total = sum(res.values())
        assert abs(float(total) - float(g8['total_loss'])) < 1e-4 * float(g8['total_loss'])
        total.backward(retain_graph=True)
    own = set(synth.make_state_dict(3, num_fusion_layers=depth))
    for k, v in sd.items():               # levels [:N] read no later layer
        if k not in own:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
    grads = {k: v.grad for k, v in sd.items() if trainable(k) and k in own}
    assert F.check_grads_against_g8(grads, g8, 2e-3, 'oracle', 14 + 28 * depth) == 14 + 28 * depth
