"""The gradient fixtures of the one- and two-layer fusion heads (tests/golden/make_golden_fusion_depth.py: the reference's
forward cut to levels [:N], its own loss() and backward) against the CPU oracle: the oracle's forward, its levels [:N],
oracle.loss, backward -- losses and gradients within the 2e-3 of test_training's oracle-versus-reference check.  No GPU."""
import numpy as np
import pytest

import head_variant_rig as R
from transcar_amd import synth


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_oracle_backward_of_the_first_levels_matches_reference(depth):
    g8 = R.gold('g8_train_grads_f%d.npz' % depth)
    assert int(g8['num_fusion_layers']) == depth and g8['all_cls_scores'].shape[0] == depth
    # the oracle's three-layer forward on G8's tiny frame, once for both depths
    cut, losses, _, grads = R.oracle_training(R.g8_frame('g5_head_tiny.npz'), levels=depth)
    for k, v in cut.items():
        assert v.shape[0] == depth and np.abs(v.numpy() - g8[k]).max() < 5e-4, k
    assert sorted('loss__' + k.replace('.', '_') for k in losses) == sorted(k for k in g8.files if k.startswith('loss__'))
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        assert abs(v - ref) < 2e-3 * max(1.0, abs(ref)), (k, v, ref)
    assert abs(sum(losses.values()) - float(g8['total_loss'])) < 1e-4 * float(g8['total_loss'])
    own = set(synth.make_state_dict(3, num_fusion_layers=depth))
    for k, g in grads.items():            # levels [:N] read no later layer
        if k not in own:
            assert g is None or float(g.abs().max()) == 0.0, k
    grads = {k: g for k, g in grads.items() if k in own}
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'oracle', 14 + 28 * depth) == 14 + 28 * depth
