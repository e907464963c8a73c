"""The CPU oracle at 23 classes against the fixtures the REFERENCE produced with a 23-class head
(tests/golden/make_golden_variants.py `classes`), with the bounds of tests/test_num_heads_golden.py, and the oracle's autograd
gradients (oracle.loss with num_classes=23) against the reference's at 2e-3.  CPU; the
fixtures are committed, so the reference itself is not needed."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import num_classes_rig as NC
from oracle import transcar_oracle as O
from transcar_amd import synth

E2E_TOL = 5e-4          # test_oracle_golden.test_g5_full_head, test_num_heads_golden


@pytest.fixture(scope='module')
def g5():
    return R.gold(NC.G5_C23)


@pytest.fixture(scope='module')
def g8():
    return R.gold(NC.G8_C23)


@pytest.fixture(scope='module')
def forward(g5):
    with torch.no_grad():
        sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_classes=NC.NC_FIXTURE))
        frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g5['radar_centres'])
        f36 = O.build_radar_features(frame)
        np.testing.assert_allclose(f36.astype(np.float32), g5['radar_tokens'], atol=1e-6, rtol=0)
        return R.oracle_head(sd, synth.make_feats('tiny', seed=1, smooth=R.SMOOTH), frame)


def _all_but_two(got, want, what):
    # [layers, B, Q, D]: at most two queries beyond the tolerance, those within 1e-2 (test_num_heads_golden)
    d = np.abs(got - want).max(axis=(0, 1, 3))
    bad = np.where(d > E2E_TOL)[0]
    assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (what, bad.tolist(), d[bad].tolist())


def test_g5_head_23_classes(g5, forward):
    outs, dbg = forward
    assert g5['all_cls_scores'].shape == (3, 1, 900, 23) and outs['all_cls_scores'].shape == (3, 1, 900, 23)
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g5['inter_refs'], atol=2e-5, rtol=0)
    hs = dbg['hs'].permute(0, 2, 1, 3).numpy()
    np.testing.assert_allclose(hs[:, ::int(g5['hs_stride']), 0, :], g5['hs_rows'], atol=5e-5, rtol=0)
    for i in range(3):
        assert len(dbg['hit_rows'][i]) == int(g5['Lq'][i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        _all_but_two(outs[k].numpy(), g5[k], k)
    # the columns of the second sub-tile on their own
    _all_but_two(outs['all_cls_scores'].numpy()[..., 16:], g5['all_cls_scores'][..., 16:], 'classes 16 .. 22')


def test_g5_decode_uses_the_coder_modulus(g5):
    """The oracle's decode of the reference's outputs with num_classes=23 gives the reference's boxes, scores and labels
    (labels above 15 among them)."""
    from parity_util import assert_rows_match
    from transcar_amd import configs
    outs = {'all_cls_scores': torch.from_numpy(g5['all_cls_scores']), 'all_bbox_preds': torch.from_numpy(g5['all_bbox_preds'])}
    pcr = configs.pts_bbox_head['bbox_coder']['post_center_range']
    assert int(g5['dec_labels'].max()) > 15
    b, s, l = O.get_bboxes(outs, pcr, num_classes=23)[0]
    got = np.concatenate([b.numpy(), s.numpy()[:, None], l.numpy()[:, None].astype(np.float32)], 1)
    want = np.concatenate([g5['dec_boxes'], g5['dec_scores'][:, None], g5['dec_labels'][:, None].astype(np.float32)], 1)
    assert_rows_match(got, want, atol=2e-5, what='decoded boxes')


def test_g8_forward_is_the_oracle_head(g5, g8):
    """The gradient fixture's forward (the radar frame of the seed it stores) is the oracle's head at 23 classes."""
    assert np.isfinite(g8['total_loss']) and int(g8['radar_seed']) == NC.G8_C23_RADAR_SEED
    host = R.g8_frame(NC.G5_C23, radar_seed=NC.G8_C23_RADAR_SEED, num_classes=23)
    outs, _, _, _ = R.oracle_training(host, num_classes=23)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        _all_but_two(outs[k].numpy(), g8[k], k)


def test_oracle_backward_matches_reference_23_classes(g5, g8):
    host = R.g8_frame(NC.G5_C23, radar_seed=NC.G8_C23_RADAR_SEED, num_classes=23)
    _, losses, matches, grads = R.oracle_training(host, num_classes=23)
    # matched labels lie above 15 in every level: the second sub-tile's columns see positive targets
    for m in matches:
        assert (host['labels'][m[m > 0].numpy() - 1] > 15).sum() >= 1
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        assert abs(v - ref) < 1e-4 * max(1.0, abs(ref)), (k, v, ref)
    assert abs(sum(losses.values()) - float(g8['total_loss'])) < 1e-4 * float(g8['total_loss'])
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'oracle c23') == 98
