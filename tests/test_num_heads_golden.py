"""The CPU oracle with a decoder self-attention of 4 and of 16 heads (head_forward(num_heads=H)) against the fixtures
the REFERENCE produced with those head counts (tests/golden/make_golden_variants.py `heads`), with the tolerances of
tests/test_num_levels_golden.py.  CPU; the fixtures are committed, so the reference itself is not needed."""
import os

import numpy as np
import pytest
import torch

from head_variant_rig import HEADS
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
E2E_TOL = 5e-4          # test_oracle_golden.test_g5_full_head


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def _forward(g, H):
    sd = O.to_torch_sd(synth.make_state_dict(seed=3))
    feats = [torch.from_numpy(f) for f in synth.make_feats('tiny', seed=1, smooth=(4, 6))]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    f36 = O.build_radar_features(synth.make_radar_frame(seed=2, n_per_radar=51, centres=g['radar_centres']))
    np.testing.assert_allclose(f36.astype(np.float32), g['radar_tokens'], atol=1e-6, rtol=1e-6)
    if H is None:
        return O.head_forward(sd, feats, l2i, HW, f36, PCR, return_debug=True)
    return O.head_forward(sd, feats, l2i, HW, f36, PCR, return_debug=True, num_heads=H)


@pytest.mark.parametrize('H', HEADS)
def test_g5_head_heads(golden_dir, H):
    g = _g(golden_dir, 'g5_head_tiny_h%d.npz' % H)
    outs, dbg = _forward(g, H)
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g['inter_refs'], atol=2e-5, rtol=0)
    hs = dbg['hs'].permute(0, 2, 1, 3).numpy()
    np.testing.assert_allclose(hs[:, ::16, 0, :], g['hs_rows'], atol=5e-5, rtol=0)
    for i in range(3):
        assert len(dbg['hit_rows'][i]) == int(g['Lq'][i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        # [layers, B, Q, D]: at most two queries beyond the tolerance, those within 1e-2 (test_num_levels_golden)
        d = np.abs(outs[k].numpy() - g[k]).max(axis=(0, 1, 3))
        bad = np.where(d > E2E_TOL)[0]
        assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (k, bad.tolist(), d[bad].tolist())


def test_the_head_count_matters(golden_dir):
    """An oracle that ignored the head count could not pass: on the H = 4 fixture's frame the 8-head oracle is O(1) away
    in the decoder states."""
    g = _g(golden_dir, 'g5_head_tiny_h4.npz')
    _, dbg = _forward(g, None)
    hs = dbg['hs'].permute(0, 2, 1, 3).numpy()
    assert np.abs(hs[:, ::16, 0, :] - g['hs_rows']).max() > 0.1


def test_g8_forward_is_the_oracle_head(golden_dir):
    """The gradient fixture's forward (4 heads, G5-H4's frame) is the oracle's head at 4 heads."""
    g8, g5 = _g(golden_dir, 'g8_train_grads_h4.npz'), _g(golden_dir, 'g5_head_tiny_h4.npz')
    assert np.isfinite(g8['total_loss'])
    outs, _ = _forward(g5, 4)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        d = np.abs(outs[k].numpy() - g8[k]).max(axis=(0, 1, 3))
        bad = np.where(d > E2E_TOL)[0]
        assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (k, bad.tolist(), d[bad].tolist())
