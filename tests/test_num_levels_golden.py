"""The CPU oracle, which reads the level count from the feature maps it is given, against the fixtures the
REFERENCE produced with 1, 2 and 3 FPN levels (tests/golden/make_golden_variants.py levels).  CPU; the fixtures are committed,
so the reference itself is not needed."""
import os

import numpy as np
import pytest
import torch

from oracle import transcar_oracle as O
from transcar_amd import configs, synth

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
E2E_TOL = 5e-4          # test_oracle_golden.test_g5_full_head
TINY, RES101 = configs.LEVEL_SHAPES['tiny'], configs.LEVEL_SHAPES['res101']

# fixture -> (level shapes, num_levels, num_points, with_box_refine)
G5 = {'g5_head_tiny_l1.npz': ([TINY[2]], 1, 1, True),
      'g5_head_tiny_l2.npz': (TINY[:2], 2, 1, True),
      'g5_head_tiny_l3.npz': (TINY[:3], 3, 1, True),
      'g5_head_res101_l2.npz': (RES101[:2], 2, 1, True),
      'g5_head_tiny_l3_p5_norefine.npz': (TINY[:3], 3, 5, False)}
G2 = {'g2_cross_atten_l1.npz': (TINY[:1], 1), 'g2_cross_atten_l3.npz': (TINY[:3], 3)}
XA = 'transformer.decoder.layers.2.attentions.1'


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


@pytest.mark.parametrize('nl', [1, 2, 3])
def test_fixture_weights_are_not_the_zero_init(nl):
    sd = synth.make_state_dict(seed=3, num_levels=nl)
    w = sd[XA + '.attention_weights.weight']
    assert w.shape == (6 * nl, 256) and w.std() > 0.01 and np.abs(w).min() > 0   # all sigmoids 0.5 would hide the order


def test_fixtures_store_their_level_shapes(golden_dir):
    for name, (shapes, *_) in list(G5.items()) + [(k, (v[0],)) for k, v in G2.items()]:
        assert _g(golden_dir, name)['level_shapes'].tolist() == [list(s) for s in shapes], name
    assert _g(golden_dir, 'g8_train_grads_l2.npz')['level_shapes'].tolist() == [list(s) for s in TINY[:2]]


def _g2_inputs(shapes):
    rng = np.random.RandomState(21)
    feats = [torch.from_numpy(f) for f in synth.make_feats(shapes, seed=22)]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    query = torch.from_numpy(rng.standard_normal((900, 1, 256)).astype(np.float32))
    qpos = torch.from_numpy(rng.standard_normal((900, 1, 256)).astype(np.float32))
    refp = torch.from_numpy(rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32))
    return feats, l2i, query, qpos, refp


@pytest.mark.parametrize('name', sorted(G2))
def test_g2_cross_atten_levels(golden_dir, name):
    shapes, nl = G2[name]
    g = _g(golden_dir, name)
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_levels=nl))
    feats, l2i, query, qpos, refp = _g2_inputs(shapes)
    out = O.cross_atten(sd, XA, query, qpos, feats, refp, PCR, l2i, HW)
    np.testing.assert_allclose(out.numpy()[::4], g['out'], atol=1e-5, rtol=0)
    if nl > 1:
        # the (camera, level) order matters: the same logits read as [L, N] give another result
        sw = dict(sd)
        for k in ('.weight', '.bias'):
            v = sd[XA + '.attention_weights' + k]
            sw[XA + '.attention_weights' + k] = v.view(6, nl, *v.shape[1:]).transpose(0, 1).reshape(v.shape).contiguous()
        other = O.cross_atten(sw, XA, query, qpos, feats, refp, PCR, l2i, HW)
        assert float(np.abs(other.numpy()[::4] - g['out']).max()) > 1e-3


@pytest.mark.parametrize('name', sorted(G5))
def test_g5_head_levels(golden_dir, name):
    shapes, nl, P, refine = G5[name]
    g = _g(golden_dir, name)
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_levels=nl, num_points=P, with_box_refine=refine))
    feats = [torch.from_numpy(f) for f in synth.make_feats(shapes, seed=1, smooth=(4, 6))]
    assert len(feats) == nl
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    f36 = O.build_radar_features(synth.make_radar_frame(seed=2, n_per_radar=51, centres=g['radar_centres']))
    np.testing.assert_allclose(f36.astype(np.float32), g['radar_tokens'], atol=1e-6, rtol=1e-6)
    outs, dbg = O.head_forward(sd, feats, l2i, HW, f36, PCR, return_debug=True, with_box_refine=refine)
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g['inter_refs'], atol=2e-5, rtol=0)
    hs = dbg['hs'].permute(0, 2, 1, 3).numpy()
    # (res101 maps: fp32 evaluation orders part by up to 7.3e-5 in a handful of the 87 552 stored elements)
    np.testing.assert_allclose(hs[:, ::16, 0, :], g['hs_rows'], atol=1e-4 if 'res101' in name else 5e-5, rtol=0)
    for i in range(3):
        assert len(dbg['hit_rows'][i]) == int(g['Lq'][i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        # [layers, B, Q, D]: at most two queries beyond the tolerance, those within 1e-2 (test_num_points_golden)
        d = np.abs(outs[k].numpy() - g[k]).max(axis=(0, 1, 3))
        bad = np.where(d > E2E_TOL)[0]
        assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (k, bad.tolist(), d[bad].tolist())


def test_g8_forward_is_the_oracle_head(golden_dir):
    """The gradient fixture's forward (two tiny levels, its own radar frame) is the oracle's head."""
    g8, g5 = _g(golden_dir, 'g8_train_grads_l2.npz'), _g(golden_dir, 'g5_head_tiny_l2.npz')
    assert np.isfinite(g8['total_loss']) and int(g8['radar_seed']) != 2
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_levels=2))
    feats = [torch.from_numpy(f) for f in synth.make_feats(TINY[:2], seed=1, smooth=(4, 6))]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    frame = synth.make_radar_frame(seed=int(g8['radar_seed']), n_per_radar=51, centres=g5['radar_centres'])
    outs = O.head_forward(sd, feats, l2i, HW, O.build_radar_features(frame), PCR)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        d = np.abs(outs[k].numpy() - g8[k]).max(axis=(0, 1, 3))
        bad = np.where(d > E2E_TOL)[0]
        assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (k, bad.tolist(), d[bad].tolist())


def test_single_level_is_not_level_zero(golden_dir):
    """g5_head_tiny_l1 samples a level that is not the finest: the same cross-attention on level 0 gives another result."""
    g = _g(golden_dir, 'g5_head_tiny_l1.npz')
    assert g['level_shapes'].tolist() == [[2, 3]]
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_levels=1))
    feats, l2i, query, qpos, refp = _g2_inputs([TINY[0]])
    a = O.cross_atten(sd, XA, query, qpos, feats, refp, PCR, l2i, HW)
    feats2, *_ = _g2_inputs([TINY[2]])
    b = O.cross_atten(sd, XA, query, qpos, feats2, refp, PCR, l2i, HW)
    assert float((a - b).abs().max()) > 1e-3
