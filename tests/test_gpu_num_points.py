"""Detr3DCrossAtten(num_points > 1) on the MI355X: the stand-alone sampling op, the module, and the whole head on every
chain path, against the CPU oracle and the reference's fixtures (tests/golden/make_golden_variants.py points); the
shared checks are head_variant_rig.py's.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import HW, PCR, SMOOTH, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from transcar_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def head5(T):
    return R.shared_head(T, num_points=5)


@pytest.mark.parametrize('P', [2, 5])
def test_cam_sample_points_vs_oracle(T, P):
    rng = np.random.RandomState(31 + P)
    feats = synth.make_feats('tiny', seed=32, smooth=SMOOTH)
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    Q = 900
    ref = rng.uniform(0, 1, (1, Q, 3)).astype(np.float32)
    logits = rng.standard_normal((1, Q, 24 * P)).astype(np.float32)
    tf = [torch.from_numpy(f) for f in feats]
    want = O.weighted_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, torch.from_numpy(logits)).permute(0, 2, 1)
    _, mask = O.feature_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW)
    nhwc = [T.ops.to_nhwc(gpu(f)) for f in feats]
    got, vis = T.ops.cam_sample_fuse(nhwc, gpu(l2i), gpu(ref), gpu(logits), PCR, HW,
                                     return_mask=True, num_points=P)
    flips = (vis[0].cpu().numpy().astype(bool) != mask[0, 0, :, :, 0, 0].numpy()).any(1)
    assert flips.sum() <= 1
    np.testing.assert_allclose(got[0].cpu().numpy()[~flips], want[0].numpy()[~flips], atol=1e-4, rtol=1e-5)
    # a wrong (p, l) order would be caught: the weights are not symmetric in p and l
    if P == 5:
        swapped = torch.from_numpy(logits).view(1, Q, 6, 5, 4).transpose(3, 4).reshape(1, Q, -1)
        other = O.weighted_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, swapped).permute(0, 2, 1)
        assert np.abs(other[0].numpy() - want[0].numpy())[~flips].max() > 1e-2


def test_cross_atten_points_vs_oracle(T, head5):
    head, sd = head5
    rng = np.random.RandomState(21)
    feats_np = synth.make_feats('tiny', seed=22)
    query = rng.standard_normal((900, 1, 256)).astype(np.float32)
    qpos = rng.standard_normal((900, 1, 256)).astype(np.float32)
    refp = rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32)
    attn = head.transformer.decoder.layers[2].attentions[1]
    assert attn.num_points == 5 and attn.attention_weights.weight.shape == (120, 256)
    out = attn(gpu(query), None, [gpu(f) for f in feats_np], query_pos=gpu(qpos),
               reference_points=gpu(refp), img_metas=synth.make_img_metas(1))
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    want = O.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', torch.from_numpy(query),
                         torch.from_numpy(qpos), [torch.from_numpy(f) for f in feats_np],
                         torch.from_numpy(refp), PCR, l2i, HW)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


def _radar_frame():
    return synth.make_radar_frame(seed=2, n_per_radar=51)


# (the camera pre-gather rides on the f16x2 attention core only)
PATHS = [('f32', 4, False), ('f32', 8, False), ('f32', 16, False), ('f16x2', 16, False), ('f16x2', 32, False),
         ('f16x2', 16, True), ('f16x2', 32, True)]


@pytest.mark.parametrize('matrix,rows,pregather', PATHS)
def test_head_points_paths(T, head5, matrix, rows, pregather):
    """Whole head at P = 5, free-running through all nine layers, on every chain path."""
    head, sd = head5
    frame = _radar_frame()
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='points paths')       # (the paths share one oracle forward)
    outs = R.run_head(head, feats_np, frame, tile_rows=rows, matrix_path=matrix, cam_pregather=pregather)
    R.check_against_oracle(outs, want, dbg, R.HS_TOL_F16X2 if matrix == 'f16x2' else R.E2E_TOL)


@pytest.mark.parametrize('P', [3])
def test_head_odd_points_auto(T, P):
    head, sd = R.make_head(T, num_points=P)
    frame = _radar_frame()
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame)
    R.check_against_oracle(R.run_head(head, feats_np, frame), want, dbg)


def test_points_frame_of_nine_is_its_own(T, head5):
    R.check_frame_of_nine(head5[0])


# ---- against the reference's own outputs ------------------------------------------------------------------------------
def test_cross_atten_points_golden(T, head5):
    """Detr3DCrossAtten.forward at P = 5 against the reference (G2-P5)."""
    gold = R.gold('g2_cross_atten_p5.npz')
    head, _ = head5
    rng = np.random.RandomState(21)
    feats = [gpu(f) for f in synth.make_feats('tiny', seed=22)]
    query = gpu(rng.standard_normal((900, 1, 256)))
    qpos = gpu(rng.standard_normal((900, 1, 256)))
    refp = gpu(rng.uniform(0.02, 0.98, (1, 900, 3)))
    attn = head.transformer.decoder.layers[2].attentions[1]
    out = attn(query, None, feats, query_pos=qpos, reference_points=refp, img_metas=synth.make_img_metas(1))
    np.testing.assert_allclose(out.cpu().numpy()[::4], gold['out'], atol=5e-5, rtol=1e-5)


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
@pytest.mark.parametrize('shapes,P', [('tiny', 5), ('res101', 5), ('tiny', 3)])
def test_head_points_golden(T, shapes, P, path):
    """The whole head, free-running, against the reference's outputs (G5-P5 tiny / res101, G5-P3) on the rows whose
    radar gate decisions agree with the oracle's."""
    gold = R.gold('g5_head_%s_p%d.npz' % (shapes, P))
    head, sd = R.make_head(T, num_points=P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, key=('points golden', shapes, P))
    outs = R.run_head(head, feats_np, frame, **({} if path == 'auto' else dict(tile_rows=32, matrix_path='f16x2')))
    R.check_against_fixture(outs, want, dbg, gold)


# ---- train mode, training, the plugin entry and the pipeline at P = 5 -------------------------------------------------
def _g8_frame():
    return R.g8_frame('g5_head_tiny_p5.npz')


def test_training_iteration_points_gradients_match_reference(T):
    R.check_training_iteration(_g8_frame(), 'g8_train_grads_p5.npz', 'fused p5', num_points=5)


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_points_matches_reference_formula(T, rows, matrix):
    R.check_train_mode_decoder(_g8_frame(), rows, matrix, num_points=5)


def test_plugin_graph_replay_points_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, num_points=5)[0], R.make_head(T, num_points=5)[0])


def test_frame_pipeline_points_equals_forward_nhwc(T, head5):
    R.check_frame_pipeline(head5[0], nlanes=2)
