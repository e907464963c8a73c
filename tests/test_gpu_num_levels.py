"""Detr3DCrossAtten(num_levels < 4) on the MI355X: the stand-alone sampling op, the module, and the whole head on every
chain path, against the CPU oracle and the reference's fixtures (tests/golden/make_golden_variants.py levels); the
shared checks are head_variant_rig.py's.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import HW, PCR, SMOOTH, TINY, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from transcar_amd import synth

pytestmark = pytest.mark.gpu

# level shapes of L levels: the first L tiny ones; ONE level is (2, 3), not level 0 (no kernel may lean on it)
LEVELS = {1: [TINY[2]], 2: TINY[:2], 3: TINY[:3]}


@pytest.fixture(scope='module')
def head2(T):
    return R.shared_head(T, num_levels=2)


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('nl', [1, 2, 3])
def test_cam_sample_levels_vs_oracle(T, nl, P):
    rng = np.random.RandomState(31 + 10 * nl + P)
    feats = synth.make_feats(LEVELS[nl], seed=32, smooth=SMOOTH)
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    Q = 900
    ref = rng.uniform(0, 1, (1, Q, 3)).astype(np.float32)
    logits = rng.standard_normal((1, Q, 6 * P * nl)).astype(np.float32)
    tf = [torch.from_numpy(f) for f in feats]
    want = O.weighted_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, torch.from_numpy(logits)).permute(0, 2, 1)
    _, mask = O.feature_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW)
    nhwc = [T.ops.to_nhwc(gpu(f)) for f in feats]
    got, vis = T.ops.cam_sample_fuse(nhwc, gpu(l2i), gpu(ref), gpu(logits), PCR, HW, return_mask=True, num_points=P)
    flips = (vis[0].cpu().numpy().astype(bool) != mask[0, 0, :, :, 0, 0].numpy()).any(1)
    assert flips.sum() <= 1
    np.testing.assert_allclose(got[0].cpu().numpy()[~flips], want[0].numpy()[~flips], atol=1e-4, rtol=1e-5)
    if nl > 1:
        # a wrong (camera, level) order would be caught
        swapped = torch.from_numpy(logits).view(1, Q, 6, P, nl).transpose(2, 4).reshape(1, Q, -1)
        other = O.weighted_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, swapped).permute(0, 2, 1)
        assert np.abs(other[0].numpy() - want[0].numpy())[~flips].max() > 1e-2


@pytest.mark.parametrize('nl', [1, 3])
def test_cross_atten_levels_golden(T, nl):
    """Detr3DCrossAtten.forward with 1 / 3 levels against the reference (G2-L1 / -L3) and the oracle."""
    gold = R.gold('g2_cross_atten_l%d.npz' % nl)
    head, sd = R.make_head(T, num_levels=nl)
    shapes = [tuple(s) for s in gold['level_shapes']]
    assert shapes == TINY[:nl]
    rng = np.random.RandomState(21)
    feats_np = synth.make_feats(shapes, seed=22)
    query = rng.standard_normal((900, 1, 256)).astype(np.float32)
    qpos = rng.standard_normal((900, 1, 256)).astype(np.float32)
    refp = rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32)
    attn = head.transformer.decoder.layers[2].attentions[1]
    assert attn.num_levels == nl and attn.attention_weights.weight.shape == (6 * nl, 256)
    out = attn(gpu(query), None, [gpu(f) for f in feats_np], query_pos=gpu(qpos), reference_points=gpu(refp),
               img_metas=synth.make_img_metas(1))
    np.testing.assert_allclose(out.cpu().numpy()[::4], gold['out'], atol=5e-5, rtol=1e-5)
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    want = O.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', torch.from_numpy(query),
                         torch.from_numpy(qpos), [torch.from_numpy(f) for f in feats_np], torch.from_numpy(refp),
                         PCR, l2i, HW)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


# (matrix path, tile rows, unfused): None = the automatic choice
PATHS = [('f32', 4, False), ('f32', 8, False), ('f32', 16, False), ('f16x2', 16, False), ('f16x2', 32, False),
         (None, None, False), (None, None, True)]


@pytest.mark.parametrize('matrix,rows,unfused', PATHS)
@pytest.mark.parametrize('nl', [1, 2, 3])
def test_head_levels_paths(T, nl, matrix, rows, unfused):
    """Whole head with 1 / 2 / 3 levels, free-running through all nine layers, on every chain path and the unfused
    path, against the oracle."""
    head, sd = R.make_head(T, num_levels=nl)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats(LEVELS[nl], seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, key=('levels paths', nl))   # (the paths share one oracle forward)
    opts = dict(unfused=True) if unfused else dict(tile_rows=rows, matrix_path=matrix) if matrix else {}
    outs = R.run_head(head, feats_np, frame, **opts)
    R.check_against_oracle(outs, want, dbg, R.HS_TOL_F16X2 if matrix == 'f16x2' else R.E2E_TOL)


def test_head_refuses_other_level_count(T, head2):
    head, _ = head2
    feats = [gpu(f) for f in synth.make_feats(TINY[:3], seed=1)]
    with pytest.raises(T.TransCARHipError, match='3 feature levels given.*num_levels=2'):
        head(feats, synth.make_img_metas(1, radar=synth.make_radar_frame(seed=2, n_per_radar=20)))


def test_explicit_pregather_is_refused(T, head2):
    """cam_pregather = 1 asked for on a shape without it keeps raising at the C boundary."""
    from transcar_amd.detr3d_head import head_options
    head, _ = head2
    head.forward_options = head_options(tile_rows=16, matrix_path='f16x2', cam_pregather=True)
    try:
        with pytest.raises(T.TransCARHipError, match='pre-gather'):
            head([gpu(f) for f in synth.make_feats(TINY[:2], seed=1)],
                 synth.make_img_metas(1, radar=synth.make_radar_frame(seed=2, n_per_radar=20)))
        torch.cuda.synchronize()
    finally:
        head.forward_options = None


# ---- against the reference's own outputs ------------------------------------------------------------------------------
G5 = {'g5_head_tiny_l1.npz': (1, 1, True), 'g5_head_tiny_l2.npz': (2, 1, True), 'g5_head_tiny_l3.npz': (3, 1, True),
      'g5_head_res101_l2.npz': (2, 1, True), 'g5_head_tiny_l3_p5_norefine.npz': (3, 5, False)}


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
@pytest.mark.parametrize('name', sorted(G5))
def test_head_levels_golden(T, name, path):
    """The whole head, free-running, against the reference's outputs (G5-L*) on the rows whose radar gate decisions
    agree with the oracle's and the reference's (with check_against_fixture's tie rule)."""
    nl, P, refine = G5[name]
    gold = R.gold(name)
    shapes = [tuple(s) for s in gold['level_shapes']]
    head, sd = R.make_head(T, num_levels=nl, num_points=P, with_box_refine=refine)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, with_box_refine=refine, key=('levels golden', name))
    outs = R.run_head(head, feats_np, frame, **({} if path == 'auto' else dict(tile_rows=32, matrix_path='f16x2')))
    R.check_against_fixture(outs, want, dbg, gold, tie_rule=True)


# ---- train mode, training, the plugin entry, the pipeline and the layer op at L = 2 ------------------------------------
def _g8_frame():
    seed = int(R.gold('g8_train_grads_l2.npz')['radar_seed'])      # (its own radar frame: make_golden_variants.py)
    return R.g8_frame('g5_head_tiny_l2.npz', TINY[:2], radar_seed=seed)


def test_training_iteration_levels_gradients_match_reference(T):
    R.check_training_iteration(_g8_frame(), 'g8_train_grads_l2.npz', 'fused l2', num_levels=2)


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_levels_matches_reference_formula(T, rows, matrix):
    R.check_train_mode_decoder(_g8_frame(), rows, matrix, num_levels=2)


def test_plugin_graph_replay_levels_is_the_eager_entry(T):
    """The camera pre-gather the entry turns on for 4 levels is off here (cam_pregather_supported): the replay runs."""
    hg, he = R.make_head(T, num_levels=2)[0], R.make_head(T, num_levels=2)[0]
    assert not hg.cam_pregather_supported()
    R.check_plugin_graph_replay(hg, he, TINY[:2])


@pytest.mark.parametrize('nlanes', [1, 3])
def test_frame_pipeline_levels_equals_forward_nhwc(T, head2, nlanes):
    """One lane (pre-gather default off for two levels) and three lanes, on the first two tiny levels."""
    R.check_frame_pipeline(head2[0], nlanes, TINY[:2], pregather_off=True)


@pytest.mark.parametrize('nl', [1, 3])
def test_levels_frame_of_nine_is_its_own(T, nl):
    R.check_frame_of_nine(R.make_head(T, num_levels=nl)[0], LEVELS[nl])


def test_layer_tail_refuses_fewer_levels(T, head2):
    """tc_decoder_layer_tail_fwd stays 4 levels only: fewer are refused, naming the count."""
    from transcar_amd import ops
    head, _ = head2
    head.head_weights()
    pv = head._packed_view
    Q = 900
    z = torch.zeros((1, Q, 256), device=R.dev())
    ref_in = torch.full((1, Q, 3), 0.5, device=R.dev())
    nhwc = [ops.to_nhwc(gpu(f)) for f in synth.make_feats(TINY[:2], seed=1)]
    with pytest.raises(T.TransCARHipError, match='num_levels=2'):
        ops.decoder_layer_tail(pv.layers[2], pv.layers[3].self_attn.in_proj, nhwc, z, z, head.query_embedding.weight,
                               gpu(synth.make_lidar2img())[None], ref_in, PCR, HW, tile_rows=4, matrix_path=0)
