"""Decoder layers with feedforward_channels 256 .. 2048 (tc_head_weights.ffn_dims; the configs: 512) on the MI355X: the
fused decoder chains run the FFN in chunks of 512 hidden units -- per chunk ffn0_c -> B_A, ffn1_c onto B_U3, the first
with the residual and the bias, the later ones accumulating.  The whole head against the CPU oracle on every tile height
and both matrix paths, one layer teacher-forced against fp64, the launch forms (nine frames per launch, FramePipeline,
the plugin graphs), outputs='all', no box refinement, the train-mode decoder with read-back masks and a training
iteration.  Tiny maps, 900 queries (28 tiles of 32 rows + 4: every tile height has a partial last tile).  The rig is
ffn_dims_rig.py; the checks and tolerances are head_variant_rig.py's and teacher_forced_checks.py's.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import ffn_dims_rig as FR
import head_variant_rig as R
import teacher_forced_checks as TF
from head_variant_rig import T, no_grad  # noqa: F401  (fixtures)
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PATHS = {(4, 'f32'): R.E2E_TOL, (8, 'f32'): R.E2E_TOL, (16, 'f32'): R.E2E_TOL, (16, 'f16x2'): R.HS_TOL_F16X2,
         (32, 'f16x2'): R.HS_TOL_F16X2}
# every width on both accumulator layouts of the f16x2 path; a full chunk + a narrow one and two full chunks on the f32 tiles too
CASES = [(F, rows, 'f16x2') for F in FR.WIDTHS for rows in (16, 32)] + \
        [(F, rows, 'f32') for F in (768, 1024) for rows in (4, 8, 16)]


# ---- 1. the whole head, free-running, against the oracle --------------------------------------------------------------------
@pytest.mark.parametrize('F,rows,matrix', CASES)
def test_head_against_oracle(T, F, rows, matrix):
    head, sd = R.shared_head(T, **FR.variant(F))
    feats_np, frame = FR.frame(F)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='ffn_dims', **FR.variant(F))
    outs = R.run_head(head, feats_np, frame, tile_rows=rows, matrix_path=matrix)
    d = (outs['aux']['inter_states'].cpu() - dbg['hs']).abs()
    print('F=%d %d rows %s: max|hs - oracle| per layer %s' % (F, rows, matrix, ['%.2e' % float(v) for v in d.amax(dim=(1, 2, 3))]))
    R.check_against_oracle(outs, want, dbg, PATHS[rows, matrix])


def test_the_width_reaches_the_kernels(T):
    """A head of 1024 hidden units parts by O(0.1) from the same head with the upper 512 switched off (ffn1's columns
    512.. zeroed): the second chunk is read, and from where the packer put it."""
    head, _ = R.make_head(T, **FR.variant(1024))
    feats_np, frame = FR.frame(1024)
    full = R.run_head(head, feats_np, frame, tile_rows=16, matrix_path='f16x2')['aux']['inter_states'].clone()
    for ly in head.transformer.decoder.layers:
        ly.ffns[0].layers[1].weight.data[:, 512:] = 0.0
    head.refresh_weights()
    cut = {p: R.run_head(head, feats_np, frame, tile_rows=p[0], matrix_path=p[1])['aux']['inter_states'].clone()
           for p in ((4, 'f32'), (16, 'f16x2'))}
    assert float((full - cut[16, 'f16x2']).abs().max()) > 0.1
    # ... and the first chunk is the 512-wide head of the lower half, bit for bit where the tile keeps fp32 activations
    # (the second chunk adds products with zero weights: + 0.0)
    half = T.build_head(configs.head_cfg())
    sd = {}
    for k, v in head.state_dict().items():
        if '.ffns.0.layers.0.0.' in k:
            v = v[:512]
        elif k.endswith('.ffns.0.layers.1.weight'):
            v = v[:, :512]
        sd[k] = v.clone()
    half.load_state_dict(sd, strict=True)
    half = half.to(R.dev()).eval()
    for p, got in cut.items():
        want = R.run_head(half, feats_np, frame, tile_rows=p[0], matrix_path=p[1])['aux']['inter_states']
        assert torch.equal(got, want), p


# ---- 2. one decoder layer at a time, teacher-forced, against fp64 ------------------------------------------------------------
@pytest.fixture(scope='module')
def tf_rig():
    """teacher_forced_checks' rig at F = 2048 on un-conditioned tiny maps (iid noise, full-scale refinement MLPs)"""
    import transcar_amd as T_
    F = 2048
    sd_np = synth.make_state_dict(seed=3, reg_out_scale=1.0, feedforward_channels=F)
    sd = O.to_torch_sd(sd_np)
    head = T_.build_head(configs.head_cfg(feedforward_channels=F))
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    head = head.to(R.dev()).eval()
    head.head_weights()
    feats_np = synth.make_feats('tiny', seed=1, smooth=None)
    feats = [torch.from_numpy(f) for f in feats_np]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    with torch.no_grad():
        hs, init_ref, inter_refs, _ = O.transformer(sd, feats, TF.PCR, l2i, TF.HW)
    nhwc = [TF.head_ops().to_nhwc(R.gpu(f)) for f in feats_np]
    return dict(F=F, sd=sd, sd64={k: v.double() for k, v in sd.items()}, head=head, feats=feats, nhwc=nhwc, l2i=l2i, hs=hs,
                init_ref=init_ref, inter_refs=inter_refs)


@pytest.mark.parametrize('rows', [16, 32])
def test_decoder_layers_teacher_forced_2048(tf_rig, rows):
    """teacher_forced_checks.decoder_layers_teacher_forced, its bounds as they are (it reads the width off the head: the C
    layer struct carries none): four chunks per layer, each layer on the oracle's state of the layer before."""
    assert tf_rig['head'].weights_struct().ffn_dims == tf_rig['F']
    TF.decoder_layers_teacher_forced(tf_rig, rows, 'f16x2', 'teacher-forced decoder layers, feedforward_channels=2048')


def test_one_layer_entry_refuses_other_widths(T):
    """The one-layer entry with a width refuses what the chains do not run, naming it."""
    from transcar_amd import ops
    head, _ = R.shared_head(T, **FR.variant(1024))
    head.head_weights()
    pv = head._packed_view
    nhwc = [ops.to_nhwc(R.gpu(f)) for f in synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)]
    z = torch.zeros((1, 900, 256), device=R.dev())
    ref = torch.full((1, 900, 3), 0.5, device=R.dev())
    l2i = R.gpu(synth.make_lidar2img()[None])
    with pytest.raises(T.TransCARHipError, match='ffn_dims=640'):
        ops.decoder_layer_tail(pv.layers[2], pv.layers[3].self_attn.in_proj, nhwc, z, z, head.query_embedding.weight, l2i, ref,
                               R.PCR, R.HW, ffn_dims=640)


# ---- 3. the launch forms at F = 1024 -----------------------------------------------------------------------------------------
def test_frame_of_nine_is_its_own(T):
    R.check_frame_of_nine(R.shared_head(T, **FR.variant(1024))[0])


@pytest.mark.parametrize('rows,matrix', [(16, 'f16x2'), (16, 'f32')])
def test_frames_of_nine_are_their_own_on_16_rows(T, rows, matrix):
    """Every frame of a nine-frame launch is bit-identical to that frame launched alone at the same tile height and
    matrix path (check_frame_of_nine: frame 4 on the 32-row tiles)."""
    from transcar_amd.detr3d_head import head_options
    head = R.shared_head(T, **FR.variant(1024))[0]
    feats = [synth.make_feats('tiny', seed=40 + i, smooth=R.SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    head.forward_options = head_options(tile_rows=rows, matrix_path=matrix)
    try:
        many = head([R.gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(4)], R.DEFAULT.metas(9, radar=frames))
        for i in range(9):
            one = head([R.gpu(f) for f in feats[i]], R.DEFAULT.metas(1, radar=frames[i]))
            for k in ('all_cls_scores', 'all_bbox_preds'):
                assert torch.equal(many[k][:, i], one[k][:, 0]), (i, k)
    finally:
        head.forward_options = None


def test_frame_pipeline_equals_forward_nhwc(T):
    R.check_frame_pipeline(R.shared_head(T, **FR.variant(1024))[0], 2)


def test_plugin_graph_replay_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, **FR.variant(1024))[0], R.make_head(T, **FR.variant(1024))[0])


# ---- 4. other paths --------------------------------------------------------------------------------------------------------
def test_all_outputs_768_against_oracle(T):
    """outputs='all' at F = 768: the decoder levels' own scores and boxes against O.decoder_outputs on the oracle's
    trace, the fusion levels behind them against the oracle's head."""
    F = 768
    head, sd = R.shared_head(T, **FR.variant(F))
    feats_np, frame = FR.frame(F)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='ffn_dims', **FR.variant(F))
    head.outputs = 'all'
    try:
        outs = R.run_head(head, feats_np, frame)
    finally:
        head.outputs = 'fusion'
    assert outs['all_cls_scores'].shape == (9, 1, 900, 10) and outs['all_bbox_preds'].shape == (9, 1, 900, 10)
    o_cls, o_box = O.decoder_outputs(sd, dbg['hs'], dbg['init_ref'], dbg['inter_refs'], list(R.DEFAULT.pc_range))
    for name, got, orc in (('logits', outs['all_cls_scores'][:6], o_cls), ('boxes', outs['all_bbox_preds'][:6], o_box)):
        print('F=%d %s: max|camera level - oracle| = %.3g' % (F, name, float((got.cpu() - orc).abs().max())))
        np.testing.assert_allclose(got.cpu().numpy(), orc.numpy(), atol=R.E2E_TOL, rtol=0)
    fusion = dict(outs, all_cls_scores=outs['all_cls_scores'][6:], all_bbox_preds=outs['all_bbox_preds'][6:])
    R.check_against_oracle(fusion, want, dbg, R.HS_TOL_F16X2)


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_no_box_refinement_1024_against_oracle(T, rows, matrix):
    """with_box_refine=False: the reg steps behind the FFN's records are switched off (and the layer-0 sequence's too)."""
    head, sd = R.shared_head(T, **FR.variant(1024, refine=False))
    feats_np, frame = FR.frame(1024, refine=False)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='ffn_dims', **FR.variant(1024, refine=False))
    outs = R.run_head(head, feats_np, frame, tile_rows=rows, matrix_path=matrix)
    R.check_against_oracle(outs, want, dbg, PATHS[rows, matrix], refs_initial=True)


# ---- 5. train mode and training -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_1024_matches_reference_formula(T, rows, matrix):
    R.check_train_mode_decoder(R.g8_frame('g5_head_tiny.npz', radar_seed=FR.SEEDS[1024, True]), rows, matrix, **FR.variant(1024))


@pytest.mark.parametrize('mode', ['chain', 'deterministic'])
@pytest.mark.parametrize('F', [256, 1024])
def test_training_iteration_against_oracle_autograd(T, F, mode):
    """One FusionTrainer iteration (frozen decoder of width F -> fusion stack -> loss -> backward) with the chain backward
    and with deterministic=True: the losses and the 98 gradient tensors against the oracle's autograd, within the rig's 2e-3."""
    frame = R.g8_frame('g5_head_tiny.npz', radar_seed=FR.SEEDS[F, True])
    _, want_losses, _, want_grads = R.oracle_training(frame, **FR.variant(F))
    h = R.train_head(**FR.variant(F))
    assert len(h.trainable_parameters()) == 98
    kw = dict(deterministic=True) if mode == 'deterministic' else {}
    losses, grads = R.trainer_iteration(frame, head=h, **kw)
    assert sorted(losses) == sorted(want_losses)
    for k, v in losses.items():
        print('F=%d %s %s: %.6f (oracle %.6f)' % (F, mode, k, v, want_losses[k]))
        assert abs(v - want_losses[k]) < 2e-3 * max(1.0, abs(want_losses[k])), (k, v, want_losses[k])
    assert R.check_grads_against_g8(grads, R.GradStats(want_grads), 2e-3, 'F=%d %s' % (F, mode), 98) == 98
