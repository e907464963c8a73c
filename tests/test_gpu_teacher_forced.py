"""Whole-head parity ON THE BENCH WORKLOAD by per-layer teacher forcing (-m gpu).

The end-to-end rigs of test_gpu_parity.py are conditioned (smooth feature fields, last layer of
every box-regression MLP scaled by 0.1) because the decoder's reference-point -> sampling ->
reference-point loop amplifies fp32 rounding by ~4x per layer on iid-noise maps: after six layers
no two fp32 implementations agree.  Here the loop is cut instead of tamed:
on the UN-conditioned inputs (``make_feats('res101', smooth=None)`` = the maps bench.py times,
``reg_out_scale=1.0`` = full xavier-scale refinements) every HIP layer is fed the ORACLE's state of
the layer before -- query features and reference points -- and must reproduce the oracle's output of
that one layer.  The kernels are the ones the timed path runs: tc_sdpa_fwd (attention core),
tc_decoder_layer_tail_fwd (the fused decoder row chain incl. camera sampling, FFN, box refinement
and the next layer's QKV projection) and tc_radar_fusion_fwd (radar encoders + the fused radar
chain), each fusion layer teacher-forced from the oracle's previous box / features as well.

Reference lines: XFMR:178-214 (decoder loop + refinement), XFMR:346-378 (cross attention),
HEAD:538-729 (three fusion layers).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import transcar_oracle as O
from teacher_forced_checks import (HW, PCR, decoder_layers_teacher_forced, dev, gpu, head_ops,
                                   qkv_from_oracle_state as _qkv_from_oracle_state, radar_layers_teacher_forced)
from transcar_amd import configs, radar as R, synth

pytestmark = pytest.mark.gpu

# The tolerances (LAYER_MAX_TOL, LAYER_MEAN_TOL, LAYER_TOL, REF_TOL), their derivation and the bodies of the two
# per-layer comparisons live in teacher_forced_checks.py: test_gpu_adverse_frame.py holds the adverse rig to the
# same assertions.


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope='module')
def rig():
    """Un-conditioned bench inputs + the oracle's trace of every layer."""
    import transcar_amd as T
    sd_np = synth.make_state_dict(seed=3, reg_out_scale=1.0)
    sd = O.to_torch_sd(sd_np)
    head = T.build_head(configs.head_cfg())
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    head = head.to(dev()).eval()
    head.head_weights()
    feats_np = synth.make_feats('res101', seed=1, smooth=None)        # iid N(0,1): bench.py:make_inputs
    feats = [torch.from_numpy(f) for f in feats_np]
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    hs, init_ref, inter_refs, _ = O.transformer(sd, feats, PCR, l2i, HW)   # hs [L,Q,1,C]
    nhwc = [head_ops().to_nhwc(gpu(f)) for f in feats_np]
    return dict(T=T, sd=sd, sd64={k: v.double() for k, v in sd.items()}, head=head, feats=feats,
                nhwc=nhwc, l2i=l2i, hs=hs, init_ref=init_ref, inter_refs=inter_refs)


@pytest.mark.parametrize('tile_rows,matrix', [(0, None), (8, None), (16, 'f16x2'), (16, 'f32'), (32, 'f16x2')])
def test_decoder_layers_teacher_forced_on_bench_inputs(rig, tile_rows, matrix):
    """Every tile height of the row chain (0 = the automatic choice, 4-row tiles at one frame; 8; 16 on BOTH
    matrix paths: the two-plane f16 operands on the matrix cores -- round 4, the default -- and the
    v_mfma_f32_16x16x4 path on the second weight copy; 32 rows with the activations as f16 planes in LDS -- round 5's
    headline tile height, here since round 6; the tolerances are the same for all):
    HIP layer l (attention core + fused row chain) on the oracle's layer-(l-1) state and
    reference points, l = 0..5, iid-noise ResNet-101 maps, full-scale refinement MLPs -- measured
    against the fp64 evaluation of the reference formula on the same inputs, next to the fp32
    oracle's own deviation from it.  Also: the refined reference points and the next layer's
    projected q / k / v^T the chain hands to the following attention core."""
    decoder_layers_teacher_forced(rig, tile_rows, matrix, 'teacher-forced decoder layers on the bench workload')


@pytest.mark.parametrize('matrix', ['f32', 'f16x2'])
def test_attention_core_teacher_forced(rig, matrix):
    """tc_sdpa_fwd (fp32 MFMA) / tc_sdpa_fwd_f16x2 (two-plane f16 operands on the matrix cores, round 4) + out_proj
    residual on the oracle's layer-3 input vs torch MHA semantics: the same tolerance for both."""
    ops = head_ops()
    sd = rig['sd']
    qe = sd['query_embedding.weight']
    pos = qe[:, :256][None]
    x_prev = rig['hs'][2].permute(1, 0, 2)
    q, k, vt = _qkv_from_oracle_state(sd, 3, x_prev, pos)
    attn_o = ops.sdpa(gpu(q), gpu(k), gpu(vt), matrix_path=matrix).cpu()
    name = 'transformer.decoder.layers.3.attentions.0.attn'
    got = F.linear(attn_o, sd[name + '.out_proj.weight'], sd[name + '.out_proj.bias'])
    qk_in = (x_prev + pos).permute(1, 0, 2)
    want = O.multihead_attention(sd, name, qk_in, qk_in, x_prev.permute(1, 0, 2)).permute(1, 0, 2)
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=3e-5, rtol=0)


@pytest.mark.parametrize('tile_rows,matrix', [(0, None), (16, 'f16x2'), (16, 'f32'), (32, 'f16x2')])
def test_radar_layers_teacher_forced_on_bench_inputs(rig, tile_rows, matrix):
    """(4-row tiles, the 16-row tiles on both matrix paths: two-plane f16 and the f32 16x16x4, and the 32-row tiles.)  The fused radar chain, ONE fusion layer at a time: layer r is fed the oracle's query
    features and box of layer r-1 (hs[5] / the decoder's last box for r = 0) and must reproduce the
    oracle's class scores, boxes and hit counts of layer r; then all three layers in one launch from
    the oracle's hs[5] (the launch tc_head_forward makes)."""
    sd = rig['sd']
    # radar frame with 80 % of the returns near the boxes the oracle's decoder predicts (bench.py)
    refs = rig['inter_refs'][-1][0].double().numpy()
    centres = np.round(np.stack([refs[:, 0] * (PCR[3] - PCR[0]) + PCR[0],
                                 refs[:, 1] * (PCR[4] - PCR[1]) + PCR[1]], 1), 2)
    frame = synth.make_radar_frame(seed=2, centres=centres)
    f36 = O.build_radar_features(frame)
    # the oracle's own trace of the radar part, layer by layer (HEAD:538-729)
    trace = O.head_forward(sd, rig['feats'], rig['l2i'], HW, f36, PCR, return_debug=True)
    tok_np, pad_mult = R.pack_tokens([R.build_radar_features(frame)])
    radar_layers_teacher_forced(rig, f36, tok_np, pad_mult, tile_rows, matrix, trace)


def test_last_level_cls_only_option(rig):
    """tc_head_options.last_level_cls_only (inference opt-in): boxes of all levels and the class
    scores of the decoded level are bit-identical to the default; the two skipped class slices are
    left untouched."""
    from transcar_amd.detr3d_head import head_options
    ops = head_ops()
    head = rig['head']
    frame = synth.make_radar_frame(seed=2)
    tok_np, pad_mult = R.pack_tokens([R.build_radar_features(frame)])
    tokens = gpu(tok_np)
    l2i = gpu(rig['l2i'])
    full = head.forward_nhwc(rig['nhwc'], l2i, HW, tokens, pad_mult)
    torch.cuda.synchronize()
    fast = head.forward_nhwc(rig['nhwc'], l2i, HW, tokens, pad_mult,
                             options=head_options(last_level_cls_only=True))
    assert torch.equal(full['all_bbox_preds'], fast['all_bbox_preds'])
    assert torch.equal(full['all_cls_scores'][2], fast['all_cls_scores'][2])
    a = head.get_bboxes(full, synth.make_img_metas(1))[0]
    b = head.get_bboxes(fast, synth.make_img_metas(1))[0]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    del ops
