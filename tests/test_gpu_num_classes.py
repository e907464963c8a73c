"""Heads of 17 .. 32 classes on the MI355X: the fusion layers' class head takes a second 16-column sub-tile (chain.hip,
K_NARROW of the radar programs).  The fused radar chain on the smallest shapes where that can go wrong, at every tile
height and matrix path, against the CPU oracle; the whole 23-class head against the oracle and the reference's fixtures
(tests/golden/make_golden_variants.py `classes`); outputs='all'; a training iteration at 23 classes against the reference's
gradients and at 32 against the oracle's autograd; the replay paths; last_level_cls_only.  The shared checks are
head_variant_rig.py's and teacher_forced_checks.py's, by import.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import num_classes_rig as NC
from head_variant_rig import SMOOTH, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from parity_util import assert_rows_match
from teacher_forced_checks import LAYER_TOL, hit_aware
from oracle import transcar_oracle as O
from transcar_amd import radar as RD, synth

pytestmark = pytest.mark.gpu


# ---- 1. the kernel at the smallest shapes where it can go wrong ------------------------------------------------------------
def _kernel_inputs(case):
    """The oracle's decoder state of the two samples as tc_radar_fusion_fwd takes it, and the oracle's fusion levels."""
    cat = lambda key: gpu(torch.cat([dbg[key] for _, dbg, _ in case['samples']], 0))       # noqa: E731
    hs5 = gpu(torch.cat([dbg['hs'][-1] for _, dbg, _ in case['samples']], 0))               # [2,Q,C]
    ref5 = gpu(torch.cat([dbg['inter_refs'][-1] for _, dbg, _ in case['samples']], 0))      # [2,Q,3]
    tok_np, pad_mult = RD.pack_tokens([f36 for _, _, f36 in case['samples']], T=NC.KT)
    want = {k: np.stack([w[k][:, 0].numpy() for w, _, _ in case['samples']], 1)             # [3,2,Q,D]
            for k in ('all_cls_scores', 'all_bbox_preds')}
    want_hits = np.stack([np.stack([h.numpy() for h in dbg['hit_counts']]) for _, dbg, _ in case['samples']], 1)
    return hs5, ref5, cat('tmp'), gpu(tok_np), pad_mult, want, want_hits


def _check_levels(cls, box, hits, want, want_hits, what):
    """radar_layers_teacher_forced's rule for one launch of three layers, per sample: a query is compared once its gate
    decisions agree in every layer so far, at most 2 new disagreements per layer, LAYER_TOL accumulating per layer."""
    for b in range(want_hits.shape[1]):
        agree = None
        for r in range(3):
            tag = '%s sample %d fusion layer %d' % (what, b, r + 1)
            if r == 0:
                agree = hit_aware(box[0, b], want['all_bbox_preds'][0, b], hits[0, b], want_hits[0, b], LAYER_TOL, tag + ' box')
                hit_aware(cls[0, b], want['all_cls_scores'][0, b], hits[0, b], want_hits[0, b], LAYER_TOL, tag + ' cls')
                agree = agree.copy()
                continue
            now = hits[r, b] == want_hits[r, b]
            assert int((agree & ~now).sum()) <= 2, '%s: %d new gate disagreements' % (tag, int((agree & ~now).sum()))
            agree &= now
            for name, got_, want_ in (('box', box[r, b], want['all_bbox_preds'][r, b]), ('cls', cls[r, b], want['all_cls_scores'][r, b])):
                d = np.abs(got_ - want_)[agree]
                print('%s %s: max|d| = %.3g over %d rows' % (tag, name, d.max(), int(agree.sum())))
                assert d.max() <= LAYER_TOL * (r + 1), '%s %s: max|d| = %.3g' % (tag, name, d.max())
        assert int(agree.sum()) >= want_hits.shape[2] - 6


@pytest.mark.parametrize('path', sorted(NC.PATHS))
@pytest.mark.parametrize('ncls', NC.KERNEL_CLASSES)
def test_radar_chain_class_counts(T, ncls, path):
    """tc_radar_fusion_fwd on 37 queries x 2 samples x 64 tokens (74 rows: a partial last tile at every tile height, a
    tile across the two samples) from the oracle's decoder state.  10 and 16 classes are the controls (one sub-tile);
    17 puts one column, 23 seven and 32 all sixteen into the second.  Without the second pass the columns from 16 on
    come back as the NaN ops.radar_fusion fills its outputs with."""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    case = NC.kernel_case(ncls)
    assert min(min(r) for r in NC.hit_rows(case)) >= NC.MIN_HIT_ROWS, NC.hit_rows(case)
    head, _ = R.shared_head(T, num_classes=ncls, num_query=NC.KQ)
    hs5, ref5, tmp, tokens, pad_mult, want, want_hits = _kernel_inputs(case)
    assert hs5.shape == (2, NC.KQ, 256) and tokens.shape == (2, NC.KT, 36)
    cls, box, hits = ops.radar_fusion(head, hs5, ref5, tmp, tokens, pad_mult, 0, 3, options=head_options(**NC.PATHS[path]))
    torch.cuda.synchronize()
    assert cls.shape == (3, 2, NC.KQ, ncls)
    assert torch.isfinite(cls).all() and torch.isfinite(box).all() and int(hits.min()) >= 0
    _check_levels(cls.cpu().numpy(), box.cpu().numpy(), hits.cpu().numpy(), want, want_hits, '%d classes %s' % (ncls, path))


@pytest.mark.parametrize('ncls', NC.KERNEL_CLASSES)
def test_operator_by_operator_path_class_counts(T, ncls):
    """options.unfused=1 has no entry of its own for the radar part: the whole 37-query head on the two samples,
    free-running, against the oracle with the bounds of head_variant_rig.check_against_oracle per sample."""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    case = NC.kernel_case(ncls)
    head, _ = R.shared_head(T, num_classes=ncls, num_query=NC.KQ)
    feats = [gpu(np.concatenate([f, f], 0)) for f in case['feats_np']]
    tok_np, pad_mult = RD.pack_tokens([f36 for _, _, f36 in case['samples']], T=NC.KT)
    metas = synth.make_img_metas(2, synth.make_lidar2img())
    outs = head.forward_nhwc(ops.to_nhwc_levels(feats), ops.lidar2img_tensor(metas, R.dev()), metas[0]['img_shape'][0][:2],
                             gpu(tok_np), pad_mult, aux=True, options=head_options(unfused=True))
    torch.cuda.synchronize()
    assert outs['all_cls_scores'].shape == (3, 2, NC.KQ, ncls)
    assert torch.isfinite(outs['all_cls_scores']).all() and torch.isfinite(outs['all_bbox_preds']).all()
    for b, (want, dbg, _) in enumerate(case['samples']):
        one = {k: outs[k][:, b:b + 1] for k in ('all_cls_scores', 'all_bbox_preds')}
        one['aux'] = {k: outs['aux'][k][:, b:b + 1] for k in ('inter_references', 'inter_states', 'radar_hit_counts')}
        R.check_against_oracle(one, want, dbg)


# ---- 2. the head, 900 queries, tiny maps, 23 classes -----------------------------------------------------------------------
def _g5_frame():
    gold = R.gold(NC.G5_C23)
    return gold, synth.make_feats('tiny', seed=1, smooth=SMOOTH), \
        synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])


ONE_LAYER = 'one-decoder-layer-'


def _one_layer_head_against_oracle(T, path):
    """A fusion head with ONE decoder layer: that layer's launch carries the whole radar encoder program (chain.hip
    launch_dual part 0), which no six-layer head asks for; 'p5-': with num_points = 5, the generic (MP) kernels.  The
    kernel case (37 queries x 2 samples x 64 tokens: 74 rows), free-running, per sample against the oracle with
    check_against_oracle's bounds (decoder states on the f16x2 path at P = 5: HS_TOL_F16X2, as test_head_points_paths)."""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    P = 5 if path.startswith('p5-') else 1
    path = path[3:] if P == 5 else path
    case = NC.kernel_case(23, num_layers=1, num_points=P)
    assert min(min(r) for r in NC.hit_rows(case)) >= NC.MIN_HIT_ROWS, NC.hit_rows(case)
    head = NC.one_layer_head(T, 23, P)
    assert head.weights_struct().num_points == P
    assert head.weights_struct().num_layers == 1 and head.weights_struct().num_radar_layers == 3
    feats = [gpu(np.concatenate([f, f], 0)) for f in case['feats_np']]
    tok_np, pad_mult = RD.pack_tokens([f36 for _, _, f36 in case['samples']], T=NC.KT)
    metas = synth.make_img_metas(2, synth.make_lidar2img())
    outs = head.forward_nhwc(ops.to_nhwc_levels(feats), ops.lidar2img_tensor(metas, R.dev()), metas[0]['img_shape'][0][:2],
                             gpu(tok_np), pad_mult, aux=True, options=head_options(**NC.PATHS[path]))
    torch.cuda.synchronize()
    assert outs['all_cls_scores'].shape == (3, 2, NC.KQ, 23) and outs['aux']['inter_states'].shape == (1, 2, NC.KQ, 256)
    assert torch.isfinite(outs['all_cls_scores']).all() and torch.isfinite(outs['all_bbox_preds']).all()
    for b, (want, dbg, _) in enumerate(case['samples']):
        one = {k: outs[k][:, b:b + 1] for k in ('all_cls_scores', 'all_bbox_preds')}
        one['aux'] = {k: outs['aux'][k][:, b:b + 1] for k in ('inter_references', 'inter_states', 'radar_hit_counts')}
        R.check_against_oracle(one, want, dbg, R.HS_TOL_F16X2 if P == 5 and path.startswith('f16x2') else R.E2E_TOL)


@pytest.mark.parametrize('path', sorted(NC.PATHS) + [ONE_LAYER + p for p in sorted(NC.PATHS)] +
                         [ONE_LAYER + 'p5-' + p for p in sorted(NC.PATHS)])
def test_head_23_classes_paths_oracle_and_golden(T, path):
    if path.startswith(ONE_LAYER):
        return _one_layer_head_against_oracle(T, path[len(ONE_LAYER):])
    gold, feats_np, frame = _g5_frame()
    head, sd = R.shared_head(T, num_classes=23)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='num_classes 23 golden')      # (the paths share one oracle forward)
    outs = R.run_head(head, feats_np, frame, **NC.PATHS[path])
    assert outs['all_cls_scores'].shape == (3, 1, 900, 23) and torch.isfinite(outs['all_cls_scores']).all()
    R.check_against_oracle(outs, want, dbg, R.E2E_TOL)
    R.check_against_fixture(outs, want, dbg, gold)


def _rows(b, s, l):
    return np.concatenate([np.asarray(b), np.asarray(s)[:, None], np.asarray(l)[:, None].astype(np.float32)], 1)


def test_get_bboxes_23_classes(T):
    """get_bboxes of the reference's outputs is the reference's decode (NMSFreeCoder(num_classes=23): labels above 15
    among them), up to neighbours swapping at near-tied scores (test_gpu_parity.test_box_decode_vs_oracle); and
    get_bboxes of the head's own forward is the oracle's decode of the same tensors."""
    gold, feats_np, frame = _g5_frame()
    head, _ = R.shared_head(T, num_classes=23)
    got = head.get_bboxes({'all_cls_scores': gpu(gold['all_cls_scores']), 'all_bbox_preds': gpu(gold['all_bbox_preds'])},
                          synth.make_img_metas(1))[0]
    np.testing.assert_allclose(got[1].cpu().numpy(), gold['dec_scores'], atol=1e-6, rtol=0)
    assert int(gold['dec_labels'].max()) > 15 and int(got[2].max()) == int(gold['dec_labels'].max())
    assert_rows_match(_rows(got[0].cpu(), got[1].cpu(), got[2].cpu()),
                      _rows(gold['dec_boxes'], gold['dec_scores'], gold['dec_labels']), atol=2e-5, what='decoded boxes')
    s = got[1].cpu().numpy()
    assert np.all(s[:-1] >= s[1:])
    outs = R.run_head(head, feats_np, frame)
    mine = head.get_bboxes(outs, synth.make_img_metas(1))[0]
    own = O.get_bboxes({k: outs[k].cpu() for k in ('all_cls_scores', 'all_bbox_preds')},
                       head.bbox_coder.post_center_range, num_classes=23)[0]
    assert_rows_match(_rows(*[t.cpu() for t in mine]), _rows(*own), atol=2e-5, what='decode of the own forward')


# ---- 3. outputs='all' ----------------------------------------------------------------------------------------------------
def test_all_outputs_23_classes(T):
    _, feats_np, frame = _g5_frame()
    head, _ = R.make_head(T, num_classes=23)
    fusion = R.run_head(head, feats_np, frame)
    head.outputs = 'all'
    try:
        both = R.run_head(head, feats_np, frame)
    finally:
        head.outputs = 'fusion'
    assert both['all_cls_scores'].shape == (6 + 3, 1, 900, 23) and torch.isfinite(both['all_cls_scores']).all()
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(both[k][6:], fusion[k]), k


# ---- 4. training -------------------------------------------------------------------------------------------------------------
def _losses_close(got, ref, what):
    for k, v in got.items():
        assert abs(v - ref[k]) < 2e-3 * max(1.0, abs(ref[k])), (what, k, v, ref[k])


@pytest.fixture(scope='module')
def c23():
    """One fused iteration at 23 classes on the gradient fixture's frame."""
    g8 = R.gold(NC.G8_C23)
    assert int(g8['radar_seed']) == NC.G8_C23_RADAR_SEED
    frame = R.g8_frame(NC.G5_C23, radar_seed=NC.G8_C23_RADAR_SEED, num_classes=23)
    with torch.no_grad():
        losses, grads = R.trainer_iteration(frame, num_classes=23)
    return g8, frame, losses, grads


def test_training_iteration_23_classes_gradients_match_reference(T, c23):
    g8, _, losses, grads = c23
    _losses_close(losses, {k: float(g8['loss__' + k.replace('.', '_')]) for k in losses}, 'fused c23')
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'fused c23') == 98


def test_training_iteration_32_classes_gradients_match_oracle_autograd(T):
    """32 classes (the full second sub-tile, no fixture): the oracle's autograd on the CPU is the reference side.  The
    radar frame: G5's rig around the centres the oracle's decoder predicts, the seed chosen as G8-C23's."""
    with torch.no_grad():
        sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_classes=32))
        _, dbg0 = R.oracle_head(sd, synth.make_feats('tiny', seed=1, smooth=SMOOTH),
                                synth.make_radar_frame(seed=2, n_per_radar=51))
    frame = R.g8_frame(None, radar_seed=NC.C32_RADAR_SEED, num_classes=32, centres=NC.centres_of(dbg0))
    _, want_losses, matches, want_grads = R.oracle_training(frame, num_classes=32)
    for m in matches:
        assert (frame['labels'][m[m > 0].numpy() - 1] > 15).sum() >= 1
    losses, grads = R.trainer_iteration(frame, num_classes=32)
    _losses_close(losses, want_losses, 'fused c32')
    assert R.check_grads_against_g8(grads, R.GradStats(want_grads), 2e-3, 'fused c32 vs oracle') == 98


def test_deterministic_backward_23_classes_twice(T, c23):
    g8, frame, _, _ = c23
    a = R.trainer_iteration(frame, num_classes=23, deterministic=True)
    b = R.trainer_iteration(frame, num_classes=23, deterministic=True)
    assert R.check_grads_against_g8(a[1], g8, 2e-3, 'deterministic c23') == 98
    for k, g in a[1].items():
        assert (g is None) == (b[1][k] is None) and (g is None or torch.equal(g, b[1][k])), k


def test_operator_training_path_agrees_with_the_fused_one_23_classes(T, c23):
    """tc_radar_train_fwd / _bwd (the operator-by-operator training path) against the reference's gradients and the
    fused path's at 2e-3."""
    g8, frame, fused_losses, fused = c23
    losses, grads = R.trainer_iteration(frame, num_classes=23, chain_forward=False, chain_backward=False)
    _losses_close(losses, fused_losses, 'operators vs fused c23')
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'operators c23') == 98
    assert R.check_grads_against_g8(grads, R.GradStats(fused), 2e-3, 'operators vs fused c23') == 98


# ---- 5. the replay paths ---------------------------------------------------------------------------------------------------
def test_plugin_graph_replay_23_classes_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, num_classes=23)[0], R.make_head(T, num_classes=23)[0])


def test_frame_pipeline_23_classes_equals_forward_nhwc(T):
    R.check_frame_pipeline(R.shared_head(T, num_classes=23)[0], 2)


def test_frame_of_nine_23_classes_is_its_own(T):
    R.check_frame_of_nine(R.shared_head(T, num_classes=23)[0])


# ---- 6. last_level_cls_only ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['f32-4', 'f16x2-32'])
def test_last_level_cls_only_23_classes(T, path):
    _, feats_np, frame = _g5_frame()
    head, _ = R.shared_head(T, num_classes=23)
    full = R.run_head(head, feats_np, frame, **NC.PATHS[path])
    fast = R.run_head(head, feats_np, frame, last_level_cls_only=True, **NC.PATHS[path])
    assert torch.equal(full['all_bbox_preds'], fast['all_bbox_preds'])
    assert torch.equal(full['all_cls_scores'][2], fast['all_cls_scores'][2]) and torch.isfinite(fast['all_cls_scores'][2]).all()
