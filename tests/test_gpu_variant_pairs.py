"""The head's configuration keys taken together, on the MI355X: every row of variant_pairs_rig's pairwise tables through the
kernels against the CPU oracle under the same combination.

Inference, per row: the head built through head_variant_rig from all the row's keys, every key asserted on
weights_struct(), one launch of one or two samples under the row's chain path, each sample against oracle_row through
head_variant_rig.check_against_oracle with the rig's tolerances as they are; with outputs='all' the decoder levels against
O.decoder_outputs.  The flat tolerances are the bound on every row: the project's arbiter of a query beyond them, the
decoder layers teacher-forced against fp64 (teacher_forced_checks), runs tc_decoder_layer_tail_fwd, which serves heads of
4 levels, one point and 8 decoder heads with box refinement -- no pairwise row is one -- so no per-query bound is applied.  Two invariants that need no oracle on the three rows with the most non-default keys: a frame
inside a nine-frame launch, and the plugin graphs' replay (of the rows with 36 radar features: the graphs serve raw sweeps).

Training, per row: one FusionTrainer.step_fused_nhwc(update=False) with the row's backward and dropout against the oracle's
autograd on the same frame and masks (read back through tc_dropout_mask), check_grads_against_g8 at 2e-3 on the oracle's
GradStats; ReLU ties as variant_pairs_rig.influential_ties sets them apart, only where the plain oracle fails; the
deterministic rows twice: gradients bit for bit, losses within 2e-6 x max(1, |loss|) of each other and both to the oracle.

tests/test_variant_pairs_host.py holds the tables and the frames on the CPU.  pytest -m gpu -s prints the measured
differences (recorded in DESIGN.md)."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import num_cams_rig as NR
import radar_heads_rig as RR
import variant_pairs_rig as VP
from head_variant_rig import T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O

pytestmark = pytest.mark.gpu

INFERENCE_IDS = ['%02d-%s' % (i, VP.row_id(r)) for i, r in enumerate(VP.INFERENCE_ROWS)]
TRAINING_IDS = ['%02d-%s' % (i, VP.row_id(r)) for i, r in enumerate(VP.TRAINING_ROWS)]


def hs_tol(row):
    return R.HS_TOL_F16X2 if row['path'].startswith('f16x2') and row['num_points'] > 1 else R.E2E_TOL


def run_row(head, row, rows_per_sample):
    """one launch of the row's samples (each its own maps, cameras and radar rows, as CUDA tensors) under the row's path"""
    geoms = [VP.ring(row, b) for b in range(row['samples'])]
    head.outputs = row['outputs']
    try:
        return NR.run_head(head, row['num_cams'], VP.feats(row), [gpu(r) for r in rows_per_sample], geoms, **VP.PATHS[row['path']])
    finally:
        head.outputs = 'fusion'


# ---- 1. inference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(VP.INFERENCE_ROWS)), ids=INFERENCE_IDS)
def test_inference_row_against_oracle(T, i):
    row = VP.INFERENCE_ROWS[i]
    oracles = [VP.oracle_row(row, b) for b in range(row['samples'])]                  # (CPU: before the GPU is touched)
    head = R.make_head(T, **VP.variant(row))[0]
    assert head.cam_pregather_supported() == (row['num_cams'] <= 8 and row['num_levels'] == 4)
    outs = run_row(head, row, [o['rows'] for o in oracles])
    levels, L = outs['all_cls_scores'].shape[0], row['num_fusion_layers']
    assert levels == (6 + L if row['outputs'] == 'all' else L)
    assert tuple(outs['all_cls_scores'].shape[1:]) == (row['samples'], row['num_query'], row['num_classes'])
    for b, o in enumerate(oracles):
        one = NR.sample(outs, b)
        fusion = dict(one, all_cls_scores=one['all_cls_scores'][levels - L:], all_bbox_preds=one['all_bbox_preds'][levels - L:])
        aux, dbg = fusion['aux'], o['dbg']
        want_hits = np.stack([R._np(h) for h in dbg['hit_counts']])
        agree = np.all(R._np(aux['radar_hit_counts'][:, 0]) == want_hits, axis=0)
        print('%s sample %d: gate margin on this CPU %.6e m' % (INFERENCE_IDS[i], b, o['margin']))
        print('%s sample %d: max|hip - oracle| refs %.2e, states %.2e, scores %.2e, boxes %.2e on %d of %d rows whose gates agree' % (
            INFERENCE_IDS[i], b, float((aux['inter_references'].cpu() - dbg['inter_refs']).abs().max()),
            float((aux['inter_states'].cpu() - dbg['hs']).abs().max()),
            float((fusion['all_cls_scores'][:, 0].cpu() - o['want']['all_cls_scores'][:, 0])[:, agree].abs().max()),
            float((fusion['all_bbox_preds'][:, 0].cpu() - o['want']['all_bbox_preds'][:, 0])[:, agree].abs().max()),
            int(agree.sum()), len(agree)))
        assert int((R._np(aux['radar_hit_counts'][0, 0]) > 0).sum()) > 0
        R.check_against_oracle(fusion, o['want'], dbg, hs_tol(row), refs_initial=not row['with_box_refine'])
        if row['outputs'] == 'all':
            cls, box = O.decoder_outputs(o['sd'], dbg['hs'], dbg['init_ref'], dbg['inter_refs'], list(VP.ring(row, b).pc_range))
            for name, got, want in (('decoder logits', one['all_cls_scores'][:6, 0], cls[:, 0]), ('decoder boxes', one['all_bbox_preds'][:6, 0], box[:, 0])):
                print('   %s: max|hip - oracle| %.2e' % (name, float((got.cpu() - want).abs().max())))
                R.assert_all_but_two_queries(got.cpu().numpy(), want.numpy(), R.E2E_TOL, name)


# ---- 2. invariants that need no oracle, on the rows with the most non-default keys -----------------------------------------------------
MOST = sorted(range(len(VP.INFERENCE_ROWS)), key=lambda i: (-VP.non_default_keys(VP.INFERENCE_ROWS[i]), i))
# the plugin graphs serve raw sweeps only, which a head takes at 36 features (plugin_graph.eligible): of those rows
GRAPHS = [i for i in MOST if VP.INFERENCE_ROWS[i]['radar_in_dims'] == 36][:3]
MOST = MOST[:3]


def _rows_of(row, seeds):
    """[n, F] rows as the row's heads take them, one frame per seed (around sample 0's gate centres)"""
    return [VP.frame_rows(row, 0, s)[0] for s in seeds]


@pytest.mark.parametrize('i', MOST, ids=[INFERENCE_IDS[i] for i in MOST])
def test_frame_of_nine_is_its_own(T, i):
    row = VP.INFERENCE_ROWS[i]
    R.check_frame_of_nine(R.make_head(T, **VP.variant(row))[0], shapes=R.TINY[:row['num_levels']], refs_initial=not row['with_box_refine'],
                          geometry=VP.ring(row), num_cams=row['num_cams'], radar=_rows_of(row, range(60, 69)))


@pytest.mark.parametrize('i', GRAPHS, ids=[INFERENCE_IDS[i] for i in GRAPHS])
def test_plugin_graph_replay_is_the_eager_entry(T, i):
    row = VP.INFERENCE_ROWS[i]
    R.check_plugin_graph_replay(R.make_head(T, **VP.variant(row))[0], R.make_head(T, **VP.variant(row))[0],
                                shapes=R.TINY[:row['num_levels']], geometry=VP.ring(row), num_cams=row['num_cams'])


# ---- 3. training ------------------------------------------------------------------------------------------------------------------
def iteration(T, row):
    """One FusionTrainer.step_fused_nhwc(update=False) of a fresh head of the row on the row's frame
    -> (losses, {name: gradient or None} of the trainable parameters, the dropout seed, the head)"""
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    full, o = VP.full(row), VP.oracle_row(row)
    h = R.train_head(**VP.variant(row))
    metas = VP.ring(row).metas(1, radar=gpu(o['rows']))
    tokens, pad_mult = h.radar_tokens(metas, R.dev())
    boxes, labels = VP.ground_truth(row)
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    tr = FusionTrainer(h, dropout=row['dropout'], seed=VP.SEED, **VP.BACKWARDS[row['backward']])
    h._train_forwards = 3
    with torch.enable_grad():
        losses = tr.step_fused_nhwc([ops.to_nhwc(gpu(f)) for f in VP.feats(row)], ops.lidar2img_tensor(metas, R.dev()),
                                    metas[0]['img_shape'][0][:2], tokens, pad_mult, [gt.to(R.dev())],
                                    [torch.from_numpy(labels).to(R.dev())], update=False)
    torch.cuda.synchronize()
    used = {n for n, _ in h.trainable_parameters()}
    assert len(used) == VP.expected_gradients(row)
    grads = {k: (p.grad.detach().cpu().clone() if (p.grad is not None and k in used) else None)
             for k, p in h.named_parameters() if R.trainable(k)}
    kept = min(len(o['kept']), full['radar_num_tokens'])
    assert np.array_equal(tokens[0, :kept].cpu().numpy(), o['kept'][:kept]) and bool((tokens[0, kept:] == 500.0).all())
    return {k: float(v) for k, v in losses.items()}, grads, getattr(tr, 'last_dropout_seed', None), h


@pytest.mark.parametrize('i', range(len(VP.TRAINING_ROWS)), ids=TRAINING_IDS)
def test_training_row_against_oracle(T, i):
    """Losses within 2e-3 x max(1, |oracle|), every trainable gradient within check_grads_against_g8's 2e-3 of the oracle's
    (its GradStats), 14 + 28 x layers of them: against the plain oracle.  Only where that fails, the frame's influential
    ReLU ties (variant_pairs_rig.influential_ties, measured on the oracle alone with the masks of this run, at most
    MAX_TIED, the others below TIE_BOUND) may be taken on the other side (matching_oracle): all losses and all gradients
    against ONE such oracle, and a tie must then have been flipped.  On the MI355X every row holds against the plain oracle."""
    row = VP.TRAINING_ROWS[i]
    what = TRAINING_IDS[i]
    VP.oracle_row(row)                                                                 # (CPU: before the GPU is touched)
    losses, grads, seed, h = iteration(T, row)
    drop = VP.dropout_masks(row, seed) if row['dropout'] else None
    if drop is not None:
        assert drop[0]['probs'].shape == (row['radar_num_heads'], row['num_query'], row['radar_num_tokens'])
    expected = VP.expected_gradients(row)

    def held_to(got_losses, want_losses, want, which):
        for k, v in got_losses.items():
            print('%s %s: %.6f (%s %.6f)' % (what, k, v, which, want_losses[k]))
            assert abs(v - want_losses[k]) < 2e-3 * max(1.0, abs(want_losses[k])), (k, v, want_losses[k])
        stats = R.GradStats({k: want[k] if grads[k] is not None else None for k in grads})
        print('%s: largest gradient figure %.2e (2e-3 allowed) against %s' % (what, RR.g8_figures(grads, stats), which))
        assert R.check_grads_against_g8(grads, stats, 2e-3, what, expected) == expected

    want_losses, want = VP.oracle_training(row, drop)
    try:
        held_to(losses, want_losses, want, 'the oracle')
    except AssertionError as plain:
        # a tie taken on the other side: only now, and only ties the oracle alone sets apart, within its caps
        flip, want_losses, want, rest, apart = VP.matching_oracle(row, grads, drop)
        print('%s: not the plain oracle (%s); ties set apart %s, taken on the other side %s; the others move the figures by %.2e at once' % (
            what, str(plain).splitlines()[0][:100], apart, flip, rest))
        assert len(apart) <= VP.MAX_TIED and rest < RR.TIE_BOUND, (apart, rest)
        if not flip:
            raise
        held_to(losses, want_losses, want, 'the oracle with %s on the other side' % flip)
    if row['backward'] == 'deterministic':
        # twice: gradients bit for bit; the loss scalars meet in float atomics, so they are held to
        # test_gpu_training.test_deterministic_backward_is_bit_identical_on_any_schedule's 2e-6 x max(1, |loss|) between
        # the runs, and the second run's to the oracle as the first run's
        again = iteration(T, row)
        assert again[2] == seed and sorted(again[0]) == sorted(losses)
        for k, v in again[0].items():
            print('%s %s: second run %.9g, first %.9g' % (what, k, v, losses[k]))
            assert abs(v - losses[k]) <= 2e-6 * max(1.0, abs(losses[k])), (k, v, losses[k])
            assert abs(v - want_losses[k]) < 2e-3 * max(1.0, abs(want_losses[k])), (k, v, want_losses[k])
        for k, g in grads.items():
            assert (g is None) == (again[1][k] is None) and (g is None or torch.equal(g, again[1][k])), k
