"""The CPU oracle with its radar fusion attention at 4 and at 16 heads (head_forward's radar_num_heads) against the
reference's fixtures of those counts (tests/golden/make_golden_radar_heads.py): the forward's outputs and hit counts, and
one training iteration's losses and gradients, with the bounds test_radar_gate_golden.py and test_fusion_depth_golden.py
apply to their fixtures.  No GPU."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import radar_heads_rig as RR
from oracle import transcar_oracle as O
from transcar_amd import synth


def _sd():
    return O.to_torch_sd(synth.make_state_dict(seed=3))


def test_the_patch_reaches_the_fusion_attention_only():
    """radar_num_heads=8 is the oracle without the argument bit for bit; at 4 / 16 heads the decoder is untouched and the
    fusion logits move by far more than any tolerance here."""
    feats, frame = R.g5_frame()
    want, wdbg = O.head_forward(_sd(), [torch.from_numpy(f) for f in feats], torch.from_numpy(synth.make_lidar2img()).float()[None],
                                R.HW, O.build_radar_features(frame), R.PCR, return_debug=True)
    got, _ = R.oracle_head(_sd(), feats, frame, radar_num_heads=8)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(got[k], want[k]), k
    outs = {8: want}
    for H in RR.HEADS:
        outs[H], dbg = R.oracle_head(_sd(), feats, frame, radar_num_heads=H)
        assert torch.equal(dbg['hs'], wdbg['hs']) and torch.equal(dbg['inter_refs'], wdbg['inter_refs'])
    for a, b in ((4, 8), (16, 8), (4, 16)):
        assert float((outs[a]['all_cls_scores'] - outs[b]['all_cls_scores']).abs().max()) > 0.1, (a, b)


@pytest.mark.parametrize('H', RR.HEADS)
def test_oracle_forward_agrees_with_the_reference(H):
    g5 = R.gold(RR.g5_name(H))
    assert int(g5['radar_num_heads']) == H
    feats, frame = RR.g5_frame(H)
    got, dbg = R.oracle_head(_sd(), feats, frame, radar_num_heads=H)
    assert int(dbg['fill_in']) == int(g5['fill_in'])
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g5['inter_refs'], atol=R.REFS_TOL, rtol=0)
    for i in range(3):                       # hit counts identical in every layer: the stored margin leaves no tie to a CPU
        rows = np.where(dbg['hit_counts'][i].numpy() > 0)[0]
        assert len(rows) == int(g5['Lq'][i]) > 32
        assert np.array_equal(dbg['hit_counts'][i].numpy()[rows], g5['hit_counts%d' % i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(got[k].numpy(), g5[k], atol=R.E2E_TOL, rtol=0)
    # the 8-head oracle computes something else on this frame: the fixture cannot be met without the count
    plain, _ = R.oracle_head(_sd(), feats, frame)
    assert float(np.abs(plain['all_cls_scores'].numpy() - g5['all_cls_scores']).max()) > 0.1
    # the margin is what the rig measures, up to the bound between two fp32 orders of the box arithmetic (BOX_TOL moves a
    # gate centre), and an order of magnitude beyond that bound: no evaluation order flips a decision of this frame
    margin, again = float(g5['gate_margin']), R.gate_margin(_sd(), feats, frame, radar_num_heads=H)
    assert margin > 10 * R.BOX_TOL and abs(margin - again) <= R.BOX_TOL, (margin, again)


def test_a_relu_tie_moves_the_gradients_of_the_forward_fixtures_frame():
    """Why the gradient fixtures have a frame of their own: on the forward fixtures' frame at 4 heads, every ReLU input
    within TIE_TAU of zero taken on the other side moves the gradients beyond the 2e-3 the gradient checks allow."""
    host = R.g8_frame('g5_head_tiny.npz', radar_seed=int(R.gold(RR.g5_name(4))['radar_seed']))
    assert RR.tie_sensitivity(host, 4) > 2e-3


@pytest.mark.parametrize('H', RR.HEADS)
def test_oracle_backward_matches_the_reference(H):
    g8 = R.gold(RR.g8_name(H))
    assert int(g8['radar_num_heads']) == H and int(g8['radar_seed']) == int(R.gold(RR.g8_name(20 - H))['radar_seed'])
    host = RR.g8_frame(H)
    # the frame keeps its gradients away from both kinds of discontinuity: a gate margin of more than four times the bound
    # between two fp32 orders of the box arithmetic (either side moves by one, and twice that), and gradients that stay
    # inside half the bound below with every ReLU input within TIE_TAU of zero taken on the other side
    sd = O.to_torch_sd(synth.make_state_dict(seed=3))
    margin = R.gate_margin(sd, host['feats_np'], host['frame'], radar_num_heads=H)
    assert margin > 4 * R.BOX_TOL and abs(margin - float(g8['gate_margin'])) <= R.BOX_TOL, margin
    ties = RR.tie_sensitivity(host, H)
    assert ties < RR.TIE_BOUND and abs(ties - float(g8['tie_sensitivity'])) < 0.25 * RR.TIE_BOUND, ties
    cut, losses, _, grads = R.oracle_training(host, radar_num_heads=H)
    for k, v in cut.items():
        assert np.abs(v.numpy() - g8[k]).max() < 5e-4, k
    assert sorted('loss__' + k.replace('.', '_') for k in losses) == sorted(k for k in g8.files if k.startswith('loss__'))
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        assert abs(v - ref) < 2e-3 * max(1.0, abs(ref)), (k, v, ref)
    assert abs(sum(losses.values()) - float(g8['total_loss'])) < 1e-4 * float(g8['total_loss'])
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'oracle rh%d' % H) == 98
