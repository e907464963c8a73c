"""Detr3DHead(with_box_refine=False) on the MI355X: the whole head on every chain path at num_points 1 and 5, against
the CPU oracle without box refinement and the reference's fixtures (tests/golden/make_golden_variants.py norefine);
the layer op without a reg branch; train mode and a training iteration; the plugin graphs, FramePipeline and
multi-frame launches.  The shared checks are head_variant_rig.py's.  pytest -m gpu"""
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import HW, PCR, SMOOTH, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from transcar_amd import synth

pytestmark = pytest.mark.gpu


def make_head(T, num_points=1, refine=False):
    """the refining head too takes the weights of with_box_refine=False: both heads use the same shared branches"""
    return R.make_head(T, num_points=num_points, with_box_refine=refine, shared_branches=True)


def head_p(T, P):
    return R.shared_head(T, num_points=P, with_box_refine=False)


def _oracle_head(sd, feats_np, frame, *key):
    """the non-refining oracle; one forward per key, for the cases that share weights, maps and radar frame"""
    return R.oracle_head(sd, feats_np, frame, with_box_refine=False, key=('norefine',) + key)


# every chain path: (matrix, tile rows, camera pre-gather, radar row order)
PATHS = [('f32', 4, False, None), ('f32', 8, False, None), ('f32', 16, False, None), ('f16x2', 16, False, None),
         ('f16x2', 32, False, None), ('f16x2', 16, True, None), ('f16x2', 32, True, None), ('f16x2', 32, False, True),
         ('f32', 4, False, True)]


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('matrix,rows,pregather,compact', PATHS)
def test_head_norefine_paths(T, P, matrix, rows, pregather, compact):
    head, sd = head_p(T, P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(sd, feats_np, frame, 'paths', P)
    outs = R.run_head(head, feats_np, frame, tile_rows=rows, matrix_path=matrix, cam_pregather=pregather,
                      radar_compact=compact)
    R.check_against_oracle(outs, want, dbg, R.HS_TOL_F16X2 if (matrix == 'f16x2' and P > 1) else R.E2E_TOL,
                           refs_initial=True)


def test_head_norefine_unfused(T):
    """The operator-by-operator cross-check path skips the reg branch below the last layer the same way."""
    head, sd = head_p(T, 1)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(sd, feats_np, frame, 'paths', 1)
    R.check_against_oracle(R.run_head(head, feats_np, frame, unfused=True), want, dbg, refs_initial=True)


def test_refining_head_differs(T):
    """The same weights with refinement give other reference points: the mode reaches the kernels."""
    head, _ = make_head(T, 1, refine=True)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    outs = R.run_head(head, synth.make_feats('tiny', seed=1, smooth=SMOOTH), frame)
    aux = outs['aux']
    assert float((aux['inter_references'][-1] - aux['init_reference']).abs().max()) > 1e-3


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
@pytest.mark.parametrize('shapes,P', [('tiny', 1), ('res101', 1), ('tiny', 5)])
def test_head_norefine_golden(T, shapes, P, path):
    """The whole head against the reference's outputs on the rows whose radar gate decisions agree with the oracle's
    and the reference's."""
    gold = R.gold('g5_head_%s%s_norefine.npz' % (shapes, '_p5' if P == 5 else ''))
    head, sd = head_p(T, P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(sd, feats_np, frame, 'golden', shapes, P)
    outs = R.run_head(head, feats_np, frame, **({} if path == 'auto' else dict(tile_rows=32, matrix_path='f16x2')))
    R.check_against_fixture(outs, want, dbg, gold, refs_initial=True)


@pytest.mark.parametrize('tile_rows,matrix', [(4, 0), (16, 2), (32, 2)])
def test_layer_tail_without_reg_branch(T, tile_rows, matrix):
    """tc_decoder_layer_tail_fwd on a layer with reg.l0.w == NULL: ref_out = ref_in bit for bit, and hs / the next
    layer's q, k, v^T exactly what the same layer with its reg branch computes."""
    from transcar_amd import ops
    hn, sd = make_head(T, 1, refine=False)
    hr, _ = make_head(T, 1, refine=True)
    hn.head_weights()
    hr.head_weights()
    pn, pr = hn._packed_view, hr._packed_view
    assert not pn.layers[2].reg.l0.w and pr.layers[2].reg.l0.w and pn.layers[5].reg.l0.w
    g = torch.Generator(device=R.dev())
    g.manual_seed(11)
    Q = 900
    attn_o = torch.randn((1, Q, 256), device=R.dev(), generator=g)
    x_in = torch.randn((1, Q, 256), device=R.dev(), generator=g)
    ref_in = torch.rand((1, Q, 3), device=R.dev(), generator=g) * 0.9 + 0.05
    nhwc = [ops.to_nhwc(gpu(f)) for f in synth.make_feats('tiny', seed=1, smooth=SMOOTH)]
    l2i = gpu(synth.make_lidar2img())[None]
    qe = hn.query_embedding.weight
    outs = []
    for pv in (pn, pr):
        outs.append(ops.decoder_layer_tail(pv.layers[2], pv.layers[3].self_attn.in_proj, nhwc, attn_o, x_in, qe, l2i,
                                           ref_in, PCR, HW, tile_rows=tile_rows, matrix_path=matrix))
    torch.cuda.synchronize()
    (hs_n, ref_n, qk_n, vt_n), (hs_r, ref_r, qk_r, vt_r) = outs
    assert torch.equal(ref_n, ref_in)
    assert float((ref_r - ref_in).abs().max()) > 1e-4
    assert torch.equal(hs_n, hs_r) and torch.equal(qk_n, qk_r) and torch.equal(vt_n, vt_r)


def test_frame_of_nine_is_its_own(T):
    """... and so are its reference points, the initial ones."""
    R.check_frame_of_nine(head_p(T, 1)[0], refs_initial=True)


# ---- train mode, training, the plugin entry and the pipeline ----------------------------------------------------------
def _g8_frame():
    return R.g8_frame('g5_head_tiny_norefine.npz')


def test_training_iteration_norefine_gradients_match_reference(T):
    """(the radar stack reads inter_references[-1], the initial reference)"""
    R.check_training_iteration(_g8_frame(), 'g8_train_grads_norefine.npz', 'fused norefine', with_box_refine=False)


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_norefine_matches_reference_formula(T, rows, matrix):
    """(the prologue's initial reference: the references are it to 1e-6, and bit for bit each other)"""
    R.check_train_mode_decoder(_g8_frame(), rows, matrix, refs_atol=1e-6, with_box_refine=False)


def test_plugin_graph_replay_norefine_is_the_eager_entry(T):
    R.check_plugin_graph_replay(make_head(T, 1)[0], make_head(T, 1)[0])


def test_frame_pipeline_norefine_equals_forward_nhwc(T):
    R.check_frame_pipeline(head_p(T, 1)[0], nlanes=2)
