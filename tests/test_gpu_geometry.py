"""The kernels at a point-cloud range and an image size that are not the configs' (head_variant_rig.GEOM: pc_range
[-30, -60, -4, 70, 36, 6], post_center_range [-40, -70, -6, 80, 45, 8], images of 640 x 1152), on the MI355X.  pytest -m gpu

Every other GPU test runs at the configs' range, whose x and y intervals are equal and centred on 0: there an x / y swap
of the offsets or extents, `2 * pc[3]` for `pc[3] - pc[0]`, `-pc[3]` for `pc[0]`, a folded 51.2 or 102.4, a range baked
in at pack time and a stale image size in a cached graph or a pipeline lane all compute what correct code computes.
The range is de-normalised in separately written places -- the camera projection (rowdev.hpp), the stand-alone row
operators (rowops.hip), the radar compaction (radar_compact.hip), the radar prologue, K_REFUPD and K_BOXSIG of the chain
(chain.hip), the training stack (train_stack.hip), the decode's range masks (decode.hip) -- and each is reached below:
the stand-alone operators, the free-running head on every chain path and both row orders, the operator path and the
module API, the decoder levels' outputs, the per-layer teacher-forced checks, a variant combination, a training
iteration and the train-mode decoder, get_bboxes, the plugin graphs, FramePipeline and a frame of nine.

tests/test_geometry_host.py shows on the CPU that the rig sees what it must and that the shared checker refuses each of
those mistakes (they move the decoder states by 3.5 to 5.7, against a tolerance of 1e-3); tests/test_geometry_golden.py
holds the oracle to the reference's fixtures.  Checkers and tolerances are head_variant_rig.py's and
teacher_forced_checks.py's, unchanged; the one case whose oracle is ill-conditioned at three queries
(test_three_levels_five_points_at_the_geometry) bounds those queries by the adverse-frame rule and says so."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import DEFAULT, GEOM, SMOOTH, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from parity_util import assert_rows_match
from teacher_forced_checks import REF_TOL, decoder_layers_teacher_forced, radar_layers_teacher_forced
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PCR = list(GEOM.pc_range)
POST = list(GEOM.post_center_range)
HW = GEOM.hw
G5, G8 = 'g5_head_tiny_geom.npz', 'g8_train_grads_geom.npz'
_CACHE = {}


def tiny_feats():
    if 'feats' not in _CACHE:
        _CACHE['feats'] = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    return _CACHE['feats']


def g5_frame():
    """G5-GEOM's radar frame: 255 points around the centres the reference's decoder predicted, 219 inside the radar
    filter's fixed range"""
    return synth.make_radar_frame(seed=2, n_per_radar=51, centres=R.gold(G5)['radar_centres'])


def l2i_t():
    return torch.from_numpy(GEOM.lidar2img()).float()[None]


@pytest.fixture(scope='module')
def head(T):
    h, sd = R.shared_head(T, geometry=GEOM)
    assert list(h.pc_range) == PCR and list(h.bbox_coder.post_center_range) == POST
    return h, sd


def oracle_g5(sd):
    return R.oracle_head(sd, tiny_feats(), g5_frame(), key='g5 geom', geometry=GEOM)


# ---- the stand-alone operators -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', [1, 3])
def test_cam_sample_fuse_vs_oracle(T, P):
    """tc_cam_sample_fuse_fwd (P = 1) and tc_cam_sample_fuse_points_fwd (P = 3): the camera projection of rowdev.hpp."""
    rng = np.random.RandomState(31 + P)
    feats = synth.make_feats('tiny', seed=32, smooth=SMOOTH)
    Q = 900
    ref = rng.uniform(0, 1, (1, Q, 3)).astype(np.float32)
    logits = rng.standard_normal((1, Q, 24 * P)).astype(np.float32)
    tf = [torch.from_numpy(f) for f in feats]
    want = O.weighted_sampling(tf, torch.from_numpy(ref), PCR, l2i_t(), HW, torch.from_numpy(logits)).permute(0, 2, 1)
    _, mask = O.feature_sampling(tf, torch.from_numpy(ref), PCR, l2i_t(), HW)
    seen = mask[0, 0, :, :, 0, 0].numpy().sum(1)
    assert (seen == 0).sum() >= 20 and (seen == 1).sum() >= 20 and (seen >= 2).sum() >= 20
    nhwc = [T.ops.to_nhwc(gpu(f)) for f in feats]
    got, vis = T.ops.cam_sample_fuse(nhwc, gpu(l2i_t()), gpu(ref), gpu(logits), PCR, HW, return_mask=True, num_points=P)
    flips = (vis[0].cpu().numpy().astype(bool) != mask[0, 0, :, :, 0, 0].numpy()).any(1)
    assert flips.sum() <= 1
    np.testing.assert_allclose(got[0].cpu().numpy()[~flips], want[0].numpy()[~flips], atol=1e-4, rtol=1e-5)


def test_cross_atten_vs_reference_and_oracle(T, head):
    """Detr3DCrossAtten.forward (tc_cross_atten_fwd, the module's OWN pc_range) against the reference (G2-GEOM)."""
    gold = R.gold('g2_cross_atten_geom.npz')
    h, sd = head
    rng = np.random.RandomState(21)
    feats_np = synth.make_feats('tiny', seed=22)
    query = rng.standard_normal((900, 1, 256)).astype(np.float32)
    qpos = rng.standard_normal((900, 1, 256)).astype(np.float32)
    refp = rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32)
    attn = h.transformer.decoder.layers[2].attentions[1]
    assert list(attn.pc_range) == PCR
    out = attn(gpu(query), None, [gpu(f) for f in feats_np], query_pos=gpu(qpos), reference_points=gpu(refp),
               img_metas=GEOM.metas(1))
    np.testing.assert_allclose(out.cpu().numpy()[::4], gold['out'], atol=5e-5, rtol=1e-5)
    want = O.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', torch.from_numpy(query), torch.from_numpy(qpos),
                         [torch.from_numpy(f) for f in feats_np], torch.from_numpy(refp), PCR, l2i_t(), HW)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


def test_refine_reference_vs_fp64(T):
    """tc_refine_reference_fwd: sigmoid(tmp[0, 1, 4] + inverse_sigmoid(ref)) in normalised space -- the entry takes no
    range and must not depend on one (its kernel also writes the metre box of HEAD:287-293 for the operator path, which
    test_head_operator_path reaches).  Bound: twice the fp32 torch formula's own deviation from fp64 on these inputs
    plus 1e-6 (the adverse-frame rule), at most REF_TOL."""
    rng = np.random.RandomState(5)
    M = 1000                                           # four blocks of 256, the last one partial
    tmp = (rng.standard_normal((M, 10)) * 0.5).astype(np.float32)
    ref = rng.uniform(0.02, 0.98, (M, 3)).astype(np.float32)
    ref[0], ref[1], ref[2] = 0.0, 1.0, 1e-6            # the clamp of inverse_sigmoid (eps 1e-5)

    def formula(t, r):
        return (t[:, [0, 1, 4]] + O.inverse_sigmoid(r)).sigmoid()
    want = formula(torch.from_numpy(tmp).double(), torch.from_numpy(ref).double())
    dev32 = float((formula(torch.from_numpy(tmp), torch.from_numpy(ref)).double() - want).abs().max())
    got = T.ops.refine_reference(gpu(tmp), gpu(ref)).cpu().double()
    d = float((got - want).abs().max())
    print('refine_reference: max|hip - fp64| %.3g, fp32 formula %.3g' % (d, dev32))
    assert d <= min(REF_TOL, 2 * dev32 + 1e-6), (d, dev32)


def test_radar_reference_l1_is_exact(T):
    """tc_radar_reference_l1: x, y = fadd(fmul(ref, extent), offset) in fp32, two roundings as the kernel is written
    (these feed the distance gate); z stays normalised (HEAD:598).  One rounding (the compiler's
    contraction of the product and the sum into v_fma_f32) moves 759 of these 1 800 values by one fp32 spacing, up to
    3.8e-6 m."""
    from transcar_amd import autograd_ops as A
    rng = np.random.RandomState(6)
    ref = rng.uniform(0, 1, (1, 900, 3)).astype(np.float32)
    ref[0, 0], ref[0, 1] = 0.0, 1.0
    pc = np.asarray(PCR, np.float32)
    cxy, addref = A.radar_reference_l1(gpu(ref), PCR)
    want = np.stack([(ref[..., 0] * np.float32(pc[3] - pc[0])).astype(np.float32) + pc[0],
                     (ref[..., 1] * np.float32(pc[4] - pc[1])).astype(np.float32) + pc[1]], -1)
    assert want.dtype == np.float32
    np.testing.assert_array_equal(cxy.cpu().numpy(), want)
    np.testing.assert_array_equal(addref.cpu().numpy()[..., :2], want)
    np.testing.assert_array_equal(addref.cpu().numpy()[..., 2], ref[..., 2])
    assert want[0, 1].tolist() == [70.0, 36.0] and want[0, 0].tolist() == [-30.0, -60.0]


# ---- one gate centre at every site --------------------------------------------------------------------------------------------
def two_roundings(refs):
    """[Q, 3] fp32 reference points -> [Q, 2] x, y in metres as fadd(fmul(ref, extent), offset) in fp32"""
    pc = np.asarray(PCR, np.float32)
    return np.stack([(refs[:, c] * np.float32(pc[3 + c] - pc[c])).astype(np.float32) + pc[c] for c in (0, 1)], -1)


def zero_final_reg_head(T, train=False):
    """The geometry's head with seed 3's weights, the last Linear of fusion layer 1's box branch zeroed: the branch gives
    0, so the layer's box carries the centre it was added to (HEAD:596-600) bit for bit -- x, y in metres, z normalised."""
    sd_np = synth.make_state_dict(seed=3)
    sd_np['final_reg.4.weight'][:] = 0
    sd_np['final_reg.4.bias'][:] = 0
    h = T.build_head(configs.head_cfg(**R.variant_kw(geometry=GEOM)))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    h = h.to(R.dev())
    return h.freeze_decoder().set_dropout(0.0) if train else h.eval()


def test_every_site_computes_the_same_gate_centre(T, monkeypatch):
    """Fusion layer 1 gates on, and adds to its box, the de-normalised last reference point.  It is computed in three
    separately written places -- tc_radar_reference_l1 (the operator path, the training stack, and the centre the
    backward chain re-evaluates the forward's gate from), the chains' radar prologue (inference and the fused training
    forward) and the compaction -- and all of them must give the same bits: two roundings, as torch.  With a zeroed box
    branch the level-0 box IS that centre, so every path's is compared exactly with fadd(fmul(ref, extent), offset) of
    the path's own reference points: the chains on every tile height, both matrix paths and both row orders, the operator
    path, and the fused training forward of FusionTrainer.  (The compaction's centre only decides
    which rows are gathered: both row orders give the same hit counts and the same bits.)"""
    h = zero_final_reg_head(T)
    frame = g5_frame()

    def check(box, refs, what):
        box, refs = box.cpu().numpy(), refs.cpu().numpy()
        np.testing.assert_array_equal(box[:, :2], two_roundings(refs), err_msg=what)
        np.testing.assert_array_equal(box[:, 4], refs[:, 2], err_msg=what)

    runs = {}
    for rows, matrix in [(4, 'f32'), (8, 'f32'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2')]:
        for compact in (False, True):
            o = R.run_head(h, tiny_feats(), frame, geometry=GEOM, tile_rows=rows, matrix_path=matrix, radar_compact=compact)
            check(o['all_bbox_preds'][0, 0], o['aux']['inter_references'][-1, 0], (rows, matrix, compact))
            runs[rows, matrix, compact] = o
        a, b = runs[rows, matrix, False], runs[rows, matrix, True]
        assert torch.equal(a['aux']['radar_hit_counts'], b['aux']['radar_hit_counts']), (rows, matrix)
        assert torch.equal(a['all_bbox_preds'], b['all_bbox_preds']), (rows, matrix)
    assert int((runs[4, 'f32', False]['aux']['radar_hit_counts'][0] > 0).sum()) >= 100
    o = R.run_head(h, tiny_feats(), frame, geometry=GEOM, unfused=True)
    check(o['all_bbox_preds'][0, 0], o['aux']['inter_references'][-1, 0], 'operator path')

    # training: the fused forward, whose backward reads tc_radar_reference_l1's centre
    from transcar_amd import autograd_ops, device_loss, ops
    from transcar_amd.trainer import FusionTrainer
    ht = zero_final_reg_head(T, train=True)
    f = R.g8_frame(G5, radar_seed=int(R.gold(G8)['radar_seed']), geometry=GEOM)
    nhwc = [ops.to_nhwc(x) for x in f['feats']]
    l2i = ops.lidar2img_tensor(f['metas'], R.dev())
    tokens, pad_mult = ht.radar_tokens(f['metas'], R.dev())
    seen = {}
    tr = FusionTrainer(ht, dropout=0.0)
    assert tr.chain_forward
    decoder, loss = tr._decoder_forward, device_loss.detr_loss_device

    def decoder_forward(*a, **kw):
        out = decoder(*a, **kw)
        seen['refs'] = out['aux']['inter_references'][-1, 0].clone()
        return out

    def detr_loss(head, all_cls, all_box, *a, **kw):
        seen['box'] = all_box[0, 0].detach().clone()
        return loss(head, all_cls, all_box, *a, **kw)
    monkeypatch.setattr(tr, '_decoder_forward', decoder_forward)
    monkeypatch.setattr(device_loss, 'detr_loss_device', detr_loss)
    with torch.enable_grad():
        tr.step_fused_nhwc(nhwc, l2i, GEOM.hw, tokens, pad_mult, [f['gt']], [f['gt_labels']], update=False)
    torch.cuda.synchronize()
    check(seen['box'], seen['refs'], 'fused training forward')
    cxy, _ = autograd_ops.radar_reference_l1(seen['refs'][None].contiguous(), PCR)
    assert torch.equal(cxy[0], seen['box'][:, :2])            # the centre the backward re-evaluates the gate from


# ---- the free-running head ---------------------------------------------------------------------------------------------------
PATHS = [(0, None), (4, 'f32'), (16, 'f16x2'), (16, 'f32'), (32, 'f16x2')]


def hs_tol(matrix):
    return R.HS_TOL_F16X2 if matrix == 'f16x2' else R.E2E_TOL


def check_last_box_centre(outs):
    """The last decoder box in metres (HEAD:287-293; the operator path: rowops.hip's ref_update_kernel, the chains:
    K_BOXSIG) de-normalises the run's OWN last reference points: columns 0, 1, 4 against their fp64 de-normalisation,
    within BOX_TOL whatever the free-running decoder did before (fp32 spacing at 70 m: 7.6e-6)."""
    aux = outs['aux']
    refs_m = O.denormalised_refs(aux['inter_references'][-1].cpu().double(), PCR)
    d = float((aux['last_box'].cpu().double()[..., [0, 1, 4]] - refs_m).abs().max())
    assert d <= R.BOX_TOL, d


@pytest.mark.parametrize('rows,matrix', PATHS)
def test_head_paths_vs_oracle_and_reference(T, head, rows, matrix):
    """All nine layers, free-running, on G5-GEOM's frame: against the oracle and against the reference's outputs."""
    h, sd = head
    want, dbg = oracle_g5(sd)
    opts = dict(tile_rows=rows, matrix_path=matrix) if rows else {}
    outs = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, **opts)
    R.check_against_oracle(outs, want, dbg, hs_tol(matrix))
    R.check_against_fixture(outs, want, dbg, R.gold(G5))
    check_last_box_centre(outs)


@pytest.mark.parametrize('compact', [False, True], ids=['order1', 'order2'])
@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (32, 'f16x2')])
def test_head_row_orders(T, head, rows, matrix, compact):
    """Both row orders of the radar chain: order2 runs the compaction (radar_compact.hip), which de-normalises the
    reference points itself."""
    h, sd = head
    want, dbg = oracle_g5(sd)
    outs = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, tile_rows=rows, matrix_path=matrix, radar_compact=compact)
    R.check_against_oracle(outs, want, dbg, hs_tol(matrix))


@pytest.mark.parametrize('rows', [16, 32])
def test_head_camera_pregather(T, head, rows):
    h, sd = head
    want, dbg = oracle_g5(sd)
    on = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, tile_rows=rows, matrix_path='f16x2', cam_pregather=True)
    R.check_against_oracle(on, want, dbg, R.HS_TOL_F16X2)
    off = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, tile_rows=rows, matrix_path='f16x2')
    for k in ('all_cls_scores', 'all_bbox_preds'):              # (bit-identical outputs: DESIGN.md section 5)
        assert torch.equal(on[k], off[k]), k


def test_head_operator_path(T, head):
    h, sd = head
    want, dbg = oracle_g5(sd)
    outs = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, unfused=True)
    R.check_against_oracle(outs, want, dbg)
    check_last_box_centre(outs)


def test_module_api_vs_oracle(T, head):
    """Detr3DTransformer.forward, operator by operator with each Detr3DCrossAtten's own range."""
    h, _ = head
    _, want_hs, want_init, want_refs = R.oracle_trace(geometry=GEOM)
    hs, init_ref, inter_refs = h.transformer([gpu(f) for f in tiny_feats()], h.query_embedding.weight,
                                             reg_branches=h.reg_branches, img_metas=GEOM.metas(1))
    np.testing.assert_allclose(init_ref.cpu().numpy(), want_init.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(inter_refs.cpu().numpy(), want_refs.numpy(), atol=R.REFS_TOL, rtol=0)
    np.testing.assert_allclose(hs.permute(0, 2, 1, 3).cpu().numpy(), want_hs.numpy(), atol=R.E2E_TOL, rtol=0)


def test_module_api_reads_the_maps_of_this_call(T, head):
    """Two calls of the module API whose maps sit at the same addresses with the same shapes and versions -- the next
    frame in blocks the allocator hands out again, or a captured backbone writing into the same tensors -- each sample
    their own maps: the NCHW -> NHWC cache of detr3d_transformer.py lives for one decoder forward (a key of addresses,
    versions and shapes would serve the maps of the call before)."""
    h, sd = head
    rng = np.random.RandomState(21)
    first, second = synth.make_feats('tiny', seed=22), synth.make_feats('tiny', seed=23)
    query, qpos = gpu(rng.standard_normal((900, 1, 256))), gpu(rng.standard_normal((900, 1, 256)))
    refp = rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32)
    attn = h.transformer.decoder.layers[2].attentions[1]
    feats = [gpu(f) for f in first]
    key = [(f.data_ptr(), f._version) for f in feats]

    def run():
        return attn(query, None, feats, query_pos=qpos, reference_points=gpu(refp), img_metas=GEOM.metas(1)).cpu().numpy()

    def want(maps):
        return O.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', query.cpu(), qpos.cpu(),
                             [torch.from_numpy(f) for f in maps], torch.from_numpy(refp), PCR, l2i_t(), HW).numpy()
    np.testing.assert_allclose(run(), want(first), atol=5e-5, rtol=1e-5)
    for f, g in zip(feats, second):
        f.data.copy_(torch.from_numpy(g))                     # (.data: the version counter of `f` stays)
    assert key == [(f.data_ptr(), f._version) for f in feats]
    assert np.abs(want(second) - want(first)).max() > 0.1
    np.testing.assert_allclose(run(), want(second), atol=5e-5, rtol=1e-5)
    # and through the decoder, which converts once for its six layers: the second frame's trace, not the first's
    hs2 = h.transformer(feats, h.query_embedding.weight, reg_branches=h.reg_branches, img_metas=GEOM.metas(1))[0]
    for f, g in zip(feats, tiny_feats()):
        f.data.copy_(torch.from_numpy(g))
    hs, _, inter_refs = h.transformer(feats, h.query_embedding.weight, reg_branches=h.reg_branches, img_metas=GEOM.metas(1))
    _, want_hs, _, want_refs = R.oracle_trace(geometry=GEOM)
    assert float((hs2 - hs).abs().max()) > 0.1
    np.testing.assert_allclose(inter_refs.cpu().numpy(), want_refs.numpy(), atol=R.REFS_TOL, rtol=0)
    np.testing.assert_allclose(hs.permute(0, 2, 1, 3).cpu().numpy(), want_hs.numpy(), atol=R.E2E_TOL, rtol=0)


# ---- the decoder levels' own outputs (K_BOXSIG, K_REFUPD) --------------------------------------------------------------------
def normalised(box):
    lo, hi = box.new_tensor(PCR[:3]), box.new_tensor(PCR[3:])
    return (box[..., [0, 1, 4]] - lo) / (hi - lo)


@pytest.mark.parametrize('rows,matrix', [(0, None), (16, 'f32'), (32, 'f16x2')])
def test_decoder_levels_vs_reference_and_oracle(T, head, rows, matrix):
    """outputs='all': the six decoder levels against G10-GEOM and the oracle, the three fusion levels behind them."""
    h, sd = head
    fixture = R.gold('g10_decoder_outputs_tiny_geom.npz')
    o_cls, o_box = R.oracle_outputs(geometry=GEOM)
    opts = dict(tile_rows=rows, matrix_path=matrix) if rows else {}
    h.outputs = 'all'
    try:
        outs = R.run_head(h, tiny_feats(), g5_frame(), geometry=GEOM, **opts)
    finally:
        h.outputs = 'fusion'
    assert outs['all_cls_scores'].shape == (9, 1, 900, 10) and outs['all_bbox_preds'].shape == (9, 1, 900, 10)
    for name, got, gold_, orc in (('logits', outs['all_cls_scores'][:6], fixture['dec_cls'], o_cls),
                                 ('boxes', outs['all_bbox_preds'][:6], fixture['dec_box'], o_box)):
        got = got[:, 0].cpu().numpy()
        print('%s: max|hip - reference| %.3g, max|hip - oracle| %.3g' % (name, np.abs(got - gold_[:, 0]).max(),
                                                                        np.abs(got - orc[:, 0]).max()))
        R.assert_all_but_two_queries(got, gold_[:, 0], R.E2E_TOL, name + ' vs reference')
        R.assert_all_but_two_queries(got, orc[:, 0], R.E2E_TOL, name + ' vs oracle')
    # level l's centre IS the refined reference point of level l: each side within REF_TOL of the fp64 value
    d = float((normalised(outs['all_bbox_preds'][:6]) - outs['aux']['inter_references']).abs().max())
    print('max|normalised centre - inter_references| = %.3g' % d)
    assert d <= 2 * REF_TOL, d
    want, dbg = oracle_g5(sd)
    fusion = dict(outs, all_cls_scores=outs['all_cls_scores'][6:], all_bbox_preds=outs['all_bbox_preds'][6:])
    R.check_against_oracle(fusion, want, dbg, hs_tol(matrix))


# ---- per layer, teacher-forced -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tf_rig(T, head):
    h, _ = head
    sd, hs, init_ref, inter_refs = R.oracle_trace(geometry=GEOM)
    h.head_weights()
    feats_np = tiny_feats()
    return dict(T=T, sd=sd, sd64={k: v.double() for k, v in sd.items()}, head=h, feats=[torch.from_numpy(f) for f in feats_np],
                nhwc=[T.ops.to_nhwc(gpu(f)) for f in feats_np], l2i=l2i_t(), hs=hs.permute(0, 2, 1, 3).contiguous(),
                init_ref=init_ref, inter_refs=inter_refs, pcr=PCR, hw=HW)


@pytest.mark.parametrize('rows,matrix', [(16, 'f32'), (32, 'f16x2')])
def test_layers_teacher_forced(tf_rig, rows, matrix):
    """teacher_forced_checks.py's per-layer comparisons at the geometry: every decoder layer on the oracle's previous
    state against the fp64 evaluation, then the radar chain one fusion layer at a time."""
    from transcar_amd import radar
    decoder_layers_teacher_forced(tf_rig, rows, matrix, 'teacher-forced decoder layers at the geometry')
    frame = g5_frame()
    tok_np, pad_mult = radar.pack_tokens([radar.build_radar_features(frame)])
    radar_layers_teacher_forced(tf_rig, O.build_radar_features(frame), tok_np, pad_mult, rows, matrix, oracle_g5(tf_rig['sd']))


# ---- a variant combination ---------------------------------------------------------------------------------------------------
def test_three_levels_five_points_at_the_geometry(T):
    """num_points = 5, num_levels = 3 on the 32-row path (the points instantiation of the projection); oracle only.

    On this rig the ORACLE is ill-conditioned at three queries: its fp32 decoder parts from the fp64 evaluation of the
    same decoder by 4.15e-3 (query 374), 1.29e-3 (548) and 1.15e-3 (442) in the states and 3.4e-3 / 7.5e-4 / 6.6e-4 in
    the scores and boxes behind them, every other query by at most 2.1e-4 / 1.8e-4 (measured on the CPU, and measured
    again here: a reference point next to a sampling discontinuity, where any two fp32 evaluation orders part; the
    library on an MI355X: 9 of 1 382 400 states beyond HS_TOL_F16X2, the largest by 2.90e-3).  So
    each query's bound is the adverse-frame rule's: twice the oracle's own deviation at THAT query plus the existing
    floor -- HS_TOL_F16X2 / E2E_TOL for 892 of the 900 queries to within 2e-4.  The deviations themselves are capped at
    twice the recorded 4.15e-3 / 3.4e-3: a change of the oracle cannot loosen the bounds unseen."""
    variant = dict(num_points=5, num_levels=3, geometry=GEOM)
    h, sd = R.make_head(T, **variant)
    feats_np = synth.make_feats(R.TINY[:3], seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, g5_frame(), **variant)
    hs_dev, out_dev = R.oracle_fp64_deviation(sd, feats_np, g5_frame(), want, dbg, **variant)
    worst = np.argsort(-hs_dev)[:4]
    print('fp32 oracle vs fp64, per query: states %s at %s, outputs %s' % (hs_dev[worst], worst, out_dev[worst]))
    assert int((hs_dev > 5e-4).sum()) <= 9             # the floor stays the bound of 99 % of the queries on any CPU
    assert hs_dev.max() <= 2 * 4.15e-3 and out_dev.max() <= 2 * 3.4e-3, (hs_dev.max(), out_dev.max())
    outs = R.run_head(h, feats_np, g5_frame(), geometry=GEOM, tile_rows=32, matrix_path='f16x2')
    d = (outs['aux']['inter_states'].cpu() - dbg['hs']).abs().amax(dim=(0, 1, 3)).numpy()
    print('max|hip - oracle| of the states at those queries %s, elsewhere %.3g' % (d[worst], np.delete(d, worst).max()))
    R.check_against_oracle(outs, want, dbg, R.HS_TOL_F16X2 + 2 * hs_dev, out_tol=R.E2E_TOL + 2 * out_dev)


# ---- training ----------------------------------------------------------------------------------------------------------------
def g8_frame():
    return R.g8_frame(G5, radar_seed=int(R.gold(G8)['radar_seed']), geometry=GEOM)


def test_training_iteration_gradients_match_reference(T):
    R.check_training_iteration(g8_frame(), G8, 'fused, geometry', geometry=GEOM)


def test_train_mode_decoder_matches_reference_formula(T):
    R.check_train_mode_decoder(g8_frame(), 16, 'f16x2', geometry=GEOM)


# ---- get_bboxes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', [1, 2], ids=['in-register', 'stream'])
def test_box_decode_kept_vs_reference_coder(T, path):
    """tc_box_decode_kept with GEOM's post_center_range on G6-GEOM's inputs, whose top 300 candidates every face of the
    range rejects some of: the rows the reference's NMSFreeCoder.decode_single keeps, exactly."""
    g = R.gold('g6_decode_geom.npz')
    kb, ks, kl, kc = T.ops.box_decode_kept(gpu(g['cls']), gpu(g['box']), POST, 300, z_shift=False, path=path)
    n = int(kc[0])
    assert n == len(g['labels'])
    np.testing.assert_array_equal(kl[0, :n].cpu().numpy(), g['labels'])
    np.testing.assert_allclose(ks[0, :n].cpu().numpy(), g['scores'], atol=1e-6, rtol=0)
    np.testing.assert_allclose(kb[0, :n].cpu().numpy(), g['bboxes'], atol=2e-5, rtol=0)
    # the kept rows are the reference's rows: the centres are copied, so they are equal bit for bit
    np.testing.assert_array_equal(kb[0, :n, :3].cpu().numpy(), g['bboxes'][:, :3])


def test_get_bboxes_vs_reference_coder(T, head):
    """Detr3DHead.get_bboxes (the coder's post_center_range, z shifted to the box bottom, HEAD:1018) on G6-GEOM's inputs
    and on the reference's own head outputs of G5-GEOM."""
    h, _ = head
    g = R.gold('g6_decode_geom.npz')
    outs = dict(all_cls_scores=gpu(g['cls'])[None], all_bbox_preds=gpu(g['box'])[None])
    b, s, l = h.get_bboxes(outs, GEOM.metas(1))[0]
    want_b = g['bboxes'].copy()
    want_b[:, 2] -= want_b[:, 5] * 0.5
    assert b.shape[0] == len(g['labels'])
    np.testing.assert_array_equal(l.cpu().numpy(), g['labels'])
    np.testing.assert_allclose(s.cpu().numpy(), g['scores'], atol=1e-6, rtol=0)
    np.testing.assert_allclose(b.cpu().numpy(), want_b, atol=2e-5, rtol=0)
    g5 = R.gold(G5)
    b, s, l = h.get_bboxes(dict(all_cls_scores=gpu(g5['all_cls_scores']), all_bbox_preds=gpu(g5['all_bbox_preds'])),
                           GEOM.metas(1))[0]
    np.testing.assert_allclose(s.cpu().numpy(), g5['dec_scores'], atol=1e-5, rtol=0)
    mine = np.concatenate([b.cpu().numpy(), s.cpu().numpy()[:, None], l.cpu().numpy()[:, None].astype(np.float32)], 1)
    gold = np.concatenate([g5['dec_boxes'], g5['dec_scores'][:, None], g5['dec_labels'][:, None].astype(np.float32)], 1)
    assert_rows_match(mine, gold, atol=2e-4, what='decoded boxes')


# ---- the plugin graphs, the pipeline, a frame of nine ------------------------------------------------------------------------
def test_plugin_graph_replay_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, geometry=GEOM)[0], R.make_head(T, geometry=GEOM)[0], geometry=GEOM)


@pytest.mark.parametrize('first', ['configs', 'geometry'])
def test_plugin_graphs_follow_the_image_size(T, first):
    """img_shape changes between calls (928 x 1600 -> 640 x 1152 -> 928 x 1600, and the converse): every call equals the
    eager entry bit for bit, so no graph captured at one image size is replayed at the other."""
    a, b = (DEFAULT, GEOM) if first == 'configs' else (GEOM, DEFAULT)
    R.check_plugin_graph_replay(R.make_head(T, geometry=GEOM)[0], R.make_head(T, geometry=GEOM)[0], geometry=[a, a, b, a])


def test_frame_pipeline_equals_forward_nhwc(T, head):
    R.check_frame_pipeline(head[0], nlanes=2, geometry=GEOM)


def test_frame_pipeline_lanes_keep_their_own_image_size(T, head):
    R.check_frame_pipeline(head[0], nlanes=2, geometry=[GEOM, DEFAULT])


def test_frame_of_nine_is_its_own(T, head):
    R.check_frame_of_nine(head[0], geometry=GEOM)
