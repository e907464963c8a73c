"""Detr3DHead(with_box_refine=False) on the MI355X: the whole head on every chain path at num_points 1 and 5, against
the CPU oracle without box refinement (box_refine_oracle.py) and the reference's fixtures
(tests/golden/make_golden_norefine.py); the layer op without a reg branch; train mode and a training iteration; the
plugin graphs, FramePipeline and multi-frame launches.  pytest -m gpu"""
import os

import numpy as np
import pytest
import torch

import box_refine_oracle as BRO
import num_points_oracle as NPO
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
SMOOTH = (4, 6)
E2E_TOL = 1e-3          # test_gpu_parity.test_head_end_to_end
HS_TOL_F16X2 = 2e-3     # test_gpu_num_points.HS_TOL_F16X2 (P = 5 on the two-plane f16 path)


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture
def oracle(monkeypatch):
    monkeypatch.setattr(O, 'transformer', BRO.transformer)
    monkeypatch.setattr(O, 'cross_atten', NPO.cross_atten)
    return O


def dev():
    return torch.device('cuda:0')


def gpu(x):
    return torch.as_tensor(x).float().contiguous().to(dev())


def _gold(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name))


@pytest.fixture(scope='module')
def T():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    return transcar_amd


def make_head(T, num_points=1, refine=False, seed=3):
    sd_np = synth.make_state_dict(seed=seed, num_points=num_points, with_box_refine=False)
    h = T.build_head(configs.head_cfg(num_points=num_points, with_box_refine=refine))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return h.to(dev()).eval(), O.to_torch_sd(sd_np)


_HEADS = {}


def head_p(T, P):
    if P not in _HEADS:
        _HEADS[P] = make_head(T, P)
    return _HEADS[P]


def _oracle_head(O_, sd, feats_np, frame):
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    return O_.head_forward(sd, [torch.from_numpy(f) for f in feats_np], l2i, HW,
                           O_.build_radar_features(frame), PCR, return_debug=True)


def _run(head, feats_np, frame, **opts):
    from transcar_amd.detr3d_head import head_options
    head.forward_options = head_options(**opts) if opts else None
    try:
        outs = head([gpu(f) for f in feats_np], synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    return outs


def _refs_are_initial(aux):
    init, refs = aux['init_reference'], aux['inter_references']
    for l in range(refs.shape[0]):
        assert torch.equal(refs[l], init), l


def _check(outs, want, dbg, hs_tol=E2E_TOL):
    aux = outs['aux']
    _refs_are_initial(aux)
    np.testing.assert_allclose(aux['inter_references'].cpu().numpy(), dbg['inter_refs'].numpy(), atol=5e-5, rtol=0)
    np.testing.assert_allclose(aux['inter_states'].cpu().numpy(), dbg['hs'].numpy(), atol=hs_tol, rtol=0)
    want_hits = np.stack([h.numpy() for h in dbg['hit_counts']])
    hits = aux['radar_hit_counts'][:, 0].cpu().numpy()
    agree = np.all(hits == want_hits, axis=0)
    assert int((~agree).sum()) <= 6
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(outs[k][:, 0].cpu().numpy()[:, agree], want[k][:, 0].numpy()[:, agree],
                                   atol=E2E_TOL, rtol=0)


# every chain path: (matrix, tile rows, camera pre-gather, radar row order)
PATHS = [('f32', 4, False, None), ('f32', 8, False, None), ('f32', 16, False, None), ('f16x2', 16, False, None),
         ('f16x2', 32, False, None), ('f16x2', 16, True, None), ('f16x2', 32, True, None), ('f16x2', 32, False, True),
         ('f32', 4, False, True)]


@pytest.mark.parametrize('P', [1, 5])
@pytest.mark.parametrize('matrix,rows,pregather,compact', PATHS)
def test_head_norefine_paths(T, oracle, P, matrix, rows, pregather, compact):
    head, sd = head_p(T, P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(oracle, sd, feats_np, frame)
    outs = _run(head, feats_np, frame, tile_rows=rows, matrix_path=matrix, cam_pregather=pregather,
                radar_compact=compact)
    _check(outs, want, dbg, HS_TOL_F16X2 if (matrix == 'f16x2' and P > 1) else E2E_TOL)


def test_head_norefine_unfused(T, oracle):
    """The operator-by-operator cross-check path skips the reg branch below the last layer the same way."""
    head, sd = head_p(T, 1)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(oracle, sd, feats_np, frame)
    _check(_run(head, feats_np, frame, unfused=True), want, dbg)


def test_refining_head_differs(T):
    """The same weights with refinement give other reference points: the mode reaches the kernels."""
    head, _ = make_head(T, 1, refine=True)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    outs = _run(head, synth.make_feats('tiny', seed=1, smooth=SMOOTH), frame)
    aux = outs['aux']
    assert float((aux['inter_references'][-1] - aux['init_reference']).abs().max()) > 1e-3


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
@pytest.mark.parametrize('shapes,P', [('tiny', 1), ('res101', 1), ('tiny', 5)])
def test_head_norefine_golden(T, oracle, shapes, P, path):
    """The whole head against the reference's outputs on the rows whose radar gate decisions agree with the oracle's
    and the reference's (test_gpu_num_points.test_head_points_golden's rule)."""
    from test_gpu_num_points import assert_all_but_two_queries
    gold = _gold('g5_head_%s%s_norefine.npz' % (shapes, '_p5' if P == 5 else ''))
    head, sd = head_p(T, P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(oracle, sd, feats_np, frame)
    outs = _run(head, feats_np, frame, **({} if path == 'auto' else dict(tile_rows=32, matrix_path='f16x2')))
    aux = outs['aux']
    _refs_are_initial(aux)
    np.testing.assert_allclose(aux['inter_references'].cpu().numpy(), gold['inter_refs'], atol=5e-5, rtol=0)
    want_hits = np.stack([h.numpy() for h in dbg['hit_counts']])
    gold_hits = np.zeros_like(want_hits)
    for i in range(3):
        rows = np.where(want_hits[i] > 0)[0]
        gold_hits[i] = want_hits[i]
        if len(rows) == int(gold['Lq'][i]):
            gold_hits[i] = 0
            gold_hits[i, rows] = gold['hit_counts%d' % i]
    hits = aux['radar_hit_counts'][:, 0].cpu().numpy()
    agree = np.all(hits == want_hits, axis=0) & np.all(hits == gold_hits, axis=0)
    assert int((~agree).sum()) <= 6
    for k in ('all_cls_scores', 'all_bbox_preds'):
        got = outs[k][:, 0].cpu().numpy()[:, agree]
        assert_all_but_two_queries(got, gold[k][:, 0][:, agree], E2E_TOL, k + ' vs reference')
        assert_all_but_two_queries(got, want[k][:, 0].numpy()[:, agree], E2E_TOL, k + ' vs oracle')


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
    g = torch.Generator(device=dev())
    g.manual_seed(11)
    Q = 900
    attn_o = torch.randn((1, Q, 256), device=dev(), generator=g)
    x_in = torch.randn((1, Q, 256), device=dev(), generator=g)
    ref_in = torch.rand((1, Q, 3), device=dev(), generator=g) * 0.9 + 0.05
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
    """One frame of a nine-frame launch (32-row tiles, radar rows reordered) is bit-identical to that frame launched
    alone with the same tile height and matrix path."""
    from transcar_amd.detr3d_head import head_options
    head, _ = head_p(T, 1)
    l2i = synth.make_lidar2img()
    feats = [synth.make_feats('tiny', seed=40 + i, smooth=SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        many = head([gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(4)],
                    synth.make_img_metas(9, l2i, radar=frames), aux=True)
        one = head([gpu(f) for f in feats[4]], synth.make_img_metas(1, l2i, radar=frames[4]), aux=True)
    finally:
        head.forward_options = None
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(many[k][:, 4], one[k][:, 0]), k
    assert torch.equal(many['aux']['inter_references'][:, 4], one['aux']['inter_references'][:, 0])
    _refs_are_initial(many['aux'])


# ---- train mode, training, the plugin entry and the pipeline ----------------------------------------------------------
def _train_head():
    import transcar_amd as T_
    cfg = configs.head_cfg(with_box_refine=False)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T_.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(3, with_box_refine=False).items()})
    return h.to(dev()).freeze_decoder().set_dropout(0.0)


def _g8_frame():
    g5 = _gold('g5_head_tiny_norefine.npz')
    feats = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    metas = synth.make_img_metas(1, l2i)
    metas[0]['radar'] = frame
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    return [gpu(f) for f in feats], metas, gt.to(dev()), torch.from_numpy(labels).to(dev()), feats, l2i


def test_training_iteration_norefine_gradients_match_reference(T):
    """One FusionTrainer iteration (frozen non-refining decoder -> radar stack reading inter_references[-1] -> loss ->
    backward) against the reference's gradients (G8 without refinement), 2e-3 as test_training's check."""
    from test_training import check_grads_against_g8, trainable
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    g8 = _gold('g8_train_grads_norefine.npz')
    h = _train_head()
    feats, metas, gt, labels, _, _ = _g8_frame()
    nhwc = [ops.to_nhwc(f) for f in feats]
    l2i = ops.lidar2img_tensor(metas, dev())
    tokens, pad_mult = h.radar_tokens(metas, dev())
    tr = FusionTrainer(h, dropout=0.0)
    with torch.enable_grad():
        losses = tr.step_fused_nhwc(nhwc, l2i, metas[0]['img_shape'][0][:2], tokens, pad_mult, [gt], [labels],
                                    update=False)
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        assert abs(float(v) - ref) < 2e-3 * max(1.0, abs(ref)), (k, float(v), ref)
    used = {n for n, _ in h.trainable_parameters()}
    grads = {k: (p.grad.clone() if (p.grad is not None and k in used) else None)
             for k, p in h.named_parameters() if trainable(k)}
    assert check_grads_against_g8(grads, g8, 2e-3, 'fused norefine') == 98


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_norefine_matches_reference_formula(T, oracle, rows, matrix):
    """The frozen decoder's train-mode forward (dropout on: layer 0 not folded, the prologue's initial reference)
    against the oracle's non-refining decoder with the SAME masks (tc_dropout_mask)."""
    import ctypes as C
    from transcar_amd import _lib as L
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    p, seed = 0.1, 0x5EED1234ABCD
    h = _train_head()
    h.set_decoder_dropout(p)
    feats, metas, _, _, feats_np, l2i_np = _g8_frame()
    nhwc = ops.to_nhwc_levels(feats)
    l2i = ops.lidar2img_tensor(metas, dev())
    img_hw = metas[0]['img_shape'][0][:2]
    tokens, pad_mult = h.radar_tokens(metas, dev())
    h.train()
    opts = dict(decoder_dropout_p=p, dropout_seed=seed, tile_rows=rows, matrix_path=matrix)
    a = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=head_options(**opts))
    hs = a['aux']['inter_states']
    _refs_are_initial(a['aux'])
    lib = L.lib()
    Q, Cd, Fd, H = h.num_query, 256, 512, 8

    def mask(site, n):
        out = torch.empty(n, dtype=torch.float32, device=dev())
        L.check(lib.tc_dropout_mask(p, seed, site, n, out.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tc_dropout_mask')
        return out.cpu()
    dec_drop = []
    for l in range(6):
        s0 = 16 + 8 * l
        dec_drop.append(dict(
            probs=mask(s0 + 0, H * Q * Q).view(H, Q, Q),
            sa=mask(s0 + 1, Q * Cd).view(Q, 1, Cd), ca=mask(s0 + 2, Q * Cd).view(Q, 1, Cd),
            ffn_h=mask(s0 + 3, Q * Fd).view(Q, 1, Fd), ffn_o=mask(s0 + 4, Q * Cd).view(Q, 1, Cd)))
    sd = O.to_torch_sd(synth.make_state_dict(3, with_box_refine=False))
    want_hs, init_ref, want_refs, _ = oracle.transformer(
        sd, [torch.from_numpy(f) for f in feats_np], PCR, torch.from_numpy(l2i_np).float()[None], HW, dec_drop=dec_drop)
    np.testing.assert_allclose(a['aux']['init_reference'].cpu().numpy(), init_ref.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), want_refs.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(hs.cpu().numpy()[:, 0], want_hs[:, :, 0].numpy(), atol=2e-3, rtol=0)


def test_plugin_graph_replay_norefine_is_the_eager_entry(T):
    hg, _ = make_head(T, 1)
    he, _ = make_head(T, 1)
    he.plugin_graphs = False
    g = torch.Generator(device=dev())
    g.manual_seed(5)
    feats = [torch.randn((1, 6, 256, h_, w_), device=dev(), generator=g) for (h_, w_) in configs.LEVEL_SHAPES['tiny']]
    hg(feats, synth.make_img_metas(1, radar=synth.make_radar_frame(seed=39, n_per_radar=30)))
    base = dict(hg._plugin_graphs.stats)
    for it in range(3):
        for f in feats:
            f.mul_(0.9).add_(0.01 * (it + 1))
        metas = synth.make_img_metas(1, radar=synth.make_radar_frame(seed=40 + it, n_per_radar=30))
        og, oe = hg(feats, metas), he(feats, metas)
        torch.cuda.synchronize()
        for k in ('all_cls_scores', 'all_bbox_preds'):
            assert torch.equal(og[k], oe[k]), (it, k)
    st = {k: v - base[k] for k, v in hg._plugin_graphs.stats.items()}
    assert st['replays'] >= 1, st


def test_frame_pipeline_norefine_equals_forward_nhwc(T):
    import bench
    bench._imports()
    from transcar_amd.pipeline import FramePipeline
    head, _ = head_p(T, 1)
    lanes = [bench.make_inputs(head, dev(), 'tiny', 1, seed=11 + i) for i in range(2)]
    want = []
    for inp in lanes:
        outs, dec = bench.one_step(head, inp)
        want.append([outs['all_cls_scores'].clone(), outs['all_bbox_preds'].clone()] + [d.clone() for d in dec])
    torch.cuda.synchronize()
    pipe = FramePipeline(head, lanes)
    for _ in range(2):
        for _ in range(2):
            pipe.launch()
    pipe.synchronize()
    for i in range(2):
        outs, dec = pipe.outputs[i]
        for a_, b_ in zip([outs['all_cls_scores'], outs['all_bbox_preds']] + list(dec), want[i]):
            assert torch.equal(a_, b_)
