"""Detr3DCrossAtten(num_points > 1) on the MI355X: the stand-alone sampling
op, the module, and the whole head on every chain path, against the CPU oracle
with a num_points-aware cross-attention (num_points_oracle.py) patched in.
pytest -m gpu"""
import numpy as np
import pytest
import torch

import num_points_oracle as NPO
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
SMOOTH = (4, 6)
E2E_TOL = 1e-3          # test_gpu_parity.test_head_end_to_end


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture
def patched_oracle(monkeypatch):
    monkeypatch.setattr(O, 'cross_atten', NPO.cross_atten)
    return O


def dev():
    return torch.device('cuda:0')


def gpu(x):
    return torch.as_tensor(x).float().contiguous().to(dev())


@pytest.fixture(scope='module')
def T():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    return transcar_amd


def make_head(T, num_points, seed=3):
    sd_np = synth.make_state_dict(seed=seed, num_points=num_points)
    h = T.build_head(configs.head_cfg(num_points=num_points))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return h.to(dev()).eval(), O.to_torch_sd(sd_np)


@pytest.fixture(scope='module')
def head5(T):
    return make_head(T, 5)


@pytest.mark.parametrize('P', [2, 5])
def test_cam_sample_points_vs_oracle(T, P):
    rng = np.random.RandomState(31 + P)
    feats = synth.make_feats('tiny', seed=32, smooth=SMOOTH)
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    Q = 900
    ref = rng.uniform(0, 1, (1, Q, 3)).astype(np.float32)
    logits = rng.standard_normal((1, Q, 24 * P)).astype(np.float32)
    tf = [torch.from_numpy(f) for f in feats]
    want = NPO.sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, torch.from_numpy(logits))
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
        other = NPO.sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, swapped)
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
    want = NPO.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', torch.from_numpy(query),
                           torch.from_numpy(qpos), [torch.from_numpy(f) for f in feats_np],
                           torch.from_numpy(refp), PCR, l2i, HW)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


def _radar_frame():
    return synth.make_radar_frame(seed=2, n_per_radar=51)


def _oracle_head(O_, sd, feats_np, frame):
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    return O_.head_forward(sd, [torch.from_numpy(f) for f in feats_np], l2i, HW,
                           O_.build_radar_features(frame), PCR, return_debug=True)


# the decoder states on the f16x2 matrix path: at P = 5 the sampling weights are sums of five sigmoids, so the sampled
# values (and the two-plane path's absolute error, which scales with them) are up to five times those of P = 1.  Measured
# on the 32-row tiles: 3 of 1 382 400 states beyond 1e-3, the largest 1.20e-3.  The f32 paths keep
# test_head_end_to_end's 1e-3, and box codes, logits and reference points keep its tolerances on every path.
HS_TOL_F16X2 = 2e-3


def _check(outs, want, dbg, hs_tol=E2E_TOL):
    aux = outs['aux']
    np.testing.assert_allclose(aux['inter_references'].cpu().numpy(), dbg['inter_refs'].numpy(), atol=5e-5, rtol=0)
    np.testing.assert_allclose(aux['inter_states'].cpu().numpy(), dbg['hs'].numpy(), atol=hs_tol, rtol=0)
    want_hits = np.stack([h.numpy() for h in dbg['hit_counts']])
    hits = aux['radar_hit_counts'][:, 0].cpu().numpy()
    agree = np.all(hits == want_hits, axis=0)
    assert int((~agree).sum()) <= 6
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(outs[k][:, 0].cpu().numpy()[:, agree], want[k][:, 0].numpy()[:, agree],
                                   atol=E2E_TOL, rtol=0)


# (the camera pre-gather rides on the f16x2 attention core only)
PATHS = [('f32', 4, False), ('f32', 8, False), ('f32', 16, False), ('f16x2', 16, False), ('f16x2', 32, False),
         ('f16x2', 16, True), ('f16x2', 32, True)]


@pytest.mark.parametrize('matrix,rows,pregather', PATHS)
def test_head_points_paths(T, head5, patched_oracle, matrix, rows, pregather):
    """Whole head at P = 5, free-running through all nine layers, on every chain path."""
    from transcar_amd.detr3d_head import head_options
    head, sd = head5
    frame = _radar_frame()
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(patched_oracle, sd, feats_np, frame)
    head.forward_options = head_options(tile_rows=rows, matrix_path=matrix, cam_pregather=pregather)
    try:
        outs = head([gpu(f) for f in feats_np],
                    synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    _check(outs, want, dbg, HS_TOL_F16X2 if matrix == 'f16x2' else E2E_TOL)


@pytest.mark.parametrize('P', [3])
def test_head_odd_points_auto(T, patched_oracle, P):
    head, sd = make_head(T, P)
    frame = _radar_frame()
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(patched_oracle, sd, feats_np, frame)
    outs = head([gpu(f) for f in feats_np],
                synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
    _check(outs, want, dbg)


def test_points_frame_of_nine_is_its_own(T, head5):
    """One frame of a nine-frame launch (32-row tiles) is bit-identical to that frame launched alone with the
    same tile height and matrix path."""
    from transcar_amd.detr3d_head import head_options
    head, _ = head5
    l2i = synth.make_lidar2img()
    feats = [synth.make_feats('tiny', seed=40 + i, smooth=SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        many = head([gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(4)],
                    synth.make_img_metas(9, l2i, radar=frames))
        one = head([gpu(f) for f in feats[4]], synth.make_img_metas(1, l2i, radar=frames[4]))
    finally:
        head.forward_options = None
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(many[k][:, 4], one[k][:, 0]), k


# ---- against the reference's own outputs (tests/golden/make_golden_points.py) ----------------------------------------
def _gold(name):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', name))


def test_cross_atten_points_golden(T, head5):
    """Detr3DCrossAtten.forward at P = 5 against the reference (G2-P5)."""
    gold = _gold('g2_cross_atten_p5.npz')
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
def test_head_points_golden(T, patched_oracle, shapes, P, path):
    """The whole head, free-running, against the reference's outputs (G5-P5 tiny / res101, G5-P3) on the rows whose
    radar gate decisions agree with the (patched) oracle's."""
    from transcar_amd.detr3d_head import head_options
    gold = _gold('g5_head_%s_p%d.npz' % (shapes, P))
    head, sd = make_head(T, P)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(patched_oracle, sd, feats_np, frame)
    if path != 'auto':
        head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        outs = head([gpu(f) for f in feats_np], synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    aux = outs['aux']
    np.testing.assert_allclose(aux['inter_references'].cpu().numpy(), gold['inter_refs'], atol=5e-5, rtol=0)
    # the radar gate is discontinuous: compare the rows whose hit counts agree with the oracle's AND the reference's
    # (the fixture stores the hit counts of the selected rows; rebuilt to [3, Q] as test_head_end_to_end does)
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
        # and the oracle it was checked against (tests/test_num_points_golden.py) on the same rows
        assert_all_but_two_queries(got, want[k][:, 0].numpy()[:, agree], E2E_TOL, k + ' vs oracle')


def assert_all_but_two_queries(got, want, tol, what):
    """[layers, Q, D]: every query within tol but at most two, and those within 1e-2.  At res101 shapes and P = 5, two
    of the 900 queries (220, 324) carry a reference point the free-running decoder puts next to a sampling
    discontinuity: there ANY two fp32 evaluation orders part by up to 3e-3 -- measured, the oracle on two different
    CPUs against the same reference fixture: 5e-4 on one, 2.4e-3 on query 324 on the other; the library: query 220
    3.0e-3 on both matrix paths, every other query within 1e-3."""
    d = np.abs(got - want).max(axis=(0, 2))
    bad = np.where(d > tol)[0]
    assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (what, bad.tolist(), d[bad].tolist())


# ---- train mode, training, the plugin entry and the pipeline at P = 5 -------------------------------------------------
def _train_head(P):
    import transcar_amd as T_
    cfg = configs.head_cfg(num_points=P)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T_.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(3, num_points=P).items()})
    return h.to(dev()).freeze_decoder().set_dropout(0.0)


def _g8_frame():
    g5 = _gold('g5_head_tiny_p5.npz')
    feats = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    metas = synth.make_img_metas(1, l2i)
    metas[0]['radar'] = frame
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    return [gpu(f) for f in feats], metas, gt.to(dev()), torch.from_numpy(labels).to(dev()), feats, l2i


def test_training_iteration_points_gradients_match_reference(T):
    """One FusionTrainer iteration (frozen P = 5 decoder -> radar stack -> loss -> backward) against the reference's
    gradients (G8-P5), 2e-3 as test_training's oracle-vs-reference check."""
    from test_training import check_grads_against_g8, trainable
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    g8 = _gold('g8_train_grads_p5.npz')
    h = _train_head(5)
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
    assert check_grads_against_g8(grads, g8, 2e-3, 'fused p5') == 98


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_points_matches_reference_formula(T, patched_oracle, rows, matrix):
    """The frozen decoder's train-mode forward at P = 5 (dropout on, layer 0 not folded: the DROP instantiations of the
    chain kernels) against the oracle's decoder with the SAME masks (tc_dropout_mask), as
    test_gpu_training.test_decoder_train_mode_dropout_matches_reference_formula does at P = 1."""
    import ctypes as C
    from transcar_amd import _lib as L
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    p, seed = 0.1, 0x5EED1234ABCD
    h = _train_head(5)
    h.set_decoder_dropout(p)
    feats, metas, _, _, feats_np, l2i_np = _g8_frame()
    nhwc = ops.to_nhwc_levels(feats)
    l2i = ops.lidar2img_tensor(metas, dev())
    img_hw = metas[0]['img_shape'][0][:2]
    tokens, pad_mult = h.radar_tokens(metas, dev())
    h.train()
    opts = dict(decoder_dropout_p=p, dropout_seed=seed, tile_rows=rows, matrix_path=matrix)
    a = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=head_options(**opts))
    b = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=head_options(**opts))
    hs = a['aux']['inter_states']
    assert torch.equal(hs, b['aux']['inter_states'])
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
    sd = O.to_torch_sd(synth.make_state_dict(3, num_points=5))
    want_hs, init_ref, want_refs, _ = patched_oracle.transformer(
        sd, [torch.from_numpy(f) for f in feats_np], PCR, torch.from_numpy(l2i_np).float()[None], HW, dec_drop=dec_drop)
    np.testing.assert_allclose(a['aux']['init_reference'].cpu().numpy(), init_ref.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), want_refs.numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(hs.cpu().numpy()[:, 0], want_hs[:, :, 0].numpy(), atol=2e-3, rtol=0)


def test_plugin_graph_replay_points_is_the_eager_entry(T):
    """At P = 5 the plugin entry's captured graphs (plugin_graph.py) replay what the eager entry computes, bit for bit."""
    hg, _ = make_head(T, 5)
    he, _ = make_head(T, 5)
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


def test_frame_pipeline_points_equals_forward_nhwc(T, head5):
    """A FramePipeline of a P = 5 head gives bit for bit what forward_nhwc gives."""
    import bench
    bench._imports()
    from transcar_amd.pipeline import FramePipeline
    head, _ = head5
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
