"""Detr3DCrossAtten(num_levels < 4) on the MI355X: the stand-alone sampling op, the module, and the whole head on every
chain path, against the CPU oracle with a levels-aware cross-attention (num_levels_oracle.py) patched in and against
the reference's fixtures (tests/golden/make_golden_levels.py).  pytest -m gpu"""
import os

import numpy as np
import pytest
import torch

import box_refine_oracle as BRO
import num_levels_oracle as NLO
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
SMOOTH = (4, 6)
E2E_TOL = 1e-3          # test_gpu_parity.test_head_end_to_end
HS_TOL_F16X2 = 2e-3     # test_gpu_num_points.HS_TOL_F16X2
TINY, RES101 = configs.LEVEL_SHAPES['tiny'], configs.LEVEL_SHAPES['res101']
# level shapes of L levels: the first L tiny ones; ONE level is (2, 3), not level 0 (no kernel may lean on it)
LEVELS = {1: [TINY[2]], 2: TINY[:2], 3: TINY[:3]}


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture
def patched_oracle(monkeypatch):
    monkeypatch.setattr(O, 'cross_atten', NLO.cross_atten)
    return O


def dev():
    return torch.device('cuda:0')


def gpu(x):
    return torch.as_tensor(x).float().contiguous().to(dev())


def _gold(name):
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', name))


@pytest.fixture(scope='module')
def T():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    return transcar_amd


def make_head(T, nl, P=1, refine=True, seed=3):
    sd_np = synth.make_state_dict(seed=seed, num_levels=nl, num_points=P, with_box_refine=refine)
    h = T.build_head(configs.head_cfg(num_levels=nl, num_points=P, with_box_refine=refine))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return h.to(dev()).eval(), O.to_torch_sd(sd_np)


@pytest.fixture(scope='module')
def head2(T):
    return make_head(T, 2)


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
    want = NLO.sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, torch.from_numpy(logits))
    _, mask = O.feature_sampling(tf, torch.from_numpy(ref), PCR, l2i, HW)
    nhwc = [T.ops.to_nhwc(gpu(f)) for f in feats]
    got, vis = T.ops.cam_sample_fuse(nhwc, gpu(l2i), gpu(ref), gpu(logits), PCR, HW, return_mask=True, num_points=P)
    flips = (vis[0].cpu().numpy().astype(bool) != mask[0, 0, :, :, 0, 0].numpy()).any(1)
    assert flips.sum() <= 1
    np.testing.assert_allclose(got[0].cpu().numpy()[~flips], want[0].numpy()[~flips], atol=1e-4, rtol=1e-5)
    if nl > 1:
        # a wrong (camera, level) order would be caught
        swapped = torch.from_numpy(logits).view(1, Q, 6, P, nl).transpose(2, 4).reshape(1, Q, -1)
        other = NLO.sampling(tf, torch.from_numpy(ref), PCR, l2i, HW, swapped)
        assert np.abs(other[0].numpy() - want[0].numpy())[~flips].max() > 1e-2


@pytest.mark.parametrize('nl', [1, 3])
def test_cross_atten_levels_golden(T, nl):
    """Detr3DCrossAtten.forward with 1 / 3 levels against the reference (G2-L1 / -L3) and the oracle."""
    gold = _gold('g2_cross_atten_l%d.npz' % nl)
    head, sd = make_head(T, nl)
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
    want = NLO.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', torch.from_numpy(query),
                           torch.from_numpy(qpos), [torch.from_numpy(f) for f in feats_np], torch.from_numpy(refp),
                           PCR, l2i, HW)
    np.testing.assert_allclose(out.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


def _oracle_head(O_, sd, feats_np, frame):
    l2i = torch.from_numpy(synth.make_lidar2img()).float()[None]
    return O_.head_forward(sd, [torch.from_numpy(f) for f in feats_np], l2i, HW,
                           O_.build_radar_features(frame), PCR, return_debug=True)


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


# (matrix path, tile rows, unfused): None = the automatic choice
PATHS = [('f32', 4, False), ('f32', 8, False), ('f32', 16, False), ('f16x2', 16, False), ('f16x2', 32, False),
         (None, None, False), (None, None, True)]


_PATHS_ORACLE = {}


@pytest.mark.parametrize('matrix,rows,unfused', PATHS)
@pytest.mark.parametrize('nl', [1, 2, 3])
def test_head_levels_paths(T, patched_oracle, nl, matrix, rows, unfused):
    """Whole head with 1 / 2 / 3 levels, free-running through all nine layers, on every chain path and the unfused
    path, against the levels-aware oracle."""
    from transcar_amd.detr3d_head import head_options
    head, sd = make_head(T, nl)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats(LEVELS[nl], seed=1, smooth=SMOOTH)
    if nl not in _PATHS_ORACLE:             # (one oracle forward per level count: the paths share it)
        _PATHS_ORACLE[nl] = _oracle_head(patched_oracle, sd, feats_np, frame)
    want, dbg = _PATHS_ORACLE[nl]
    head.forward_options = head_options(unfused=True) if unfused else \
        head_options(tile_rows=rows, matrix_path=matrix) if matrix else None
    try:
        outs = head([gpu(f) for f in feats_np], synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    _check(outs, want, dbg, HS_TOL_F16X2 if matrix == 'f16x2' else E2E_TOL)


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


def assert_all_but_two_queries(got, want, tol, what):
    """[layers, Q, D]: every query within tol but at most two, and those within 1e-2
    (test_gpu_num_points.assert_all_but_two_queries)."""
    d = np.abs(got - want).max(axis=(0, 2))
    bad = np.where(d > tol)[0]
    assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (what, bad.tolist(), d[bad].tolist())


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
@pytest.mark.parametrize('name', sorted(G5))
def test_head_levels_golden(T, monkeypatch, name, path):
    """The whole head, free-running, against the reference's outputs (G5-L*) on the rows whose radar gate decisions
    agree with the (patched) oracle's and the reference's."""
    from transcar_amd.detr3d_head import head_options
    nl, P, refine = G5[name]
    monkeypatch.setattr(O, 'cross_atten', NLO.cross_atten)
    if not refine:
        monkeypatch.setattr(O, 'transformer', BRO.transformer)
    gold = _gold(name)
    shapes = [tuple(s) for s in gold['level_shapes']]
    head, sd = make_head(T, nl, P, refine)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    want, dbg = _oracle_head(O, sd, feats_np, frame)
    if path != 'auto':
        head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        outs = head([gpu(f) for f in feats_np], synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    aux = outs['aux']
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
    # A radar gate decision of the rig can sit within 1e-4 m of its radius (G5-L2: query 880, 2.1e-4 m in fusion layer 3):
    # where the oracle on this machine and the reference took it differently, the stored hit counts cannot say which
    # row flipped (the fixture keeps the selected rows only, and their count then differs).  Such a query departs from
    # the reference in the ORACLE too; it is left out of the comparison with the reference only -- the library is held
    # to the oracle on every agreeing row.
    tie = np.zeros(agree.shape, bool)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        tie |= np.abs(want[k][:, 0].numpy() - gold[k][:, 0]).max(axis=(0, 2)) > 1e-2
    assert int(tie.sum()) <= 2, np.where(tie)[0].tolist()
    for k in ('all_cls_scores', 'all_bbox_preds'):
        got = outs[k][:, 0].cpu().numpy()
        assert_all_but_two_queries(got[:, agree & ~tie], gold[k][:, 0][:, agree & ~tie], E2E_TOL, k + ' vs reference')
        assert_all_but_two_queries(got[:, agree], want[k][:, 0].numpy()[:, agree], E2E_TOL, k + ' vs oracle')


# ---- train mode, training, the plugin entry, the pipeline and the layer op at L = 2 ------------------------------------
def _train_head(nl):
    import transcar_amd as T_
    cfg = configs.head_cfg(num_levels=nl)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T_.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(3, num_levels=nl).items()})
    return h.to(dev()).freeze_decoder().set_dropout(0.0)


def _g8_frame():
    g5 = _gold('g5_head_tiny_l2.npz')
    feats = synth.make_feats(TINY[:2], seed=1, smooth=SMOOTH)
    l2i = synth.make_lidar2img()
    seed = int(_gold('g8_train_grads_l2.npz')['radar_seed'])       # (its own radar frame: make_golden_levels.py)
    frame = synth.make_radar_frame(seed=seed, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    metas = synth.make_img_metas(1, l2i)
    metas[0]['radar'] = frame
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    return [gpu(f) for f in feats], metas, gt.to(dev()), torch.from_numpy(labels).to(dev()), feats, l2i


def test_training_iteration_levels_gradients_match_reference(T):
    """One FusionTrainer iteration (frozen two-level decoder -> radar stack -> loss -> backward) against the reference's
    gradients (G8-L2), 2e-3 as test_training's oracle-vs-reference check."""
    from test_training import check_grads_against_g8, trainable
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    g8 = _gold('g8_train_grads_l2.npz')
    h = _train_head(2)
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
    assert check_grads_against_g8(grads, g8, 2e-3, 'fused l2') == 98


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (8, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_train_mode_decoder_levels_matches_reference_formula(T, patched_oracle, rows, matrix):
    """The frozen decoder's train-mode forward with two levels (dropout on: the DROP instantiations of the generic chain
    kernels) against the oracle's decoder with the SAME masks (tc_dropout_mask), as
    test_gpu_num_points.test_train_mode_decoder_points_matches_reference_formula does at P = 5."""
    import ctypes as C
    from transcar_amd import _lib as L
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    p, seed = 0.1, 0x5EED1234ABCD
    h = _train_head(2)
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
    sd = O.to_torch_sd(synth.make_state_dict(3, num_levels=2))
    want_hs, init_ref, want_refs, _ = patched_oracle.transformer(
        sd, [torch.from_numpy(f) for f in feats_np], PCR, torch.from_numpy(l2i_np).float()[None], HW, dec_drop=dec_drop)
    np.testing.assert_allclose(a['aux']['init_reference'].cpu().numpy(), init_ref.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), want_refs.numpy(), atol=2e-4, rtol=0)
    np.testing.assert_allclose(hs.cpu().numpy()[:, 0], want_hs[:, :, 0].numpy(), atol=2e-3, rtol=0)


def test_plugin_graph_replay_levels_is_the_eager_entry(T):
    """With two levels the plugin entry's captured graphs replay what the eager entry computes, bit for bit -- the
    camera pre-gather the entry turns on for 4 levels is off here (cam_pregather_supported): the replay runs."""
    hg, _ = make_head(T, 2)
    he, _ = make_head(T, 2)
    he.plugin_graphs = False
    assert not hg.cam_pregather_supported()
    g = torch.Generator(device=dev())
    g.manual_seed(5)
    feats = [torch.randn((1, 6, 256, h_, w_), device=dev(), generator=g) for (h_, w_) in TINY[:2]]
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


def _lane_inputs(head, seed):
    """bench.make_inputs' lane layout on the first two tiny levels"""
    import bench
    bench._imports()
    return bench.make_inputs(head, dev(), TINY[:2], 1, seed=seed)


@pytest.mark.parametrize('nlanes', [1, 3])
def test_frame_pipeline_levels_equals_forward_nhwc(T, head2, nlanes):
    """A one-lane (pre-gather default off for two levels) and a three-lane FramePipeline of a two-level head give bit
    for bit what forward_nhwc gives."""
    import bench
    from transcar_amd.pipeline import FramePipeline
    head, _ = head2
    lanes = [_lane_inputs(head, 11 + i) for i in range(nlanes)]
    want = []
    for inp in lanes:
        outs, dec = bench.one_step(head, inp)
        want.append([outs['all_cls_scores'].clone(), outs['all_bbox_preds'].clone()] + [d.clone() for d in dec])
    torch.cuda.synchronize()
    pipe = FramePipeline(head, lanes)
    assert pipe.options.cam_pregather == 0
    for _ in range(2):
        for _ in range(nlanes):
            pipe.launch()
    pipe.synchronize()
    for i in range(nlanes):
        outs, dec = pipe.outputs[i]
        for a_, b_ in zip([outs['all_cls_scores'], outs['all_bbox_preds']] + list(dec), want[i]):
            assert torch.equal(a_, b_)


@pytest.mark.parametrize('nl', [1, 3])
def test_levels_frame_of_nine_is_its_own(T, nl):
    """One frame of a nine-frame launch (32-row tiles) is bit-identical to that frame launched alone with the same
    tile height and matrix path."""
    from transcar_amd.detr3d_head import head_options
    head, _ = make_head(T, nl)
    l2i = synth.make_lidar2img()
    feats = [synth.make_feats(LEVELS[nl], seed=40 + i, smooth=SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        many = head([gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(nl)],
                    synth.make_img_metas(9, l2i, radar=frames))
        one = head([gpu(f) for f in feats[4]], synth.make_img_metas(1, l2i, radar=frames[4]))
    finally:
        head.forward_options = None
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(many[k][:, 4], one[k][:, 0]), k


def test_layer_tail_refuses_fewer_levels(T, head2):
    """tc_decoder_layer_tail_fwd stays 4 levels only: fewer are refused, naming the count."""
    from transcar_amd import ops
    head, _ = head2
    head.head_weights()
    pv = head._packed_view
    Q = 900
    z = torch.zeros((1, Q, 256), device=dev())
    ref_in = torch.full((1, Q, 3), 0.5, device=dev())
    nhwc = [ops.to_nhwc(gpu(f)) for f in synth.make_feats(TINY[:2], seed=1)]
    with pytest.raises(T.TransCARHipError, match='num_levels=2'):
        ops.decoder_layer_tail(pv.layers[2], pv.layers[3].self_attn.in_proj, nhwc, z, z, head.query_embedding.weight,
                               gpu(synth.make_lidar2img())[None], ref_in, PCR, HW, tile_rows=4, matrix_path=0)
