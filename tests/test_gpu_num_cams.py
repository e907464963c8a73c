"""Detr3DCrossAtten(num_cams=N), 1 .. 16 cameras, on the MI355X: the whole head on every chain path against the CPU
oracle (told the ring's count by argument) on the ring rig of num_cams_rig.py, two samples per launch;
the decoder layers teacher-forced against fp64; the other generic corners with many cameras; the reference's 12-camera
fixtures (tests/golden/make_golden_num_cams.py); invariants that need no oracle (camera permutation, dead cameras, a
frame inside a nine-frame launch); the entries around the forward; the refusals.  Up to 8 cameras at 4 levels and one
point run the fixed-level kernels, more cameras the generic ones; cameras with index >= 8 are the new ground, and
tests/test_num_cams_host.py holds the rig to exercising them.  The shared checks, constants and the gate-aware
comparison are head_variant_rig.py's.  pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
import num_cams_rig as NR
from head_variant_rig import T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from transcar_amd import synth

pytestmark = pytest.mark.gpu

F32, F16 = 'f32-16', 'f16x2-32'          # "one f32 and one f16x2 tile height" of the cases that do not walk every path


def hs_tol(path):
    return R.HS_TOL_F16X2 if path.startswith('f16x2') else R.E2E_TOL


def batch_of_two(N, **kw):
    """The rig's two-sample launch: (maps [2, N, ...], [frame, frame], [Ring(N), Ring(N, JITTER)]) -- the second sample
    has its own maps and its own lidar2img set, so b * N + cam indexing is exercised"""
    return NR.feats(N, batch=2, **kw), [NR.frame(N, **kw)] * 2, [NR.Ring(N), NR.Ring(N, NR.JITTER)]


def check_batch_of_two(head, N, path, **kw):
    feats, frames, geoms = batch_of_two(N, **kw)
    outs = NR.run_head(head, N, feats, frames, geoms, **NR.PATHS[path])
    for b, js in enumerate((None, NR.JITTER)):
        _, _, _, want, dbg = NR.oracle(N, jitter_seed=js, **kw)
        R.check_against_oracle(NR.sample(outs, b), want, dbg, hs_tol(path), refs_initial=not kw.get('with_box_refine', True))
    return outs


# ---- 1. the free-running head against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize('path', sorted(NR.PATHS))
@pytest.mark.parametrize('N', NR.COUNTS)
def test_head_camera_counts_vs_oracle(T, N, path):
    head, _ = R.shared_head(T, **NR.variant(N))
    assert head.weights_struct().num_cams == N and head.cam_pregather_supported() == (N <= 8)
    outs = check_batch_of_two(head, N, path)
    # the pair counter: visible (query, camera) pairs of the six layers, both samples -- the oracle's count but for the
    # few projections fp32 puts on the other side of an image border
    vis = sum(int(NR.visibility(N, NR.oracle(N, jitter_seed=js)[4], js).sum()) for js in (None, NR.JITTER))
    assert abs(int(outs['aux']['sample_pairs'].item()) - vis) <= 4, (int(outs['aux']['sample_pairs'].item()), vis)


# ---- 2. the decoder layers, teacher-forced against fp64 --------------------------------------------------------------------------
_TF = {}


def tf_rig(T, N):
    if N not in _TF:
        from transcar_amd import ops
        head, sd = R.shared_head(T, **NR.variant(N))
        head.head_weights()
        feats = [torch.from_numpy(f) for f in NR.feats(N)]
        l2i = torch.from_numpy(NR.Ring(N).lidar2img()).float()[None]
        hs, init_ref, inter_refs, _ = O.transformer(sd, feats, list(R.PCR), l2i, R.HW, num_cams=N)
        _TF[N] = dict(sd=sd, sd64={k: v.double() for k, v in sd.items()}, head=head, feats=feats,
                      nhwc=[ops.to_nhwc(gpu(f)) for f in feats], l2i=l2i, hs=hs, init_ref=init_ref, inter_refs=inter_refs)
    return _TF[N]


@pytest.mark.parametrize('tile_rows,matrix', [(16, 'f32'), (32, 'f16x2')])
@pytest.mark.parametrize('N', [12, 16])
def test_decoder_layers_teacher_forced_many_cameras(T, N, tile_rows, matrix):
    """teacher_forced_checks.decoder_layers_teacher_forced (it reads the count off the head): tc_decoder_layer_tail_fwd (the
    generic kernels at N > 8) on the oracle's previous state against the fp64 evaluation of the layer -- its constants,
    and its rule of twice the fp32 oracle's own deviation from fp64, re-measured on the same inputs.  The arbiter of the
    free-running cases.  Prints the measured pairs (pytest -s; recorded in DESIGN.md section 5)."""
    from teacher_forced_checks import decoder_layers_teacher_forced
    report = decoder_layers_teacher_forced(tf_rig(T, N), tile_rows, matrix, 'ring rig, %d cameras' % N)
    assert len(report) == 6


# ---- 3. the other generic corners with many cameras ------------------------------------------------------------------------------
CORNERS = {'16x2': (16, dict(num_levels=2)),             # 32 logits: generic because of the levels
           '16x4x4': (16, dict(num_points=4)),           # 256 logits: the TC_MAX_CAM_LOGITS edge
           '12-norefine': (12, dict(with_box_refine=False))}


@pytest.mark.parametrize('path', [F32, F16])
@pytest.mark.parametrize('corner', sorted(CORNERS))
def test_generic_corners_with_many_cameras(T, corner, path):
    N, kw = CORNERS[corner]
    head, _ = R.shared_head(T, **NR.variant(N, **kw))
    w = head.weights_struct()
    assert w.num_cams * w.num_levels * max(w.num_points, 1) == {'16x2': 32, '16x4x4': 256, '12-norefine': 48}[corner]
    check_batch_of_two(head, N, path, **kw)


# ---- 4. the reference's fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['auto', F32, F16])
def test_head_twelve_cameras_golden(T, path):
    """The whole head, free-running, against the reference head built with num_cams=12 (G5-cams12, on the radar frame
    of the seed it stores).  With check_against_fixture's tie rule, as the other variants' fixtures: the oracle's
    torch.cdist cancels to some 5e-4 m at 50 m and another CPU's matrix product may take a gate decision the other way
    than the reference did where the fixture was written; the head is held to the oracle on every agreeing row."""
    gold = R.gold(NR.G5_CAMS12)
    head, sd = R.shared_head(T, **NR.variant(12))
    frame = synth.make_radar_frame(seed=int(gold['radar_seed']), n_per_radar=51, centres=gold['radar_centres'])
    feats = NR.feats(12)
    want, dbg = R.oracle_head(sd, feats, frame, key='cams12 golden', **NR.variant(12))
    outs = NR.run_head(head, 12, feats, [frame], [NR.Ring(12)], **NR.PATHS[path])
    R.check_against_fixture(outs, want, dbg, gold, tie_rule=True)


def test_training_iteration_twelve_cameras_gradients_match_reference(T):
    """FusionTrainer.step_fused_nhwc on 12 cameras against the reference's gradients (G8-cams12), 2e-3"""
    g8 = R.gold(NR.G8_CAMS12)
    assert int(g8['radar_seed']) == NR.G8_CAMS12_RADAR_SEED
    frame = R.g8_frame(NR.G5_CAMS12, radar_seed=NR.G8_CAMS12_RADAR_SEED, geometry=NR.Ring(12))
    frame['feats_np'] = NR.feats(12)                 # (g8_frame draws the configs' six cameras' maps)
    frame['feats'] = [gpu(f) for f in frame['feats_np']]
    R.check_training_iteration(frame, NR.G8_CAMS12, 'fused cams12', **NR.variant(12))


# ---- 5. invariants that need no oracle, at 12 cameras -----------------------------------------------------------------------------
PERM = [9, 0, 10, 3, 8, 5, 1, 11, 2, 7, 4, 6]       # new camera i is old camera PERM[i]: six cameras cross index 8


def _load(T, sd_np, N):
    from transcar_amd import configs
    h = T.build_head(configs.head_cfg(num_query=NR.NQ, num_cams=N))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return h.to(R.dev()).eval()


def _run(head, feats, l2i, frame, path):
    metas = synth.make_img_metas(1, l2i, radar=frame)
    from transcar_amd.detr3d_head import head_options
    head.forward_options = head_options(**NR.PATHS[path])
    try:
        outs = head([gpu(f) for f in feats], metas, aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    return outs


AW = 'transformer.decoder.layers.%d.attentions.1.attention_weights.'


def _close(a, b, path):
    """two evaluations that differ in the order of the camera sum only"""
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), b['aux']['inter_references'].cpu().numpy(), atol=R.REFS_TOL, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_states'].cpu().numpy(), b['aux']['inter_states'].cpu().numpy(), atol=hs_tol(path), rtol=0)
    assert torch.equal(a['aux']['radar_hit_counts'], b['aux']['radar_hit_counts'])
    np.testing.assert_allclose(a['all_cls_scores'].cpu().numpy(), b['all_cls_scores'].cpu().numpy(), atol=R.E2E_TOL, rtol=0)
    np.testing.assert_allclose(a['all_bbox_preds'].cpu().numpy(), b['all_bbox_preds'].cpu().numpy(), atol=R.BOX_TOL, rtol=0)
    return all(torch.equal(a[k], b[k]) for k in ('all_cls_scores', 'all_bbox_preds'))


@pytest.mark.parametrize('path', [F32, F16])
def test_camera_permutation(T, path):
    """Maps, lidar2img and the attention_weights rows permuted together: the camera sum changes its order only"""
    sd_np, feats, l2i, frame = NR.state_dict(12), NR.feats(12), NR.Ring(12).lidar2img(), NR.frame(12)
    sd_p = dict(sd_np)
    for l in range(6):
        for s in ('weight', 'bias'):
            k = AW % l + s
            sd_p[k] = np.ascontiguousarray(sd_np[k].reshape((12, 4) + sd_np[k].shape[1:])[PERM].reshape(sd_np[k].shape))
    a = _run(R.shared_head(T, **NR.variant(12))[0], feats, l2i, frame, path)
    b = _run(_load(T, sd_p, 12), [np.ascontiguousarray(f[:, PERM]) for f in feats], l2i[PERM], frame, path)
    assert int(a['aux']['sample_pairs'].item()) == int(b['aux']['sample_pairs'].item())
    _close(a, b, path)


@pytest.mark.parametrize('path', [F32, F16])
def test_dead_cameras(T, path):
    """A 12-camera head whose cameras 6 .. 11 are never visible (all-zero lidar2img: depth 0) and whose first 24
    attention_weights rows are a 6-camera head's gives that head's outputs, generic kernels against fixed-level ones.
    Measured on an MI355X: bit-identical on the 16-row f32 tiles; within the tolerances but not bit-identical on the
    32-row f16x2 tiles (printed)."""
    sd6, sd12 = NR.state_dict(6), dict(NR.state_dict(12))
    for k in sd6:
        if 'attentions.1.attention_weights' in k:
            sd12[k] = np.concatenate([sd6[k], sd12[k][24:]])
        else:
            assert sd6[k].shape == sd12[k].shape, k
            sd12[k] = sd6[k]
    feats6, l2i6, frame = NR.feats(6), NR.Ring(6).lidar2img(), NR.frame(12)
    feats12 = [np.concatenate([f, g[:, 6:]], 1) for f, g in zip(feats6, NR.feats(12))]
    l2i12 = np.concatenate([l2i6, np.zeros((6, 4, 4))])
    a = _run(_load(T, sd6, 6), feats6, l2i6, frame, path)
    b = _run(_load(T, sd12, 12), feats12, l2i12, frame, path)
    assert int(a['aux']['sample_pairs'].item()) == int(b['aux']['sample_pairs'].item())
    print('dead cameras, %s: outputs bit-identical to the six-camera head: %s' % (path, _close(a, b, path)))


@pytest.mark.parametrize('path', [F32, F16])
def test_frame_of_nine_is_its_own(T, path):
    """A frame inside a nine-frame launch is bit-identical to the frame launched alone (same tile height, same path)"""
    head, _ = R.shared_head(T, **NR.variant(12))
    feats = synth.make_feats('tiny', seed=41, batch=9, num_cams=12, smooth=R.SMOOTH)
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    geoms = [NR.Ring(12, None if i % 2 == 0 else i) for i in range(9)]
    many = NR.run_head(head, 12, feats, frames, geoms, **NR.PATHS[path])
    one = NR.run_head(head, 12, [f[4:5] for f in feats], frames[4:5], geoms[4:5], **NR.PATHS[path])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(many[k][:, 4], one[k][:, 0]), k
    assert torch.equal(many['aux']['inter_states'][:, 4], one['aux']['inter_states'][:, 0])


# ---- 6. the entries around the forward, at 12 cameras ---------------------------------------------------------------------------
def test_unfused_path_agrees(T):
    head, _ = R.shared_head(T, **NR.variant(12))
    feats, frames, geoms = batch_of_two(12)
    a = NR.run_head(head, 12, feats, frames, geoms, unfused=True)
    b = NR.run_head(head, 12, feats, frames, geoms)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), atol=R.E2E_TOL, rtol=0)
    assert int(a['aux']['sample_pairs'].item()) == int(b['aux']['sample_pairs'].item())
    for b_, js in enumerate((None, NR.JITTER)):
        _, _, _, want, dbg = NR.oracle(12, jitter_seed=js)
        R.check_against_oracle(NR.sample(a, b_), want, dbg)


def test_cam_sample_and_cross_atten_ops_many_cameras(T):
    """tc_cam_sample_fuse_fwd with its vis output and tc_cross_atten_fwd at 12 and 16 cameras, two samples"""
    rng = np.random.RandomState(77)
    Q = 150
    for N in (12, 16):
        feats = NR.feats(N, batch=2)
        l2i = torch.from_numpy(np.stack([NR.Ring(N).lidar2img(), NR.Ring(N, NR.JITTER).lidar2img()])).float()
        ref = torch.from_numpy(rng.uniform(0, 1, (2, Q, 3)).astype(np.float32))
        logits = torch.from_numpy(rng.standard_normal((2, Q, N * 4)).astype(np.float32))
        tf = [torch.from_numpy(f) for f in feats]
        want = O.weighted_sampling(tf, ref, R.PCR, l2i, R.HW, logits, N).permute(0, 2, 1)
        _, mask = O.feature_sampling(tf, ref, R.PCR, l2i, R.HW)
        nhwc = [T.ops.to_nhwc(gpu(f)) for f in feats]
        got, vis = T.ops.cam_sample_fuse(nhwc, gpu(l2i), gpu(ref), gpu(logits), R.PCR, R.HW, num_cams=N, return_mask=True)
        assert vis.shape == (2, Q, N)
        want_vis = mask[:, 0, :, :, 0, 0].numpy()
        assert want_vis[:, :, 8:].sum() > Q / 4                      # cameras from index 8 up are seen
        flips = (vis.cpu().numpy().astype(bool) != want_vis).any(2)
        assert flips.sum() <= 2
        np.testing.assert_allclose(got.cpu().numpy()[~flips], want.numpy()[~flips], atol=1e-4, rtol=1e-5)
        head, sd = R.shared_head(T, **NR.variant(N))
        name = 'transformer.decoder.layers.2.attentions.1'
        query = torch.from_numpy(rng.standard_normal((Q, 2, 256)).astype(np.float32))
        qpos = torch.from_numpy(rng.standard_normal((Q, 2, 256)).astype(np.float32))
        attn = head.transformer.decoder.layers[2].attentions[1]
        metas = [g.metas(1)[0] for g in (NR.Ring(N), NR.Ring(N, NR.JITTER))]
        out = attn(gpu(query), None, [gpu(f) for f in feats], query_pos=gpu(qpos), reference_points=gpu(ref), img_metas=metas)
        want = O.cross_atten(sd, name, query, qpos, tf, ref, R.PCR, l2i, R.HW, num_cams=N)
        keep = ~flips.T                                              # [Q, 2]
        np.testing.assert_allclose(out.cpu().numpy()[keep], want.numpy()[keep], atol=5e-5, rtol=1e-5)


def _rand_feats(N, seed):
    g = torch.Generator(device=R.dev())
    g.manual_seed(seed)
    return [torch.randn((1, N, 256, h_, w_), device=R.dev(), generator=g) for (h_, w_) in R.TINY]


def test_plugin_graph_replay_is_the_eager_entry(T):
    """head_variant_rig.check_plugin_graph_replay on twelve cameras: the graphs run the chain's own gather"""
    hg, he = R.make_head(T, **NR.variant(12))[0], R.make_head(T, **NR.variant(12))[0]
    assert not hg.cam_pregather_supported()
    he.plugin_graphs = False
    feats, geom = _rand_feats(12, 5), NR.Ring(12)
    hg(feats, geom.metas(1, radar=synth.make_radar_frame(seed=39, n_per_radar=30)))
    base = dict(hg._plugin_graphs.stats)
    for it in range(3):
        for f in feats:
            f.mul_(0.9).add_(0.01 * (it + 1))
        metas = geom.metas(1, radar=synth.make_radar_frame(seed=40 + it, n_per_radar=30))
        og, oe = hg(feats, metas), he(feats, metas)
        torch.cuda.synchronize()
        for k in ('all_cls_scores', 'all_bbox_preds'):
            assert torch.equal(og[k], oe[k]), (it, k)
    assert hg._plugin_graphs.stats['replays'] - base['replays'] >= 1


def test_one_lane_frame_pipeline_runs_the_chains_own_gather(T):
    from transcar_amd import ops, radar
    from transcar_amd.pipeline import FramePipeline
    head, _ = R.shared_head(T, **NR.variant(12))
    tok, pm = radar.pack_tokens([radar.build_radar_features(NR.frame(12))])
    inp = dict(nhwc=[ops.to_nhwc(gpu(f)) for f in NR.feats(12)], l2i=gpu(NR.Ring(12).lidar2img()[None]), hw=R.HW,
               tokens=torch.from_numpy(tok).to(R.dev()), pad_mult=pm)
    want = head.forward_nhwc(inp['nhwc'], inp['l2i'], inp['hw'], inp['tokens'], inp['pad_mult'])
    want = [want['all_cls_scores'].clone(), want['all_bbox_preds'].clone()]
    torch.cuda.synchronize()
    pipe = FramePipeline(head, [inp])
    assert pipe.options.cam_pregather == 0
    for _ in range(2):
        pipe.launch()
    pipe.synchronize()
    outs, _ = pipe.outputs[0]
    assert torch.equal(outs['all_cls_scores'], want[0]) and torch.equal(outs['all_bbox_preds'], want[1])


@pytest.mark.parametrize('outputs', ['camera', 'all'])
def test_camera_and_all_outputs(T, outputs):
    head, _ = R.make_head(T, **NR.variant(12))
    sd, feats, frame, want, dbg = NR.oracle(12)
    cls, box = O.decoder_outputs(sd, dbg['hs'], dbg['init_ref'], dbg['inter_refs'], list(R.PCR))
    head.outputs = outputs
    outs = NR.run_head(head, 12, feats, [frame], [NR.Ring(12)])
    assert outs['all_cls_scores'].shape[0] == (6 if outputs == 'camera' else 9)
    np.testing.assert_allclose(outs['all_cls_scores'][:6].cpu().numpy(), cls.numpy(), atol=R.E2E_TOL, rtol=0)
    np.testing.assert_allclose(outs['all_bbox_preds'][:6].cpu().numpy(), box.numpy(), atol=R.E2E_TOL, rtol=0)
    if outputs == 'all':
        fusion = dict(outs, all_cls_scores=outs['all_cls_scores'][6:], all_bbox_preds=outs['all_bbox_preds'][6:])
        R.check_against_oracle(fusion, want, dbg)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_camera_counts_outside_the_limit_are_refused(T):
    from transcar_amd import _lib as L, configs, ops
    from transcar_amd.detr3d_transformer import Detr3DCrossAtten
    for bad in (0, 17, True, 6.0):
        with pytest.raises(T.TransCARHipError, match='num_cams='):
            configs.head_cfg(num_cams=bad)
        with pytest.raises(T.TransCARHipError, match='num_cams='):
            Detr3DCrossAtten(num_cams=bad, num_points=1, pc_range=R.PCR)
    head, _ = R.shared_head(T, **NR.variant(12))
    w = head.head_weights()
    lib = L.lib()
    for bad in (0, 17):
        w2 = L.tc_head_weights()
        ctypes.memmove(ctypes.byref(w2), ctypes.byref(w), ctypes.sizeof(w))
        w2.num_cams = bad
        assert lib.tc_head_packed_bytes(ctypes.byref(w2)) == 0 and ('num_cams=%d' % bad) in lib.tc_last_error().decode()
        assert lib.tc_head_workspace_bytes(ctypes.byref(w2), 1, 64) == 0 and ('num_cams=%d' % bad) in lib.tc_last_error().decode()
        # the entries that take the count by itself
        Q = 40
        z = torch.zeros((1, Q, max(bad, 1) * 4), device=R.dev())
        ref = torch.full((1, Q, 3), 0.5, device=R.dev())
        nhwc = [ops.to_nhwc(gpu(f)) for f in NR.feats(1)]
        with pytest.raises(T.TransCARHipError, match='num_cams=%d' % bad):
            ops.cam_sample_fuse(nhwc, gpu(NR.Ring(1).lidar2img()[None]), ref, z, R.PCR, R.HW, num_cams=bad)
        pv = head._packed_view
        x = torch.zeros((1, Q, 256), device=R.dev())
        with pytest.raises(T.TransCARHipError, match='num_cams=%d' % bad):
            ops.decoder_layer_tail(pv.layers[2], pv.layers[3].self_attn.in_proj, nhwc, x, x, head.query_embedding.weight,
                                   gpu(NR.Ring(1).lidar2img()[None]), ref, R.PCR, R.HW, num_cams=bad, tile_rows=4, matrix_path=0)


def test_explicit_pregather_is_refused_beyond_eight_cameras(T):
    from transcar_amd.detr3d_head import head_options
    head, _ = R.shared_head(T, **NR.variant(12))
    head.forward_options = head_options(tile_rows=16, matrix_path='f16x2', cam_pregather=True)
    try:
        with pytest.raises(T.TransCARHipError, match='pre-gather.*num_cams=12|num_cams=12.*pre-gather'):
            head([gpu(f) for f in NR.feats(12)], NR.Ring(12).metas(1, radar=NR.frame(12)))
        torch.cuda.synchronize()
    finally:
        head.forward_options = None


def test_frame_of_another_rig_is_refused_before_any_launch(T):
    """11 lidar2img matrices, or maps of 11 cameras, handed to a 12-camera head: a TransCARHipError naming both numbers
    from every entry, and nothing was enqueued (the parent launched and read past the frame)"""
    from transcar_amd import ops, radar
    head, _ = R.shared_head(T, **NR.variant(12))
    frame = NR.frame(12)
    feats12, feats11 = [gpu(f) for f in NR.feats(12)], [gpu(f) for f in NR.feats(11)]
    with pytest.raises(T.TransCARHipError, match='11 lidar2img.*num_cams=12'):
        head(feats12, NR.Ring(11).metas(1, radar=frame))
    with pytest.raises(T.TransCARHipError, match='11 images.*12'):
        head(feats11, NR.Ring(12).metas(1, radar=frame))
    tok, pm = radar.pack_tokens([radar.build_radar_features(frame)])
    tok = torch.from_numpy(tok).to(R.dev())
    nhwc12, nhwc11 = [ops.to_nhwc(f) for f in feats12], [ops.to_nhwc(f) for f in feats11]
    l2i12, l2i11 = gpu(NR.Ring(12).lidar2img()[None]), gpu(NR.Ring(11).lidar2img()[None])
    with pytest.raises(T.TransCARHipError, match='11 lidar2img.*num_cams=12'):
        head.forward_nhwc(nhwc12, l2i11, R.HW, tok, pm)
    with pytest.raises(T.TransCARHipError, match='11 images.*12'):
        head.forward_nhwc(nhwc11, l2i12, R.HW, tok, pm)
    from transcar_amd.pipeline import FramePipeline
    with pytest.raises(T.TransCARHipError, match='11 lidar2img.*num_cams=12'):
        FramePipeline(head, [dict(nhwc=nhwc12, l2i=l2i11, hw=R.HW, tokens=tok, pad_mult=pm)])
    # the trainer's entry
    from transcar_amd.trainer import FusionTrainer
    th = R.train_head(**NR.variant(12))
    tr = FusionTrainer(th, dropout=0.0)
    boxes, labels = synth.make_gt(seed=7, n=24)
    gt = torch.from_numpy(boxes).to(R.dev())
    with pytest.raises(T.TransCARHipError, match='11 lidar2img.*num_cams=12'), torch.enable_grad():
        tr.step_fused_nhwc(nhwc12, l2i11, R.HW, tok, pm, [gt], [torch.from_numpy(labels).to(R.dev())], update=False)
    torch.cuda.synchronize()
