"""Detr3DHead(num_fusion_layers=N), N = 1 and 2, on the MI355X.  The fusion layers are causally ordered (level k reads
layers <= k, the row order comes from layer 0's gate), so an N-layer head with the first N layers' weights must give
levels [:N] of the three-layer head BIT FOR BIT on the same tile height and matrix path: that identity on every chain
path, the reference's fixture on levels [:N], the entry points that size their buffers by the depth (outputs='all',
get_bboxes, the plugin graphs, FramePipeline), and a training iteration against the reference's gradients
(tests/golden/make_golden_fusion_depth.py) with the trainer's other paths held to it.  Tiny level shapes, 900 queries
(28 x 32 + 4 rows), the G5 / G8 radar frames.  pytest -m gpu"""
import ctypes as C

import pytest
import torch

import head_variant_rig as R
from head_variant_rig import T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from transcar_amd import synth

pytestmark = pytest.mark.gpu

#: (tile rows, matrix path) of the chains: 4- / 8-row tiles compute in fp32 on either path, 32 rows exist on f16x2 only
PATHS = [(4, 'f32'), (4, 'f16x2'), (8, 'f32'), (8, 'f16x2'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2')]
KEYS = ('all_cls_scores', 'all_bbox_preds')
_FULL = {}


def full_outputs(T, frame_name, rows, matrix, compact, **extra):
    """The three-layer head's outputs on a frame and path, once for both depths."""
    key = (frame_name, rows, matrix, compact, tuple(sorted(extra.items())))
    if key not in _FULL:
        feats, frame = R.g5_frame()
        if frame_name == 'empty':
            frame = R.empty_frame()
        h3, _ = R.shared_head(T)
        _FULL[key] = R.run_head(h3, feats, frame, tile_rows=rows, matrix_path=matrix, radar_compact=compact, **extra)
    return _FULL[key]


def depth_outputs(T, depth, frame_name, rows, matrix, compact, **extra):
    feats, frame = R.g5_frame()
    if frame_name == 'empty':
        frame = R.empty_frame()
    return R.run_head(R.shared_head(T, num_fusion_layers=depth)[0], feats, frame, tile_rows=rows, matrix_path=matrix,
                      radar_compact=compact, **extra)


def assert_first_levels(got, full, depth):
    for k in KEYS:
        assert got[k].shape[0] == depth and got[k].shape[1:] == full[k].shape[1:], (k, got[k].shape)
        assert torch.equal(got[k], full[k][:depth]), k
    hits = got['aux']['radar_hit_counts']
    assert hits.shape == (depth,) + tuple(full['aux']['radar_hit_counts'].shape[1:])
    assert torch.equal(hits, full['aux']['radar_hit_counts'][:depth])
    for k in ('inter_states', 'inter_references', 'last_box'):           # the decoder in front is the same launch sequence
        assert torch.equal(got['aux'][k], full['aux'][k]), k


# ---- 1. identity with the three-layer head --------------------------------------------------------------------------------
@pytest.mark.parametrize('compact', [False, True], ids=['order1', 'order2'])
@pytest.mark.parametrize('rows,matrix', PATHS)
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_first_levels_of_the_three_layer_head_bit_for_bit(T, depth, rows, matrix, compact):
    full = full_outputs(T, 'g5', rows, matrix, compact)
    assert int((full['aux']['radar_hit_counts'][0] > 0).sum()) > 32            # hit and no-hit tiles
    assert_first_levels(depth_outputs(T, depth, 'g5', rows, matrix, compact), full, depth)


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_first_levels_inside_a_nine_frame_launch(T, depth):
    """check_frame_of_nine's launch (32-row tiles, nine frames): every frame's levels [:N] equal the three-layer head's,
    and frame 4 launched alone equals its place in the nine."""
    from transcar_amd.detr3d_head import head_options
    l2i = synth.make_lidar2img()
    feats = [synth.make_feats('tiny', seed=40 + i, smooth=R.SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)]
    stacked = [gpu(torch.cat([torch.from_numpy(f[l]) for f in feats], 0)) for l in range(len(feats[0]))]
    res = {}
    for name, head in (('full', R.shared_head(T)[0]), ('depth', R.shared_head(T, num_fusion_layers=depth)[0])):
        head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
        try:
            res[name] = head(stacked, synth.make_img_metas(9, l2i, radar=frames))
            if name == 'depth':
                one = head([gpu(f) for f in feats[4]], synth.make_img_metas(1, l2i, radar=frames[4]))
        finally:
            head.forward_options = None
    for k in KEYS:
        assert res['depth'][k].shape[:2] == (depth, 9)
        assert torch.equal(res['depth'][k], res['full'][k][:depth]), k
        assert torch.equal(res['depth'][k][:, 4], one[k][:, 0]), k


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_last_level_cls_only_means_level_n_minus_1(T, depth, rows, matrix):
    """options.last_level_cls_only: the class MLPs of level N - 1 run, those before are skipped (their slices are left
    as they were); the boxes of every level and the scores of level N - 1 are the three-layer head's."""
    full = full_outputs(T, 'g5', rows, matrix, True)
    got = depth_outputs(T, depth, 'g5', rows, matrix, True, last_level_cls_only=True)
    assert torch.equal(got['all_bbox_preds'], full['all_bbox_preds'][:depth])
    assert torch.equal(got['all_cls_scores'][depth - 1], full['all_cls_scores'][depth - 1])
    assert torch.equal(got['aux']['radar_hit_counts'], full['aux']['radar_hit_counts'][:depth])


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_first_levels_on_a_frame_without_a_radar_return(T, depth, rows, matrix):
    """Every tile skips the gated part; N = 1 has no K/V half B (its second decoder layer is launched alone)."""
    full = full_outputs(T, 'empty', rows, matrix, None)
    assert int(full['aux']['radar_hit_counts'].abs().sum()) == 0
    assert_first_levels(depth_outputs(T, depth, 'empty', rows, matrix, None), full, depth)


# ---- 2. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,matrix', PATHS)
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_first_levels_against_the_reference_fixture(T, depth, rows, matrix):
    """head_variant_rig.check_against_fixture's rule on levels [:N] of the three-layer oracle and of g5_head_tiny.npz"""
    want, dbg = R.oracle_head(R.shared_head(T)[1], *R.g5_frame(), key='g5')
    R.check_against_fixture(depth_outputs(T, depth, 'g5', rows, matrix, None), want, dbg, R.gold('g5_head_tiny.npz'))


# ---- 3. levels and decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_outputs_all_and_get_bboxes(T, depth):
    feats, frame = R.g5_frame()
    metas = synth.make_img_metas(1, synth.make_lidar2img(), radar=frame)
    h3, hn = R.make_head(T)[0], R.make_head(T, num_fusion_layers=depth)[0]
    h3.plugin_graphs = hn.plugin_graphs = False
    res = {}
    for name, head in (('full', h3), ('depth', hn)):
        fusion = head([gpu(f) for f in feats], metas)
        boxes = head.get_bboxes(fusion, metas)
        head.outputs = 'all'
        every = head([gpu(f) for f in feats], metas)
        head.outputs = 'camera'
        camera = head([gpu(f) for f in feats], metas)
        res[name] = (fusion, boxes, every, camera)
    fusion, boxes, every, camera = res['depth']
    for k in KEYS:
        assert every[k].shape[0] == 6 + depth
        assert torch.equal(every[k][:6], camera[k]) and torch.equal(every[k][:6], res['full'][2][k][:6]), k
        assert torch.equal(every[k][6:], fusion[k]) and torch.equal(fusion[k], res['full'][0][k][:depth]), k
    # get_bboxes decodes level N - 1: the decode of the three-layer head's level N - 1
    cut = {k: res['full'][0][k][:depth] for k in KEYS}
    want = h3.get_bboxes(cut, metas)
    assert len(boxes) == len(want) == 1
    for a_, b_ in zip(boxes[0], want[0]):
        assert torch.equal(a_, b_)
    assert boxes[0][0].shape[0] > 0


# ---- 4. the entry points that replay captured graphs ------------------------------------------------------------------------
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_plugin_graph_replay(T, depth):
    R.check_plugin_graph_replay(R.make_head(T, num_fusion_layers=depth)[0], R.make_head(T, num_fusion_layers=depth)[0])


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_frame_pipeline_two_lanes(T, depth):
    R.check_frame_pipeline(R.make_head(T, num_fusion_layers=depth)[0], nlanes=2)


# ---- 5. training ------------------------------------------------------------------------------------------------------------
def _iteration_inputs(h):
    return R.iteration_inputs(h, R.g8_frame('g5_head_tiny.npz'))


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_training_iteration_against_the_reference(T, depth):
    """One step_fused_nhwc(update=False): losses and every trainable parameter's gradient against the reference's own
    loss() and backward on levels [:N], 2e-3; the parameter count is the head's and must be the fixture's."""
    from transcar_amd.trainer import FusionTrainer
    assert len(FusionTrainer(R.train_head(num_fusion_layers=depth), dropout=0.0).bucket.chunk_ranges) == depth + 1
    R.check_training_iteration(R.g8_frame('g5_head_tiny.npz'), 'g8_train_grads_f%d.npz' % depth,
                               'fused iteration, %d layers' % depth, expected=14 + 28 * depth, num_fusion_layers=depth)


@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_chain_paths_equal_operator_paths(T, depth, p):
    """test_gpu_training's test_chain_forward_equals_operator_forward_with_dropout and
    test_chain_backward_equals_operator_backward for N layers: the same dropout masks, the same losses and gradients."""
    from transcar_amd.trainer import FusionTrainer
    h = R.train_head(num_fusion_layers=depth)
    inputs = _iteration_inputs(h)
    tr = FusionTrainer(h, dropout=p, seed=7, decoder_dropout=0.0)
    res = {}
    with torch.enable_grad():
        for name, fwd, bwd in (('chains', True, True), ('operator forward', False, True), ('operator backward', True, False)):
            tr.chain_forward, tr.chain_backward = fwd, bwd
            h._train_forwards = 11                                   # same forward counter: same masks
            losses = tr.step_fused_nhwc(*inputs, update=False)
            torch.cuda.synchronize()
            res[name] = ({k: float(v) for k, v in losses.items()},
                         {n: q.grad.detach().clone() for n, q in h.trainable_parameters()}, tr.last_dropout_seed)
    assert len(res['chains'][1]) == 14 + 28 * depth
    assert res['chains'][2] == res['operator forward'][2] == res['operator backward'][2]
    want_l, want_g, _ = res['operator forward']
    assert len(want_l) == 2 * depth
    for k, v in want_l.items():
        assert abs(res['chains'][0][k] - v) < 2e-4 * max(1.0, abs(v)), (k, res['chains'][0][k], v)
    flat = lambda g: torch.cat([g[n].flatten() for n in sorted(g)])      # noqa: E731
    d = (flat(res['chains'][1]) - flat(want_g)).abs().max() / flat(want_g).abs().max()
    assert float(d) < 5e-4, float(d)
    for n, want in res['operator backward'][1].items():
        got, scale = res['chains'][1][n], float(want.abs().max())
        assert torch.isfinite(got).all() and torch.isfinite(want).all(), n
        assert float((got - want).abs().max()) <= 2e-4 * max(scale, 1e-6) + 1e-7, (n, scale)


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_deterministic_backward_twice(T, depth):
    from transcar_amd.trainer import FusionTrainer
    grads = {}
    for mode in ('det', 'det2', 'atomic'):
        h = R.train_head(num_fusion_layers=depth)
        tr = FusionTrainer(h, dropout=0.1, seed=2, lr=1e-5, deterministic=mode != 'atomic')
        with torch.enable_grad():
            tr.step_fused_nhwc(*_iteration_inputs(h), update=False)
        torch.cuda.synchronize()
        grads[mode] = tr.bucket.grads.clone()
        if mode != 'atomic':
            assert int(tr._shadow[:-8].abs().max()) == 0        # the call leaves its shadow zero (the last 8 words: scratch)
            B_, T_ = tr._tape_key                               # the shadow: the bucket + dK | dV of N layers + 8 words
            assert tr._shadow.numel() == tr.bucket.numel + depth * B_ * T_ * 2 * h.embed_dims + 8
    assert float(grads['det'].abs().max()) > 0
    assert torch.equal(grads['det'], grads['det2'])
    assert float((grads['det'] - grads['atomic']).abs().max()) <= 2e-6 * float(grads['det'].abs().max())


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_weight_gradient_groups_sum_to_the_grouped_launch(T, depth):
    """tc_radar_train_bwd_weights(group 0 .. N): fusion layer N .. 1, then the encoders -- each writes only its chunk of the
    bucket, together they add the grouped launch's gradients; group N + 1 and -1 are refused, naming the group."""
    from transcar_amd import _lib as L
    from transcar_amd.trainer import FusionTrainer, exchange_chunk_of
    h = R.train_head(num_fusion_layers=depth)
    tr = FusionTrainer(h, dropout=0.1, seed=4)
    tr.keep_last = True
    with torch.enable_grad():
        tr.step_fused_nhwc(*_iteration_inputs(h), update=False)
    torch.cuda.synchronize()
    want = tr.bucket.grads.clone()
    assert float(want.abs().max()) > 0
    k, lib = tr._last, L.lib()
    rngs = tr.bucket.chunk_ranges
    assert len(rngs) == depth + 1 and rngs[0][0] == 0 and rngs[-1][1] == tr.bucket.numel
    assert all(a[1] == b[0] for a, b in zip(rngs, rngs[1:]))
    for n, off in zip(tr.bucket.names, tr.bucket.offsets):
        a, b = rngs[exchange_chunk_of(n, depth)]
        assert a <= off < b, n
    tr.bucket.zero_grad()
    L.check(lib.tc_radar_train_bwd_fused_ex(
        C.byref(k['w']), C.byref(k['g']), k['hs_last'].data_ptr(), k['last_box'].data_ptr(), k['tokens'].data_ptr(),
        k['B'], k['T'], k['pad_mult'], k['all_box'].data_ptr(), k['d_cls'].data_ptr(), k['d_box'].data_ptr(),
        k['tape'].data_ptr(), k['tape'].numel(), tr._bws.data_ptr(), tr._bws.numel(), tr.dropout, k['seed'], None, None,
        2, tr._stream()), 'bwd (weights deferred)')
    torch.cuda.synchronize()
    before = tr.bucket.grads.clone()

    def weights(group):
        L.check(lib.tc_radar_train_bwd_weights(
            C.byref(k['w']), C.byref(k['g']), k['hs_last'].data_ptr(), k['tokens'].data_ptr(), k['B'], k['T'],
            k['tape'].data_ptr(), k['tape'].numel(), tr._bws.data_ptr(), tr._bws.numel(), group, tr._stream()),
            'weights %d' % group)
    for gi, (a, b) in enumerate(rngs):
        weights(gi)
        torch.cuda.synchronize()
        now = tr.bucket.grads.clone()
        changed = (now != before).nonzero().flatten()
        assert changed.numel() > 0 and int(changed.min()) >= a and int(changed.max()) < b, (gi, a, b)
        before = now
    assert float((before - want).abs().max()) <= 2e-6 * float(want.abs().max())
    for bad in (depth + 1, -1):
        with pytest.raises(L.TransCARHipError, match='group=%d' % bad):
            weights(bad)


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_optimizer_step_then_inference(T, depth):
    """One real step, then an eval forward: the lazy re-pack of the trainable weights works for N layers -- the forward
    equals that of a fresh head loaded with the updated parameters."""
    from transcar_amd.trainer import FusionTrainer
    feats, frame = R.g5_frame()
    h = R.train_head(num_fusion_layers=depth)
    before = R.run_head(h.eval(), feats, frame, tile_rows=16, matrix_path='f16x2')
    tr = FusionTrainer(h, lr=1e-3, dropout=0.0)
    h.train()
    with torch.enable_grad():
        tr.step_fused_nhwc(*_iteration_inputs(h), update=True)
    assert h._packed_dirty
    after = R.run_head(h.eval(), feats, frame, tile_rows=16, matrix_path='f16x2')
    assert not h._packed_dirty
    fresh = R.make_head(T, num_fusion_layers=depth)[0]
    fresh.load_state_dict(h.state_dict(), strict=True)
    want = R.run_head(fresh, feats, frame, tile_rows=16, matrix_path='f16x2')
    for k in KEYS:
        assert after[k].shape[0] == depth
        assert float((after[k] - before[k]).abs().max()) > 1e-3, k
        assert torch.equal(after[k], want[k]), k


# ---- 6. the C boundary ------------------------------------------------------------------------------------------------------
def test_c_boundary_refuses_four_layers_naming_the_value(T):
    from transcar_amd import _lib as L
    lib = L.lib()
    h, _ = R.shared_head(T)
    w = h.weights_struct()
    w.num_radar_layers = 4
    assert lib.tc_head_workspace_bytes(C.byref(w), 1, 64) == 0
    assert 'num_radar_layers=4' in lib.tc_last_error().decode()
    for entry in (lib.tc_radar_train_tape_bytes, lib.tc_radar_train_bwd_workspace_bytes):
        for n in (4, 0):
            w.num_radar_layers = n
            assert entry(C.byref(w), 1, 64) == 0
            assert 'num_radar_layers=%d' % n in lib.tc_last_error().decode()
    for n in (1, 2, 3):
        w.num_radar_layers = n
        assert lib.tc_radar_train_tape_bytes(C.byref(w), 1, 64) > 0
    sizes = []
    for n in (1, 2, 3):
        w.num_radar_layers = n
        sizes.append((lib.tc_radar_train_tape_bytes(C.byref(w), 1, 64), lib.tc_radar_train_bwd_workspace_bytes(C.byref(w), 1, 64)))
    for i in (0, 1):                                       # the tape and the backward workspace are sized by the depth
        assert sizes[0][i] < sizes[1][i] < sizes[2][i]
