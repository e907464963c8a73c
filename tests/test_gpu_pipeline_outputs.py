"""Detr3DHead.outputs 'camera' and 'all' in a FramePipeline and in the plugin entry's graphs, and the level-range entry
(tc_decoder_outputs_levels_fwd) they launch, on the tiny rig.

The project's standing claim -- a frame in a launch is bit-identical to the frame alone at the same tile height and matrix
path -- extended to the new modes: every comparison below is ``torch.equal`` with the tile height and path pinned on both
sides (``head_options(tile_rows=, matrix_path=)`` for a pipeline, ``head.forward_options`` for the eager entry), at two of
the existing variants.  The one tolerance is the rig's own (E2E_TOL and its two-query allowance, measured for the
g10 fixtures with the oracle alone inside them), exactly as test_gpu_decoder_outputs holds the eager path."""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import T, no_grad           # noqa: F401 (fixtures)
from transcar_amd import _lib as L
from transcar_amd import ops, synth

pytestmark = pytest.mark.gpu

VARIANTS = ((16, 'f32'), (32, 'f16x2'))
FIXTURES = {True: 'g10_decoder_outputs_tiny.npz', False: 'g10_decoder_outputs_tiny_norefine.npz'}
KEYS = ('all_cls_scores', 'all_bbox_preds')
SENTINEL = -12345.0
GUARD = 64                   # rows of the output's width in front of and behind it

_FEATS, _STREAMS, _EAGER, _PIPES = {}, [], {}, {}


def feats_np(seed):
    if seed not in _FEATS:
        _FEATS[seed] = synth.make_feats('tiny', seed=seed, smooth=R.SMOOTH)
    return _FEATS[seed]


def radar_frame():
    return synth.make_radar_frame(seed=2, n_per_radar=51)


def streams(n):
    """one pool of lane streams for every pipeline of this module (a process has a handful of hardware queues)"""
    while len(_STREAMS) < n:
        _STREAMS.append(torch.cuda.Stream())
    return _STREAMS[:n]


def options(variant):
    from transcar_amd.detr3d_head import head_options
    return head_options(tile_rows=variant[0], matrix_path=variant[1])


def eager(T, refine, variant, mode, seed):
    """One frame alone through the module entry (no plugin graphs) -> the outputs dict, computed once and left unchanged."""
    key = (refine, variant, mode, seed)
    if key not in _EAGER:
        head, _ = R.shared_head(T, with_box_refine=refine)
        metas = synth.make_img_metas(1, synth.make_lidar2img(), radar=None if mode == 'camera' else radar_frame())
        keep = head.plugin_graphs
        head.outputs, head.forward_options, head.plugin_graphs = mode, options(variant), False
        try:
            outs = head([R.gpu(f) for f in feats_np(seed)], metas)
            torch.cuda.synchronize()
        finally:
            head.outputs, head.forward_options, head.plugin_graphs = 'fusion', None, keep
        _EAGER[key] = outs
    return _EAGER[key]


def lane_inputs(head, mode, seeds):
    """A lane's static tensors with frame seeds[j] in slot j; 'camera' lanes carry neither tokens nor pad_mult."""
    P = len(seeds)
    nhwc = [ops.to_nhwc(R.gpu(np.concatenate([feats_np(s)[l] for s in seeds], 0))) for l in range(len(feats_np(seeds[0])))]
    l2i = R.gpu(np.stack([synth.make_lidar2img()] * P))
    lane = dict(nhwc=nhwc, l2i=l2i, hw=R.HW)
    if mode != 'camera':
        metas = synth.make_img_metas(P, synth.make_lidar2img(), radar=radar_frame())
        lane['tokens'], lane['pad_mult'] = head.radar_tokens(metas, R.dev())
    return lane


def pipeline(T, refine, variant, mode, seeds_per_lane=((1,),), levels='all'):
    """-> (pipe, [(outs, decoded)] per lane after one full launch of every lane); built once per key and kept alive."""
    from transcar_amd.pipeline import FramePipeline
    key = (refine, variant, mode, seeds_per_lane, levels)
    if key not in _PIPES:
        head, _ = R.shared_head(T, with_box_refine=refine)
        head.outputs = mode
        try:
            kw = {} if mode == 'fusion' else dict(outputs=mode, decoder_levels=levels)
            pipe = FramePipeline(head, [lane_inputs(head, mode, s) for s in seeds_per_lane], options=options(variant),
                                 streams=streams(len(seeds_per_lane)), **kw)
            for i in range(pipe.lanes):
                pipe.launch(i)
            for i in range(pipe.lanes):
                pipe.wait(i)
                assert pipe.range_status(i) == 0
        finally:
            head.outputs = 'fusion'
        _PIPES[key] = (pipe, [pipe.outputs[i] for i in range(pipe.lanes)])
    return _PIPES[key]


# ---- 1. a camera lane against the eager entry and the reference's fixture ---------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('refine', [True, False])
def test_camera_lane_equals_eager_and_holds_against_the_reference(T, refine, variant):
    want = eager(T, refine, variant, 'camera', 1)
    pipe, res = pipeline(T, refine, variant, 'camera')
    assert pipe.mode == 'camera' and pipe.lanes == 1 and pipe.frames_per_launch == 1 and pipe.radar_stage is None
    outs, dec = res[0]
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    for k in KEYS:
        assert outs[k].shape == (6, 1, 900, 10)
        assert torch.equal(outs[k], want[k]), (refine, variant, k)
    fixture = R.gold(FIXTURES[refine])
    for name, k, gold_ in (('logits', 'all_cls_scores', fixture['dec_cls']), ('boxes', 'all_bbox_preds', fixture['dec_box'])):
        got = outs[k][:, 0].cpu().numpy()
        print('refine=%s %s %s: max|pipeline - reference| %.3g' % (refine, variant, name, np.abs(got - gold_[:, 0]).max()))
        R.assert_all_but_two_queries(got, gold_[:, 0], R.E2E_TOL, name + ' of a camera lane vs reference')


# ---- 2. several frames per launch, two lanes, a partial launch ----------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
def test_two_frames_per_launch_and_flush(T, variant):
    refine = True
    pipe, res = pipeline(T, refine, variant, 'camera', seeds_per_lane=((1, 2), (2, 1)))
    assert pipe.frames_per_launch == 2 and pipe.lanes == 2
    for lane, seeds in enumerate(((1, 2), (2, 1))):
        outs, _ = res[lane]
        for slot, seed in enumerate(seeds):
            want = eager(T, refine, variant, 'camera', seed)
            for k in KEYS:
                assert outs[k].shape == (6, 2, 900, 10)
                assert torch.equal(outs[k][:, slot], want[k][:, 0]), (variant, lane, slot, k)
    assert not torch.equal(res[0][0]['all_cls_scores'][:, 0], res[0][0]['all_cls_scores'][:, 1])     # two different frames
    head, _ = R.shared_head(T, with_box_refine=refine)
    head.outputs = 'camera'
    try:
        assert pipe.flush() == 0                               # nothing pending
        lane, slot, launched = pipe.submit()                   # slot 0 of the lane being filled: seed 1 lies there
        assert (slot, launched) == (0, False)
        seed = ((1, 2), (2, 1))[lane][0]
        assert pipe.flush() == 1
        pipe.wait(lane)
        n, (outs, dec) = pipe.results(lane)
    finally:
        head.outputs = 'fusion'
    assert n == 1 and pipe.last_flush[:2] == (lane, 1)
    want = eager(T, refine, variant, 'camera', seed)
    for k in KEYS:
        assert outs[k].shape == (6, 1, 900, 10)
        assert torch.equal(outs[k], want[k]), (variant, k)
    assert dec[0].shape[0] == 1
    # the full graph's tensors keep the full launch's frames
    assert torch.equal(pipe.outputs[lane][0]['all_cls_scores'][:, 1], eager(T, refine, variant, 'camera', 2 if seed == 1 else 1)['all_cls_scores'][:, 0])


# ---- 3. decoder_levels='last' ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('refine', [True, False])
def test_last_level_alone_equals_level_five_of_all_levels(T, refine, variant):
    _, every = pipeline(T, refine, variant, 'camera')
    pipe, last = pipeline(T, refine, variant, 'camera', levels='last')
    assert pipe.decoder_levels == 'last'
    for k in KEYS:
        assert last[0][0][k].shape == (1, 1, 900, 10)
        assert torch.equal(last[0][0][k][0], every[0][0][k][5]), (refine, variant, k)
        assert last[0][0][k].data_ptr() != every[0][0][k].data_ptr()
    for a, b in zip(last[0][1], every[0][1]):                  # the decode reads [-1] in both
        assert torch.equal(a, b)


# ---- 4. an 'all' lane ---------------------------------------------------------------------------------------------------------
def _extent(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('refine', [True, False])
def test_all_lane_is_camera_levels_then_fusion_levels(T, refine, variant):
    _, cam = pipeline(T, refine, variant, 'camera')
    _, fus = pipeline(T, refine, variant, 'fusion')
    pipe, both = pipeline(T, refine, variant, 'all')
    assert pipe.mode == 'all'
    for k in KEYS:
        assert both[0][0][k].shape == (9, 1, 900, 10) and both[0][0][k].is_contiguous()
        assert fus[0][0][k].shape == (3, 1, 900, 10)
        assert torch.equal(both[0][0][k][:6], cam[0][0][k]), (refine, variant, k)
        assert torch.equal(both[0][0][k][6:], fus[0][0][k]), (refine, variant, k)
    assert torch.equal(both[0][0]['all_cls_scores'][6:], eager(T, refine, variant, 'fusion', 1)['all_cls_scores'])
    # one allocation for the nine levels: the boxes lie right behind the class scores
    c, b = both[0][0]['all_cls_scores'], both[0][0]['all_bbox_preds']
    assert _extent(c)[1] == _extent(b)[0]
    # nothing of one mode's results lies in another's (three live pipelines)
    spans = []
    for res in (cam, fus, both):
        outs, dec = res[0]
        spans += [_extent(outs[k]) for k in KEYS] + [_extent(d) for d in dec]
    spans.sort()
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo, spans


# ---- 5. the decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', VARIANTS)
def test_decode_reads_the_last_level_of_the_mode(T, variant):
    refine = True
    head, _ = R.shared_head(T, with_box_refine=refine)
    want = eager(T, refine, variant, 'camera', 1)
    own = ops.box_decode_topk(want['all_cls_scores'][-1], want['all_bbox_preds'][-1], head.bbox_coder.post_center_range,
                              head.bbox_coder.max_num)
    torch.cuda.synchronize()
    _, cam = pipeline(T, refine, variant, 'camera')
    assert len(cam[0][1]) == len(own) == 4
    for a, b in zip(cam[0][1], own):
        assert torch.equal(a, b)
    _, fus = pipeline(T, refine, variant, 'fusion')
    _, both = pipeline(T, refine, variant, 'all')
    for a, b in zip(both[0][1], fus[0][1]):
        assert torch.equal(a, b)
    assert not torch.equal(cam[0][1][0], fus[0][1][0])            # (the camera detector's boxes are not the fused ones)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_value_and_leave_the_pipeline_usable(T):
    from transcar_amd.pipeline import FramePipeline
    variant = VARIANTS[0]
    head, _ = R.shared_head(T, with_box_refine=True)
    cam_lane, rad_lane = lane_inputs(head, 'camera', (1,)), lane_inputs(head, 'fusion', (1,))
    kw = dict(options=options(variant), streams=streams(1))
    generation = head.buffers_generation
    try:
        with pytest.raises(L.TransCARHipError, match=r"outputs='fusion' is not supported in a pipeline built for outputs='camera'"):
            FramePipeline(head, [cam_lane], outputs='camera', **kw)
        with pytest.raises(L.TransCARHipError, match="outputs='bev'"):
            FramePipeline(head, [rad_lane], outputs='bev', **kw)
        head.outputs = 'camera'
        with pytest.raises(L.TransCARHipError, match=r"outputs='camera' is not supported in a pipeline built for outputs='fusion'"):
            FramePipeline(head, [rad_lane], **kw)
        with pytest.raises(L.TransCARHipError, match=r"radar_raw_capacity=256 with outputs='camera'"):
            FramePipeline(head, [cam_lane], outputs='camera', radar_raw_capacity=256, **kw)
        head.outputs = 'all'
        with pytest.raises(L.TransCARHipError, match=r"decoder_levels='last' with outputs='all'"):
            FramePipeline(head, [rad_lane], outputs='all', decoder_levels='last', **kw)
    finally:
        head.outputs = 'fusion'
    assert head.buffers_generation == generation
    pipe, res = pipeline(T, True, variant, 'camera')
    before = [res[0][0][k].clone() for k in KEYS]
    with pytest.raises(L.TransCARHipError, match=r"outputs='fusion' is not supported in a pipeline built for outputs='camera'"):
        pipe.launch()                                          # (the shared head is back on 'fusion')
    with pytest.raises(L.TransCARHipError, match='not supported in a pipeline'):
        pipe.recapture()
    head.outputs = 'all'
    try:
        with pytest.raises(L.TransCARHipError, match=r"outputs='all' is not supported in a pipeline built for outputs='camera'"):
            pipe.launch()
        head.outputs = 'camera'
        with pytest.raises(L.TransCARHipError, match='tokens given to a lane'):
            pipe.write_inputs(0, tokens=rad_lane['tokens'])
        with pytest.raises(L.TransCARHipError, match='radar_frame given to a lane'):
            pipe.write_inputs(0, radar_frame=radar_frame())
        pipe.write_inputs(0, l2i=cam_lane['l2i'])
        # the packed decoder heads are written again where they lie: same buffer, same generation, the capture replays
        packed = head._dec_heads[0].data_ptr()
        head.refresh_weights()
        head.decoder_heads()
        assert head._dec_heads[0].data_ptr() == packed and head.buffers_generation == generation
        lane, outs = pipe.launch()
        pipe.wait(lane)
    finally:
        head.outputs = 'fusion'
    for k, b in zip(KEYS, before):
        assert torch.equal(outs[0][k], b), k


# ---- 7. the plugin entry's graphs ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['camera', 'all'])
def test_plugin_graphs_replay_the_mode_bit_for_bit(T, mode):
    head, _ = R.make_head(T, with_box_refine=True)             # a head of its own: its graph cache starts empty
    frame = radar_frame()
    cam_metas = synth.make_img_metas(1, synth.make_lidar2img())
    rad_metas = synth.make_img_metas(1, synth.make_lidar2img(), radar=frame)
    assert 'radar' not in cam_metas[0]
    metas = cam_metas if mode == 'camera' else rad_metas
    feats = [R.gpu(f) for f in feats_np(1)]
    head.outputs = mode
    head.plugin_graphs = False
    want = head(feats, metas)
    assert head._plugin_graphs is None or head._plugin_graphs.stats['captures'] == 0
    head.plugin_graphs = True
    got = [head(feats, metas) for _ in range(3)]
    torch.cuda.synchronize()
    st = head._plugin_graphs.stats
    assert st['captures'] == 1 and st['replays'] >= 1 and st['replays'] + st['eager'] == 3, st
    assert '_decoded' in got[-1] and '_decoded' not in want
    levels = 6 if mode == 'camera' else 9
    for o in got:
        for k in KEYS:
            assert o[k].shape == (levels, 1, 900, 10)
            assert torch.equal(o[k], want[k]), (mode, k)
    (key,) = head._plugin_graphs.entries
    assert key[0] == mode
    if mode == 'camera':
        e = head._plugin_graphs.entries[key]
        assert e.stage is None and e.g2 is None and len(key) == 10            # nothing of the radar in the entry or its key
    # get_bboxes takes the graph's decode: the same rows as the eager dict's
    a, b = head.get_bboxes(got[-1], metas)[0], head.get_bboxes(want, metas)[0]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the same tensors under another mode: another key, so the entry above is not replayed
    replays = st['replays']
    head.outputs = 'fusion'
    fus = head(feats, rad_metas)
    assert head._plugin_graphs.stats['replays'] == replays and head._plugin_graphs.stats['captures'] == 1
    head.plugin_graphs = False
    plain = head(feats, rad_metas)
    torch.cuda.synchronize()
    for k in KEYS:
        assert fus[k].shape == (3, 1, 900, 10) and torch.equal(fus[k], plain[k])
    if mode == 'all':
        for k in KEYS:
            assert torch.equal(want[k][6:], plain[k])


# ---- 8. the level-range entry alone -------------------------------------------------------------------------------------------
def branch_weights(levels, ncls, code, seed):
    """cls_branches.{l} / reg_branches.{l} at synth.make_state_dict's scale (as tests/test_gpu_decoder_outputs.py)"""
    rng = np.random.RandomState(seed)
    sd = {}

    def lin(key, n, k, scale=1.0):
        a = np.sqrt(6.0 / (n + k))
        sd[key + '.weight'] = (rng.uniform(-a, a, (n, k)) * scale).astype(np.float32)
        sd[key + '.bias'] = (rng.standard_normal(n) * 0.05 * scale).astype(np.float32)

    def ln(key):
        sd[key + '.weight'] = (1.0 + rng.standard_normal(256) * 0.1).astype(np.float32)
        sd[key + '.bias'] = (rng.standard_normal(256) * 0.05).astype(np.float32)
    for l in range(levels):
        c, r = 'cls_branches.%d' % l, 'reg_branches.%d' % l
        lin(c + '.0', 256, 256); ln(c + '.1'); lin(c + '.3', 256, 256); ln(c + '.4'); lin(c + '.6', ncls, 256)
        lin(r + '.0', 256, 256); lin(r + '.2', 256, 256); lin(r + '.4', code, 256, 0.1)
    return sd


def heads_struct(sd_gpu, levels, ncls, code):
    h = L.tc_decoder_heads()
    h.abi_version, h.num_levels, h.embed_dims, h.num_classes, h.code_size = L.TC_ABI_VERSION, levels, 256, ncls, code
    for i in range(6):
        h.pc_range[i] = float(R.PCR[i])

    def lin(key):
        return L.tc_linear(sd_gpu[key + '.weight'].data_ptr(), sd_gpu[key + '.bias'].data_ptr())

    def norm(key):
        return L.tc_lnorm(sd_gpu[key + '.weight'].data_ptr(), sd_gpu[key + '.bias'].data_ptr())
    for l in range(levels):
        c, r = 'cls_branches.%d' % l, 'reg_branches.%d' % l
        h.cls[l] = L.tc_cls_branch(lin(c + '.0'), norm(c + '.1'), lin(c + '.3'), norm(c + '.4'), lin(c + '.6'))
        h.reg[l] = L.tc_reg_branch(lin(r + '.0'), lin(r + '.2'), lin(r + '.4'))
    return h


@pytest.mark.parametrize('rows,path', [(4, 'f32'), (32, 'f16x2')])
def test_level_range_entry_equals_the_slices_of_the_full_launch(T, rows, path):
    from transcar_amd.detr3d_head import head_options
    lib = T.lib()
    Lv, B, Q, ncls, code = 3, 1, 70, 10, 10          # 70 rows a level: a partial last tile at every height
    M = B * Q
    sd_gpu = {k: R.gpu(v) for k, v in branch_weights(Lv, ncls, code, seed=21).items()}
    rng = np.random.RandomState(8)
    hs = R.gpu(rng.standard_normal((Lv, B, Q, 256)).astype(np.float32))
    init_ref = R.gpu(rng.uniform(0.02, 0.98, (B, Q, 3)).astype(np.float32))
    inter_refs = R.gpu(rng.uniform(0.02, 0.98, (Lv, B, Q, 3)).astype(np.float32))
    h = heads_struct(sd_gpu, Lv, ncls, code)
    nbytes = lib.tc_decoder_heads_packed_bytes(ctypes.byref(h))
    assert nbytes == Lv * 4 * 3 * 256 * 256 * 4, lib.tc_last_error()
    packed = torch.empty(nbytes, dtype=torch.uint8, device=R.dev())
    view = L.tc_decoder_heads()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.tc_decoder_heads_pack(ctypes.byref(h), packed.data_ptr(), nbytes, ctypes.byref(view), stream), 'tc_decoder_heads_pack')
    status = torch.zeros(4, dtype=torch.int32, device=R.dev())
    opt = head_options(tile_rows=rows, matrix_path=path)
    opt.range_status = status.data_ptr()
    full = {name: torch.empty((Lv, B, Q, width), dtype=torch.float32, device=R.dev()) for name, width in (('cls', ncls), ('box', code))}
    L.check(lib.tc_decoder_outputs_fwd(ctypes.byref(view), hs.data_ptr(), init_ref.data_ptr(), inter_refs.data_ptr(), B, Q,
                                       full['cls'].data_ptr(), full['box'].data_ptr(), ctypes.byref(opt), stream),
            'tc_decoder_outputs_fwd')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(full['cls']).all()) and bool(torch.isfinite(full['box']).all())
    for l in range(1, Lv):
        assert not torch.equal(full['cls'][l], full['cls'][0])           # levels differ: a wrong slice would show
    for first, count in ((0, 3), (1, 1), (2, 1), (1, 2)):
        bufs = {name: torch.full(((2 * GUARD + count * M) * width,), SENTINEL, dtype=torch.float32, device=R.dev())
                for name, width in (('cls', ncls), ('box', code))}
        L.check(lib.tc_decoder_outputs_levels_fwd(
            ctypes.byref(view), hs.data_ptr(), init_ref.data_ptr(), inter_refs.data_ptr(), B, Q, first, count,
            bufs['cls'][GUARD * ncls:].data_ptr(), bufs['box'][GUARD * code:].data_ptr(), ctypes.byref(opt), stream),
            'tc_decoder_outputs_levels_fwd')
        torch.cuda.synchronize()
        for name, width in (('cls', ncls), ('box', code)):
            flat = bufs[name]
            assert bool((flat[:GUARD * width] == SENTINEL).all()) and bool((flat[-GUARD * width:] == SENTINEL).all()), \
                (rows, path, first, count, name, 'guard rows were written')
            got = flat[GUARD * width:-GUARD * width].view(count, B, Q, width)
            assert torch.equal(got, full[name][first:first + count]), (rows, path, first, count, name)
    assert int(status[0]) == 0
