"""The DETR3D decoder levels' own class scores and boxes on the GPU: tc_decoder_outputs_fwd (chain.hip
PROG_DECODER_HEADS) at the smallest shapes that can still go wrong, against the fp64 value of the formula, and
Detr3DHead(outputs='camera' | 'all') on the tiny rig against the reference's fixtures and the CPU oracle.

Bounds of the kernel test (the project's own for this arithmetic, tests/teacher_forced_checks.py): LAYER_TOL for the
logits and the box columns the branch gives as they are, REF_TOL for columns 0, 1, 4 in normalised space.  Where
twice the fp32 formula's own deviation from fp64 on the test's inputs exceeds a constant, that is the bound (the
adverse-frame rule).  Measured on MI355X: see DESIGN.md "Decoder heads"."""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import T, no_grad           # noqa: F401 (fixtures)
from oracle import transcar_oracle as O
from parity_util import assert_rows_match
from teacher_forced_checks import LAYER_TOL, REF_TOL
from transcar_amd import _lib as L
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

VARIANTS = ((4, 'f32'), (8, 'f32'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2'))
SENTINEL = -12345.0
GUARD = 64                   # rows of the output's width in front of and behind it


# ---- the kernel through the C entry ---------------------------------------------------------------------------------
def branch_weights(levels, ncls, code, seed):
    """cls_branches.{l} / reg_branches.{l} at synth.make_state_dict's scale: xavier-uniform matrices, biases of
    0.05 sigma, LayerNorm gamma around 1, the last Linear of a box branch times 0.1."""
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


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def normalised(box):
    """columns 0, 1, 4 of boxes in metres -> (0, 1)"""
    lo = box.new_tensor(R.PCR[:3])
    hi = box.new_tensor(R.PCR[3:])
    return (box[..., [0, 1, 4]] - lo) / (hi - lo)


@pytest.mark.parametrize('ncls,code', [(10, 10), (17, 8), (32, 9)])
def test_kernel_against_fp64_at_every_tile_height_and_path(T, ncls, code):
    from transcar_amd.detr3d_head import head_options
    lib = T.lib()
    Lv, B, Q = 2, 2, 37                     # 74 rows a level: a partial last tile at every height, two weight sets
    M = B * Q
    sd = branch_weights(Lv, ncls, code, seed=100 + ncls)
    rng = np.random.RandomState(7)
    hs = rng.standard_normal((Lv, B, Q, 256)).astype(np.float32)
    init_ref = rng.uniform(0.02, 0.98, (B, Q, 3)).astype(np.float32)
    inter_refs = rng.uniform(0.02, 0.98, (Lv, B, Q, 3)).astype(np.float32)
    for refs in (init_ref, inter_refs[0]):                  # the clamp of inverse_sigmoid (eps 1e-5), both levels
        refs[0, 3] = 0.0
        refs[0, 4] = 1.0
        refs[1, 5] = 1e-6
        refs[1, 36] = 1.0 - 1e-6
    t = lambda a, dt: torch.from_numpy(a).to(dt)            # noqa: E731
    sd64 = {k: t(v, torch.float64) for k, v in sd.items()}
    sd32 = {k: t(v, torch.float32) for k, v in sd.items()}
    want_cls, want_box = O.decoder_outputs(sd64, t(hs, torch.float64), t(init_ref, torch.float64), t(inter_refs, torch.float64), R.PCR)
    o32_cls, o32_box = O.decoder_outputs(sd32, t(hs, torch.float32), t(init_ref, torch.float32), t(inter_refs, torch.float32), R.PCR)
    other = [j for j in range(code) if j not in (0, 1, 4)]
    dev32 = dict(cls=float((o32_cls.double() - want_cls).abs().max()),
                 box=float((o32_box.double() - want_box)[..., other].abs().max()),
                 ctr=float((normalised(o32_box.double()) - normalised(want_box)).abs().max()))
    tol = dict(cls=max(LAYER_TOL, 2 * dev32['cls']), box=max(LAYER_TOL, 2 * dev32['box']), ctr=max(REF_TOL, 2 * dev32['ctr']))
    print('ncls=%d code=%d: fp32 formula vs fp64: logits %.3g, box %.3g, centre (normalised) %.3g -> bounds %.3g / %.3g / %.3g'
          % (ncls, code, dev32['cls'], dev32['box'], dev32['ctr'], tol['cls'], tol['box'], tol['ctr']))

    sd_gpu = {k: R.gpu(v) for k, v in sd.items()}
    h = heads_struct(sd_gpu, Lv, ncls, code)
    nbytes = lib.tc_decoder_heads_packed_bytes(ctypes.byref(h))
    assert nbytes == Lv * 4 * 3 * 256 * 256 * 4, lib.tc_last_error()
    packed = torch.empty(nbytes, dtype=torch.uint8, device=R.dev())
    view = L.tc_decoder_heads()
    L.check(lib.tc_decoder_heads_pack(ctypes.byref(h), packed.data_ptr(), nbytes, ctypes.byref(view), stream()),
            'tc_decoder_heads_pack')
    assert view.cls[1].l6.w == h.cls[1].l6.w and view.reg[0].l4.w == h.reg[0].l4.w      # the narrow heads stay unpacked
    assert view.cls[1].l0.w != h.cls[1].l0.w
    g_hs, g_init, g_refs = R.gpu(hs), R.gpu(init_ref), R.gpu(inter_refs)
    status = torch.zeros(4, dtype=torch.int32, device=R.dev())
    got = {}
    for rows, path in VARIANTS:
        bufs = {}
        for name, width in (('cls', ncls), ('box', code)):
            bufs[name] = torch.full(((2 * GUARD + Lv * M) * width,), SENTINEL, dtype=torch.float32, device=R.dev())
        opt = head_options(tile_rows=rows, matrix_path=path)
        opt.range_status = status.data_ptr()
        L.check(lib.tc_decoder_outputs_fwd(
            ctypes.byref(view), g_hs.data_ptr(), g_init.data_ptr(), g_refs.data_ptr(), B, Q,
            bufs['cls'][GUARD * ncls:].data_ptr(), bufs['box'][GUARD * code:].data_ptr(), ctypes.byref(opt), stream()),
            'tc_decoder_outputs_fwd')
        torch.cuda.synchronize()
        res = {}
        for name, width in (('cls', ncls), ('box', code)):
            flat = bufs[name].cpu()
            assert bool((flat[:GUARD * width] == SENTINEL).all()) and bool((flat[-GUARD * width:] == SENTINEL).all()), \
                (rows, path, name, 'guard rows were written')
            res[name] = flat[GUARD * width:-GUARD * width].view(Lv, B, Q, width).double()
            assert bool(torch.isfinite(res[name]).all()) and not bool((res[name] == SENTINEL).any()), (rows, path, name)
        got[(rows, path)] = res
        # level 0 alone into a guarded buffer: a tail row of its last tile stored past B * Q would land in the guard
        # (in the launch above it would land in level 1's first rows, which level 1 overwrites)
        one = L.tc_decoder_heads()
        ctypes.memmove(ctypes.byref(one), ctypes.byref(view), ctypes.sizeof(view))
        one.num_levels = 1
        b1 = {name: torch.full(((2 * GUARD + M) * width,), SENTINEL, dtype=torch.float32, device=R.dev())
              for name, width in (('cls', ncls), ('box', code))}
        L.check(lib.tc_decoder_outputs_fwd(
            ctypes.byref(one), g_hs.data_ptr(), g_init.data_ptr(), g_refs.data_ptr(), B, Q,
            b1['cls'][GUARD * ncls:].data_ptr(), b1['box'][GUARD * code:].data_ptr(), ctypes.byref(opt), stream()),
            'tc_decoder_outputs_fwd (one level)')
        torch.cuda.synchronize()
        for name, width in (('cls', ncls), ('box', code)):
            flat = b1[name].cpu()
            assert bool((flat[:GUARD * width] == SENTINEL).all()) and bool((flat[-GUARD * width:] == SENTINEL).all()), \
                (rows, path, name, 'guard rows behind level 0 were written')
            # (the same kernel -- the tile height is forced -- on the same rows: the same bits)
            assert torch.equal(flat[GUARD * width:-GUARD * width].view(B, Q, width).double(), res[name][0]), (rows, path, name)
        d = dict(cls=float((res['cls'] - want_cls).abs().max()),
                 box=float((res['box'] - want_box)[..., other].abs().max()),
                 ctr=float((normalised(res['box']) - normalised(want_box)).abs().max()))
        print('  %2d rows %-5s vs fp64: logits %.3g, box %.3g, centre (normalised) %.3g' % (rows, path, d['cls'], d['box'], d['ctr']))
        for k in d:
            assert d[k] <= tol[k], (rows, path, k, d[k], tol[k])
    assert int(status[0]) == 0
    keys = list(got)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert float((got[a]['cls'] - got[b]['cls']).abs().max()) <= tol['cls'], (a, b)
            assert float((got[a]['box'] - got[b]['box'])[..., other].abs().max()) <= tol['box'], (a, b)
            assert float((normalised(got[a]['box']) - normalised(got[b]['box'])).abs().max()) <= tol['ctr'], (a, b)


# ---- the head on the tiny rig ---------------------------------------------------------------------------------------
FIXTURES = {True: 'g10_decoder_outputs_tiny.npz', False: 'g10_decoder_outputs_tiny_norefine.npz'}
FEATS = {}


def tiny_feats():
    if 'np' not in FEATS:
        FEATS['np'] = synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)
    return FEATS['np']


def run(head, outputs, matrix_path=None, radar=None, aux=True):
    """One frame of the g5_head_tiny rig through the module entry; radar=None: img_metas WITHOUT a 'radar' key."""
    from transcar_amd.detr3d_head import head_options
    metas = synth.make_img_metas(1, synth.make_lidar2img()) if radar is None else \
        synth.make_img_metas(1, synth.make_lidar2img(), radar=radar)
    assert radar is not None or 'radar' not in metas[0]
    head.outputs = outputs
    head.forward_options = head_options(matrix_path=matrix_path) if matrix_path else None
    try:
        outs = head([R.gpu(f) for f in tiny_feats()], metas, aux=aux)
        torch.cuda.synchronize()
    finally:
        head.outputs = 'fusion'
        head.forward_options = None
    return outs


@pytest.mark.parametrize('matrix_path', [None, 'f32'])
@pytest.mark.parametrize('refine', [True, False])
def test_camera_outputs_against_reference_and_oracle(T, refine, matrix_path):
    head, _ = R.shared_head(T, with_box_refine=refine)
    fixture = R.gold(FIXTURES[refine])
    o_cls, o_box = R.oracle_outputs(with_box_refine=refine)
    outs = run(head, 'camera', matrix_path)
    assert outs['enc_cls_scores'] is None and outs['enc_bbox_preds'] is None
    aux = outs['aux']
    assert outs['all_cls_scores'].shape == (6, 1, 900, 10) and outs['all_bbox_preds'].shape == (6, 1, 900, 10)
    for name, got, gold_, orc in (('logits', outs['all_cls_scores'], fixture['dec_cls'], o_cls),
                                 ('boxes', outs['all_bbox_preds'], fixture['dec_box'], o_box)):
        got = got[:, 0].cpu().numpy()
        print('refine=%s %s: max|hip - reference| %.3g, max|hip - oracle| %.3g, max|oracle - reference| %.3g'
              % (refine, name, np.abs(got - gold_[:, 0]).max(), np.abs(got - orc[:, 0]).max(), np.abs(orc - gold_).max()))
        R.assert_all_but_two_queries(orc[:, 0], gold_[:, 0], R.E2E_TOL, name + ': oracle vs reference')
        R.assert_all_but_two_queries(got, gold_[:, 0], R.E2E_TOL, name + ' vs reference')
        R.assert_all_but_two_queries(got, orc[:, 0], R.E2E_TOL, name + ' vs oracle')
    box = outs['all_bbox_preds']
    ctr = normalised(box)
    if refine:
        # level l's centre IS the refined reference point of level l: each side within REF_TOL of the fp64 value
        d = float((ctr - aux['inter_references']).abs().max())
        print('max|normalised centre - inter_references| = %.3g' % d)
        assert d <= 2 * REF_TOL, d
    else:
        R.refs_are_initial(aux)
        assert float((ctr - aux['inter_references']).abs().max()) > 1.0 / 102.4      # the boxes move, the references do not
    d = float((box[-1] - aux['last_box']).abs().max())
    print('max|level 5 box - last_box| = %.3g' % d)
    assert d <= LAYER_TOL, d


@pytest.mark.parametrize('refine', [True, False])
def test_all_outputs_are_camera_levels_then_fusion_levels(T, refine):
    head, _ = R.shared_head(T, with_box_refine=refine)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    cam = run(head, 'camera', aux=False)
    assert 'aux' not in cam
    both = run(head, 'all', radar=frame, aux=False)
    fus = run(head, 'fusion', radar=frame, aux=False)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert both[k].shape == (9, 1, 900, 10) and fus[k].shape == (3, 1, 900, 10)
        assert torch.equal(both[k][6:], fus[k]), k
        assert torch.equal(both[k][:6], cam[k]), k
    with pytest.raises(KeyError, match='radar'):            # 'all' reads the radar as the default does
        run(head, 'all')


def decoded_rows(boxes, scores, labels, codes):
    """[n, 12]: centre, size, (r sin yaw, r cos yaw), velocity, score, label of decoded rows; codes [n, code_size] are the
    box codes the rows were decoded from, r = |(sin code, cos code)|.  The DECODED yaw enters weighted by r: yaw is
    atan2 of two codes, and an error delta of the codes moves it by ~ delta / r (r is down to 0.0026 on this rig, whose
    box heads are scaled by 0.1) and across the +-pi wrap -- r (sin yaw, cos yaw) is conditioned like the codes."""
    b = np.asarray(boxes, np.float64)
    r = np.hypot(np.asarray(codes, np.float64)[:, 6], np.asarray(codes, np.float64)[:, 7])
    return np.concatenate([b[:, :6], (r * np.sin(b[:, 6]))[:, None], (r * np.cos(b[:, 6]))[:, None], b[:, 7:9],
                           np.asarray(scores, np.float64)[:, None], np.asarray(labels, np.float64)[:, None]], 1)


def topk_codes(cls, box, k=300):
    """the box codes of the k best (query, class) scores in score order, as the coder selects them (CODER:62-68)"""
    idx = torch.as_tensor(cls).sigmoid().reshape(-1).topk(k)[1] // cls.shape[-1]
    return torch.as_tensor(box)[idx].numpy()


def test_get_bboxes_decodes_the_last_decoder_level(T):
    """get_bboxes on the 'camera' dict is a DETR3D detection: boxes, scores and labels against the oracle's get_bboxes
    on the reference fixture's level 5 (= [-1]), ALL rows, parity_util.assert_rows_match.

    The bound: the raw outputs agree with the fixture within the rig's E2E_TOL (checked above; measured 1.8e-4).  A
    decoded centre / velocity moves by as much, a score by a quarter of it, a size exp(code) by exp(|code|) times it
    (|code| <= 0.23 in the fixture's rows: 1.26), r (sin yaw, cos yaw) by sqrt(2) times it plus the change of r, at
    most as much again: 2 * E2E_TOL covers every column.  Preconditions read from the FIXTURE, not from the code under
    test: the 300th and 301st score are further apart than two scores can move (so both select the same rows), every
    selected centre is well inside post_center_range (so the range mask keeps all 300 on both sides)."""
    head, _ = R.shared_head(T, with_box_refine=True)
    fixture = R.gold(FIXTURES[True])
    pcr = configs.pts_bbox_head['bbox_coder']['post_center_range']
    f_cls, f_box = torch.from_numpy(fixture['dec_cls']), torch.from_numpy(fixture['dec_box'])
    srt = f_cls[5, 0].sigmoid().reshape(-1).sort(descending=True)[0]
    assert float(srt[299] - srt[300]) > 2 * R.E2E_TOL / 4
    want_b, want_s, want_l = O.get_bboxes({'all_cls_scores': f_cls, 'all_bbox_preds': f_box}, pcr)[0]
    want_codes = topk_codes(f_cls[5, 0], f_box[5, 0])
    assert want_b.shape == (300, 9) and float((want_b[:, :3].abs() - torch.tensor(pcr[3:])).max()) < -1.0
    assert float(np.abs(want_codes[:, [2, 3, 5]]).max()) < np.log(1.5)
    outs = run(head, 'camera', aux=False)
    boxes, scores, labels = head.get_bboxes(outs, synth.make_img_metas(1))[0]
    assert boxes.shape == (300, 9)
    o_cls, o_box = outs['all_cls_scores'].cpu(), outs['all_bbox_preds'].cpu()
    mine_codes = topk_codes(o_cls[5, 0], o_box[5, 0])
    # the rows come out in score order on both sides: row i was decoded from code row i
    assert np.all(np.diff(scores.cpu().numpy()) <= 0)
    mine = decoded_rows(boxes.cpu(), scores.cpu(), labels.cpu(), mine_codes)
    want = decoded_rows(want_b, want_s, want_l, want_codes)
    d = np.abs(mine - want).max(axis=0) if np.array_equal(mine[:, 11], want[:, 11]) else None
    print('decoded rows, max|hip - reference| per column (same order):', d)
    assert_rows_match(mine, want, atol=2 * R.E2E_TOL, what='DETR3D detection vs the reference (level 5)')
    # ... and the decode step itself on the very tensors it read, at the existing decode tests' bound (yaw as it is)
    own = O.get_bboxes({'all_cls_scores': o_cls, 'all_bbox_preds': o_box}, pcr)[0]

    def rows(b, s, l):
        return np.concatenate([np.asarray(b), np.asarray(s)[:, None], np.asarray(l)[:, None].astype(np.float32)], 1)
    assert_rows_match(rows(boxes.cpu(), scores.cpu(), labels.cpu()), rows(*own), atol=2e-5, what='decode of the camera outputs')


def test_frame_pipeline_refuses_outputs_changed_after_construction(T):
    """``outputs`` is a plain attribute: a pipeline built on the default refuses to launch once it is 'camera'."""
    import bench
    from transcar_amd.pipeline import FramePipeline
    head, _ = R.shared_head(T, with_box_refine=True)
    pipe = FramePipeline(head, [bench.make_inputs(head, R.dev(), 'tiny', 1, seed=11)])
    pipe.launch()
    pipe.synchronize()
    head.outputs = 'camera'
    try:
        with pytest.raises(L.TransCARHipError, match='not supported in a pipeline'):
            pipe.launch()
        with pytest.raises(L.TransCARHipError, match='not supported in a pipeline'):
            pipe.recapture()
    finally:
        head.outputs = 'fusion'
    pipe.launch()
    pipe.synchronize()


def test_range_guard_reaches_the_decoder_heads(T):
    """A weight of cls_branches.3 beyond the f16 planes' range (65 504): the automatic path (32-row tiles on the f16
    matrix cores at 6 x 900 rows) sets tc_head_options.range_status, the exact-fp32 path does not."""
    head, _ = R.make_head(T)
    head.cls_branches[3][0].weight.data[5, 7] = 1.0e5
    assert head.last_range_status == 0
    run(head, 'camera', 'f32', aux=False)
    assert head.last_range_status == 0
    outs = run(head, 'camera', aux=False)
    assert not torch.isfinite(outs['all_cls_scores'][3]).all()
    assert torch.isfinite(outs['all_cls_scores'][[0, 1, 2, 4, 5]]).all() and torch.isfinite(outs['all_bbox_preds']).all()
    with pytest.warns(UserWarning, match='f16x2'):
        assert head.last_range_status == 1
