"""The box decode's streaming kernel (decode.hip: box_decode_stream_kernel) on the MI355X: bit for bit the in-register
kernel where both apply, exact selections at the shapes only it takes (more than 12 288 scores, max_num beyond 512),
ties and the select's catch-all buckets at 13 541 scores, the refusals beyond its caps, the reference's own coder at 26
classes (tests/golden/make_golden_decode.py), and a 1 300-query head end to end.  pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import SMOOTH, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from parity_util import assert_rows_match
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

PCR = configs.pts_bbox_head['bbox_coder']['post_center_range']
TIE_CASES = ['ties', 'all_equal', 'random_batch', 'tiny_scores', 'saturated', 'extremes', 'few_candidates']


def _np(t):
    return t.cpu().numpy()


def _sigmoid64(x):
    return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


def _adverse_logits(case, cls):
    """The score distributions of test_gpu_parity.test_box_decode_ties_and_batches from standard normal draws `cls`:
    equal scores, the select's lower and upper catch-all buckets."""
    if case == 'ties':
        return np.round(cls * 2) / 2                   # ~15 distinct values
    if case == 'all_equal':
        return np.full_like(cls, 0.25)
    if case == 'tiny_scores':                          # every score below 2^-16
        return (cls * 2 - 20).astype(np.float32)
    if case == 'saturated':                            # 1 - 2^-24 .. 1 and ties at exactly 1.0
        return (np.abs(cls) * 3 + 12).astype(np.float32)
    return cls


def _tie_case(case):
    """The inputs of test_gpu_parity.test_box_decode_ties_and_batches, same seed, same draws."""
    rng = np.random.RandomState(7)
    B = 3 if case == 'random_batch' else 1
    cls = rng.standard_normal((B, 900, 10)).astype(np.float32)
    if case == 'extremes':                             # a few hundred saturated, the rest tiny, the 300th in between
        cls = (cls - 18).astype(np.float32)
        cls.reshape(-1)[rng.permutation(9000)[:170]] = 25.0
        cls.reshape(-1)[rng.permutation(9000)[:100]] = rng.standard_normal(100).astype(np.float32)
    else:
        cls = _adverse_logits(case, cls)
    Qn = 20 if case == 'few_candidates' else 900
    cls = np.ascontiguousarray(cls[:, :Qn])
    box = rng.standard_normal((B, Qn, 10)).astype(np.float32) * 0.3
    return cls, box


# ---- 1. both kernels agree where both apply ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', TIE_CASES)
def test_stream_kernel_equals_in_register_kernel(T, case):
    """Both kernels build the same key and resolve ties the same way: every output is equal, no tolerance."""
    from transcar_amd import ops
    cls, box = _tie_case(case)
    c, b = gpu(cls), gpu(box)
    reg = ops.box_decode_topk(c, b, PCR, 300, path=1)
    stream = ops.box_decode_topk(c, b, PCR, 300, path=2)
    for name, x, y in zip(('boxes', 'scores', 'labels', 'valid'), reg, stream):
        assert torch.equal(x, y), (case, name)
    auto = ops.box_decode_topk(c, b, PCR, 300)
    assert all(torch.equal(x, y) for x, y in zip(reg, auto))
    assert float(reg[1].max()) > 0.0
    for thr in (None, 0.0, float(np.median(_np(reg[1])))):
        for z_shift in (True, False):
            kr = ops.box_decode_kept(c, b, PCR, 300, score_threshold=thr, z_shift=z_shift, path=1)
            ks = ops.box_decode_kept(c, b, PCR, 300, score_threshold=thr, z_shift=z_shift, path=2)
            assert torch.equal(kr[3], ks[3]), (case, thr, z_shift)
            for bi in range(cls.shape[0]):
                n = int(kr[3][bi])
                for name, x, y in zip(('boxes', 'scores', 'labels'), kr[:3], ks[:3]):
                    assert torch.equal(x[bi, :n], y[bi, :n]), (case, thr, z_shift, bi, name)


# ---- 2. shapes only the streaming kernel takes, exact ------------------------------------------------------------------------
def _check_kept(c, b, max_num, topk, path):
    """tc_box_decode_kept against a mask select over the fixed-size rows, as test_box_decode_ties_and_batches."""
    from transcar_amd import ops
    boxes, scores, labels, valid = topk
    for thr in (None, 0.0, float(np.median(_np(scores)))):
        for z_shift in (True, False):
            kb, ks, kl, kc = ops.box_decode_kept(c, b, PCR, max_num, score_threshold=thr, z_shift=z_shift, path=path)
            assert kl.dtype == torch.int64 and kc.dtype == torch.int32
            for bi in range(c.shape[0]):
                m = valid[bi].bool()
                if thr:
                    m = m & (scores[bi] > thr)
                n = int(kc[bi])
                assert n == int(m.sum())
                want = boxes[bi][m].clone()
                if not z_shift:
                    want[:, 2] = boxes[bi][m][:, 2] + boxes[bi][m][:, 5] * 0.5
                    assert float((kb[bi, :n] - want).abs().max() if n else 0.0) < 2e-6
                else:
                    assert torch.equal(kb[bi, :n], want)
                assert torch.equal(ks[bi, :n], scores[bi][m]) and torch.equal(kl[bi, :n], labels[bi][m].long())


def _check_empty_rows(boxes, scores, labels, valid, kk):
    assert np.all(_np(labels)[kk:] == -1) and not _np(valid)[kk:].any()
    assert np.all(_np(scores)[kk:] == 0) and np.all(_np(boxes)[kk:] == 0)


STREAM_SHAPES = [(1229, 10, 300, 1, 0), (900, 26, 300, 1, 0), (1231, 11, 300, 2, 0), (900, 10, 513, 1, 0),
                 (700, 3, 2048, 1, 0), (41, 7, 287, 1, 2), (3, 5, 300, 1, 2), (4096, 32, 1000, 1, 0)]


@pytest.mark.parametrize('Q,C,max_num,B,path', STREAM_SHAPES)
def test_stream_kernel_exact_selection(T, Q, C, max_num, B, path):
    """Logits on a permuted grid, np.linspace(-8, 4, n): neighbouring fp32 sigmoids are tens to hundreds of ulps apart
    (26 at n = 131 072), so the order is that of the logits under any sigmoid good to a few ulps, and the expected
    selection is np.argsort(-logits)[:K] exactly."""
    from transcar_amd import ops
    rng = np.random.RandomState(Q + C + max_num)
    n = Q * C
    cls = np.stack([np.linspace(-8.0, 4.0, n).astype(np.float32)[rng.permutation(n)] for _ in range(B)]).reshape(B, Q, C)
    box = rng.standard_normal((B, Q, 10)).astype(np.float32) * 0.3
    box[..., 0] *= 150.0                               # a fifth of the centres outside post_center_range
    c, b = gpu(cls), gpu(box)
    topk = ops.box_decode_topk(c, b, PCR, max_num, path=path)
    boxes, scores, labels, valid = topk
    assert boxes.shape == (B, max_num, 9) and scores.shape == labels.shape == valid.shape == (B, max_num)
    kk = min(max_num, n)
    for bi in range(B):
        flat = cls[bi].reshape(-1)
        idx = np.argsort(-flat, kind='stable')[:kk]
        np.testing.assert_array_equal(_np(labels[bi])[:kk], idx % C)
        np.testing.assert_array_equal(_np(boxes[bi])[:kk, 0], box[bi][idx // C, 0])
        np.testing.assert_allclose(_np(scores[bi])[:kk], _sigmoid64(flat[idx]), atol=1e-6, rtol=0)
        cx = box[bi][idx // C, 0]
        want_valid = (cx >= PCR[0]) & (cx <= PCR[3])
        for j, (lo, hi) in ((1, (PCR[1], PCR[4])), (4, (PCR[2], PCR[5]))):
            v = box[bi][idx // C, j]
            want_valid &= (v >= np.float32(lo)) & (v <= np.float32(hi))
        np.testing.assert_array_equal(_np(valid[bi])[:kk].astype(bool), want_valid)
        assert kk < 100 or 0 < want_valid.sum() < kk        # the range mask has work to do
        _check_empty_rows(boxes[bi], scores[bi], labels[bi], valid[bi], kk)
    _check_kept(c, b, max_num, topk, path)


@pytest.mark.parametrize('max_num', [300, 1000])
@pytest.mark.parametrize('name', ['none', 'thr'])
def test_stream_kernel_matches_reference_coder_26_classes(T, max_num, name):
    """The rows the REFERENCE's NMSFreeCoder(num_classes=26).decode_single returns (g6_decode_c26.npz)."""
    from transcar_amd import ops
    g = R.gold('g6_decode_c26.npz')
    thr = None if name == 'none' else float(g['score_threshold'])
    kb, ks, kl, kc = ops.box_decode_kept(gpu(g['cls']), gpu(g['box']), [float(v) for v in g['post_center_range']], max_num,
                                         score_threshold=thr, z_shift=False)
    want_l = g['labels_%d_%s' % (max_num, name)]
    n = int(kc[0])
    assert n == len(want_l)
    np.testing.assert_array_equal(_np(kl[0, :n]), want_l)
    np.testing.assert_allclose(_np(kb[0, :n]), g['bboxes_%d_%s' % (max_num, name)], atol=2e-5, rtol=0)
    np.testing.assert_allclose(_np(ks[0, :n]), g['scores_%d_%s' % (max_num, name)], atol=1e-6, rtol=0)


# ---- 3. ties at large n --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['ties', 'all_equal', 'tiny_scores', 'saturated', 'extremes'])
def test_stream_kernel_ties_at_13541_scores(T, case):
    """n = 1231 x 11 = 13 541, max_num 300, the automatic path (the streaming kernel: n > 12 288).  Equal scores keep the
    select going through the index digits; ties resolve to the lower flat index."""
    from transcar_amd import ops
    Q, C, K = 1231, 11, 300
    n = Q * C
    rng = np.random.RandomState(11)
    cls = rng.standard_normal((1, Q, C)).astype(np.float32)
    if case == 'extremes':
        cls = (cls - 18).astype(np.float32)
        cls.reshape(-1)[rng.permutation(n)[:170]] = 25.0
        cls.reshape(-1)[rng.permutation(n)[:100]] = rng.standard_normal(100).astype(np.float32)
    else:
        cls = _adverse_logits(case, cls)
    box = rng.standard_normal((1, Q, 10)).astype(np.float32) * 0.3
    c, b = gpu(cls), gpu(box)
    topk = ops.box_decode_topk(c, b, PCR, K)
    boxes, scores, labels, valid = (_np(x[0]) for x in topk)
    flat = _sigmoid64(cls[0].reshape(-1))
    order = np.lexsort((np.arange(n), -flat))[:K]                      # score descending, index ascending
    np.testing.assert_allclose(scores, flat[order], atol=1e-6, rtol=0)
    if case == 'all_equal':
        np.testing.assert_array_equal(order, np.arange(K))             # flat indices 0 .. 299, in order
    if case in ('ties', 'all_equal'):                                  # distinct logits, distinct fp32 scores: exact
        np.testing.assert_array_equal(labels, order % C)
        np.testing.assert_array_equal(boxes[:, 0], box[0][order // C, 0])
    else:
        # distinct logits may round to one fp32 sigmoid (order free): sorted scores, every row a real (query, class)
        # pair with that score, no pair twice
        s32 = (1.0 / (1.0 + np.exp(-cls[0].astype(np.float32).reshape(-1)))).astype(np.float32)
        assert np.all(scores[:-1] >= scores[1:])
        cand = {}
        for i in np.argsort(-s32, kind='stable')[:K + 200]:
            cand.setdefault((np.float32(box[0][i // C, 0]).item(), int(i % C)), []).append(i)
        seen = set()
        for r in range(K):
            ids = [i for i in cand.get((np.float32(boxes[r, 0]).item(), int(labels[r])), [])
                   if i not in seen and abs(s32[i] - scores[r]) <= 1e-6]
            assert ids, (case, r)
            seen.add(ids[0])
    assert valid.all()
    _check_kept(c, b, K, topk, 0)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_beyond_the_caps(T):
    from transcar_amd import _lib as L
    from transcar_amd import ops
    c, b = gpu(np.zeros((1, 900, 10), np.float32)), gpu(np.zeros((1, 900, 10), np.float32))
    for fn in (ops.box_decode_topk, ops.box_decode_kept):
        with pytest.raises(T.TransCARHipError, match='max_num=2049'):
            fn(c, b, PCR, 2049)
        with pytest.raises(T.TransCARHipError, match='Q\\*num_classes=12290'):
            fn(gpu(np.zeros((1, 1229, 10), np.float32)), gpu(np.zeros((1, 1229, 10), np.float32)), PCR, 300, path=1)
    # 2^20 + 1 scores with sixteen floats of storage behind the pointer: refused before anything reads it
    tiny = gpu(np.zeros(16, np.float32))
    out = torch.zeros(300 * 9, dtype=torch.float32, device=R.dev())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())        # noqa: E731
    with pytest.raises(T.TransCARHipError, match='Q\\*num_classes=1048577'):
        L.check(L.lib().tc_box_decode_topk(p(tiny), p(tiny), 1, (1 << 20) + 1, 1, 10, 300, L.f6(PCR), p(out), p(out), p(out),
                                           p(out), None, 0, stream), 'tc_box_decode_topk')
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0               # nothing was launched
    # a correctly shaped tensor of 2^20 scores is fine
    rng = np.random.RandomState(5)
    cls = np.linspace(-8.0, 4.0, 1 << 20).astype(np.float32)[rng.permutation(1 << 20)].reshape(1, 1 << 15, 32)
    box = rng.standard_normal((1, 1 << 15, 10)).astype(np.float32) * 0.3
    _, scores, labels, _ = ops.box_decode_topk(gpu(cls), gpu(box), PCR, 300)
    idx = np.argsort(-cls.reshape(-1), kind='stable')[:300]
    np.testing.assert_array_equal(_np(labels[0]), idx % 32)
    np.testing.assert_allclose(_np(scores[0]), _sigmoid64(cls.reshape(-1)[idx]), atol=1e-6, rtol=0)


# ---- 5. a head beyond the old limit, end to end ---------------------------------------------------------------------------
NQ = 1300


def _head_1300(T):
    sd_np = synth.make_state_dict(seed=5, num_query=NQ)
    h = T.build_head(configs.head_cfg(num_query=NQ))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return h.to(R.dev()).eval(), sd_np


def test_head_1300_queries_forward_and_get_bboxes(T):
    """1 300 x 10 = 13 000 scores: the forward against the oracle, then get_bboxes (the streaming kernel) against the
    oracle's decode of the head's OWN scores and boxes, at test_box_decode_vs_oracle's tolerance."""
    head, sd_np = _head_1300(T)
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    want, dbg = R.oracle_head(O.to_torch_sd(sd_np), feats_np, frame)
    outs = R.run_head(head, feats_np, frame)
    assert outs['all_cls_scores'].shape == (3, 1, NQ, 10)
    R.check_against_oracle(outs, want, dbg)
    got = head.get_bboxes(outs, synth.make_img_metas(1))[0]
    ref = O.get_bboxes({'all_cls_scores': outs['all_cls_scores'].cpu(), 'all_bbox_preds': outs['all_bbox_preds'].cpu()},
                       head.bbox_coder.post_center_range, head.bbox_coder.max_num, 10)[0]
    assert got[0].shape[0] == ref[0].shape[0] > 0
    np.testing.assert_allclose(_np(got[1]), ref[1].numpy(), atol=1e-6, rtol=0)
    mine = np.concatenate([_np(got[0]), _np(got[1])[:, None], _np(got[2])[:, None].astype(np.float32)], 1)
    theirs = np.concatenate([ref[0].numpy(), ref[1].numpy()[:, None], ref[2].numpy()[:, None].astype(np.float32)], 1)
    assert_rows_match(mine, theirs, atol=2e-5, what='decoded boxes of 1300 queries')
    s = _np(got[1])
    assert np.all(s[:-1] >= s[1:])


def test_head_1300_queries_plugin_graph_replay(T):
    R.check_plugin_graph_replay(_head_1300(T)[0], _head_1300(T)[0])


def test_head_1300_queries_frame_pipeline(T):
    R.check_frame_pipeline(_head_1300(T)[0], 2)
