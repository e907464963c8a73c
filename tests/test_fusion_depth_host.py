"""Detr3DHead(num_fusion_layers=N), N = 1, 2, 3: the host side -- the keyword and its refusals, the modules and
state_dict keys an N-layer head has, the C struct, the gradient exchange's chunks.  No GPU."""
import pytest
import torch

import transcar_amd as T
from transcar_amd import _lib as L
from transcar_amd import configs, synth
from transcar_amd.trainer import FlatBucket, exchange_chunk_of

LAYER_STEMS = ('final_cls', 'final_reg', 'rf_multihead_attn', 'rf_linear1', 'rf_linear2', 'rf_norm1', 'rf_norm2', 'rf_norm3')
BAD = (0, 4, -1, True, False, 2.0, '2', None)


def _head(depth=None, **kw):
    return T.build_head(configs.head_cfg(num_query=20, **({} if depth is None else {'num_fusion_layers': depth}), **kw))


def _layer_of(key):
    """0-based fusion layer of a state_dict key, spelled out on its own (not synth.fusion_layer_of)"""
    mod = key.split('.')[0]
    for stem in LAYER_STEMS:
        if mod.startswith(stem):
            tail = mod[len(stem):]
            if tail in ('', '2', '3', '_2', '_3'):
                return 0 if tail == '' else int(tail[-1]) - 1
    return None


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_constructor_and_head_cfg_accept_the_depth(depth):
    cfg = configs.head_cfg(num_fusion_layers=depth)
    assert cfg['num_fusion_layers'] == depth
    h = T.build_head(dict(cfg, num_query=20))
    assert h.num_fusion_layers == depth
    assert h.weights_struct().num_radar_layers == depth
    for sfx, asfx in (('', ''), ('_2', '2'), ('_3', '3'))[:depth]:
        for name in ('final_cls' + asfx, 'final_reg' + asfx, 'rf_multihead_attn' + asfx, 'rf_linear1' + sfx,
                     'rf_linear2' + sfx, 'rf_norm1' + sfx, 'rf_norm2' + sfx, 'rf_norm3' + sfx, 'rf_dropout' + sfx,
                     'rf_dropout1' + sfx, 'rf_dropout2' + sfx, 'rf_dropout3' + sfx):
            assert hasattr(h, name), name
    for sfx, asfx in (('', ''), ('_2', '2'), ('_3', '3'))[depth:]:
        for name in ('final_cls' + asfx, 'final_reg' + asfx, 'rf_multihead_attn' + asfx, 'rf_linear1' + sfx,
                     'rf_norm2' + sfx, 'rf_dropout' + sfx, 'rf_dropout3' + sfx):
            assert not hasattr(h, name), name
    # the reference's unused modules stay at every depth
    for name in ('attention_weights2', 'attention_weights3', 'output_proj2', 'output_proj3'):
        assert hasattr(h, name)


def test_default_is_three_layers():
    assert 'num_fusion_layers' not in configs.head_cfg()
    h = _head()
    assert h.num_fusion_layers == 3 and h.weights_struct().num_radar_layers == 3


@pytest.mark.parametrize('bad', BAD, ids=repr)
def test_refusals_name_the_value(bad):
    named = 'num_fusion_layers=%s' % repr(bad).replace('.', r'\.')
    h = _head()

    def struct_of_bad_attribute():
        h.num_fusion_layers = bad                           # (a public attribute: weights_struct() checks it again)
        h.weights_struct()
    calls = [lambda: L.check_num_fusion_layers(bad),
             lambda: T.build_head(dict(configs.head_cfg(num_query=20), num_fusion_layers=bad)),
             lambda: synth.make_state_dict(num_query=20, num_fusion_layers=bad),
             struct_of_bad_attribute]
    if bad is not None:                                     # head_cfg(num_fusion_layers=None): the default, as its other keys
        calls.append(lambda: configs.head_cfg(num_fusion_layers=bad))
    for call in calls:
        with pytest.raises(L.TransCARHipError, match=named):
            call()


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_state_dict_is_the_three_layer_one_minus_the_absent_layers(depth):
    full = synth.make_state_dict(seed=3, num_query=20)
    sd = synth.make_state_dict(seed=3, num_query=20, num_fusion_layers=depth)
    want = {k for k in full if _layer_of(k) is None or _layer_of(k) < depth}
    assert len(full) - len(want) == (3 - depth) * 30          # 28 used + rf_norm1's two, per layer
    assert set(sd) == want
    for k, v in sd.items():
        assert v.dtype == full[k].dtype and (v == full[k]).all(), k      # nothing drawn again
    h = _head(depth)
    assert set(h.state_dict()) == want
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    if depth < 3:
        with pytest.raises(RuntimeError, match='Unexpected key'):
            h.load_state_dict({k: torch.from_numpy(v) for k, v in full.items()}, strict=True)
    assert len(h.freeze_decoder().trainable_parameters()) == 14 + 28 * depth      # the encoders' 14, 28 per fusion layer


def test_fusion_layer_of():
    for k in synth.make_state_dict(seed=3, num_query=20):
        assert synth.fusion_layer_of(k) == _layer_of(k), k
    assert synth.fusion_layer_of('attention_weights2.weight') is None and synth.fusion_layer_of('output_proj3.bias') is None


# the names of the fusion stack's trainable modules (HEAD:74-189), in named_parameters order: NOT grouped by layer
NAMES = ['final_cls.0.weight', 'final_cls2.0.weight', 'final_cls3.0.weight', 'final_reg.4.bias', 'final_reg3.4.bias',
         'rf_multihead_attn.in_proj_weight', 'rf_multihead_attn2.in_proj_weight', 'rf_multihead_attn3.out_proj.bias',
         'rf_linear1.weight', 'rf_linear1_2.weight', 'rf_linear2_3.bias', 'rf_norm2.weight', 'rf_norm3_2.bias', 'rf_norm3_3.bias',
         'radar_position_encoder.0.weight', 'radar_feat_encoder.4.bias']
LAYERS = [0, 1, 2, 0, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, None, None]


def test_exchange_chunks_of_three_layers_are_todays():
    assert [exchange_chunk_of(n) for n in NAMES] == [2, 1, 0, 2, 0, 2, 1, 0, 2, 1, 0, 2, 1, 0, 3, 3]
    assert [exchange_chunk_of(n, 3) for n in NAMES] == [exchange_chunk_of(n) for n in NAMES]
    params = lambda: [(n, torch.nn.Parameter(torch.randn(3 + i))) for i, n in enumerate(NAMES)]      # noqa: E731
    a, b = FlatBucket(params(), chunk_of=exchange_chunk_of), FlatBucket(params(), chunk_of=lambda n: exchange_chunk_of(n, 3))
    assert a.chunk_ranges == b.chunk_ranges and a.offsets == b.offsets and len(a.chunk_ranges) == 4
    for bad in BAD:
        with pytest.raises(L.TransCARHipError, match='num_fusion_layers='):
            exchange_chunk_of(NAMES[0], bad)


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_exchange_chunks_follow_the_depth(depth):
    """N + 1 contiguous chunks: fusion layer N, ..., 1, then the encoders."""
    names = [n for n, l in zip(NAMES, LAYERS) if l is None or l < depth]
    layers = [l for l in LAYERS if l is None or l < depth]
    want = [depth if l is None else depth - 1 - l for l in layers]
    assert [exchange_chunk_of(n, depth) for n in names] == want
    params = [(n, torch.nn.Parameter(torch.randn(3 + i))) for i, n in enumerate(names)]
    b = FlatBucket(params, chunk_of=lambda n: exchange_chunk_of(n, depth))
    r = b.chunk_ranges
    assert len(r) == depth + 1 and r[0][0] == 0 and r[-1][1] == b.numel
    assert all(x[1] == y[0] and x[1] > x[0] for x, y in zip(r, r[1:]))
    for (n, p), off, ch in zip(params, b.offsets, want):
        assert r[ch][0] <= off and off + p.numel() <= r[ch][1], n
        assert p.grad.data_ptr() == b.grads.data_ptr() + 4 * off and p.data_ptr() == b.params.data_ptr() + 4 * off


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_loss_names_follow_the_depth(depth, golden_dir):
    """loss(): the last level's terms are loss_cls / loss_bbox, the levels before are d0 .. d{N-2}."""
    import numpy as np
    import os
    g5 = np.load(os.path.join(golden_dir, 'g5_head_tiny.npz'))
    cfg = configs.head_cfg(num_fusion_layers=depth)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T.build_head(cfg)
    boxes, labels = synth.make_gt(seed=7, n=24)
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    outs = {'all_cls_scores': torch.from_numpy(g5['all_cls_scores'][:depth]),
            'all_bbox_preds': torch.from_numpy(g5['all_bbox_preds'][:depth])}
    out = h.loss([gt], [torch.from_numpy(labels)], outs)
    assert sorted(out) == sorted(['loss_cls', 'loss_bbox'] + ['d%d.loss_%s' % (i, k) for i in range(depth - 1)
                                                              for k in ('cls', 'bbox')])
