"""Detr3DCrossAtten(num_points > 1) on the host side: construction, the head's
parameters and state_dict, the packed C struct and the limit.  No GPU."""
import ctypes

import pytest
import torch

from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth
from transcar_amd.detr3d_transformer import Detr3DCrossAtten


def test_cross_atten_constructs_with_reference_default():
    m = Detr3DCrossAtten(num_points=5)          # the reference class's default (XFMR:236-247)
    assert m.num_points == 5
    assert tuple(m.attention_weights.weight.shape) == (6 * 5 * 4, 256)
    assert float(m.attention_weights.weight.detach().abs().sum()) == 0.0     # XFMR:297-300


def test_head_state_dict_at_four_points():
    head = build_head(configs.head_cfg(num_points=4))
    sd = head.state_dict()
    for i in range(6):
        w = sd['transformer.decoder.layers.%d.attentions.1.attention_weights.weight' % i]
        b = sd['transformer.decoder.layers.%d.attentions.1.attention_weights.bias' % i]
        assert tuple(w.shape) == (96, 256) and tuple(b.shape) == (96,)
    spec = {k: shape for k, shape, _ in synth.state_dict_spec(num_points=4)}
    assert set(spec) <= set(sd)
    for k, shape in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    new = synth.make_state_dict(seed=7, num_points=4)
    head.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=True)
    # a P = 1 checkpoint does not load into a P = 4 head
    old = synth.make_state_dict(seed=7)
    with pytest.raises(RuntimeError):
        head.load_state_dict({k: torch.from_numpy(v) for k, v in old.items()}, strict=True)


@pytest.mark.reference
def test_head_keys_match_reference_at_four_points():
    from oracle import ref_harness
    if not ref_harness.available():
        pytest.skip('reference not present')
    ref = ref_harness.build_reference_head(configs.head_cfg(num_points=4))
    mine = build_head(configs.head_cfg(num_points=4)).state_dict()
    theirs = ref.state_dict()
    assert set(mine) == set(theirs)
    for k in mine:
        assert tuple(mine[k].shape) == tuple(theirs[k].shape), k


def test_packed_struct_carries_num_points():
    assert L.TC_ABI_VERSION == 13
    names = [f[0] for f in L.tc_head_weights._fields_]
    assert names[-1] == 'num_points'
    w = L.tc_head_weights()
    w.num_points = 5
    assert w.num_points == 5
    lib = L.lib()
    assert lib.tc_abi_version() == 13
    for fn in ('tc_cam_sample_fuse_points_fwd', 'tc_cross_atten_points_workspace_bytes',
               'tc_cross_atten_points_fwd'):
        assert hasattr(lib, fn), fn
    # workspace grows with the N * P * L logits only
    one = lib.tc_cross_atten_workspace_bytes(1, 900, 256, 6, 4)
    assert lib.tc_cross_atten_points_workspace_bytes(1, 900, 256, 6, 4, 1) == one
    five = lib.tc_cross_atten_points_workspace_bytes(1, 900, 256, 6, 4, 5)
    assert five >= one + 900 * 96 * 4


@pytest.mark.parametrize('P', [0, 11, 64])
def test_over_limit_num_points_raises(P):
    with pytest.raises(L.TransCARHipError, match='num_points=%d' % P):
        Detr3DCrossAtten(num_points=P)
    with pytest.raises(L.TransCARHipError, match='num_points=%d' % P):
        build_head(configs.head_cfg(num_points=P))


def test_library_refuses_over_limit_num_points():
    """The C boundary checks the limit itself (no silent fallback)."""
    lib = L.lib()
    fv = L.tc_feats_nhwc()
    fv.num_levels = 4
    rc = lib.tc_cross_atten_points_fwd(None, None, None, ctypes.byref(fv), 1, 900, 256, 6, 11,
                                       None, None, None, None, L.f6([0] * 6), 1.0, 1.0, None, None, 0, None)
    assert rc != 0
    assert 'num_points=11' in lib.tc_last_error().decode()
