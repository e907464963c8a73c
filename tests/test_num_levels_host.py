"""Detr3DCrossAtten(num_levels < 4) on the host side: construction, the head's parameters and state_dict, the C struct,
the limits at the module, the head and the library, and the camera pre-gather predicate.  No GPU."""
import ctypes

import pytest
import torch

from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth
from transcar_amd.detr3d_transformer import Detr3DCrossAtten


@pytest.mark.parametrize('nl', [1, 2, 3])
def test_cross_atten_constructs(nl):
    m = Detr3DCrossAtten(num_levels=nl, num_points=1)
    assert m.num_levels == nl
    assert tuple(m.attention_weights.weight.shape) == (6 * nl, 256)
    m5 = Detr3DCrossAtten(num_levels=nl, num_points=5)
    assert tuple(m5.attention_weights.weight.shape) == (6 * 5 * nl, 256)


@pytest.mark.parametrize('nl', [1, 2, 3])
def test_head_state_dict(nl):
    cfg = configs.head_cfg(num_levels=nl)
    assert cfg['transformer']['num_feature_levels'] == nl
    head = build_head(cfg)
    assert head.transformer.num_feature_levels == nl
    sd = head.state_dict()
    for i in range(6):
        w = sd['transformer.decoder.layers.%d.attentions.1.attention_weights.weight' % i]
        assert tuple(w.shape) == (6 * nl, 256)
    assert tuple(sd['attention_weights2.weight'].shape) == (24, 256)      # HEAD:191, whatever the levels
    spec = {k: shape for k, shape, _ in synth.state_dict_spec(num_levels=nl)}
    assert set(spec) == set(sd)
    for k, shape in spec.items():
        assert tuple(sd[k].shape) == tuple(shape), k
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=7, num_levels=nl).items()},
                         strict=True)
    # a 4-level checkpoint does not load into it
    with pytest.raises(RuntimeError):
        head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=7).items()}, strict=True)
    assert head.weights_struct().num_levels == nl


def test_defaults_unchanged():
    assert configs.head_cfg() == configs.head_cfg(num_levels=None)
    assert 'num_feature_levels' not in configs.head_cfg()['transformer']
    a, b = synth.make_state_dict(seed=3), synth.make_state_dict(seed=3, num_levels=4)
    assert set(a) == set(b) and all((a[k] == b[k]).all() for k in a)
    assert build_head(configs.head_cfg()).weights_struct().num_levels == 4


@pytest.mark.reference
def test_head_keys_match_reference_at_two_levels():
    from oracle import ref_harness
    if not ref_harness.available():
        pytest.skip('reference not present')
    ref = ref_harness.build_reference_head(configs.head_cfg(num_levels=2))
    mine = build_head(configs.head_cfg(num_levels=2)).state_dict()
    theirs = ref.state_dict()
    assert set(mine) == set(theirs)
    for k in mine:
        assert tuple(mine[k].shape) == tuple(theirs[k].shape), k


@pytest.mark.parametrize('nl', [0, 5])
def test_unsupported_num_levels_raise(nl):
    with pytest.raises(L.TransCARHipError, match='num_levels=%d' % nl):
        Detr3DCrossAtten(num_levels=nl, num_points=1)
    with pytest.raises(L.TransCARHipError, match='num_levels=%d' % nl):
        build_head(configs.head_cfg(num_levels=nl))


def test_num_points_limit_counts_levels():
    # N * P * L <= 256: at 6 cameras and 3 levels P = 14 fits, 15 does not
    Detr3DCrossAtten(num_levels=3, num_points=14)
    with pytest.raises(L.TransCARHipError, match='num_points=15'):
        Detr3DCrossAtten(num_levels=3, num_points=15)
    Detr3DCrossAtten(num_levels=1, num_points=42)


def test_head_refuses_other_level_count():
    head = build_head(configs.head_cfg(num_levels=2))
    with pytest.raises(L.TransCARHipError, match='3 feature levels given.*num_levels=2'):
        head.check_feature_levels(3)
    head.check_feature_levels(2)


def test_library_refuses_num_levels_5():
    """The C boundary checks the level count itself (tc_feats_nhwc holds TC_MAX_LEVELS entries)."""
    lib = L.lib()
    fv = L.tc_feats_nhwc()
    fv.num_levels = 5
    rc = lib.tc_cross_atten_points_fwd(None, None, None, ctypes.byref(fv), 1, 900, 256, 6, 1,
                                       None, None, None, None, L.f6([0] * 6), 1.0, 1.0, None, None, 0, None)
    assert rc != 0
    assert 'num_levels=5' in lib.tc_last_error().decode()
    w = build_head(configs.head_cfg(num_levels=2)).weights_struct()
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) > 0       # 2 levels: accepted
    w.num_levels = 5
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) == 0
    assert 'num_levels=5' in lib.tc_last_error().decode()


def test_workspace_grows_with_levels():
    lib = L.lib()
    one = lib.tc_cross_atten_points_workspace_bytes(1, 900, 256, 6, 1, 5)
    four = lib.tc_cross_atten_points_workspace_bytes(1, 900, 256, 6, 4, 5)
    assert four >= one + 900 * 6 * 5 * 3 * 4
    w = build_head(configs.head_cfg(num_levels=2)).weights_struct()
    assert lib.tc_cam_pregather_workspace_bytes(ctypes.byref(w), 1) == 900 * (6 * 2 * 256 * 4 + 4)


def test_cam_pregather_predicate():
    assert L.cam_pregather_supported(256, 4, 6)
    assert L.cam_pregather_supported(256, 4, 8)
    assert not L.cam_pregather_supported(256, 4, 9)
    assert not L.cam_pregather_supported(256, 4, 16)
    for nl in (1, 2, 3):
        assert not L.cam_pregather_supported(256, nl, 6)
    assert not L.cam_pregather_supported(128, 4, 6)
    assert build_head(configs.head_cfg()).cam_pregather_supported()
    assert not build_head(configs.head_cfg(num_levels=2)).cam_pregather_supported()


def test_plugin_graph_options_follow_predicate():
    from transcar_amd.plugin_graph import PluginGraphs
    for nl, want in ((4, 1), (2, 0)):
        pg = PluginGraphs(build_head(configs.head_cfg(num_levels=nl)))
        assert pg._options(None, 1).cam_pregather == want
