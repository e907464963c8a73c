"""The decoder self-attention's head count (attn_cfgs[0].num_heads: 4, 8 or 16 at embed_dims 256) on the host side:
configs.head_cfg, construction and the state dict, the C struct, and the refusals at the config, the brick and the
library.  No GPU."""
import ctypes

import pytest
import torch

from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth
from transcar_amd.bricks import MultiheadAttention

FIELDS = ['abi_version', 'num_query', 'embed_dims', 'num_heads', 'ffn_dims', 'num_layers', 'num_cams', 'num_levels',
          'num_classes', 'code_size', 'radar_in_dims', 'num_radar_layers', 'num_radar_tokens_ref', 'pc_range',
          'query_embedding', 'reference_points', 'layers', 'radar_position_encoder', 'radar_feat0', 'radar_feat2',
          'radar_feat4', 'radar', 'l0_init_reference', 'l0_attn_out', 'packed16_delta', 'num_points']


def _attn_cfg(cfg):
    return cfg['transformer']['decoder']['transformerlayers']['attn_cfgs'][0]


def test_abi_is_unchanged():
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13
    assert [f[0] for f in L.tc_head_weights._fields_] == FIELDS
    assert ctypes.sizeof(L.tc_head_weights) == 3080
    assert L.TC_RADAR_HEADS == 8 and L.TC_NUM_HEADS == (4, 8, 16)


def test_head_cfg_default_is_pts_bbox_head():
    assert configs.head_cfg() == configs.pts_bbox_head
    assert configs.head_cfg() == configs.head_cfg(num_heads=None) == configs.head_cfg(num_heads=8)
    assert _attn_cfg(configs.head_cfg())['num_heads'] == 8


@pytest.mark.parametrize('H', [4, 16])
def test_head_cfg_overrides_only_the_decoder_attention(H):
    cfg = configs.head_cfg(num_heads=H)
    assert _attn_cfg(cfg)['num_heads'] == H
    _attn_cfg(cfg)['num_heads'] = 8
    assert cfg == configs.pts_bbox_head
    assert _attn_cfg(configs.pts_bbox_head)['num_heads'] == 8           # the module's own dict is not touched


@pytest.mark.parametrize('H', [4, 16])
def test_head_builds_and_loads_the_same_state_dict(H):
    head = build_head(configs.head_cfg(num_heads=H))
    ref = build_head(configs.head_cfg()).state_dict()
    sd = head.state_dict()
    assert set(sd) == set(ref) and all(sd[k].shape == ref[k].shape for k in sd)    # the head count adds no parameter
    head.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed=3).items()}, strict=True)
    for ly in head.transformer.decoder.layers:
        assert ly.attentions[0].num_heads == H and ly.attentions[0].attn.num_heads == H
    for m in (head.rf_multihead_attn, head.rf_multihead_attn2, head.rf_multihead_attn3):
        assert m.num_heads == L.TC_RADAR_HEADS                           # the radar attention keeps its 8
    w = head.weights_struct()
    assert w.num_heads == H and w.embed_dims == 256


def _sizes(w):
    lib = L.lib()
    return lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256), lib.tc_head_packed_bytes(ctypes.byref(w))


@pytest.mark.parametrize('H', [4, 16])
def test_library_sizes_do_not_depend_on_the_head_count(H):
    want = _sizes(build_head(configs.head_cfg()).weights_struct())
    assert want[0] > 0 and want[1] > 0
    assert _sizes(build_head(configs.head_cfg(num_heads=H)).weights_struct()) == want


@pytest.mark.parametrize('H', [2, 32])
def test_library_refuses_other_head_counts(H):
    lib = L.lib()
    w = build_head(configs.head_cfg()).weights_struct()
    w.num_heads = H
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) == 0
    assert 'num_heads=%d' % H in lib.tc_last_error().decode()
    assert lib.tc_head_packed_bytes(ctypes.byref(w)) == 0
    assert 'num_heads=%d' % H in lib.tc_last_error().decode()
    # the stand-alone operator: refused before anything is launched (no GPU needed)
    rc = lib.tc_self_attn_fwd(None, None, None, None, 1, 900, 256, H, None, 0, None)
    assert rc != 0 and 'num_heads=%d' % H in lib.tc_last_error().decode()


@pytest.mark.parametrize('H', [2, 3, 32, 8.0, True])
def test_python_refuses_other_head_counts(H):
    with pytest.raises(L.TransCARHipError, match='num_heads=%r' % (H,)):
        configs.head_cfg(num_heads=H)
    with pytest.raises(L.TransCARHipError, match='num_heads=%r' % (H,)):
        L.check_num_heads(H)
    with pytest.raises(L.TransCARHipError, match='num_heads=%r' % (H,)):
        MultiheadAttention(256, H, dropout=0.1)


def test_head_refuses_a_config_edited_by_hand():
    cfg = configs.head_cfg()
    _attn_cfg(cfg)['num_heads'] = 2
    with pytest.raises(L.TransCARHipError, match='num_heads=2'):
        build_head(cfg)


def test_explicit_head_dimension_entry_points_check_it():
    """tc_sdpa_fwd_hd / tc_sdpa_fwd_f16x2_hd refuse a head dimension the cores do not have, naming it, before a launch."""
    lib = L.lib()
    for hd in (8, 24, 128):
        assert lib.tc_sdpa_fwd_hd(None, None, 512, None, 912, None, 256, 1, 900, 256 // hd if 256 % hd == 0 else 8, hd, None) != 0
        assert 'head dimension %d' % hd in lib.tc_last_error().decode()
        assert lib.tc_sdpa_fwd_f16x2_hd(None, None, 912, None, 256, 1, 900, 8, hd, None) != 0
        assert 'head dimension %d' % hd in lib.tc_last_error().decode()
