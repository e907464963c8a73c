"""The decoder layers' feedforward_channels (tc_head_weights.ffn_dims: a multiple of 256 from 256 to 2048) on the host
side: configs.head_cfg, construction and the state dict, the C struct, the refusals at the config, the brick, the head and
the library, and the training entries' sizes, which follow the fusion layers' own width (TC_RADAR_FFN_DIMS).  No GPU."""
import ctypes

import pytest
import torch

from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth
from transcar_amd.bricks import DetrTransformerDecoderLayer

WIDTHS = (256, 768, 1024, 2048)
REFUSED = (0, 128, 640, 2304)


def _layers(cfg):
    return cfg['transformer']['decoder']['transformerlayers']


def test_constants_and_abi():
    assert (L.TC_FFN_DIMS_MIN, L.TC_FFN_DIMS_MAX, L.TC_FFN_DIMS_STEP, L.TC_RADAR_FFN_DIMS) == (256, 2048, 256, 512)
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13
    assert ctypes.sizeof(L.tc_head_weights) == 3080              # ffn_dims was a field already: no struct changes


def test_head_cfg_default_is_todays_dict():
    assert configs.head_cfg() == configs.pts_bbox_head
    assert configs.head_cfg(feedforward_channels=None) == configs.head_cfg(feedforward_channels=512) == configs.pts_bbox_head
    assert _layers(configs.pts_bbox_head)['feedforward_channels'] == 512


@pytest.mark.parametrize('F', WIDTHS)
def test_head_cfg_overrides_only_the_decoder_ffn(F):
    cfg = configs.head_cfg(feedforward_channels=F)
    assert _layers(cfg)['feedforward_channels'] == F
    _layers(cfg)['feedforward_channels'] = 512
    assert cfg == configs.pts_bbox_head
    assert _layers(configs.pts_bbox_head)['feedforward_channels'] == 512        # the module's own dict is not touched


@pytest.mark.parametrize('F', WIDTHS)
def test_head_builds_and_loads_the_synth_state_dict(F):
    head = build_head(configs.head_cfg(feedforward_channels=F))
    sd = synth.make_state_dict(seed=3, feedforward_channels=F)
    ref = synth.make_state_dict(seed=3)
    assert set(sd) == set(ref)
    for k in sd:                                  # only the decoder's FFN follows the width; rf_linear* keep 512
        if '.ffns.0.layers.0.0.' in k:
            assert sd[k].shape[0] == F, k
        elif k.endswith('.ffns.0.layers.1.weight'):
            assert sd[k].shape == (256, F), k
        else:
            assert sd[k].shape == ref[k].shape, k
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    for ly in head.transformer.decoder.layers:
        assert ly.ffns[0].feedforward_channels == F
    assert head.rf_linear1.out_features == head.rf_linear2.in_features == L.TC_RADAR_FFN_DIMS
    w = head.weights_struct()
    assert w.ffn_dims == F and w.embed_dims == 256
    lib = L.lib()
    assert lib.tc_head_packed_bytes(ctypes.byref(w)) > 0 and lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) > 0


def test_packed_bytes_follow_the_width():
    """Three copies of ffn0 [F, 256] and ffn1 [256, F] per layer: 6 * 3 * 2 * 256 * 4 bytes per hidden unit."""
    lib = L.lib()
    size = {F: lib.tc_head_packed_bytes(ctypes.byref(build_head(configs.head_cfg(feedforward_channels=F)).weights_struct()))
            for F in (256, 512, 1024)}
    assert size[1024] - size[512] == 2 * (size[512] - size[256]) == 512 * 6 * 3 * 2 * 256 * 4


@pytest.mark.parametrize('F', REFUSED + (512.0, True, None))
def test_python_refuses_other_widths(F):
    with pytest.raises(L.TransCARHipError, match='ffn_dims=%r' % (F,)):
        L.check_ffn_dims(F)
    if F is not None:                             # (None is head_cfg's "leave the configs' value")
        with pytest.raises(L.TransCARHipError, match='ffn_dims=%r' % (F,)):
            configs.head_cfg(feedforward_channels=F)
    with pytest.raises(L.TransCARHipError, match='ffn_dims=%r' % (F,)):
        DetrTransformerDecoderLayer(_layers(configs.pts_bbox_head)['attn_cfgs'], F, ffn_dropout=0.1,
                                    operation_order=('self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm'))


@pytest.mark.parametrize('F', REFUSED)
def test_head_refuses_a_config_edited_by_hand(F):
    cfg = configs.head_cfg()
    _layers(cfg)['feedforward_channels'] = F
    with pytest.raises(L.TransCARHipError, match='ffn_dims=%d' % F):
        build_head(cfg)


@pytest.mark.parametrize('F', REFUSED)
def test_library_refuses_other_widths(F):
    """tc_head_packed_bytes validates before it touches a device: the fused entries' refusal, naming ffn_dims and the set."""
    lib = L.lib()
    w = build_head(configs.head_cfg()).weights_struct()
    w.ffn_dims = F
    assert lib.tc_head_packed_bytes(ctypes.byref(w)) == 0
    msg = lib.tc_last_error().decode()
    assert 'ffn_dims=%d' % F in msg and '256' in msg and '2048' in msg, msg
    # ... and so does the packer itself (null buffers: refused before them)
    assert lib.tc_head_pack_weights(ctypes.byref(w), None, 0, None, None) != 0
    assert 'ffn_dims=%d' % F in lib.tc_last_error().decode()
    # the one-layer entry with a width
    rc = lib.tc_decoder_layer_tail_fwd_ffn(None, None, None, 1, 900, 6, 10, None, None, None, None, None, None, 928.0, 1600.0,
                                           None, None, None, None, 912, 0, F, None)
    assert rc != 0


def test_operator_by_operator_sizes_keep_accepting_multiples_of_32():
    """tc_head_workspace_bytes serves the unfused forward too, which runs any multiple of 32 as it did."""
    lib = L.lib()
    w = build_head(configs.head_cfg()).weights_struct()
    w.ffn_dims = 640
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) > 0
    w.ffn_dims = 100
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 256) == 0
    assert 'ffn_dims=100' in lib.tc_last_error().decode()


def test_differing_widths_per_layer_are_refused():
    head = build_head(configs.head_cfg())
    wide = build_head(configs.head_cfg(feedforward_channels=1024))
    head.transformer.decoder.layers[3].ffns[0] = wide.transformer.decoder.layers[3].ffns[0]
    with pytest.raises(NotImplementedError, match='ffn_dims'):
        head.weights_struct()


def test_training_sizes_do_not_depend_on_the_decoder_width():
    """The tapes and workspaces of the training entries hold the FUSION layers' hidden activations, TC_RADAR_FFN_DIMS wide
    (rf_linear1 is Linear(256, 512) whatever the decoder's feedforward_channels)."""
    lib = L.lib()
    sizes = {}
    for F in (256, 512, 2048):
        w = build_head(configs.head_cfg(feedforward_channels=F)).weights_struct()
        sizes[F] = (lib.tc_radar_train_tape_bytes(ctypes.byref(w), 1, 256),
                    lib.tc_radar_train_bwd_workspace_bytes(ctypes.byref(w), 1, 256))
        assert min(sizes[F]) > 0, (F, lib.tc_last_error().decode())
    assert sizes[256] == sizes[512] == sizes[2048]
