"""Detr3DHead(radar_num_heads=H), the head count of the radar fusion attention (4, 8 or 16 at embed_dims 256): the host
side -- the keyword and its refusals, the count in the upper 16 bits of tc_head_weights.num_heads, the library's own
refusals, the ABI, checkpoints.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

import transcar_amd as T
from transcar_amd import _lib as L
from transcar_amd import configs, synth
from transcar_amd.detr3d_head import fusion_modules

HEADS = (4, 16)
FIELDS = ['abi_version', 'num_query', 'embed_dims', 'num_heads', 'ffn_dims', 'num_layers', 'num_cams', 'num_levels',
          'num_classes', 'code_size', 'radar_in_dims', 'num_radar_layers', 'num_radar_tokens_ref', 'pc_range',
          'query_embedding', 'reference_points', 'layers', 'radar_position_encoder', 'radar_feat0', 'radar_feat2',
          'radar_feat4', 'radar', 'l0_init_reference', 'l0_attn_out', 'packed16_delta', 'num_points']


def _head(H=None, **kw):
    return T.build_head(configs.head_cfg(num_query=20, radar_num_heads=H, **kw))


def _raw(w):
    return ctypes.string_at(ctypes.addressof(w), ctypes.sizeof(w))


def test_abi_and_layout_did_not_move():
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13
    assert ctypes.sizeof(L.tc_head_weights) == 3080
    assert [f[0] for f in L.tc_head_weights._fields_] == FIELDS
    assert L.TC_RADAR_HEADS == 8 and L.TC_NUM_HEADS == (4, 8, 16)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'transcar_hip.h')).read()
    assert re.search(r'#define TC_RADAR_HEADS 8\b', text) and re.search(r'#define TC_ABI_VERSION 13\b', text)
    for name in ('TC_NUM_HEADS_PACK', 'TC_NUM_HEADS_DECODER', 'TC_NUM_HEADS_RADAR'):
        assert re.search(r'#define %s\(' % name, text), name


def test_packing():
    assert L.pack_num_heads(8) == L.pack_num_heads(8, 8) == 8 and L.pack_num_heads(4, 8) == 4
    assert L.pack_num_heads(8, 4) == (4 << 16) | 8 and L.pack_num_heads(16, 16) == (16 << 16) | 16
    assert L.pack_num_heads(4, 16) == 0x00100004


def test_default_config_is_untouched():
    assert configs.head_cfg() == configs.pts_bbox_head == configs.head_cfg(radar_num_heads=None) == configs.head_cfg(radar_num_heads=8)
    assert 'radar_num_heads' not in configs.head_cfg(radar_num_heads=8)


@pytest.mark.parametrize('H', HEADS)
def test_head_cfg_sets_that_key_only(H):
    cfg = configs.head_cfg(radar_num_heads=H)
    assert cfg.pop('radar_num_heads') == H
    assert cfg == configs.head_cfg() == configs.pts_bbox_head


@pytest.mark.parametrize('H', (4, 8, 16))
def test_head_builds_with_the_same_parameters(H):
    head = T.build_head(configs.head_cfg(radar_num_heads=H))
    sd = synth.make_state_dict(seed=3)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    assert list(head.state_dict()) == list(T.build_head(configs.head_cfg()).state_dict())
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert head.radar_num_heads == H
    for r in range(3):
        m = fusion_modules(head, r).attn
        assert m.num_heads == H and m.head_dim == 256 // H and float(m.dropout) == 0.1
    for ly in head.transformer.decoder.layers:
        assert ly.attentions[0].num_heads == 8 and ly.attentions[0].attn.num_heads == 8      # the decoder keeps its own count
    w = head.weights_struct()
    assert w.num_heads == (8 if H == 8 else (H << 16) | 8) and w.embed_dims == 256


def test_the_two_counts_are_not_confused():
    head = _head(16, num_heads=4)
    w = head.weights_struct()
    assert w.num_heads == (16 << 16) | 4
    assert all(fusion_modules(head, r).attn.num_heads == 16 for r in range(3))
    assert all(ly.attentions[0].num_heads == 4 for ly in head.transformer.decoder.layers)
    w = _head(4, num_heads=16).weights_struct()
    assert w.num_heads == (4 << 16) | 16


def test_default_struct_is_byte_identical_to_one_built_without_the_keyword():
    plain = T.build_head(configs.head_cfg(num_query=20))
    want = _raw(plain.weights_struct())
    assert plain.radar_num_heads == 8 and plain.weights_struct().num_heads == 8
    assert _head(8).weights_struct().num_heads == 8
    # a struct holds its modules' addresses: compare the bytes on ONE set of modules
    plain.radar_num_heads = _head(8).radar_num_heads
    assert _raw(plain.weights_struct()) == want


@pytest.mark.parametrize('H', HEADS)
def test_library_sizes_do_not_depend_on_the_count(H):
    lib = L.lib()

    def sizes(w):
        return (lib.tc_head_workspace_bytes(ctypes.byref(w), 2, 256), lib.tc_head_packed_bytes(ctypes.byref(w)),
                lib.tc_radar_train_tape_bytes(ctypes.byref(w), 2, 256), lib.tc_radar_train_bwd_workspace_bytes(ctypes.byref(w), 2, 256),
                lib.tc_cam_pregather_workspace_bytes(ctypes.byref(w), 2))
    want = sizes(T.build_head(configs.head_cfg()).weights_struct())
    assert all(v > 0 for v in want), want
    assert sizes(T.build_head(configs.head_cfg(radar_num_heads=H)).weights_struct()) == want


@pytest.mark.parametrize('upper', [2, 3, 32])
def test_library_refuses_other_upper_halves(upper):
    lib = L.lib()
    w = _head().weights_struct()
    w.num_heads = (upper << 16) | 8
    text = 'radar_num_heads=%d' % upper
    for query in (lambda: lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64), lambda: lib.tc_head_packed_bytes(ctypes.byref(w)),
                  lambda: lib.tc_radar_train_tape_bytes(ctypes.byref(w), 1, 64),
                  lambda: lib.tc_radar_train_bwd_workspace_bytes(ctypes.byref(w), 1, 64),
                  lambda: lib.tc_cam_pregather_workspace_bytes(ctypes.byref(w), 1)):
        assert query() == 0
        assert text in lib.tc_last_error().decode(), lib.tc_last_error().decode()
    rc = lib.tc_head_pack_weights(ctypes.byref(w), None, 0, ctypes.byref(L.tc_head_weights()), None)
    assert rc != 0 and text in lib.tc_last_error().decode()


def test_library_reads_the_halves_apart():
    lib = L.lib()
    w = _head().weights_struct()
    for upper in (0, 4, 8, 16):
        for lower in (4, 8, 16):
            w.num_heads = (upper << 16) | lower
            assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) > 0, (upper, lower)
    # a bad lower half keeps the existing text, whatever the upper half says
    for upper in (0, 4):
        w.num_heads = (upper << 16) | 2
        assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) == 0
        err = lib.tc_last_error().decode()
        assert 'num_heads=2 ' in err and 'radar_num_heads' not in err, err


@pytest.mark.parametrize('H', [2, 3, 32, 8.0, True])
def test_python_refuses_other_counts(H):
    named = re.escape('radar_num_heads=%r' % (H,))
    head = _head()

    def struct_of_bad_attribute():
        head.radar_num_heads = H                # (a public attribute: weights_struct() checks it again)
        head.weights_struct()
    for call in (lambda: L.check_radar_num_heads(H), lambda: configs.head_cfg(radar_num_heads=H), lambda: _head(H),
                 lambda: T.build_head(dict(configs.head_cfg(num_query=20), radar_num_heads=H)), struct_of_bad_attribute):
        with pytest.raises(L.TransCARHipError, match=named):
            call()


def test_struct_refuses_modules_of_another_count():
    head = _head(4)
    head.radar_num_heads = 16
    with pytest.raises(L.TransCARHipError, match='radar_num_heads=16'):
        head.weights_struct()


def test_stand_alone_entries_refuse_before_a_launch():
    lib = L.lib()
    rc = lib.tc_radar_attn_core_fwd(None, 1.0, None, None, 2, None, 10, None, 2, 1, 8, 64, 256, 2, 1, 1.0, 2.0,
                                    None, None, 0.0, 0, 0, None)
    assert rc != 0 and 'num_heads=2' in lib.tc_last_error().decode(), lib.tc_last_error().decode()
    rc = lib.tc_radar_attn_core_bwd(None, 1.0, None, None, 2, None, 10, None, 2, 1, 8, 64, 256, 2, 1, 1.0, 2.0,
                                    None, None, None, None, 0.0, 0, 0, None)
    assert rc != 0 and 'num_heads=2' in lib.tc_last_error().decode(), lib.tc_last_error().decode()
    rc = lib.tc_radar_gated_xattn_fwd(None, None, None, None, 10, None, None, 1, 8, 64, 256, 2, 1, 1.0, 2.0, None, None, None, 0, None)
    assert rc != 0 and 'num_heads=2' in lib.tc_last_error().decode(), lib.tc_last_error().decode()
    # 4 and 16 get past the count: the next refusal is about something else
    for H in HEADS:
        rc = lib.tc_radar_attn_core_fwd(None, 1.0, None, None, 2, None, 10, None, 2, 1, 8, 64, 256, H, 1, 1.0, 2.0,
                                        None, None, 0.0, 0, 0, None)
        assert rc != 0 and 'num_heads' not in lib.tc_last_error().decode(), lib.tc_last_error().decode()
        rc = lib.tc_radar_gated_xattn_fwd(None, None, None, None, 10, None, None, 1, 8, 64, 256, H, 1, 1.0, 2.0, None, None,
                                          None, 0, None)
        assert rc != 0 and 'num_heads' not in lib.tc_last_error().decode(), lib.tc_last_error().decode()


def test_checkpoint_of_an_eight_head_head_loads_into_a_four_head_one(tmp_path):
    eight = _head()
    path = str(tmp_path / 'head.pth')
    torch.save(eight.state_dict(), path)
    four = _head(4)
    four.load_state_dict(torch.load(path), strict=True)
    for (ka, a), (kb, b) in zip(eight.state_dict().items(), four.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
    assert not any('num_heads' in k for k in four.state_dict())
    assert four.weights_struct().num_heads == (4 << 16) | 8
