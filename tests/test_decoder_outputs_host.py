"""Detr3DHead(outputs=...) and the C entries behind it (tc_decoder_heads_pack, tc_decoder_outputs_fwd) on the host
side: declarations, bindings, the unchanged ABI, every refusal and its message.  No GPU: each call below fails on its
argument check before anything is launched."""
import ctypes
import re

import pytest
import torch

import transcar_amd as T
from parity_util import header_text
from transcar_amd import _lib as L
from transcar_amd import configs, synth

ENTRIES = ('tc_decoder_heads_packed_bytes', 'tc_decoder_heads_pack', 'tc_decoder_outputs_fwd')


def _head(refine=True, **kw):
    h = T.build_head(dict(configs.head_cfg(with_box_refine=refine), **kw))
    sd = synth.make_state_dict(seed=3, with_box_refine=refine)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return h.eval()


def test_entries_are_declared_exported_and_bound():
    text = header_text(comments=False)
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert hasattr(dll, name) and name in L.SIGNATURES, name
    assert 'tc_decoder_heads' in text and hasattr(L, 'tc_decoder_heads')


def test_abi_version_stays_13_and_head_weights_unchanged():
    assert L.TC_ABI_VERSION == 13 and T.lib().tc_abi_version() == 13
    assert L.tc_head_weights._fields_[-1][0] == 'num_points'
    assert [f[0] for f in L.tc_decoder_heads._fields_][:8] == [
        'abi_version', 'num_levels', 'embed_dims', 'num_classes', 'code_size', 'pc_range', 'cls', 'reg']


def test_struct_names_every_level_and_shares_without_refinement():
    h = _head(True).decoder_heads_struct()
    assert (h.num_levels, h.embed_dims, h.num_classes, h.code_size) == (6, 256, 10, 10)
    assert len({h.cls[l].l0.w for l in range(6)}) == 6 and len({h.reg[l].l4.w for l in range(6)}) == 6
    full = T.lib().tc_decoder_heads_packed_bytes(ctypes.byref(h))
    s = _head(False).decoder_heads_struct()
    assert len({s.cls[l].l0.w for l in range(6)}) == 1 and len({s.reg[l].l2.w for l in range(6)}) == 1
    shared = T.lib().tc_decoder_heads_packed_bytes(ctypes.byref(s))
    # four 256 x 256 matrices a level, three copies of 4 bytes a weight; shared levels are packed once
    assert full == 6 * 4 * 3 * 256 * 256 * 4 and shared == 4 * 3 * 256 * 256 * 4


def _copy(h):
    c = L.tc_decoder_heads()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(h), ctypes.sizeof(h))
    return c


def test_library_refuses_and_names_the_value():
    lib = T.lib()
    good = _head(True).decoder_heads_struct()

    def refused(h, *words):
        assert lib.tc_decoder_heads_packed_bytes(ctypes.byref(h)) == 0
        msg = lib.tc_last_error()
        assert all(w in msg for w in words), msg
        assert lib.tc_decoder_heads_pack(ctypes.byref(h), None, 0, None, None) != 0
        msg = lib.tc_last_error()
        assert all(w in msg for w in words), msg
        assert lib.tc_decoder_outputs_fwd(ctypes.byref(h), None, None, None, 1, 900, None, None, None, None) != 0
        msg = lib.tc_last_error()
        assert all(w in msg for w in words), msg
    for field, values in (('embed_dims', (128, 512)), ('num_levels', (0, L.TC_MAX_LAYERS + 1)),
                          ('num_classes', (0, 33)), ('code_size', (7, 11))):
        for v in values:
            h = _copy(good)
            setattr(h, field, v)
            refused(h, ('%s=%d' % (field, v)).encode())
    h = _copy(good)
    h.abi_version = L.TC_ABI_VERSION - 1
    refused(h, b'abi_version=12')
    h = _copy(good)
    h.cls[3].l3.w = None
    refused(h, b'level 3', b'cls_branches')
    h = _copy(good)
    h.reg[5].l4.b = None
    refused(h, b'level 5', b'reg_branches')
    # a level beyond num_levels may be empty
    h = _copy(good)
    h.num_levels = 2
    h.cls[4] = L.tc_cls_branch()
    assert lib.tc_decoder_heads_packed_bytes(ctypes.byref(h)) == 2 * 4 * 3 * 256 * 256 * 4
    # pack: outputs and size
    assert lib.tc_decoder_heads_pack(ctypes.byref(good), None, 0, None, None) != 0 and b'null output' in lib.tc_last_error()
    view = L.tc_decoder_heads()
    assert lib.tc_decoder_heads_pack(ctypes.byref(good), ctypes.c_void_p(256), 16, ctypes.byref(view), None) != 0
    assert b'too small' in lib.tc_last_error()


def test_forward_entry_refuses_options_and_unpacked_views():
    from transcar_amd.detr3d_head import head_options
    lib = T.lib()
    good = _head(True).decoder_heads_struct()
    p = ctypes.c_void_p(256)

    def fwd(h, opt, B=1, Q=900):
        return lib.tc_decoder_outputs_fwd(ctypes.byref(h), p, p, p, B, Q, p, p, ctypes.byref(opt) if opt else None, None)
    assert fwd(good, None) != 0 and b'tc_decoder_heads_pack' in lib.tc_last_error()      # not a packed view
    view = _copy(good)
    view.packed16_delta = 4 * 65536
    assert fwd(view, head_options(decoder_dropout_p=0.1)) != 0 and b'decoder_dropout_p=0.1' in lib.tc_last_error()
    assert fwd(view, head_options(unfused=True)) != 0 and b'unfused=1' in lib.tc_last_error()
    o = head_options()
    o.chain_tile_rows = 5
    assert fwd(view, o) != 0 and b'chain_tile_rows=5' in lib.tc_last_error()
    assert fwd(view, head_options(tile_rows=32, matrix_path='f32')) != 0 and b'chain_tile_rows=32' in lib.tc_last_error()
    assert fwd(view, None, B=0) != 0 and b'B=0' in lib.tc_last_error()
    assert lib.tc_decoder_outputs_fwd(ctypes.byref(view), None, p, p, 1, 900, p, p, None, None) != 0
    assert b'null argument' in lib.tc_last_error()


def test_outputs_keyword_default_and_bogus_value():
    assert _head().outputs == 'fusion'
    for v in ('camera', 'all'):
        assert _head(outputs=v).outputs == v
    with pytest.raises(ValueError, match='bogus'):
        _head(outputs='bogus')
    h = _head()
    h.outputs = 'decoder'                                  # a plain attribute: checked again by forward
    with pytest.raises(ValueError, match='decoder'):
        h([torch.zeros(1, 6, 256, 2, 2)] * 4, synth.make_img_metas(1))


@pytest.mark.parametrize('outputs', ['camera', 'all'])
def test_training_mode_and_pipeline_refuse(outputs):
    from transcar_amd.pipeline import FramePipeline
    h = _head(outputs=outputs)
    h.train()
    with pytest.raises(L.TransCARHipError, match='not supported in training mode'):
        h([torch.zeros(1, 6, 256, 2, 2)] * 4, synth.make_img_metas(1))
    h.eval()
    with pytest.raises(L.TransCARHipError, match='not supported in a pipeline'):
        FramePipeline(h, [dict(l2i=torch.zeros(1, 6, 4, 4))])
    from transcar_amd.plugin_graph import PluginGraphs
    feats = [torch.zeros(1, 6, 256, 2, 2)] * 4
    assert PluginGraphs(h).eligible(feats, synth.make_img_metas(1, radar=synth.make_radar_frame(seed=1, n_per_radar=3)),
                                    False) is False
