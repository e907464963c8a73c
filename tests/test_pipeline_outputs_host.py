"""tc_decoder_outputs_levels_fwd (the decoder levels' heads over a level range) and the pipeline keywords that use it,
on the host side: declaration, binding, the unchanged ABI, every refusal and its message.  No GPU: each call below fails
on its argument check before anything is launched."""
import ctypes
import re

import pytest
import torch

import transcar_amd as T
from parity_util import header_text
from transcar_amd import _lib as L
from transcar_amd import configs, synth

ENTRY = 'tc_decoder_outputs_levels_fwd'


def _head(refine=True, **kw):
    h = T.build_head(dict(configs.head_cfg(with_box_refine=refine), **kw))
    sd = synth.make_state_dict(seed=3, with_box_refine=refine)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return h.eval()


def _packed_like(h):
    """a copy of the unpacked struct that passes for a packed view (nothing is launched below)"""
    v = L.tc_decoder_heads()
    ctypes.memmove(ctypes.byref(v), ctypes.byref(h), ctypes.sizeof(h))
    v.packed16_delta = 4 * 65536
    return v


def test_entry_is_declared_exported_and_bound():
    text = header_text(comments=False)
    dll = ctypes.CDLL(L.LIB_PATH)
    assert re.search(r'\b%s\s*\(' % ENTRY, text)
    assert hasattr(dll, ENTRY) and ENTRY in L.SIGNATURES
    res, args = L.SIGNATURES[ENTRY]
    assert res is ctypes.c_int and len(args) == 12
    # the existing entry's prototype with (first_level, num_levels) behind (B, Q)
    old = L.SIGNATURES['tc_decoder_outputs_fwd'][1]
    assert list(args[:6]) == list(old[:6]) and list(args[8:]) == list(old[6:])
    assert args[6] is ctypes.c_int and args[7] is ctypes.c_int
    assert T.lib().tc_decoder_outputs_levels_fwd.argtypes == args


def test_abi_version_and_structs_unchanged():
    assert L.TC_ABI_VERSION == 13 and T.lib().tc_abi_version() == 13
    assert [f[0] for f in L.tc_decoder_heads._fields_] == [
        'abi_version', 'num_levels', 'embed_dims', 'num_classes', 'code_size', 'pc_range', 'cls', 'reg', 'packed16_delta']
    assert L.tc_head_weights._fields_[-1][0] == 'num_points'


def test_level_range_is_refused_before_the_device_is_touched():
    lib = T.lib()
    view = _packed_like(_head(True).decoder_heads_struct())
    Lv = view.num_levels
    assert Lv == 6
    p = ctypes.c_void_p(256)

    def fwd(first, count, v=view):
        return lib.tc_decoder_outputs_levels_fwd(ctypes.byref(v), p, p, p, 1, 900, first, count, p, p, None, None)
    assert fwd(-1, 1) != 0
    assert b'first_level=-1' in lib.tc_last_error(), lib.tc_last_error()
    assert fwd(0, 0) != 0
    assert b'num_levels=0' in lib.tc_last_error(), lib.tc_last_error()
    assert fwd(2, -3) != 0
    assert b'num_levels=-3' in lib.tc_last_error(), lib.tc_last_error()
    for first, count in ((0, Lv + 1), (Lv, 1), (Lv - 1, 2), (1, Lv)):
        assert first + count == Lv + 1 or first == Lv
        assert fwd(first, count) != 0
        msg = lib.tc_last_error()
        assert (b'first_level=%d' % first) in msg and (b'num_levels=%d' % count) in msg and (b'%d levels' % Lv) in msg, msg
    # a sum that would wrap an int is refused as a range, not added up
    assert fwd(2 ** 31 - 1, 2 ** 31 - 1) != 0
    assert b'first_level=2147483647' in lib.tc_last_error(), lib.tc_last_error()


def test_refusals_of_the_existing_entry_are_kept():
    from transcar_amd.detr3d_head import head_options
    lib = T.lib()
    good = _head(True).decoder_heads_struct()
    view = _packed_like(good)
    p = ctypes.c_void_p(256)

    def fwd(v, opt=None, B=1, Q=900, hs=p):
        return lib.tc_decoder_outputs_levels_fwd(ctypes.byref(v), hs, p, p, B, Q, 5, 1, p, p,
                                                 ctypes.byref(opt) if opt else None, None)
    assert fwd(good) != 0 and b'tc_decoder_heads_pack' in lib.tc_last_error()          # not a packed view
    assert lib.tc_decoder_outputs_levels_fwd(None, p, p, p, 1, 900, 0, 1, p, p, None, None) != 0
    assert b'null tc_decoder_heads' in lib.tc_last_error()
    assert lib.tc_decoder_outputs_fwd(None, p, p, p, 1, 900, p, p, None, None) != 0
    assert b'null tc_decoder_heads' in lib.tc_last_error()
    assert fwd(view, head_options(decoder_dropout_p=0.1)) != 0 and b'decoder_dropout_p=0.1' in lib.tc_last_error()
    assert fwd(view, head_options(unfused=True)) != 0 and b'unfused=1' in lib.tc_last_error()
    o = head_options()
    o.chain_tile_rows = 5
    assert fwd(view, o) != 0 and b'chain_tile_rows=5' in lib.tc_last_error()
    assert fwd(view, head_options(tile_rows=32, matrix_path='f32')) != 0 and b'chain_tile_rows=32' in lib.tc_last_error()
    assert fwd(view, B=0) != 0 and b'B=0' in lib.tc_last_error()
    assert fwd(view, hs=None) != 0 and b'null argument' in lib.tc_last_error()
    bad = _packed_like(good)
    bad.abi_version = L.TC_ABI_VERSION - 1
    assert fwd(bad) != 0 and b'abi_version=12' in lib.tc_last_error()


def test_head_level_ranges():
    h = _head()
    assert h.decoder_level_range(None) == (0, 6) and h.decoder_level_range('all') == (0, 6)
    assert h.decoder_level_range('last') == (5, 1) and h.decoder_level_range((1, 2)) == (1, 2)
    for bad in ((-1, 1), (0, 0), (5, 2), (6, 1)):
        with pytest.raises(L.TransCARHipError, match=r'levels=\(%d, %d\)' % bad):
            h.decoder_level_range(bad)
    with pytest.raises(L.TransCARHipError, match='first'):
        h.decoder_level_range('first')


def test_pipeline_keywords_are_checked_before_any_input_is_read():
    """Each refusal names the offending value and comes before a lane's tensors are looked at (the lane dict below has
    nothing a capture could use)."""
    from transcar_amd.pipeline import FramePipeline
    lane = [dict(l2i=torch.zeros(1, 6, 4, 4))]
    h = _head()
    with pytest.raises(L.TransCARHipError, match="outputs='panoptic'"):
        FramePipeline(h, lane, outputs='panoptic')
    with pytest.raises(L.TransCARHipError, match="decoder_levels='first'"):
        FramePipeline(h, lane, decoder_levels='first')
    with pytest.raises(L.TransCARHipError, match=r"outputs='fusion' is not supported in a pipeline built for outputs='camera'"):
        FramePipeline(h, lane, outputs='camera')
    with pytest.raises(L.TransCARHipError, match=r"decoder_levels='last' with outputs='fusion'"):
        FramePipeline(h, lane, decoder_levels='last')
    h.outputs = 'all'
    with pytest.raises(L.TransCARHipError, match=r"decoder_levels='last' with outputs='all'"):
        FramePipeline(h, lane, outputs='all', decoder_levels='last')
    with pytest.raises(L.TransCARHipError, match=r"outputs='all' is not supported in a pipeline built for outputs='fusion'"):
        FramePipeline(h, lane)
    h.outputs = 'camera'
    with pytest.raises(L.TransCARHipError, match=r"outputs='camera' is not supported in a pipeline built for outputs='all'"):
        FramePipeline(h, lane, outputs='all')
    with pytest.raises(L.TransCARHipError, match='radar_raw_capacity=256'):
        FramePipeline(h, lane, outputs='camera', radar_raw_capacity=256)
    with pytest.raises(L.TransCARHipError, match='radar_rows_capacity=64'):
        FramePipeline(h, lane, outputs='camera', radar_rows_capacity=64)
