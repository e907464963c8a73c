"""The packed buffer with decoder layer 0's pack-time constants, host side: tc_head_packed_bytes still refuses what it
refused, still orders the refining and the non-refining head, and counts the constants for the heads that have them.
No GPU."""
import ctypes

import torch

from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth

Q, C = 900, 256
PLANE = ((Q * C * 4 + 255) // 256) * 256          # one [Q, C] fp32 tensor as a 256-byte slice
VARIANTS = 5                                       # 4 / 8 / 16 rows fp32, 16 / 32 rows f16x2


def _head(**kw):
    h = build_head(configs.head_cfg(**kw))
    sd = synth.make_state_dict(seed=3, **kw)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return h


def _bytes(w):
    return L.lib().tc_head_packed_bytes(ctypes.byref(w))


def test_abi_is_unchanged():
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13
    assert L.tc_head_weights._fields_[-1][0] == 'num_points'


def test_refused_structs_still_give_zero():
    lib = L.lib()
    w = _head(with_box_refine=True).weights_struct()
    w.layers[2].reg = L.tc_reg_branch()
    assert _bytes(w) == 0 and b'layers[2]' in lib.tc_last_error()
    w = _head(with_box_refine=False).weights_struct()
    w.layers[3].reg = w.layers[5].reg
    assert _bytes(w) == 0 and b'layers[3]' in lib.tc_last_error()
    w = _head(with_box_refine=False).weights_struct()
    w.layers[5].reg = L.tc_reg_branch()
    assert _bytes(w) == 0 and b'layers[5]' in lib.tc_last_error()
    for field, bad in (('embed_dims', 128), ('num_levels', 0), ('num_levels', 5), ('abi_version', 12)):
        w = _head().weights_struct()
        setattr(w, field, bad)
        assert _bytes(w) == 0, field


def test_refining_and_non_refining_heads_keep_their_order():
    full = _bytes(_head(with_box_refine=True).weights_struct())
    lean = _bytes(_head(with_box_refine=False).weights_struct())
    assert lean > 0
    # reg.0 and reg.2 of five layers, three 256 x 256 copies each (tests/test_box_refine_host.py); both carry the constants
    assert full - lean >= 5 * 2 * 3 * 256 * 256 * 4
    assert lean > VARIANTS * 3 * PLANE


def test_constants_are_counted_where_they_exist():
    """One point at four levels: five blocks of three [Q, C] tensors behind l0_init_reference and l0_attn_out.  The
    generic heads (num_points > 1, fewer levels) keep layer 0's full chain and carry only the pack-time scratch
    (qk [Q, 2C] + v^T [C, qpad]), which the constants otherwise overwrite."""
    scratch = 2 * PLANE + ((C * ((Q + 15) // 16) * 16 * 4 + 255) // 256) * 256
    one = _bytes(_head().weights_struct())
    two_levels = _bytes(_head(num_levels=2).weights_struct())
    five_points = _bytes(_head(num_points=5).weights_struct())
    assert one > 0 and two_levels > 0 and five_points > 0
    # attention_weights is the only packed weight that depends on levels / points: 24 rows at most 64 -> one 64-row tile
    # either way for 2 levels (12 rows); 120 rows -> two tiles for five points, three copies, six layers
    assert one - two_levels == VARIANTS * 3 * PLANE - scratch
    assert one - five_points == VARIANTS * 3 * PLANE - scratch - 6 * 3 * 64 * 256 * 4
