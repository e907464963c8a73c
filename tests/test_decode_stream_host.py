"""The box decode's second kernel on the host side: the entries that name a kernel are exported and bound, the ABI
version is what it was, the caps of the header and of the binding agree, and the refusals that need no launch.  No GPU."""
import ctypes

import pytest

from parity_util import header_define
from transcar_amd import _lib as L

PCR = (ctypes.c_float * 6)(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)


def test_path_entries_are_exported_and_bound():
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ('tc_box_decode_topk_path', 'tc_box_decode_kept_path'):
        assert hasattr(dll, name), name
        assert name in L.SIGNATURES
        # the entry without a path + one trailing int
        res, args = L.SIGNATURES[name]
        res0, args0 = L.SIGNATURES[name[:-len('_path')]]
        assert res is res0 and args == args0 + [ctypes.c_int]
    assert L.lib().tc_box_decode_topk_path.argtypes[-1] is ctypes.c_int


def test_abi_version_stays_13():
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13 and header_define('TC_ABI_VERSION') == 13


def test_caps_of_header_and_binding_agree():
    for name in ('TC_BOX_DECODE_MAX_SCORES', 'TC_BOX_DECODE_MAX_NUM', 'TC_BOX_DECODE_STREAM_MAX_SCORES',
                 'TC_BOX_DECODE_STREAM_MAX_NUM'):
        assert getattr(L, name) == header_define(name), name
    assert (L.TC_BOX_DECODE_MAX_SCORES, L.TC_BOX_DECODE_MAX_NUM) == (12288, 512)
    assert (L.TC_BOX_DECODE_STREAM_MAX_SCORES, L.TC_BOX_DECODE_STREAM_MAX_NUM) == (1 << 20, 2048)
    assert (L.TC_DECODE_AUTO, L.TC_DECODE_REGISTERS, L.TC_DECODE_STREAM) == (0, 1, 2)
    assert L.lib().tc_box_decode_workspace_bytes(9, 4096, 32) == 256       # the streaming kernel needs no workspace


def _topk(Q, ncls, K, path, code=10):
    lib = L.lib()
    rc = lib.tc_box_decode_topk_path(None, None, 1, Q, ncls, code, K, PCR, None, None, None, None, None, 0, None, path)
    return rc, lib.tc_last_error().decode()


def _kept(Q, ncls, K, path):
    lib = L.lib()
    rc = lib.tc_box_decode_kept_path(None, None, 1, Q, ncls, 10, K, PCR, 0.0, 0, 1, None, None, None, None, None, path)
    return rc, lib.tc_last_error().decode()


@pytest.mark.parametrize('call', [_topk, _kept])
def test_refusals_name_the_value_before_any_launch(call):
    """Every argument check comes before the outputs are looked at: with null outputs, a shape inside the caps gets as
    far as the refusal of the missing outputs, a shape beyond them is refused by name."""
    for path in (0, 1, 2):
        rc, msg = call(900, 10, 2049, path)
        assert rc != 0 and 'max_num=2049' in msg, msg
        rc, msg = call((1 << 20) + 1, 1, 300, path)
        assert rc != 0 and 'Q*num_classes=1048577' in msg, msg
        rc, msg = call(70000, 70000, 300, path)               # the product does not fit 32 bits
        assert rc != 0 and 'Q*num_classes=4900000000' in msg, msg
    # the in-register kernel named at a shape it cannot take
    rc, msg = call(1229, 10, 300, 1)
    assert rc != 0 and 'Q*num_classes=12290' in msg and 'path 1' in msg, msg
    rc, msg = call(900, 10, 513, 1)
    assert rc != 0 and 'max_num=513' in msg and 'path 1' in msg, msg
    rc, msg = call(900, 10, 300, 3)
    assert rc != 0 and 'path=3' in msg, msg
    # inside the caps: only the missing outputs are left to refuse
    for Q, ncls, K, path in ((1229, 10, 300, 0), (900, 10, 513, 0), (900, 10, 300, 2), (32768, 32, 2048, 0),
                             (900, 10, 300, 1)):
        rc, msg = call(Q, ncls, K, path)
        assert rc != 0 and 'output' in msg, (Q, ncls, K, path, msg)
