"""The device Hungarian assignment beyond 1 024 queries / 128 boxes on the host side: the two entries are declared,
exported and bound under the unchanged ABI version, the caps and path constants of the header and of the binding
agree, the workspace query answers without a device, and the gate of device_loss.py states the same caps.  No GPU."""
import ctypes
import re

import pytest

from parity_util import header_define, header_text
from transcar_amd import _lib as L

ENTRIES = ('tc_lsa_workspace_bytes', 'tc_lsa_assign_ws')


def test_entries_are_declared_exported_and_bound_under_abi_13():
    text = header_text()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r'\b%s\(' % name, text), name
        assert name in L.SIGNATURES, name
        assert hasattr(dll, name), name
    assert L.SIGNATURES['tc_lsa_workspace_bytes'] == (ctypes.c_size_t, [ctypes.c_int] * 4)
    # tc_lsa_assign_ex + (workspace, workspace_bytes, path) in front of the stream
    res, args = L.SIGNATURES['tc_lsa_assign_ws']
    res0, args0 = L.SIGNATURES['tc_lsa_assign_ex']
    assert res is res0 and args == args0[:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int] + args0[-1:]
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13 and header_define('TC_ABI_VERSION') == 13


def test_caps_and_paths_of_header_and_binding_agree():
    for name in ('TC_LSA_MAX_QUERIES', 'TC_LSA_MAX_GT', 'TC_LSA_SMALL_MAX_QUERIES', 'TC_LSA_SMALL_MAX_GT',
                 'TC_LSA_AUTO', 'TC_LSA_SMALL', 'TC_LSA_LARGE'):
        assert getattr(L, name) == header_define(name), name
    assert (L.TC_LSA_MAX_QUERIES, L.TC_LSA_MAX_GT) == (4096, 512)
    assert (L.TC_LSA_SMALL_MAX_QUERIES, L.TC_LSA_SMALL_MAX_GT) == (1024, 128)
    assert (L.TC_LSA_AUTO, L.TC_LSA_SMALL, L.TC_LSA_LARGE) == (0, 1, 2)


def test_workspace_bytes_is_zero_where_the_small_kernel_runs():
    lib = L.lib()
    assert lib.tc_lsa_workspace_bytes(3, 1, 4097, 24) == 0 and lib.tc_last_error() != b''
    # an accepted shape clears the message: 0 + an empty tc_last_error is "no workspace", not a refusal
    assert lib.tc_lsa_workspace_bytes(3, 2, 900, 24) == 0 and lib.tc_last_error() == b''
    assert lib.tc_lsa_workspace_bytes(3, 1, 1024, 128) == 0 and lib.tc_last_error() == b''


def test_workspace_bytes_is_the_documented_formula():
    """[P][Gmax][Qpad] floats (Qpad = Q rounded up to 64), then one flag word per problem; each of the two rounded up
    to 256 bytes."""
    lib = L.lib()
    P, Q, G = 3 * 2, 1300, 150
    qpad = 1344
    want = (P * G * qpad * 4 + 255) // 256 * 256 + 256
    assert lib.tc_lsa_workspace_bytes(3, 2, Q, G) == want == 4838656
    assert L.lsa_large_workspace_bytes(3, 2, Q, G) == want
    # the first shapes past either limit of the small kernel, and both caps
    for Lyr, B, Q, G in ((3, 1, 1025, 1), (3, 1, 900, 129), (1, 1, 4096, 512)):
        assert lib.tc_lsa_workspace_bytes(Lyr, B, Q, G) == L.lsa_large_workspace_bytes(Lyr, B, Q, G) > 0


@pytest.mark.parametrize('Q,G,named', [(4097, 24, 'Q=4097'), (900, 513, 'Gmax=513'), (100, 101, 'Gmax=101')])
def test_workspace_bytes_refuses_shapes_beyond_the_caps(Q, G, named):
    lib = L.lib()
    assert lib.tc_lsa_workspace_bytes(3, 1, Q, G) == 0
    assert named in lib.tc_last_error().decode(), lib.tc_last_error().decode()


def test_device_assign_supported_states_the_caps():
    from transcar_amd.device_loss import device_assign_supported
    for Q, G in ((900, 24), (900, 129), (1300, 150), (4096, 512), (512, 512)):
        assert device_assign_supported(Q, G) is True, (Q, G)
    for Q, G in ((4097, 1), (900, 513), (100, 101), (900, 0)):
        assert device_assign_supported(Q, G) is False, (Q, G)
