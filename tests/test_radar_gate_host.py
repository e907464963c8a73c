"""Detr3DHead(radar_gate=...): the host side -- the keyword and its refusals, the (radius_min, radius_max) encoding in the
C struct, the library's own refusals, the ABI.  No GPU."""
import ctypes

import pytest

import transcar_amd as T
from head_variant_rig import CIRCLE, WIDE3
from transcar_amd import _lib as L
from transcar_amd import configs
from transcar_amd import detr3d_head as D

DEFAULT3 = dict(type='three_circle', radii=((1.0, 2.0), (1.0, 2.0), (0.5, 1.0)))


def _head(gate=None, **kw):
    return T.build_head(configs.head_cfg(num_query=20, radar_gate=gate, **kw))


def _raw(w):
    return ctypes.string_at(ctypes.addressof(w), ctypes.sizeof(w))


def test_constants_and_abi_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'transcar_hip.h')).read()
    for name, want in (('TC_RADAR_GATE_CIRCLE', -1.0), ('TC_RADAR_RADIUS_MIN', 0.125), ('TC_RADAR_RADIUS_MAX', 16.0)):
        m = re.search(r'#define %s \(?(-?[0-9.]+)f\)?' % name, text)
        assert m and float(m.group(1)) == want == getattr(L, name), name
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13
    assert ctypes.sizeof(L.tc_head_weights) == 3080
    rl = L.tc_radar_layer
    assert rl.radius_max.offset == rl.radius_min.offset + 4 and rl.packed16_delta.offset == rl.radius_min.offset + 8
    assert D.RADAR_RADII == ((1.0, 2.0), (1.0, 2.0), (0.5, 1.0))


def test_normalised_gates():
    assert L.check_radar_gate(None) == DEFAULT3 == L.check_radar_gate(dict(type='three_circle'))
    assert L.check_radar_gate(dict(type='three_circle', radii=[[1, 2], (1.0, 2.0), (0.5, 1)])) == DEFAULT3
    assert L.check_radar_gate(CIRCLE) == dict(type='circle', radii=(2.0, 2.0, 1.0))
    assert L.check_radar_gate(L.check_radar_gate(CIRCLE)) == L.check_radar_gate(CIRCLE)          # idempotent
    assert L.check_radar_gate(WIDE3)['radii'] == ((0.75, 3.0), (0.5, 1.5), (0.25, 0.75))
    # the end points of the accepted range
    assert L.check_radar_gate(dict(type='circle', radii=[0.125, 16, 16.0]))['radii'] == (0.125, 16.0, 16.0)
    assert L.check_radar_gate(dict(type='three_circle', radii=[(0.125, 16.0)] * 3))['radii'] == ((0.125, 16.0),) * 3
    assert L.radar_gate_pairs(L.check_radar_gate(CIRCLE)) == [(-1.0, 2.0), (-1.0, 2.0), (-1.0, 1.0)]
    assert L.radar_gate_pairs(L.check_radar_gate(None)) == list(D.RADAR_RADII)
    for gate in (None, CIRCLE, WIDE3):
        h = _head(gate)
        assert h.radar_gate == L.check_radar_gate(gate)
    assert 'radar_gate' not in configs.head_cfg()
    assert configs.head_cfg(radar_gate=CIRCLE)['radar_gate'] == dict(type='circle', radii=[2.0, 2.0, 1.0])


BAD = [
    ('length', dict(type='circle', radii=[2.0, 2.0])),
    ('length', dict(type='circle', radii=[2.0, 2.0, 1.0, 1.0])),
    ('length', dict(type='circle', radii=[])),
    ('length', dict(type='three_circle', radii=[(1.0, 2.0)])),
    ('missing radii', dict(type='circle')),
    ('radii type', dict(type='circle', radii=2.0)),
    ('order', dict(type='three_circle', radii=[(2.0, 1.0), (1.0, 2.0), (0.5, 1.0)])),
    ('range low', dict(type='circle', radii=[0.1, 2.0, 1.0])),
    ('range high', dict(type='circle', radii=[2.0, 16.5, 1.0])),
    ('range low', dict(type='three_circle', radii=[(0.0, 2.0), (1.0, 2.0), (0.5, 1.0)])),
    ('range high', dict(type='three_circle', radii=[(1.0, 17.0), (1.0, 2.0), (0.5, 1.0)])),
    ('negative', dict(type='circle', radii=[-1.0, 2.0, 1.0])),
    ('nan', dict(type='circle', radii=[float('nan'), 2.0, 1.0])),
    ('inf', dict(type='circle', radii=[2.0, float('inf'), 1.0])),
    ('unknown type', dict(type='square', radii=[2.0, 2.0, 1.0])),
    ('no type', dict(radii=[2.0, 2.0, 1.0])),
    ('unknown key', dict(type='circle', radii=[2.0, 2.0, 1.0], radius=2.0)),
    ('not a dict', 'circle'),
    ('not a dict', [2.0, 2.0, 1.0]),
    ('non-number', dict(type='circle', radii=['2', 2.0, 1.0])),
    ('non-number', dict(type='circle', radii=[True, 2.0, 1.0])),
    ('non-number', dict(type='circle', radii=[None, 2.0, 1.0])),
    ('pair for a circle', dict(type='circle', radii=[(1.0, 2.0), 2.0, 1.0])),
    ('number for a pair', dict(type='three_circle', radii=[2.0, 2.0, 1.0])),
    ('triple', dict(type='three_circle', radii=[(1.0, 2.0, 3.0), (1.0, 2.0), (0.5, 1.0)])),
    ('non-number', dict(type='three_circle', radii=[(1.0, '2'), (1.0, 2.0), (0.5, 1.0)])),
]


@pytest.mark.parametrize('why,bad', BAD, ids=['%s-%d' % (w, i) for i, (w, _) in enumerate(BAD)])
def test_refusals_name_the_value(why, bad):
    import re
    named = re.escape('radar_gate=%r' % (bad,))
    h = _head()

    def struct_of_bad_attribute():
        h.radar_gate = bad                      # (a public attribute: weights_struct() checks it again)
        h.weights_struct()
    for call in (lambda: L.check_radar_gate(bad), lambda: _head(bad), lambda: configs.head_cfg(radar_gate=bad),
                 lambda: T.build_head(dict(configs.head_cfg(num_query=20), radar_gate=bad)), struct_of_bad_attribute):
        with pytest.raises(L.TransCARHipError, match=named):
            call()


def test_default_struct_is_byte_identical_to_one_built_without_the_keyword():
    plain = T.build_head(configs.head_cfg(num_query=20))          # no keyword at all
    want = _raw(plain.weights_struct())
    for gate in (None, dict(type='three_circle'), DEFAULT3):
        h = _head(gate)
        w = h.weights_struct()
        assert [(w.radar[r].radius_min, w.radar[r].radius_max) for r in range(3)] == list(D.RADAR_RADII)
        # a struct holds its modules' addresses: compare the bytes on ONE set of modules, under each head's gate
        plain.radar_gate = h.radar_gate
        assert _raw(plain.weights_struct()) == want, gate
    plain.radar_gate = L.check_radar_gate(CIRCLE)
    assert _raw(plain.weights_struct()) != want


def test_sentinel_and_radii_land_in_the_struct():
    w = _head(CIRCLE).weights_struct()
    assert [(w.radar[r].radius_min, w.radar[r].radius_max) for r in range(3)] == [(-1.0, 2.0), (-1.0, 2.0), (-1.0, 1.0)]
    w = _head(WIDE3).weights_struct()
    assert [(w.radar[r].radius_min, w.radar[r].radius_max) for r in range(3)] == [(0.75, 3.0), (0.5, 1.5), (0.25, 0.75)]
    # the circle head has the three-circle head's parameters: its trained weights load unchanged
    assert list(_head(CIRCLE).state_dict()) == list(_head().state_dict())


@pytest.mark.parametrize('depth', [1, 2])
def test_shallower_heads_take_the_first_entries(depth):
    for gate in (CIRCLE, WIDE3):
        full = L.check_radar_gate(gate)
        h = _head(gate, num_fusion_layers=depth)
        assert h.radar_gate == dict(type=full['type'], radii=full['radii'][:depth])
        assert h.radar_gate == _head(dict(gate, radii=gate['radii'][:depth]), num_fusion_layers=depth).radar_gate
        w = h.weights_struct()
        assert w.num_radar_layers == depth
        assert [(w.radar[r].radius_min, w.radar[r].radius_max) for r in range(depth)] == L.radar_gate_pairs(full)[:depth]
        assert [(w.radar[r].radius_min, w.radar[r].radius_max) for r in range(depth, 3)] == [(0.0, 0.0)] * (3 - depth)
    with pytest.raises(L.TransCARHipError, match='radar_gate='):
        _head(dict(type='circle', radii=[2.0, 2.0] if depth == 1 else [2.0]), num_fusion_layers=depth)


def _refused(w, text):
    lib = L.lib()
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) == 0
    err = lib.tc_last_error().decode()
    assert text in err, err
    assert lib.tc_head_packed_bytes(ctypes.byref(w)) == 0 and text in lib.tc_last_error().decode()


def test_library_refusals_name_the_value():
    lib = L.lib()
    w = _head(CIRCLE).weights_struct()
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) > 0
    for r, (rmin, rmax, text) in enumerate(((float('nan'), 2.0, 'radius_min=nan'), (1.0, float('inf'), 'radius_max=inf'),
                                            (-0.5, 2.0, 'radius_min=-0.5'))):
        w = _head().weights_struct()
        w.radar[r].radius_min, w.radar[r].radius_max = rmin, rmax
        _refused(w, text)
        assert 'radar[%d]' % r in lib.tc_last_error().decode()
    for rmin, rmax, text in ((-2.0, 2.0, 'radius_min=-2'), (2.0, 1.0, 'radius_max=1 below radius_min=2'),
                             (1.0, 16.5, 'radius_max=16.5'), (-1.0, 16.5, 'radius_max=16.5'), (-1.0, -1.0, 'radius_max=-1'),
                             (-1.0, float('nan'), 'radius_max=nan')):
        w = _head().weights_struct()
        w.radar[1].radius_min, w.radar[1].radius_max = rmin, rmax
        _refused(w, text)
    # a layer the head does not have is not read
    w = _head(num_fusion_layers=2).weights_struct()
    w.radar[2].radius_min = -7.0
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) > 0
    # the end points
    for pair in ((-1.0, 16.0), (16.0, 16.0), (0.125, 0.125), (-1.0, 0.125)):
        w = _head().weights_struct()
        w.radar[0].radius_min, w.radar[0].radius_max = pair
        assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) > 0, pair


def test_stand_alone_entries_refuse_before_a_launch():
    lib = L.lib()
    for rmin, rmax, text in ((-0.5, 2.0, 'radius_min=-0.5'), (1.0, 17.0, 'radius_max=17'), (float('nan'), 1.0, 'radius_min=nan')):
        rc = lib.tc_radar_attn_core_fwd(None, 1.0, None, None, 2, None, 10, None, 2, 1, 8, 64, 256, 8, 1, rmin, rmax,
                                        ctypes.c_void_p(8), ctypes.c_void_p(8), 0.0, 0, 0, None)
        assert rc != 0 and text in lib.tc_last_error().decode(), lib.tc_last_error().decode()
        rc = lib.tc_radar_attn_core_bwd(None, 1.0, None, None, 2, None, 10, None, 2, 1, 8, 64, 256, 8, 1, rmin, rmax,
                                        None, None, None, None, 0.0, 0, 0, None)
        assert rc != 0 and text in lib.tc_last_error().decode(), lib.tc_last_error().decode()
    rc = lib.tc_radar_gate_selfcheck_range(16, 1, 0.0625, 2.0, 1, ctypes.c_void_p(8), None)
    assert rc != 0 and 'rad_lo=0.0625' in lib.tc_last_error().decode()
    rc = lib.tc_radar_gate_selfcheck_range(16, 1, 0.5, 32.0, 0, ctypes.c_void_p(8), None)
    assert rc != 0 and 'rad_hi=32' in lib.tc_last_error().decode()
    rc = lib.tc_radar_gate_selfcheck_range(16, 1, 0.5, 2.0, 2, ctypes.c_void_p(8), None)
    assert rc != 0 and 'inclusive=2' in lib.tc_last_error().decode()


def test_zeroed_struct_is_still_accepted():
    lib = L.lib()
    w = _head().weights_struct()
    for r in range(3):
        w.radar[r].radius_min = w.radar[r].radius_max = 0.0
    assert lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64) > 0
    assert lib.tc_head_packed_bytes(ctypes.byref(w)) > 0
