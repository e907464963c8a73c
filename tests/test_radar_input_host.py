"""Radar input as configuration, host side (no GPU): Detr3DHead(radar_num_tokens=, radar_in_dims=, radar_point_range=)
through configs.head_cfg, the checks that name a refused value, the packed struct, radar.pack_tokens at another token
count, and the library's new entries under ABI 13."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import transcar_amd as T
from transcar_amd import _lib as L
from transcar_amd import configs, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)
NEW_ENTRIES = ('tc_radar_build_tokens_n', 'tc_radar_build_tokens_batch_n', 'tc_radar_pack_rows_batch', 'tc_radar_attn_core_fwd_n',
               'tc_radar_attn_core_bwd_n')


def _head(**kw):
    return T.build_head(configs.head_cfg(num_query=128, **kw))


# ---- the three arguments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [64, 128, 1500, 2048, 4096])
def test_accepted_token_counts(N):
    h = _head(radar_num_tokens=N)
    assert h.radar_num_tokens == N and h.weights_struct().num_radar_tokens_ref == N


@pytest.mark.parametrize('N', [0, 63, 4097, -1500, 1500.0, True, None, '1500'])
def test_refused_token_counts_are_named(N):
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_num_tokens=%r' % (N,))):
        L.check_radar_input(N, 36, None)
    if N is not None:                      # (None leaves head_cfg's default)
        with pytest.raises(L.TransCARHipError, match=re.escape('radar_num_tokens=%r' % (N,))):
            configs.head_cfg(radar_num_tokens=N)
    cfg = configs.head_cfg(num_query=128)
    cfg['radar_num_tokens'] = N
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_num_tokens=%r' % (N,))):
        T.build_head(cfg)


@pytest.mark.parametrize('F', list(range(4, 65, 4)))
def test_accepted_feature_counts_shape_the_encoder(F):
    h = _head(radar_in_dims=F)
    assert h.radar_in_dims == F and h.weights_struct().radar_in_dims == F
    assert tuple(h.state_dict()['radar_feat_encoder.0.weight'].shape) == (64, F)
    assert tuple(h.state_dict()['radar_feat_encoder.2.weight'].shape) == (128, 64)


@pytest.mark.parametrize('F', [0, 3, 6, 35, 68, 128, 36.0, True, '36'])
def test_refused_feature_counts_are_named(F):
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_in_dims=%r' % (F,))):
        configs.head_cfg(radar_in_dims=F)
    cfg = configs.head_cfg(num_query=128)
    cfg['radar_in_dims'] = F
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_in_dims=%r' % (F,))):
        T.build_head(cfg)


def test_a_checkpoint_of_another_feature_count_fails_by_shape():
    sd = _head(radar_in_dims=8).state_dict()
    with pytest.raises(RuntimeError, match='radar_feat_encoder.0.weight'):
        _head().load_state_dict(sd)


@pytest.mark.parametrize('rng', [(-80.0, -80.0, -6.0, 80.0, 80.0, 4.0), [-51.2, -51.2, -5, 20, 51.2, 3], REF_RANGE])
def test_accepted_point_ranges(rng):
    h = _head(radar_point_range=rng)
    assert h.radar_point_range == tuple(float(v) for v in rng)


@pytest.mark.parametrize('rng', [(-51.2, -51.2, -5.0, 51.2, 51.2), (51.2, -51.2, -5.0, -51.2, 51.2, 3.0),
                                 (-51.2, -51.2, 3.0, 51.2, 51.2, 3.0), (-51.2, -51.2, -5.0, float('nan'), 51.2, 3.0),
                                 (-float('inf'), -51.2, -5.0, 51.2, 51.2, 3.0), 'wide', 51.2])
def test_refused_point_ranges_are_named(rng):
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_point_range=%r' % (rng,))):
        configs.head_cfg(radar_point_range=rng)
    cfg = configs.head_cfg(num_query=128)
    cfg['radar_point_range'] = rng
    with pytest.raises(L.TransCARHipError, match=re.escape('radar_point_range=%r' % (rng,))):
        T.build_head(cfg)


def test_the_range_does_not_follow_pc_range():
    """the default stays the reference's constant (HEAD:304) whatever pc_range is"""
    h = T.build_head(configs.head_cfg(num_query=128, pc_range=(-80.0, -80.0, -5.0, 80.0, 80.0, 3.0)))
    assert h.radar_point_range == REF_RANGE == radar.POINT_RANGE == L.RADAR_POINT_RANGE_REF


def test_head_cfg_sets_the_keys_only_off_the_defaults():
    plain = configs.head_cfg()
    assert configs.head_cfg(radar_num_tokens=1500, radar_in_dims=36, radar_point_range=REF_RANGE) == plain
    assert not any(k.startswith('radar_num_tokens') or k in ('radar_in_dims', 'radar_point_range') for k in plain)
    cfg = configs.head_cfg(radar_num_tokens=2048, radar_in_dims=8, radar_point_range=(-60, -60, -5, 60, 60, 3))
    assert (cfg['radar_num_tokens'], cfg['radar_in_dims']) == (2048, 8)
    assert cfg['radar_point_range'] == [-60.0, -60.0, -5.0, 60.0, 60.0, 3.0]
    h = T.build_head(cfg)
    assert (h.radar_num_tokens, h.radar_in_dims, h.radar_point_range) == (2048, 8, (-60.0, -60.0, -5.0, 60.0, 60.0, 3.0))


def test_public_attributes_are_checked_again():
    h = _head()
    h.radar_num_tokens = 5000
    with pytest.raises(L.TransCARHipError, match='radar_num_tokens=5000'):
        h.weights_struct()
    h.radar_num_tokens, h.radar_in_dims = 1500, 40          # (the encoder was built for 36)
    with pytest.raises(L.TransCARHipError, match='radar_in_dims=40'):
        h.weights_struct()


def test_default_struct_bytes_are_unchanged():
    """A default head packs 36 and 1500, and a head with the defaults spelled out packs the same bytes apart from the
    parameters' own addresses."""
    a = _head()
    wa = a.weights_struct()
    assert (wa.radar_in_dims, wa.num_radar_tokens_ref, wa.num_radar_layers) == (36, 1500, 3)
    names = [f[0] for f in L.tc_head_weights._fields_]
    assert names[-1] == 'num_points' and L.TC_ABI_VERSION == 13
    assert names[names.index('radar_in_dims'):names.index('radar_in_dims') + 3] == ['radar_in_dims', 'num_radar_layers',
                                                                                   'num_radar_tokens_ref']
    off = L.tc_head_weights.radar_in_dims.offset
    assert bytes(wa)[off:off + 12] == np.array([36, 3, 1500], np.int32).tobytes()
    # the scalar head of the struct (everything in front of the first pointer) byte for byte
    b = T.build_head(configs.head_cfg(num_query=128, radar_num_tokens=1500, radar_in_dims=36, radar_point_range=REF_RANGE))
    end = L.tc_head_weights.query_embedding.offset
    assert bytes(wa)[:end] == bytes(b.weights_struct())[:end]
    assert ctypes.sizeof(L.tc_head_weights) == ctypes.sizeof(wa)


# ---- radar.pack_tokens at another token count --------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [4, 36])
@pytest.mark.parametrize('N', [128, 2048])
def test_pack_tokens_at_n(N, F):
    rng = np.random.RandomState(N + F)
    for n in (0, N - 1, N, N + 37):
        rows = rng.standard_normal((n, F))
        tok, pad_mult = radar.pack_tokens([rows], num_tokens=N)
        T_ = tok.shape[1]
        assert tok.dtype == np.float32 and tok.shape == (1, T_, F) and (T_ % 64 == 0 or T_ == N)
        assert pad_mult == N - T_ + 1
        kept = min(n, N)
        assert np.array_equal(tok[0, :kept], rows[:kept].astype(np.float32))              # truncation to the first N
        assert np.all(tok[0, kept:] == 500.0)
        if n < N - 1:
            assert T_ < N and np.all(tok[0, T_ - 1] == 500.0)                              # row T - 1 stays the pad row
        else:
            assert T_ == N and pad_mult == 1                                               # n = N - 1: one pad row; n >= N: none
            assert bool(np.all(tok[0, N - 1] == 500.0)) == (n == N - 1)
    # an explicit T: it must hold the frame plus the pad row, or be N
    rows = rng.standard_normal((100, F))
    tok, pad_mult = radar.pack_tokens([rows], T=N, num_tokens=N)
    assert tok.shape == (1, N, F) and pad_mult == 1
    with pytest.raises(ValueError, match='T=%d' % (N + 64)):
        radar.pack_tokens([rows], T=N + 64, num_tokens=N)
    with pytest.raises(ValueError, match='T=64'):
        radar.pack_tokens([rows], T=64, num_tokens=N)
    # the default is the reference's 1500
    tok, pad_mult = radar.pack_tokens([rows])
    assert tok.shape == (1, 128, F) and pad_mult == 1500 - 128 + 1


def test_tokens_T_and_fit_follow_the_count():
    from transcar_amd import ops
    assert ops.radar_tokens_T(255) == 256 and ops.radar_tokens_T(5000) == 1500
    assert ops.radar_tokens_T(1700, num_tokens=2048) == 1728 and ops.radar_tokens_T(2047, num_tokens=2048) == 2048
    assert ops.radar_tokens_T(40, num_tokens=128) == 64 and ops.radar_tokens_T(4000, num_tokens=128) == 128


def test_raw_sweeps_off_36_features_are_refused():
    from transcar_amd import synth
    frame = synth.make_radar_frame(seed=2, n_per_radar=5)
    h = _head(radar_in_dims=8)
    for ingest in ('device', 'host'):
        with pytest.raises(L.TransCARHipError, match='radar_in_dims=8'):
            h._radar_tokens_plan([frame], 'cpu', ingest=ingest)
    with pytest.raises(ValueError, match='radar_in_dims=8'):
        radar.build_radar_features(frame, num_features=8)
    with pytest.raises(ValueError, match='radar_in_dims=8'):
        radar.build_radar_features(np.zeros((5, 36)), num_features=8)
    # [n,F] rows take the host route
    rows = np.random.RandomState(0).standard_normal((10, 8))
    tok, pad_mult, fill = h._radar_tokens_plan([rows], 'cpu')
    assert tuple(tok.shape) == (1, 64, 8) and pad_mult == 1500 - 64 + 1 and fill is None
    tok_t, _, _ = h._radar_tokens_plan([torch.from_numpy(rows).float()], 'cpu')           # rows as a host tensor: the same
    assert torch.equal(tok_t, tok)
    h2 = _head(radar_num_tokens=128)
    tok, pad_mult, _ = h2._radar_tokens_plan([np.zeros((500, 36))], 'cpu')
    assert tuple(tok.shape) == (1, 128, 36) and pad_mult == 1


def test_host_filter_takes_the_heads_range():
    """raw sweeps on the host route: the head's radar_point_range reaches radar.build_radar_features"""
    from transcar_amd import synth
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    full = radar.build_radar_features(frame)
    cut = radar.build_radar_features(frame, point_range=(-51.2, -51.2, -5.0, 10.0, 51.2, 3.0))
    assert 0 < len(cut) < len(full) and np.array_equal(cut, full[full[:, 0] < 10.0])
    h = _head(radar_point_range=(-51.2, -51.2, -5.0, 10.0, 51.2, 3.0))
    tok, _, _ = h._radar_tokens_plan([frame], 'cpu', ingest='host')
    assert np.array_equal(tok[0, :len(cut)].numpy(), cut.astype(np.float32)) and float(tok[0, len(cut), 0]) == 500.0


# ---- the library boundary ------------------------------------------------------------------------------------------------------
def _define(name):
    with open(os.path.join(ROOT, 'include', 'transcar_hip.h')) as f:
        return int(re.search(r'#define %s (\d+)\b' % name, f.read()).group(1))


def test_new_entries_are_declared_exported_and_bound_under_abi_13():
    assert L.TC_ABI_VERSION == 13 and L.lib().tc_abi_version() == 13 and _define('TC_ABI_VERSION') == 13
    assert (_define('TC_MAX_RADAR_TOKENS'), _define('TC_MAX_RADAR_IN_DIMS')) == (4096, 64)
    assert (L.TC_MIN_RADAR_TOKENS, L.TC_MAX_RADAR_TOKENS, L.TC_MAX_RADAR_IN_DIMS) == (_define('TC_MIN_RADAR_TOKENS'), 4096, 64)
    assert L.TC_RADAR_TOKENS_REF == _define('TC_RADAR_TOKENS_REF') == radar.NUM_RADAR_TOKENS == 1500
    assert L.RADAR_IN_DIMS_REF == radar.NUM_FEATURES == 36
    with open(os.path.join(ROOT, 'include', 'transcar_hip.h')) as f:
        text = f.read()
    dll = ctypes.CDLL(L.LIB_PATH)
    for name in NEW_ENTRIES:
        assert re.search(r'\bint %s\(' % name, text), name
        assert hasattr(dll, name) and name in L.SIGNATURES, name
    # the entries without a count keep their signatures
    assert len(L.SIGNATURES['tc_radar_build_tokens'][1]) == 11 and len(L.SIGNATURES['tc_radar_build_tokens_n'][1]) == 12
    assert len(L.SIGNATURES['tc_radar_build_tokens_batch'][1]) == 9 and len(L.SIGNATURES['tc_radar_build_tokens_batch_n'][1]) == 10
    for name in ('tc_radar_attn_core_fwd', 'tc_radar_attn_core_bwd'):
        assert L.SIGNATURES[name + '_n'][1] == L.SIGNATURES[name][1][:-1] + [ctypes.c_int, ctypes.c_void_p]


def _struct(tokens_ref=1500, in_dims=36, layers=3):
    w = L.tc_head_weights()
    w.abi_version = L.TC_ABI_VERSION
    w.num_query, w.embed_dims, w.num_heads, w.ffn_dims = 128, 256, 8, 512
    w.num_layers, w.num_cams, w.num_levels = 6, 6, 4
    w.num_classes, w.code_size, w.radar_in_dims, w.num_radar_layers = 10, 10, in_dims, layers
    w.num_radar_tokens_ref = tokens_ref
    return w


def test_check_dims_names_the_refused_value():
    lib = L.lib()

    def ws(w, T_=64):
        return lib.tc_head_workspace_bytes(ctypes.byref(w), 1, T_)
    assert ws(_struct()) > 0 and ws(_struct(64)) > 0 and ws(_struct(4096)) > 0
    assert ws(_struct(0)) == ws(_struct(1500))                 # a zeroed count reads as the reference's
    for bad in (63, 4097, -1):
        assert ws(_struct(bad)) == 0 and ('num_radar_tokens_ref=%d' % bad).encode() in lib.tc_last_error()
    assert ws(_struct(63, layers=0)) > 0                       # a camera-only head reads no token ...
    assert ws(_struct(0, in_dims=0, layers=0)) > 0             # ... of any width (a zeroed struct field, as before)
    assert ws(_struct(in_dims=2, layers=0)) == 0 and b'radar_in_dims=2' in lib.tc_last_error()      # (the old alignment rule)
    for F in (4, 8, 64):
        assert ws(_struct(in_dims=F)) > 0
    for bad in (0, 2, 38, 68):
        assert ws(_struct(in_dims=bad)) == 0 and ('radar_in_dims=%d' % bad).encode() in lib.tc_last_error()


def test_entries_refuse_tokens_above_the_count_and_an_index_beyond_32_bits():
    lib = L.lib()
    keep = (ctypes.c_float * 4)()
    buf = ctypes.cast(keep, ctypes.c_void_p)
    w = _struct(128)
    w.l0_attn_out = ctypes.cast(keep, dict(L.tc_head_weights._fields_)['l0_attn_out'])
    # the forward entries
    rc = lib.tc_radar_fusion_fwd(ctypes.byref(w), buf, buf, buf, buf, 1, 192, 1, 0, 3, buf, buf, None, None, None, 0, None)
    assert rc != 0 and b'T=192 is above num_radar_tokens_ref=128' in lib.tc_last_error()
    fv = L.tc_feats_nhwc()
    fv.num_levels = 4
    rc = lib.tc_head_forward(ctypes.byref(w), None, ctypes.byref(fv), 1, None, 928.0, 1600.0, buf, 192, 1, None, None, None,
                             None, None, 0, None)
    assert rc != 0 and b'T=192 is above num_radar_tokens_ref=128' in lib.tc_last_error()
    # the training and backward entries: T, and rows * heads * N against the dropout index
    assert lib.tc_radar_train_tape_bytes(ctypes.byref(w), 1, 192) == 0 and b'T=192 is above' in lib.tc_last_error()
    assert lib.tc_radar_train_tape_bytes(ctypes.byref(w), 1, 128) > 0
    assert lib.tc_radar_train_bwd_workspace_bytes(ctypes.byref(w), 1, 192) == 0 and b'T=192 is above' in lib.tc_last_error()
    big = _struct(4096)
    big.num_query = 4096
    B = 2 ** 32 // (4096 * 8 * 4096)

    def train_fwd(w_, B_, p):
        return lib.tc_radar_train_fwd(ctypes.byref(w_), buf, buf, buf, buf, B_, 64, 4033, buf, buf, None, 0, p, 1, None)
    assert train_fwd(big, B, 0.1) != 0 and b'dropout index' in lib.tc_last_error() and b'4096' in lib.tc_last_error()
    assert train_fwd(big, B - 1, 0.1) != 0 and b'dropout index' not in lib.tc_last_error()      # (refused for its NULL tape)
    assert train_fwd(big, B, 0.0) != 0 and b'dropout index' not in lib.tc_last_error()          # no mask drawn: no index
    assert lib.tc_radar_train_tape_bytes(ctypes.byref(big), B, 64) > 0
    # a default head of 900 queries runs at any batch size without dropout, as it did
    dflt = _struct(1500)
    dflt.num_query = 900
    assert lib.tc_radar_train_tape_bytes(ctypes.byref(dflt), 400, 64) > 0
    # the attention core's entries with a stride: the count, T and the index are named
    def core(T_, N, p, B_=1, Q_=8):
        return lib.tc_radar_attn_core_fwd_n(None, 1.0, None, None, 2, None, 10, None, 2, B_, Q_, T_, 256, 8, 1, 1.0, 2.0, buf, buf,
                                            p, 1, 0, N, None)
    assert core(64, 5000, 0.0) != 0 and b'num_tokens=5000' in lib.tc_last_error()
    assert core(192, 128, 0.0) != 0 and b'T=192' in lib.tc_last_error()
    assert core(64, 4096, 0.1, B_=1 << 10, Q_=1 << 7) != 0 and b'dropout index' in lib.tc_last_error()
    # the ingest entries: the count and T are named before anything is launched
    rc = lib.tc_radar_pack_rows_batch(buf, 0, buf, 1, 36, None, buf, 64, 5000, None, None)
    assert rc != 0 and b'num_tokens=5000' in lib.tc_last_error()
    rc = lib.tc_radar_pack_rows_batch(buf, 0, buf, 1, 36, None, buf, 129, 128, None, None)
    assert rc != 0 and b'T=129' in lib.tc_last_error()
    rc = lib.tc_radar_pack_rows_batch(buf, 0, buf, 1, 38, None, buf, 64, 128, None, None)
    assert rc != 0 and b'radar_in_dims=38' in lib.tc_last_error()
    rc = lib.tc_radar_build_tokens_batch_n(buf, buf, buf, 1, 64, buf, 64, 32, None, None)
    assert rc != 0 and b'num_tokens=32' in lib.tc_last_error()
    rc = lib.tc_radar_build_tokens_n(None, None, None, 5, None, None, None, buf, 2049, 2048, None, None)
    assert rc != 0 and b'T=2049' in lib.tc_last_error()


def test_host_rows_are_filtered_by_a_range_of_the_heads_own():
    """[n,F] rows on the host: a radar_point_range other than the default applies to them as the device route applies it
    to CUDA rows; at the default they are taken as their producer filtered them (as before)."""
    rows = np.random.RandomState(1).uniform(-60.0, 60.0, (200, 36))
    rows[:, 2] = 0.0
    rng = (-51.2, -51.2, -5.0, 20.0, 51.2, 3.0)
    keep = radar.in_range(rows, rng)
    assert 0 < keep.sum() < 200 and not radar.in_range(rows, REF_RANGE).all()
    for frame in (rows, torch.from_numpy(rows).float()):
        tok, pad_mult, _ = _head(radar_point_range=rng)._radar_tokens_plan([frame], 'cpu')
        kept = rows[keep].astype(np.float32)
        assert np.array_equal(tok[0, :len(kept)].numpy(), kept) and float(tok[0, len(kept), 0]) == 500.0
        tok, _, _ = _head()._radar_tokens_plan([frame], 'cpu')
        assert np.array_equal(tok[0, :200].numpy(), rows.astype(np.float32))
    nan = rows.copy()
    nan[3, 1] = np.nan
    assert not radar.in_range(nan, rng)[3]
