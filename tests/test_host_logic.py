"""CPU tests of the host side: registry/config building, checkpoint contract,
radar ingest, C-ABI surface, frame sharding (gloo, world size 2)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import transcar_amd as T
from oracle import transcar_oracle as O
from parity_util import header_functions
from transcar_amd import _lib, configs, radar, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_head_builds_from_reference_config_and_loads_checkpoint_keys():
    head = T.build_head(configs.head_cfg())
    sd = synth.make_state_dict(seed=3)
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in sd.items()}
    head.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    # trainable set of the reference recipe (tools/train.py:238-252): everything
    # outside transformer / cls_branches / reg_branches / query_embedding
    frozen = ('transformer.', 'cls_branches.', 'reg_branches.', 'query_embedding.')
    n = sum(p.numel() for k, p in head.named_parameters()
            if not k.startswith(frozen) and k != 'code_weights')
    assert n == 2646316
    assert sum(p.numel() for p in head.parameters()) == 8728385 


@pytest.mark.parametrize('cfg_file', ['detr3d_res101_gridmask.py', 'detr3d_res101_gridmask_cbgs.py',
                                      'detr3d_vovnet_gridmask_det_final_trainval_cbgs.py'])
def test_the_references_own_config_files_build_the_head(cfg_file, golden_dir):
    """north_star's "config files ... drop-in" (VERDICT r5 missing 5): what the reference's three config files
    define (tests/golden/g9_reference_configs.json, written by `make_golden.py configs`, which executes each file
    as it lies) -- model['pts_bbox_head'] + model['train_cfg']['pts'] go to build_head UNCHANGED (CFG:51-114;
    CFG_VOV:55 `code_weights`); transcar_amd/configs.py -- the transcription every other test uses -- must equal them."""
    import json
    with open(os.path.join(golden_dir, 'g9_reference_configs.json')) as f:
        ns = json.load(f)[cfg_file]
    ref_head, ref_train = ns['pts_bbox_head'], ns['train_cfg_pts']
    mine = configs.head_cfg()
    extra = {k: v for k, v in ref_head.items() if k not in mine}
    assert set(extra) <= {'code_weights'}, extra              # the VoVNet file's only addition (CFG_VOV:55)

    def norm(x):                                               # tuples / lists, ints / floats compare by value
        if isinstance(x, dict):
            return {k: norm(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [norm(v) for v in x]
        return float(x) if isinstance(x, (int, float)) and not isinstance(x, bool) else x
    assert norm({k: v for k, v in ref_head.items() if k != 'code_weights'}) == norm(mine)
    assert norm(ref_train) == norm(configs.train_cfg_pts)
    assert ns['point_cloud_range'] == configs.point_cloud_range and ns['voxel_size'] == configs.voxel_size
    head = T.build_head(ref_head, train_cfg=ref_train)
    assert sum(p.numel() for p in head.parameters()) == 8728385
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in synth.make_state_dict(seed=3).items()}
    if 'code_weights' in ref_head:
        np.testing.assert_allclose(head.code_weights.detach().numpy(), np.asarray(ref_head['code_weights'], np.float32))
    assert head.assigner is not None and type(head.assigner).__name__ == 'HungarianAssigner3D'


def test_registry_names_match_reference():
    from transcar_amd import registry as R
    assert 'Detr3DHead' in R.HEADS.module_dict
    assert 'Detr3DTransformer' in R.TRANSFORMER.module_dict
    assert 'Detr3DTransformerDecoder' in R.TRANSFORMER_LAYER_SEQUENCE.module_dict
    assert {'Detr3DCrossAtten', 'MultiheadAttention'} <= set(R.ATTENTION.module_dict)
    assert 'DetrTransformerDecoderLayer' in R.TRANSFORMER_LAYER.module_dict
    assert 'NMSFreeCoder' in R.BBOX_CODERS.module_dict
    with pytest.raises(KeyError):
        R.HEADS.build(dict(type='NoSuchHead'))


def test_no_cpu_fallback():
    head = T.build_head(configs.head_cfg()).eval()
    feats = [torch.from_numpy(f) for f in synth.make_feats('tiny')]
    metas = synth.make_img_metas(1, radar=synth.make_radar_frame())
    with pytest.raises(T.TransCARHipError):
        head(feats, metas)
    with pytest.raises(T.TransCARHipError):
        T.ops.linear(torch.zeros(4, 256), torch.zeros(8, 256), torch.zeros(8))


def test_radar_ingest_matches_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g5_head_tiny.npz'))
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g['radar_centres'])
    f36 = radar.build_radar_features(frame)
    assert f36.shape == (int(g['fill_in']), 36)
    np.testing.assert_allclose(f36.astype(np.float32), g['radar_tokens'], atol=1e-6, rtol=1e-6)
    # and equals the oracle's independent restatement bit for bit
    assert np.array_equal(f36, O.build_radar_features(frame))
    g4 = np.load(os.path.join(golden_dir, 'g4_radar_ragged.npz'))
    f = radar.build_radar_features(synth.make_radar_frame(seed=5, n_per_radar=[7, 0, 3, 0, 12]))
    np.testing.assert_allclose(f.astype(np.float32), g4['radar_tokens'], atol=1e-6, rtol=1e-6)


def test_pack_tokens_padding_and_multiplicity():
    f = [np.ones((255, 36)), np.ones((10, 36)) * 2, np.zeros((0, 36))]
    tok, pad_mult = radar.pack_tokens(f)
    assert tok.shape == (3, 256, 36) and pad_mult == 1500 - 256 + 1
    assert (tok[0, :255] == 1).all() and (tok[0, 255] == 500).all()
    assert (tok[1, 10:] == 500).all() and (tok[2] == 500).all()
    big = [np.ones((1700, 36))]
    tok, pad_mult = radar.pack_tokens(big)                 # HEAD:528: min(1500, n)
    assert tok.shape == (1, 1500, 36) and pad_mult == 1
    # every sample keeps 1500 - n_i pad tokens in total
    for b, n in enumerate((255, 10, 0)):
        pads_in_T = 256 - n
        assert pads_in_T - 1 + (1500 - 256 + 1) == 1500 - n


def test_c_abi_exports_every_declared_symbol():
    names = header_functions()
    assert len(names) >= 15
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(dll, n), 'library does not export %s' % n
    assert sorted(_lib.SIGNATURES) == names          # binding covers the header
    lib = T.lib()
    assert lib.tc_abi_version() == _lib.TC_ABI_VERSION
    # struct layouts: sizes the C side and the ctypes mirror must agree on are
    # checked through the workspace query (a wrong layout gives a wrong answer)
    assert ctypes.sizeof(_lib.tc_decoder_layer) == 8 * (4 + 2 + 2 + 2 + 8 + 2 + 2 + 2 + 2 + 6 + 1)    # + packed16_delta


def test_workspace_query_runs_without_gpu():
    head = T.build_head(configs.head_cfg())
    w = _lib.tc_head_weights()
    w.abi_version = _lib.TC_ABI_VERSION
    w.num_query, w.embed_dims, w.num_heads, w.ffn_dims = 900, 256, 8, 512
    w.num_layers, w.num_cams, w.num_levels = 6, 6, 4
    w.num_classes, w.code_size, w.radar_in_dims, w.num_radar_layers = 10, 10, 36, 3
    n1 = T.lib().tc_head_workspace_bytes(ctypes.byref(w), 1, 256)
    n2 = T.lib().tc_head_workspace_bytes(ctypes.byref(w), 2, 256)
    assert 10e6 < n1 < 64e6 and 1.9 * n1 < n2 < 2.1 * n1
    w.embed_dims = 128                                   # unsupported -> 0 + message
    assert T.lib().tc_head_workspace_bytes(ctypes.byref(w), 1, 256) == 0
    assert b'embed_dims' in T.lib().tc_last_error()


def test_tuning_knob_validates_without_gpu():
    """tc_head_options.chain_tile_rows is validated before anything is launched (no GPU needed:
    the call fails on the argument check), and the host-side env knob is validated at import."""
    lib = T.lib()
    w = _lib.tc_head_weights()
    w.abi_version = _lib.TC_ABI_VERSION
    w.num_query, w.embed_dims, w.num_heads, w.ffn_dims = 900, 256, 8, 512
    w.num_layers, w.num_cams, w.num_levels = 6, 6, 4
    w.num_classes, w.code_size, w.radar_in_dims, w.num_radar_layers = 10, 10, 36, 0
    fv = _lib.tc_feats_nhwc()
    fv.num_levels = 4
    from transcar_amd.detr3d_head import head_options
    opt = head_options(tile_rows=8)
    assert opt.chain_tile_rows == 8
    opt.chain_tile_rows = 5
    rc = lib.tc_head_forward(ctypes.byref(w), None, ctypes.byref(fv), 1, None, 928.0, 1600.0, None, 0, 0,
                             None, None, None, ctypes.byref(opt), None, 0, None)
    assert rc != 0 and b'chain_tile_rows' in lib.tc_last_error()
    import subprocess
    r = subprocess.run([sys.executable, '-c', 'import transcar_amd'], cwd=ROOT,
                       env=dict(os.environ, TRANSCAR_CHAIN_ROWS='5'), capture_output=True, text=True)
    assert r.returncode != 0 and 'TRANSCAR_CHAIN_ROWS' in r.stderr


#: tc_chain_tile_rows(rows, tile_rows, matrix_path), written out: rows -> tile_rows -> (AUTO, F32, F16X2); None = refused
_X = None
_TILE_ROWS = {
    1:    {0: (4, 4, 4),    4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    1024: {0: (4, 4, 4),    4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    1025: {0: (8, 8, 8),    4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    2048: {0: (8, 8, 8),    4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    2049: {0: (16, 16, 16), 4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    4096: {0: (16, 16, 16), 4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    4097: {0: (32, 16, 32), 4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
    8100: {0: (32, 16, 32), 4: (4, 4, 4), 8: (8, 8, 8), 16: (16, 16, 16), 32: (32, _X, 32)},
}


def test_chain_tile_rows_is_the_one_rule_without_gpu():
    """tc_chain_tile_rows: the tile height every chain launch (and the attention core's choice) follows, against the
    table above; 32 rows on the f32 path, another tile_rows and another matrix_path are refused by name."""
    lib = T.lib()
    paths = (_lib.TC_MATRIX_AUTO, _lib.TC_MATRIX_F32, _lib.TC_MATRIX_F16X2)
    assert paths == (0, 1, 2) and sorted(_TILE_ROWS) == [1, 1024, 1025, 2048, 2049, 4096, 4097, 8100]
    for rows, by_opt in _TILE_ROWS.items():
        assert sorted(by_opt) == [0, 4, 8, 16, 32]
        for opt, want in by_opt.items():
            for mp, w in zip(paths, want):
                got = lib.tc_chain_tile_rows(rows, opt, mp)
                if w is None:
                    assert got < 0 and b'f16x2' in lib.tc_last_error(), (rows, opt, mp, got)
                else:
                    assert got == w, (rows, opt, mp, got)
    assert _TILE_ROWS[4097][0] == (32, 16, 32) and _TILE_ROWS[4096][0][0] == 16
    assert lib.tc_chain_tile_rows(900, 5, 0) < 0 and b'tile_rows' in lib.tc_last_error()
    assert lib.tc_chain_tile_rows(900, 0, 3) < 0 and b'matrix_path' in lib.tc_last_error()
    assert _lib.chain_tile_rows(8100) == 32 and _lib.chain_tile_rows(8100, 0, _lib.TC_MATRIX_F32) == 16
    with pytest.raises(_lib.TransCARHipError):
        _lib.chain_tile_rows(900, 32, _lib.TC_MATRIX_F32)


def test_entry_points_refuse_bad_arguments_without_gpu():
    """Error behaviour of the C ABI: every call below fails on its argument check -- before anything is launched, so
    no GPU is needed -- with a non-zero code and a message that names the argument (tc_last_error)."""
    lib = T.lib()
    w = _lib.tc_head_weights()
    w.abi_version = _lib.TC_ABI_VERSION
    w.num_query, w.embed_dims, w.num_heads, w.ffn_dims = 900, 256, 8, 512
    w.num_layers, w.num_cams, w.num_levels = 6, 6, 4
    w.num_classes, w.code_size, w.radar_in_dims, w.num_radar_layers = 10, 10, 36, 0
    fv = _lib.tc_feats_nhwc()
    fv.num_levels = 4
    from transcar_amd.detr3d_head import head_options

    def fwd(opt, B=1):
        return lib.tc_head_forward(ctypes.byref(w), None, ctypes.byref(fv), B, None, 928.0, 1600.0, None, 0, 0,
                                   None, None, None, ctypes.byref(opt), None, 0, None)
    assert fwd(head_options(phase=3)) != 0 and b'phase' in lib.tc_last_error()
    assert fwd(head_options(phase=1, unfused=True)) != 0 and b'phase' in lib.tc_last_error()
    o = head_options()
    o.radar_row_order = 7
    assert fwd(o) != 0 and b'radar_row_order' in lib.tc_last_error()
    o = head_options(matrix_path='f32')
    assert o.matrix_path == _lib.TC_MATRIX_F32 and head_options().matrix_path == _lib.TC_MATRIX_AUTO
    o.matrix_path = 3
    assert fwd(o) != 0 and b'matrix_path' in lib.tc_last_error()
    o = head_options()
    o.decoder_dropout_p = 1.5
    assert fwd(o) != 0 and b'decoder_dropout_p' in lib.tc_last_error()
    assert fwd(head_options(), B=0) != 0 and b'B=' in lib.tc_last_error()
    w2 = _lib.tc_head_weights()
    ctypes.memmove(ctypes.byref(w2), ctypes.byref(w), ctypes.sizeof(w))
    w2.abi_version = _lib.TC_ABI_VERSION - 1               # a caller built against another header
    assert lib.tc_head_workspace_bytes(ctypes.byref(w2), 1, 256) == 0 and b'abi_version' in lib.tc_last_error()
    # box decode: max_num outside 1..512, more candidates than the kernel holds, a code size without velocities
    pcr = (ctypes.c_float * 6)(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0)
    for args, word in (((1, 900, 10, 10, 0), b'max_num'), ((1, 900, 10, 10, 513), b'max_num'),
                       ((1, 2000, 10, 10, 300), b'num_classes'), ((1, 900, 10, 7, 300), b'code_size')):
        B, Q, ncls, code, K = args
        rc = lib.tc_box_decode_topk(None, None, B, Q, ncls, code, K, pcr, None, None, None, None, None, 0, None)
        assert rc != 0 and word in lib.tc_last_error(), (args, lib.tc_last_error())
    # optimizer: an empty bucket, a step count that is not 1-based
    assert lib.tc_sq_norm(None, 0, None, None) != 0 and b'n=0' in lib.tc_last_error()
    assert lib.tc_adamw_step(None, None, None, None, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 1.0, 35.0, None, None) != 0
    assert b'step' in lib.tc_last_error()
    assert lib.tc_dropout_mask(1.0, 1, 0, 16, None, None) != 0            # p = 1 drops everything: refused


def _fusion_head_struct(packed=True):
    """A tc_head_weights of the default fusion head that passes the dimension checks; `packed`: it looks like a view of
    tc_head_pack_weights (l0_attn_out set -- to a host buffer nothing reads: the calls below fail before any launch)."""
    w = _lib.tc_head_weights()
    w.abi_version = _lib.TC_ABI_VERSION
    w.num_query, w.embed_dims, w.num_heads, w.ffn_dims = 900, 256, 8, 512
    w.num_layers, w.num_cams, w.num_levels = 6, 6, 4
    w.num_classes, w.code_size, w.radar_in_dims, w.num_radar_layers = 10, 10, 36, 3
    keep = (ctypes.c_float * 4)()
    if packed:
        w.l0_attn_out = ctypes.cast(keep, dict(_lib.tc_head_weights._fields_)['l0_attn_out'])
    return w, keep


def test_radar_fusion_refuses_bad_layers_and_unpacked_view_without_gpu():
    """tc_radar_fusion_fwd names the layer range it was asked for and the argument that is no packed view."""
    lib = T.lib()
    w, keep = _fusion_head_struct()
    buf = ctypes.cast(keep, ctypes.c_void_p)

    def fusion(view, first, n):
        return lib.tc_radar_fusion_fwd(ctypes.byref(view), buf, buf, buf, buf, 1, 64, 1, first, n, buf, buf, None, None, None, 0, None)
    assert fusion(w, 2, 2) != 0
    assert b'radar_fusion' in lib.tc_last_error() and b'layers [2, 4) of 3' in lib.tc_last_error()
    assert fusion(w, 0, 0) != 0 and b'layers [0, 0) of 3' in lib.tc_last_error()
    raw, _ = _fusion_head_struct(packed=False)
    assert fusion(raw, 0, 3) != 0 and b'packed_view' in lib.tc_last_error()


def test_training_entry_points_name_themselves_when_the_tape_is_too_small_without_gpu():
    """Every training entry point lays out its tape (and the fused backward its workspace) before it launches anything;
    a buffer that is too small is refused with a message that begins with the entry point's own name."""
    lib = T.lib()
    w, keep = _fusion_head_struct()
    g, _ = _fusion_head_struct()
    buf = ctypes.cast(keep, ctypes.c_void_p)
    B, Tk = 1, 64
    wp, gp = ctypes.byref(w), ctypes.byref(g)
    calls = {
        'radar_train_fwd': lambda: lib.tc_radar_train_fwd(wp, buf, buf, buf, buf, B, Tk, 1, buf, buf, buf, 0, 0.0, 0, None),
        'radar_train_fwd_fused': lambda: lib.tc_radar_train_fwd_fused(wp, buf, buf, buf, buf, B, Tk, 1, buf, buf, buf, 0, 0.0, 0, None),
        'radar_train_bwd': lambda: lib.tc_radar_train_bwd(wp, gp, buf, buf, buf, B, Tk, 1, buf, buf, buf, buf, 0, 0.0, 0, None),
        'radar_train_bwd_fused': lambda: lib.tc_radar_train_bwd_fused(wp, gp, buf, buf, buf, B, Tk, 1, buf, buf, buf, buf, 0, buf, 0,
                                                                     0.0, 0, None, None, None),
        'radar_train_bwd_weights': lambda: lib.tc_radar_train_bwd_weights(wp, gp, buf, buf, B, Tk, buf, 0, buf, 0, 0, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert lib.tc_last_error() == name.encode() + b': tape too small', (name, lib.tc_last_error())
    tape_bytes = lib.tc_radar_train_tape_bytes(wp, B, Tk)
    assert tape_bytes > 0 and lib.tc_radar_train_bwd_workspace_bytes(wp, B, Tk) > 0
    rc = lib.tc_radar_train_bwd_fused(wp, gp, buf, buf, buf, B, Tk, 1, buf, buf, buf, buf, tape_bytes, buf, 0, 0.0, 0, None, None, None)
    assert rc != 0 and lib.tc_last_error() == b'radar_train_bwd_fused: workspace too small', lib.tc_last_error()


_WORKER = r'''
import os, sys
sys.path.insert(0, %r)
import torch.distributed as dist
from transcar_amd import dist as D
rank, world = D.init_process_group('gloo')
mine = D.shard_frames(7, rank, world)
res = {i: ('frame%%d' %% i, rank) for i in mine}
allr = D.gather_results(res, 7)
assert [a[0] for a in allr] == ['frame%%d' %% i for i in range(7)]
assert [a[1] for a in allr] == [i %% world for i in range(7)]
assert D.max_over_ranks(1.0 + rank) == float(world)
D.barrier()
dist.destroy_process_group()
print('ok', rank)
'''


def test_frame_sharding_gloo_world2(tmp_path):
    script = tmp_path / 'w.py'
    script.write_text(_WORKER % ROOT)
    port = 29500 + os.getpid() % 2000
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        out, _ = p.communicate(timeout=120)
        assert p.returncode == 0, out.decode()
        assert b'ok' in out


def test_shard_frames_partition():
    from transcar_amd import dist as D
    for world in (1, 2, 4, 8):
        seen = sorted(i for r in range(world) for i in D.shard_frames(37, r, world))
        assert seen == list(range(37))


def test_radar_frame_descriptor_layout_and_rotations():
    """ops.RadarRawStage packs tc_radar_frame_desc through a numpy structured dtype: same size and field offsets as
    the ctypes mirror of include/transcar_hip.h, and the vectorised quaternion -> matrix conversion of
    ops.radar_raw_arrays is bit-identical to radar.quaternion_rotation_matrix (the host builder's)."""
    import ctypes as C
    from transcar_amd import _lib as L, ops, radar as R
    dt = ops.RadarRawStage.DESC_DTYPE
    assert dt.itemsize == C.sizeof(L.tc_radar_frame_desc)
    for name in ('chan_start', 'num_chan', 'radar_rot', 'lidar_rot', 'point_range'):
        assert dt.fields[name][1] == getattr(L.tc_radar_frame_desc, name).offset, name
    for seed in range(4):
        fr = synth.make_radar_frame(seed=seed, n_per_radar=[3, 0, 5, 1, 2])
        raw, times, start, rr, lr = ops.radar_raw_arrays(fr)
        assert raw.shape == (11, 18) and times.shape == (11,) and list(start) == [0, 3, 3, 8, 9, 11]
        for i, c in enumerate(R.RADAR_CHANNELS):
            assert np.array_equal(rr[i], R.quaternion_rotation_matrix(fr['radar_rot'][c]).reshape(9))
        assert np.array_equal(lr, R.quaternion_rotation_matrix(fr['lidar_rot']).reshape(9))
