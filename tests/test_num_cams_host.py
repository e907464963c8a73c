"""Detr3DCrossAtten.num_cams 1 .. 16, host side: the configuration key, the check, the library's refusals through its
size queries, the packed buffer of a head beyond eight cameras (no layer-0 constants), the synthetic state dict against
the reference head's own shapes, the ring rig's coverage and radar seeds, and the oracle against the reference's
12-camera fixture.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
import num_cams_rig as NR
from oracle import transcar_oracle as O
from transcar_amd import _lib as L
from transcar_amd import build_head, configs, synth


def _head(num_cams=None, num_query=NR.NQ, **kw):
    h = build_head(configs.head_cfg(num_query=num_query, num_cams=num_cams, **kw))
    sd = synth.make_state_dict(seed=3, num_query=num_query, **dict(kw, **({} if num_cams is None else {'num_cams': num_cams})))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return h


def _attn_cfg(cfg):
    return cfg['transformer']['decoder']['transformerlayers']['attn_cfgs'][1]


def test_head_cfg_key_reaches_every_layer():
    for n in (None, 6):
        cfg = configs.head_cfg(num_cams=n)
        assert cfg == configs.head_cfg() and 'num_cams' not in _attn_cfg(cfg) and 'num_cams' not in cfg['transformer']
    cfg = configs.head_cfg(num_cams=12)
    assert _attn_cfg(cfg)['num_cams'] == cfg['transformer']['num_cams'] == 12
    h = build_head(cfg)
    assert h.transformer.num_cams == 12 and len(h.transformer.decoder.layers) == 6
    for ly in h.transformer.decoder.layers:
        assert ly.attentions[1].num_cams == 12 and ly.attentions[1].attention_weights.out_features == 48
    assert h.attention_weights2.out_features == h.attention_weights3.out_features == 24      # HEAD:191-192


def test_check_num_cams():
    assert L.TC_MAX_CAMS == 16
    for n in range(1, 17):
        assert L.check_num_cams(n) == n
    from transcar_amd.detr3d_transformer import Detr3DCrossAtten
    for bad in (0, 17, -1, True, False, 6.0, '6', None):
        with pytest.raises(L.TransCARHipError, match='num_cams='):
            L.check_num_cams(bad)
        if bad is not None:
            with pytest.raises(L.TransCARHipError, match='num_cams='):
                configs.head_cfg(num_cams=bad)
        with pytest.raises(L.TransCARHipError, match='num_cams='):
            Detr3DCrossAtten(num_cams=bad, num_points=1, pc_range=configs.point_cloud_range)
    # a count set on the modules after construction is caught before anything is packed
    h = _head()
    for ly in h.transformer.decoder.layers:
        ly.attentions[1].num_cams = 17
    with pytest.raises(L.TransCARHipError, match='num_cams=17'):
        h.weights_struct()


def test_frame_is_checked_against_the_head():
    L.check_frame_cams(12, 12, 2, [24, 24, 24, 24])
    with pytest.raises(L.TransCARHipError, match='11 lidar2img.*num_cams=12'):
        L.check_frame_cams(12, 11)
    with pytest.raises(L.TransCARHipError, match=r'22 images.*2 \* 12 = 24'):
        L.check_frame_cams(12, 12, 2, [24, 22])


def test_struct_fields_and_library_refusals():
    lib = L.lib()
    w = _head(12).weights_struct()
    assert (w.num_cams, w.num_levels, w.num_points, w.num_query) == (12, 4, 1, NR.NQ)
    assert L.TC_ABI_VERSION == 13 and lib.tc_abi_version() == 13 and L.tc_head_weights._fields_[-1][0] == 'num_points'
    queries = (lambda: lib.tc_head_packed_bytes(ctypes.byref(w)), lambda: lib.tc_head_workspace_bytes(ctypes.byref(w), 1, 64),
               lambda: lib.tc_cam_pregather_workspace_bytes(ctypes.byref(w), 1))
    for q in queries:
        assert q() > 0
    for bad in (0, 17, -3):
        w.num_cams = bad
        for q in queries:
            assert q() == 0 and ('num_cams=%d' % bad) in lib.tc_last_error().decode(), lib.tc_last_error()
    for n in (1, 16):
        w.num_cams = n
        assert queries[1]() > 0
    # 16 cameras x 4 levels x 5 points are more logits than a row's activation unit holds: still refused, by that name
    w.num_cams, w.num_points = 16, 5
    assert queries[0]() == 0 and b'num_points=5' in lib.tc_last_error()


def test_packed_buffer_beyond_eight_cameras_has_no_layer0_constants():
    """As a num_points > 1 head (tests/test_layer0_fold_host.py): the five blocks of three [Q, C] constants give way to
    the pack-time scratch; attention_weights stays one 64-row tile up to 16 cameras at 4 levels."""
    Q, C, VARIANTS = NR.NQ, 256, 5
    plane = ((Q * C * 4 + 255) // 256) * 256
    scratch = 2 * plane + ((C * ((Q + 15) // 16) * 16 * 4 + 255) // 256) * 256
    size = {n: L.lib().tc_head_packed_bytes(ctypes.byref(_head(n).weights_struct())) for n in (6, 8, 9, 12, 16)}
    assert size[6] == size[8] > 0 and size[9] == size[12] == size[16] > 0
    assert size[8] - size[9] == VARIANTS * 3 * plane - scratch


def test_synth_state_dict_has_the_reference_heads_shapes():
    """The reference head built at 12 cameras (its state dict's keys and shapes are in the fixture): attention_weights
    [48, 256], the unused attention_weights2/3 [24, 256] whatever the count."""
    g = R.gold(NR.G5_CAMS12)
    ref = {str(k): tuple(int(v) for v in s[:n]) for k, s, n in zip(g['sd_keys'], g['sd_shapes'], g['sd_ndim'])}
    mine = {k: tuple(v.shape) for k, v in NR.state_dict(12).items()}
    assert mine == ref
    assert ref['transformer.decoder.layers.0.attentions.1.attention_weights.weight'] == (48, 256)
    assert ref['attention_weights2.weight'] == ref['attention_weights3.weight'] == (24, 256)
    for n in (1, 9, 16):
        spec = {k: s for k, s, _ in synth.state_dict_spec(num_cams=n)}
        assert spec['attention_weights2.weight'] == spec['attention_weights3.weight'] == (24, 256)
        assert spec['transformer.decoder.layers.5.attentions.1.attention_weights.weight'] == (4 * n, 256)
    # the configs' count draws what it drew
    a, b = synth.make_state_dict(seed=3), synth.make_state_dict(seed=3, num_cams=6)
    assert all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def test_ring_yaws():
    assert synth.ring_yaws(4) == (-180.0, -90.0, 0.0, 90.0)
    for n in NR.COUNTS:
        y = synth.ring_yaws(n)
        assert len(y) == n and y[0] == -180.0 and np.allclose(np.diff(y), 360.0 / n)
        assert NR.Ring(n).lidar2img().shape == (n, 4, 4)
    assert NR.Ring(12) == NR.Ring(12) != NR.Ring(12, 9) and NR.Ring(6) != R.DEFAULT
    assert R.variant_kw(**NR.variant(12)) == dict(num_query=NR.NQ, num_cams=12)
    assert R.variant_kw(**NR.variant(6)) == dict(num_query=NR.NQ)


@pytest.mark.parametrize('N', [9, 12, 16])
def test_rig_coverage(N):
    """What a rig of more than eight cameras must exercise, in every decoder layer (the oracle's visibility): queries
    that see only cameras from index 8 up, queries that see one below and one above, three cameras at once (12, 16), the
    last camera -- on both lidar2img sets of the batch."""
    cov = NR.coverage(N)
    print(N, cov)
    NR.assert_coverage(N)
    NR.assert_coverage(N, NR.oracle(N, jitter_seed=NR.JITTER)[4], NR.JITTER)


@pytest.mark.parametrize('key', sorted(NR.RADAR_SEEDS, key=str), ids=str)
def test_stored_radar_seeds_are_the_search_results(key):
    """The stored seed is the gate-margin search's choice among seeds 2 .. 39 on the oracle's own centres, and its
    closest gate decision keeps the stored distance: far from the radius next to BOX_TOL, so that the oracle's own gate
    rows are not the ones MAX_GATE_ROWS is there for."""
    seed, margin = NR.RADAR_SEEDS[key]
    got_seed, got = NR.search_seed(key[0], **dict(key[1:]))
    assert got_seed == seed and abs(got - margin) <= R.BOX_TOL and got > 8 * R.BOX_TOL, (got_seed, got)


def test_oracle_against_the_reference_at_twelve_cameras():
    """tests/test_oracle_golden.py::test_g5_full_head on the 12-camera fixture, the count given by argument"""
    g = R.gold(NR.G5_CAMS12)
    sd = O.to_torch_sd(NR.state_dict(12))
    feats = [torch.from_numpy(f) for f in NR.feats(12)]
    l2i = torch.from_numpy(NR.Ring(12).lidar2img()).float()[None]
    assert int(g['radar_seed']) == NR.G8_CAMS12_RADAR_SEED and float(g['gate_margin']) > 8 * R.BOX_TOL
    f36 = O.build_radar_features(synth.make_radar_frame(seed=int(g['radar_seed']), n_per_radar=51, centres=g['radar_centres']))
    assert f36.shape[0] == int(g['fill_in'])
    np.testing.assert_allclose(f36.astype(np.float32), g['radar_tokens'], atol=1e-6, rtol=1e-6)
    with torch.no_grad():
        outs, dbg = O.head_forward(sd, feats, l2i, R.HW, f36, R.PCR, return_debug=True, num_cams=12)
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g['inter_refs'], atol=2e-5, rtol=0)
    np.testing.assert_allclose(dbg['init_ref'].numpy(), g['init_ref'], atol=1e-6, rtol=0)
    np.testing.assert_allclose(dbg['hs'].numpy()[:, 0, ::16], g['hs_rows'], atol=5e-5, rtol=0)
    for i in range(3):
        assert len(dbg['hit_rows'][i]) == int(g['Lq'][i])
        assert np.array_equal(dbg['hit_counts'][i][dbg['hit_rows'][i]].numpy(), g['hit_counts%d' % i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(outs[k].numpy(), g[k], atol=R.E2E_TOL, rtol=0)
    # the fixture's rig has the coverage too (the reference's reference points are the oracle's within 2e-5)
    NR.assert_coverage(12, dbg)


def test_gradient_fixture_names_its_frame():
    g8 = R.gold(NR.G8_CAMS12)
    assert int(g8['radar_seed']) == NR.G8_CAMS12_RADAR_SEED
    assert float(g8['gate_margin']) > 8 * R.BOX_TOL
    assert sum(k.endswith('__stats') for k in g8.files) == 98
