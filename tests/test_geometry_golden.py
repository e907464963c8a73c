"""The CPU oracle at a point-cloud range and an image size that are not the configs' (head_variant_rig.GEOM) against
the fixtures tests/golden/make_golden_variants.py `geometry` recorded from the reference, with the tolerances of
test_oracle_golden.py, test_decoder_outputs_golden.py and test_training.py.  No GPU, no reference.

The GPU tests of tests/test_gpu_geometry.py hold the library to this oracle and to the same fixtures; here the oracle
itself is held to the reference, so that a range site the oracle got wrong could not pass on both sides."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import GEOM
from oracle import transcar_oracle as O
from parity_util import assert_rows_match
from test_decoder_outputs_golden import CLS_ULPS
from test_oracle_golden import E2E_TOL
from transcar_amd import synth

PCR = list(GEOM.pc_range)
HW = GEOM.hw


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope='module')
def sd():
    return O.to_torch_sd(synth.make_state_dict(seed=3))


def _l2i():
    return torch.from_numpy(GEOM.lidar2img()).float()[None]


def test_the_geometry_is_the_issues():
    assert GEOM.pc_range == (-30.0, -60.0, -4.0, 70.0, 36.0, 6.0)
    assert GEOM.post_center_range == (-40.0, -70.0, -6.0, 80.0, 45.0, 8.0)
    assert GEOM.img_shape == (640, 1152, 3) and GEOM.hw == (640, 1152)
    assert GEOM.focal == 1266 * 1152 / 1600 and GEOM.pp == (576.0, 320.0)
    assert len({abs(v) for v in GEOM.pc_range}) == 6            # six distinct magnitudes
    m = GEOM.metas(2)
    assert len(m) == 2 and m[1]['img_shape'] == [(640, 1152, 3)] * 6
    np.testing.assert_array_equal(np.stack(m[0]['lidar2img']), synth.make_lidar2img(focal=911.52, pp=(576.0, 320.0)))


def test_g2_cross_atten_geom(sd):
    g = R.gold('g2_cross_atten_geom.npz')
    rng = np.random.RandomState(21)
    feats = [torch.from_numpy(f) for f in synth.make_feats('tiny', seed=22)]
    query = torch.from_numpy(rng.standard_normal((900, 1, 256)).astype(np.float32))
    qpos = torch.from_numpy(rng.standard_normal((900, 1, 256)).astype(np.float32))
    refp = torch.from_numpy(rng.uniform(0.02, 0.98, (1, 900, 3)).astype(np.float32))
    out = O.cross_atten(sd, 'transformer.decoder.layers.2.attentions.1', query, qpos, feats, refp, PCR, _l2i(), HW)
    np.testing.assert_allclose(out.numpy()[::4], g['out'], atol=2e-5, rtol=0)
    # and it is no fixture of the configs' geometry under another name
    assert np.abs(g['out'] - R.gold('g2_cross_atten.npz')['out']).max() > 0.1


def test_g5_full_head_geom(sd):
    """test_oracle_golden.test_g5_full_head at the geometry, its tolerances unchanged."""
    g = R.gold('g5_head_tiny_geom.npz')
    feats_np = synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g['radar_centres'])
    f36 = O.build_radar_features(frame)
    assert f36.shape[0] == int(g['fill_in'])
    np.testing.assert_allclose(f36.astype(np.float32), g['radar_tokens'], atol=1e-6, rtol=1e-6)
    outs, dbg = R.oracle_head(sd, feats_np, frame, key='g5 geom', geometry=GEOM)
    np.testing.assert_allclose(dbg['inter_refs'].numpy(), g['inter_refs'], atol=2e-5, rtol=0)
    np.testing.assert_allclose(dbg['init_ref'].numpy(), g['init_ref'], atol=1e-6, rtol=0)
    hs = dbg['hs'].permute(0, 2, 1, 3).numpy()
    np.testing.assert_allclose(hs[:, ::16, 0, :], g['hs_rows'], atol=5e-5, rtol=0)
    for i in range(3):
        assert len(dbg['hit_rows'][i]) == int(g['Lq'][i])
        assert np.array_equal(dbg['hit_counts'][i][dbg['hit_rows'][i]].numpy(), g['hit_counts%d' % i])
    np.testing.assert_allclose(outs['all_cls_scores'].numpy(), g['all_cls_scores'], atol=E2E_TOL, rtol=0)
    np.testing.assert_allclose(outs['all_bbox_preds'].numpy(), g['all_bbox_preds'], atol=E2E_TOL, rtol=0)
    b, s, l = O.get_bboxes(outs, list(GEOM.post_center_range))[0]
    np.testing.assert_allclose(s.numpy(), g['dec_scores'], atol=1e-5, rtol=0)
    mine = np.concatenate([b.numpy(), s.numpy()[:, None], l.numpy()[:, None].astype(np.float32)], 1)
    gold = np.concatenate([g['dec_boxes'], g['dec_scores'][:, None], g['dec_labels'][:, None].astype(np.float32)], 1)
    assert_rows_match(mine, gold, atol=2e-4, what='decoded boxes')
    # the boxes are not the configs' geometry's: up to 25.9 m apart, measured where the fixture was made
    assert np.abs(g['all_bbox_preds'][..., :2] - R.gold('g5_head_tiny.npz')['all_bbox_preds'][..., :2]).max() > 10.0


def test_decoder_levels_geom_on_the_references_states(sd):
    """test_decoder_outputs_golden.test_helper_matches_the_references_decoder_levels at the geometry: K_BOXSIG's and
    K_REFUPD's formula on the reference's own states, boxes within BOX_TOL -- at 70 m still 6 fp32 spacings."""
    g10, g5 = R.gold('g10_decoder_outputs_tiny_geom.npz'), R.gold('g5_head_tiny_geom.npz')
    assert g10['dec_cls'].shape == (6, 1, 900, 10) and g10['dec_box'].shape == (6, 1, 900, 10)
    cls, box = O.decoder_outputs(sd, torch.from_numpy(g5['hs_rows'])[:, None], torch.from_numpy(g5['init_ref'])[:, ::16],
                                 torch.from_numpy(g5['inter_refs'])[:, :, ::16], PCR)
    d_cls = np.abs(cls.numpy() - g10['dec_cls'][:, :, ::16]).max()
    d_box = np.abs(box.numpy() - g10['dec_box'][:, :, ::16]).max()
    print('reference states: max|helper - reference| logits %.3g, boxes %.3g m' % (d_cls, d_box))
    if not np.array_equal(cls.numpy(), g10['dec_cls'][:, :, ::16]):
        assert d_cls <= CLS_ULPS * float(np.spacing(np.float32(4.0))), d_cls
    assert d_box <= R.BOX_TOL, d_box
    refs_m = O.denormalised_refs(torch.from_numpy(g5['inter_refs']), PCR).numpy()
    d_ref = np.abs(g10['dec_box'][..., [0, 1, 4]] - refs_m).max()
    print('max|box centre - denormalised inter_references| = %.3g m' % d_ref)
    assert d_ref <= R.BOX_TOL, d_ref


def test_decoder_levels_geom_on_the_oracles_trace():
    g10 = R.gold('g10_decoder_outputs_tiny_geom.npz')
    cls, box = R.oracle_outputs(geometry=GEOM)
    print('oracle trace: max|oracle - reference| logits %.3g, boxes %.3g m'
          % (np.abs(cls - g10['dec_cls']).max(), np.abs(box - g10['dec_box']).max()))
    R.assert_all_but_two_queries(cls[:, 0], g10['dec_cls'][:, 0], R.E2E_TOL, 'logits: oracle vs reference')
    R.assert_all_but_two_queries(box[:, 0], g10['dec_box'][:, 0], R.E2E_TOL, 'boxes: oracle vs reference')


def test_oracle_backward_matches_reference_geom():
    """test_training.test_oracle_backward_matches_reference at the geometry (G8-GEOM), 2e-3."""
    g8 = R.gold('g8_train_grads_geom.npz')
    f = R.g8_frame('g5_head_tiny_geom.npz', radar_seed=int(g8['radar_seed']), geometry=GEOM)
    outs, losses, _, grads = R.oracle_training(f, geometry=GEOM)
    assert np.abs(outs['all_cls_scores'].numpy() - g8['all_cls_scores']).max() < 5e-4
    assert abs(sum(losses.values()) - float(g8['total_loss'])) < 1e-4 * float(g8['total_loss'])
    R.check_grads_against_g8(grads, g8, 2e-3, 'oracle, geometry')


def test_decode_geom():
    """NMSFreeCoder.decode_single with GEOM's post_center_range (G6-GEOM): the oracle keeps the reference's rows."""
    g = R.gold('g6_decode_geom.npz')
    assert tuple(float(v) for v in g['post_center_range']) == GEOM.post_center_range
    b, s, l = O.nms_free_decode(torch.from_numpy(g['cls'][0]), torch.from_numpy(g['box'][0]), list(GEOM.post_center_range))
    np.testing.assert_array_equal(l.numpy(), g['labels'])
    np.testing.assert_allclose(s.numpy(), g['scores'], atol=1e-6, rtol=0)
    np.testing.assert_allclose(b.numpy(), g['bboxes'], atol=2e-5, rtol=0)
