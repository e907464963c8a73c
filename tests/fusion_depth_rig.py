"""What the tests of Detr3DHead(num_fusion_layers=N) share: N-layer heads with the first N layers' weights of the
three-layer state dict (head_variant_rig.variant_kw asserts its keys, so these are built here), G5's tiny frame, and
the gradient check of a fixture whose parameter count follows N.

A plain helper module, as head_variant_rig.py."""
import numpy as np
import torch

import head_variant_rig as R
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

DEPTHS = (1, 2)


def num_trained(head):
    """The parameters one iteration produces a gradient for, counted on the head (three layers: test_training's 98)."""
    return len(head.trainable_parameters())


def state_dict(depth, seed=3):
    return synth.make_state_dict(seed=seed, num_fusion_layers=depth)


def make_head(T, depth, seed=3, train_cfg=False):
    """A fresh eval-mode head with `depth` fusion layers and the seeded weights (the three-layer head's, minus the absent
    layers), on the GPU where there is one."""
    cfg = configs.head_cfg(num_fusion_layers=depth)
    if train_cfg:
        cfg['train_cfg'] = configs.train_cfg_pts
    h = T.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict(depth, seed).items()}, strict=True)
    assert h.num_fusion_layers == depth and h.weights_struct().num_radar_layers == depth
    return h.to(R.dev()).eval() if torch.cuda.is_available() else h.eval()


_HEADS = {}


def shared_head(T, depth):
    """make_head(T, depth), one per depth for the tests that leave it as they found it."""
    if depth not in _HEADS:
        _HEADS[depth] = make_head(T, depth)
    return _HEADS[depth]


def train_head(depth):
    import transcar_amd as T
    return make_head(T, depth, train_cfg=True).freeze_decoder().set_dropout(0.0)


def g5_frame():
    """G5's tiny rig: (feats_np, radar frame) of tests/golden/g5_head_tiny.npz."""
    feats = synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=R.gold('g5_head_tiny.npz')['radar_centres'])
    return feats, frame


def empty_frame():
    """A radar frame without a single return: every token is padding, no query has a hit in any layer."""
    return synth.make_radar_frame(seed=5, n_per_radar=[0, 0, 0, 0, 0])


_ORACLE = {}


def oracle_g5():
    """The oracle's three-layer forward on G5's frame with its debug dict, once."""
    if 'g5' not in _ORACLE:
        feats, frame = g5_frame()
        with torch.no_grad():
            _ORACLE['g5'] = R.oracle_head(O.to_torch_sd(synth.make_state_dict(seed=3)), feats, frame)
    return _ORACLE['g5']


def check_against_fixture(outs, depth):
    """head_variant_rig.check_against_fixture's rule on levels [:depth]: the rows whose gate decisions agree with the
    oracle's AND the reference's (g5_head_tiny.npz), at most MAX_GATE_ROWS left out, E2E_TOL."""
    want, dbg = oracle_g5()
    fixture = R.gold('g5_head_tiny.npz')
    aux = outs['aux']
    np.testing.assert_allclose(aux['inter_references'].cpu().numpy(), fixture['inter_refs'], atol=R.REFS_TOL, rtol=0)
    want_hits = np.stack([h.cpu().numpy() for h in dbg['hit_counts']])[:depth]
    gold_hits = np.zeros_like(want_hits)
    for i in range(depth):
        rows = np.where(want_hits[i] > 0)[0]
        gold_hits[i] = want_hits[i]
        if len(rows) == int(fixture['Lq'][i]):
            gold_hits[i] = 0
            gold_hits[i, rows] = fixture['hit_counts%d' % i]
    hits = aux['radar_hit_counts'][:, 0].cpu().numpy()
    assert hits.shape == want_hits.shape
    agree = np.all(hits == want_hits, axis=0) & np.all(hits == gold_hits, axis=0)
    assert int((~agree).sum()) <= R.MAX_GATE_ROWS
    for k in ('all_cls_scores', 'all_bbox_preds'):
        got = outs[k][:, 0].cpu().numpy()
        assert got.shape[0] == depth
        R.assert_all_but_two_queries(got[:, agree], fixture[k][:depth, 0][:, agree], R.E2E_TOL, k + ' vs reference')
        R.assert_all_but_two_queries(got[:, agree], want[k][:depth, 0].cpu().numpy()[:, agree], R.E2E_TOL, k + ' vs oracle')


def check_grads_against_g8(grads, g8, rtol, what, expected):
    """test_training.check_grads_against_g8's comparison (that function asserts the three-layer head's 98 entries) for a
    fixture of `expected` gradient entries: every parameter of `grads` has an entry in the fixture -- its gradient's
    [sum, sum|.|, l2] and first 16 values, or `__none` -- and the fixture has no entry beyond them."""
    stats = {k[:-len('__stats')] for k in g8.files if k.endswith('__stats')}
    nones = {k[:-len('__none')] for k in g8.files if k.endswith('__none')}
    assert len(stats) == expected, (what, len(stats), expected)
    keys = {k.replace('.', '__') for k in grads}
    assert keys == stats | nones, (what, sorted(keys ^ (stats | nones)))
    checked = 0
    for k, g in grads.items():
        key = k.replace('.', '__')
        if key in nones:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        assert g is not None, (what, k)
        ref = g8[key + '__stats']
        gd = g.detach().double().flatten().cpu()
        got = np.array([gd.sum(), gd.abs().sum(), gd.norm()])
        scale = ref[1]                      # sum |g|: the natural magnitude for all three
        assert abs(got[1] - ref[1]) <= rtol * scale, (what, k, got, ref)
        assert abs(got[2] - ref[2]) <= rtol * max(ref[2], 1e-12), (what, k, got, ref)
        assert abs(got[0] - ref[0]) <= rtol * scale, (what, k, got, ref)
        head = g8[key + '__head']
        tol = rtol * max(np.abs(head).max(), ref[2] / np.sqrt(gd.numel()))
        assert np.abs(gd[:16].float().numpy() - head).max() <= 4 * tol, (what, k)
        checked += 1
    assert checked == expected, (what, checked, expected)
    return checked
