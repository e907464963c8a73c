"""The configurable radar gate on the CPU oracle (head_forward(radar_gate=...), as head_variant_rig passes the variant's):
the default gate's spellings are the call without the argument bit for bit, each layer gets its own entry, and under the
single circle the oracle computes what the circle's definition and the reference's single-circle head say.  No GPU."""
import numpy as np
import torch

import head_variant_rig as R
from oracle import transcar_oracle as O
from transcar_amd import _lib as L
from transcar_amd import synth


def _sd():
    return O.to_torch_sd(synth.make_state_dict(seed=3))


def _head_forward(feats, frame, **kw):
    with torch.no_grad():
        return O.head_forward(_sd(), [torch.from_numpy(f) for f in feats], torch.from_numpy(synth.make_lidar2img()).float()[None],
                              (928, 1600), O.build_radar_features(frame), [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], **kw)


def test_circle_oracle_agrees_with_the_references_backup_head():
    """The oracle under dict(type='circle', radii=(2, 2, 1)) against the reference's single-circle head on the same frame
    (g5_head_tiny_gate_circle.npz): outputs within E2E_TOL, hit counts exact; the stored gate margin is positive and is
    what the rig measures."""
    g5 = R.gold(R.G5_CIRCLE)
    assert tuple(g5['radii']) == tuple(R.CIRCLE['radii'])
    feats, frame = R.g5_frame(int(g5['radar_seed']))
    with torch.no_grad():
        got, dbg = R.oracle_head(_sd(), feats, frame, radar_gate=R.CIRCLE)
    assert int(dbg['fill_in']) == int(g5['fill_in'])
    for i in range(3):
        rows = np.where(dbg['hit_counts'][i].numpy() > 0)[0]
        assert len(rows) == int(g5['Lq'][i]) > 32
        assert np.array_equal(dbg['hit_counts'][i].numpy()[rows], g5['hit_counts%d' % i])
    for k in ('all_cls_scores', 'all_bbox_preds'):
        np.testing.assert_allclose(got[k].numpy(), g5[k], atol=R.E2E_TOL, rtol=0)
    # the three-circle head computes something else on this frame: the fixture cannot be met without the circle
    with torch.no_grad():
        plain, _ = R.oracle_head(_sd(), feats, frame)
    assert float(np.abs(plain['all_cls_scores'].numpy() - g5['all_cls_scores']).max()) > 0.1
    # The margin is a distance between fp32 gate centres (the free-running decoder's boxes) and tokens: another CPU's
    # evaluation order moves a centre by up to BOX_TOL (head_variant_rig: the bound between two fp32 orders of the box
    # arithmetic), so a recomputation equals the stored value to that, and bit for bit on the machine that wrote it
    # (measured on a second CPU: 1.6587e-3 m against the stored 1.6720e-3 m).  The margin itself is 30 times that bound:
    # no evaluation order flips a decision of this frame.
    margin, again = float(g5['gate_margin']), R.gate_margin(_sd(), feats, frame, radar_gate=R.CIRCLE)
    assert margin > 20 * R.BOX_TOL and abs(margin - again) <= R.BOX_TOL, (margin, again)
    assert again == R.gate_margin(_sd(), feats, frame, radar_gate=R.CIRCLE)


def test_default_gate_through_the_rig_is_the_unpatched_oracle():
    """The three spellings of the default gate, passed as radar_gate= through the rig, give the call that names no gate."""
    feats, frame = R.g5_frame()
    want, dbg = _head_forward(feats, frame, return_debug=True)
    for gate in (None, dict(type='three_circle'), dict(type='three_circle', radii=[(1.0, 2.0), (1.0, 2.0), (0.5, 1.0)])):
        with torch.no_grad():
            got, gdbg = R.oracle_head(_sd(), feats, frame, radar_gate=gate)
        for k in ('all_cls_scores', 'all_bbox_preds'):
            assert torch.equal(got[k], want[k]), (gate, k)
        for a, b in zip(gdbg['hit_counts'], dbg['hit_counts']):
            assert torch.equal(a, b)


def test_the_rig_hands_each_layer_its_own_entry():
    feats, frame = R.g5_frame()
    for gate, want in ((None, [(1.0, 2.0), (1.0, 2.0), (0.5, 1.0)]),           # the reference's constants, in layer order
                       (R.WIDE3, [tuple(p) for p in R.WIDE3['radii']]),
                       (R.CIRCLE, [(L.TC_RADAR_GATE_CIRCLE, r) for r in R.CIRCLE['radii']])):
        calls = []
        _head_forward(feats, frame, gate_probe=lambda *args: calls.append(args[5:]),
                      **({} if gate is None else {'radar_gate': gate}))
        assert calls == want, (gate, calls)


def test_circle_gate_on_the_oracle():
    feats, frame = R.g5_frame()
    plain = R.oracle_head(_sd(), feats, frame, key='g5')[0]
    with torch.no_grad():
        got, dbg = R.oracle_head(_sd(), feats, frame, radar_gate=R.CIRCLE)
    rows = [int((h > 0).sum()) for h in dbg['hit_counts']]
    assert min(rows) > 32 and rows[2] < rows[0], rows                # hit and no-hit tiles; the 1 m circle gates fewer
    assert float((got['all_cls_scores'] - plain['all_cls_scores']).abs().max()) > 0.1
    margin = R.gate_margin(_sd(), feats, frame, radar_gate=R.CIRCLE)
    assert margin > 0.0 and margin == R.gate_margin(_sd(), feats, frame, radar_gate=R.CIRCLE)
    # the definition at the edge: inclusive, and a NaN distance is attended
    c = torch.zeros((1, 2, 2))
    c[0, 1] = float('nan')
    y = torch.tensor([[[2.0, 0.0], [0.0, -2.0], [float(np.nextafter(np.float32(2.0), np.float32(np.inf))), 0.0]]])
    assert O.single_circle_mask(c, y, 2.0).tolist() == [[False, False, True], [False, False, False]]
