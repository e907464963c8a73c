"""The caps of head_variant_rig.py's checkers, on small synthetic tensors (CPU; no reference): the GPU tests of every
head variant go through these checkers, so a loosened cap here would loosen all of them.  And the variant keys: what
each reaches, and that the oracle's arguments for them default to the configs' head (37 queries on the tiny maps) --
its first N fusion layers being the first N levels of the three."""
import numpy as np
import pytest
import torch

import head_variant_rig as R

LAYERS, Q, C = 6, 16, 256


def _case(seed=0, depth=3):
    """(outs, want, dbg, fixture) of a head that agrees with the oracle and the reference exactly: 6 decoder layers,
    batch 1, 16 queries, 3 fusion layers; queries 0 .. 11 hit radar returns in every fusion layer.  depth < 3: the head
    has the first `depth` fusion layers, the oracle's run and the fixture keep their three."""
    g = torch.Generator().manual_seed(seed)
    refs = torch.rand((LAYERS, 1, Q, 3), generator=g)
    hs = torch.randn((LAYERS, 1, Q, C), generator=g)
    hits = torch.zeros((3, Q), dtype=torch.int64)
    hits[:, :12] = torch.randint(1, 9, (3, 12), generator=g)
    want = {k: torch.randn((3, 1, Q, 10), generator=g) for k in ('all_cls_scores', 'all_bbox_preds')}
    outs = {k: v.clone() for k, v in want.items()}
    outs['aux'] = dict(inter_references=refs.clone(), inter_states=hs.clone(), init_reference=refs[0].clone(),
                       radar_hit_counts=hits[:, None].clone())
    dbg = dict(inter_refs=refs, hs=hs, hit_counts=list(hits))
    fixture = dict(inter_refs=refs.numpy().copy(), Lq=np.array([12, 12, 12]),
                   **{'hit_counts%d' % i: hits[i, :12].numpy().copy() for i in range(3)},
                   **{k: v.numpy().copy() for k, v in want.items()})
    for k in want:
        outs[k] = outs[k][:depth]
    outs['aux']['radar_hit_counts'] = outs['aux']['radar_hit_counts'][:depth]
    return outs, want, dbg, fixture


def test_checkers_accept_an_exact_copy():
    outs, want, dbg, fixture = _case()
    R.check_against_oracle(outs, want, dbg)
    R.check_against_fixture(outs, want, dbg, fixture)
    R.check_against_fixture(outs, want, dbg, fixture, tie_rule=True)
    outs['aux']['inter_references'][:] = outs['aux']['init_reference']
    R.refs_are_initial(outs['aux'])


@pytest.mark.parametrize('hs_tol', [R.E2E_TOL, R.HS_TOL_F16X2])
def test_oracle_check_rejects_one_state_beyond_its_tolerance(hs_tol):
    assert (R.E2E_TOL, R.HS_TOL_F16X2) == (1e-3, 2e-3)
    outs, want, dbg, _ = _case()
    outs['aux']['inter_states'][3, 0, 5, 100] += 2 * hs_tol
    with pytest.raises(AssertionError):
        R.check_against_oracle(outs, want, dbg, hs_tol)


def test_checks_reject_one_reference_coordinate_off_by_1e_4():
    outs, want, dbg, fixture = _case()
    outs['aux']['inter_references'][4, 0, 7, 1] += 1e-4
    with pytest.raises(AssertionError):
        R.check_against_oracle(outs, want, dbg)
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture)


def _flip_gates(outs, n):
    outs['aux']['radar_hit_counts'][1, 0, :n] += 1


def test_gate_rows_six_may_disagree_and_carry_wrong_scores_seven_may_not():
    outs, want, dbg, fixture = _case()
    _flip_gates(outs, 6)
    outs['all_cls_scores'][2, 0, 3, 4] += 0.5
    R.check_against_oracle(outs, want, dbg)
    R.check_against_fixture(outs, want, dbg, fixture)
    _flip_gates(outs, 7)
    with pytest.raises(AssertionError):
        R.check_against_oracle(outs, want, dbg)
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture)


@pytest.mark.parametrize('k', ['all_cls_scores', 'all_bbox_preds'])
def test_oracle_check_rejects_one_score_off_by_2e_3_on_an_agreeing_row(k):
    outs, want, dbg, _ = _case()
    _flip_gates(outs, 6)
    outs[k][0, 0, 9, 2] += 2e-3
    with pytest.raises(AssertionError):
        R.check_against_oracle(outs, want, dbg)


@pytest.mark.parametrize('depth', R.DEPTHS)
def test_fixture_check_of_a_shallower_head_is_the_three_level_matrix_on_its_levels(depth):
    """levels [:depth] of the oracle's run and of the fixture: the exact copy passes, six flipped gate rows with a wrong
    score on one of them pass and seven do not, a third query off by 5e-3 is refused"""
    last = depth - 1
    outs, want, dbg, fixture = _case(depth=depth)
    assert outs['all_cls_scores'].shape[0] == depth and want['all_cls_scores'].shape[0] == 3
    R.check_against_fixture(outs, want, dbg, fixture)
    R.check_against_fixture(outs, want, dbg, fixture, tie_rule=True)
    outs['aux']['radar_hit_counts'][last, 0, :6] += 1
    outs['all_cls_scores'][last, 0, 3, 4] += 0.5
    R.check_against_fixture(outs, want, dbg, fixture)
    outs['aux']['radar_hit_counts'][last, 0, :7] += 1
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture)
    outs, want, dbg, fixture = _case(depth=depth)
    outs['all_bbox_preds'][last, 0, 2:4, 1] += 5e-3
    R.check_against_fixture(outs, want, dbg, fixture)
    outs['all_bbox_preds'][last, 0, 4, 1] += 5e-3
    for tie_rule in (False, True):
        with pytest.raises(AssertionError):
            R.check_against_fixture(outs, want, dbg, fixture, tie_rule=tie_rule)
    # a head with a level the fixture's cut does not cover is refused on its shape
    outs, want, dbg, fixture = _case(depth=depth)
    outs['aux']['radar_hit_counts'] = torch.cat([outs['aux']['radar_hit_counts']] * 2)[:depth + 1]
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture)


def _queries_off(n, by):
    want = np.zeros((3, Q, 10), np.float32)
    got = want.copy()
    got[1, :n, 3] += by
    return got, want


def test_all_but_two_queries():
    R.assert_all_but_two_queries(*_queries_off(2, 5e-3), 1e-3, 'two')
    with pytest.raises(AssertionError):
        R.assert_all_but_two_queries(*_queries_off(3, 5e-3), 1e-3, 'three')
    with pytest.raises(AssertionError):
        R.assert_all_but_two_queries(*_queries_off(1, 2e-2), 1e-3, 'one, far')


def test_fixture_check_holds_the_head_to_both():
    """three queries off by 5e-3 from the reference and the oracle alike are refused, with or without the tie rule"""
    outs, want, dbg, fixture = _case()
    outs['all_bbox_preds'][0, 0, 2:4, 1] += 5e-3
    R.check_against_fixture(outs, want, dbg, fixture)
    outs['all_bbox_preds'][0, 0, 4, 1] += 5e-3
    for tie_rule in (False, True):
        with pytest.raises(AssertionError):
            R.check_against_fixture(outs, want, dbg, fixture, tie_rule=tie_rule)


def test_tie_rule_leaves_two_queries_to_the_oracle_alone_and_rejects_three():
    outs, want, dbg, fixture = _case()
    for n in (1, 2):
        fixture['all_cls_scores'][2, 0, n, 0] += 0.1         # oracle and reference part: a gate tie
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture)    # (without the rule the head is off the reference)
    R.check_against_fixture(outs, want, dbg, fixture, tie_rule=True)
    outs['all_cls_scores'][2, 0, 1, 0] += 2e-2               # ... but a tie query is still held to the oracle
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture, tie_rule=True)
    outs['all_cls_scores'][2, 0, 1, 0] = want['all_cls_scores'][2, 0, 1, 0]
    fixture['all_cls_scores'][2, 0, 3, 0] += 0.1
    with pytest.raises(AssertionError, match=r'\[1, 2, 3\]'):
        R.check_against_fixture(outs, want, dbg, fixture, tie_rule=True)


def test_refs_are_initial_rejects_one_ulp():
    outs, want, dbg, fixture = _case()
    aux = outs['aux']
    aux['inter_references'][:] = aux['init_reference']
    v = aux['inter_references'][5, 0, 3, 2]
    aux['inter_references'][5, 0, 3, 2] = torch.nextafter(v, v + 1)
    with pytest.raises(AssertionError):
        R.refs_are_initial(aux)
    dbg['inter_refs'], fixture['inter_refs'] = aux['inter_references'], aux['inter_references'].numpy()
    R.check_against_oracle(outs, want, dbg)
    with pytest.raises(AssertionError):
        R.check_against_oracle(outs, want, dbg, refs_initial=True)
    with pytest.raises(AssertionError):
        R.check_against_fixture(outs, want, dbg, fixture, refs_initial=True)


# ---- the gradient check ------------------------------------------------------------------------------------------------------
def _grads(seed=0):
    """{name: gradient or None} of five parameters, two of them unused, and its GradStats"""
    g = torch.Generator().manual_seed(seed)
    grads = {'rf_linear1.weight': torch.randn((64, 32), generator=g), 'rf_linear1.bias': torch.randn(64, generator=g),
             'final_cls.0.weight': torch.randn((32, 32), generator=g), 'rf_norm1.weight': None, 'rf_norm1.bias': None}
    return grads, R.GradStats(grads)


def test_grads_check_accepts_itself_and_refuses_what_differs():
    grads, g8 = _grads()
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'itself', 3) == 3
    grads['rf_norm1.bias'] = torch.zeros(32)                        # an unused parameter may carry a zero gradient
    assert R.check_grads_against_g8(grads, g8, 2e-3, 'a zero', 3) == 3

    def refused(grads, g8, expected=3):
        with pytest.raises(AssertionError):
            R.check_grads_against_g8(grads, g8, 2e-3, 'refused', expected)
    grads, g8 = _grads()
    g8['rf_linear1__bias__stats'][1] *= 1.01                        # one entry's sum|.| off by 1 %
    refused(grads, g8)
    grads, g8 = _grads()
    for name in ('final_cls.0.weight', 'rf_norm1.weight'):          # one name missing from the gradients
        refused({k: v for k, v in grads.items() if k != name}, g8)
    g8['final_reg__0__weight__none'] = np.zeros(1)                  # one extra name in the fixture
    refused(grads, g8)
    del g8['final_reg__0__weight__none']
    g8['final_reg__0__weight__stats'], g8['final_reg__0__weight__head'] = np.ones(3), np.zeros(16, np.float32)
    refused(grads, g8, 3)
    refused(grads, g8, 4)
    grads, g8 = _grads()
    refused(grads, g8, 98)                                          # a wrong expected count
    refused(grads, g8, 2)
    grads['rf_norm1.weight'] = torch.full((32,), 1e-30)             # a non-zero gradient under a __none key
    refused(grads, g8)


# ---- the variant keys, and the oracle's arguments for them ---------------------------------------------------------------
def test_variant_kw_takes_the_configs_keys_and_refuses_others():
    assert R.CONFIGS == dict(num_levels=4, num_points=1, with_box_refine=True, num_heads=8, num_classes=10, num_query=900,
                             num_fusion_layers=3, radar_gate=None, radar_num_heads=8, radar_num_tokens=1500, radar_in_dims=36,
                             radar_point_range=None, feedforward_channels=512)
    assert R.variant_kw(**R.CONFIGS) == {} and R.variant_key(**R.CONFIGS) == ()
    kw = dict(num_heads=4, num_classes=23, num_query=37)
    assert R.variant_kw(num_points=1, **kw) == kw
    assert R.state_dict_kw(**kw) == dict(num_classes=23, num_query=37)         # the state dict has no head count
    assert R.decoder_kw(**kw) == dict(with_box_refine=True, num_heads=4, num_cams=6)
    assert R.oracle_kw(**kw) == dict(R.decoder_kw(**kw), radar_num_heads=8, num_radar_tokens=1500)
    assert R.variant_key(num_heads=4, num_classes=10) != R.variant_key(num_heads=16)
    # the radar side's keys and the FFN's width: all reach configs.head_cfg, two reach the state dict (one under synth's
    # name for it), two reach the oracle by argument (it reads the feature count and the width off the weights)
    face = (-40.0, -30.0, -2.0, 25.0, 35.0, 1.5)
    kw = dict(radar_num_heads=4, radar_num_tokens=64, radar_in_dims=64, radar_point_range=face, feedforward_channels=1024)
    assert R.variant_kw(**kw) == kw
    assert R.state_dict_kw(**kw) == dict(radar_in=64, feedforward_channels=1024)
    assert R.oracle_kw(**kw) == dict(with_box_refine=True, num_heads=8, num_cams=6, radar_num_heads=4, num_radar_tokens=64)
    keys = [R.variant_key(**{k: v}) for k, v in kw.items()] + [R.variant_key(), R.variant_key(**kw)]
    assert len(set(keys)) == len(keys) and R.variant_key(radar_point_range=list(face)) == R.variant_key(radar_point_range=face)
    for fn in (R.variant_kw, R.state_dict_kw, R.decoder_kw, R.oracle_kw, R.variant_key):
        with pytest.raises(AssertionError):
            fn(num_head=4)


def test_depth_and_gate_as_variant_keys():
    default3 = dict(type='three_circle', radii=[(1.0, 2.0), (1.0, 2.0), (0.5, 1.0)])
    assert R.variant_kw(num_fusion_layers=3, radar_gate=None) == {} and R.variant_key(num_fusion_layers=3, radar_gate=None) == ()
    kw = dict(num_fusion_layers=2, radar_gate=R.CIRCLE)
    assert R.variant_kw(**kw) == kw                                  # both reach configs.head_cfg as they are spelled
    assert R.variant_kw(radar_gate=default3) == dict(radar_gate=default3)     # ... the default's explicit spelling too
    assert R.state_dict_kw(**kw) == dict(num_fusion_layers=2)        # the gate reaches no state dict
    assert R.state_dict_kw(radar_gate=R.WIDE3, num_heads=4) == {}
    assert R.decoder_kw(**kw) == dict(with_box_refine=True, num_heads=8, num_cams=6)      # the oracle's decoder reads neither
    keys = [R.variant_key(**v) for v in (dict(), dict(radar_gate=R.CIRCLE), dict(radar_gate=R.WIDE3), dict(num_fusion_layers=2),
                                         dict(num_fusion_layers=1), kw, dict(num_fusion_layers=2, radar_gate=R.WIDE3),
                                         dict(radar_gate=R.CIRCLE, num_heads=4))]
    assert len(set(keys)) == len(keys)                               # two gates, two depths: different heads, different caches
    hash(keys[5])
    # a key holds the gate normalised: two spellings of one gate share a head, a shallower head keeps its own entries
    assert R.variant_key(radar_gate=dict(type='circle', radii=(2, 2.0, 1))) == R.variant_key(radar_gate=R.CIRCLE)
    assert R.variant_key(**kw) == R.variant_key(num_fusion_layers=2, radar_gate=dict(type='circle', radii=[2.0, 2.0]))
    for fn in (R.variant_kw, R.state_dict_kw, R.decoder_kw, R.oracle_kw, R.variant_key):
        with pytest.raises(AssertionError):
            fn(fusion_layers=2)


def test_oracle_cache_is_keyed_by_depth_and_gate():
    """oracle_head(key=) under a gate or a depth does not return what was kept for another"""
    calls = []
    real = R.oracle_forward
    R.oracle_forward = lambda sd, feats, frame, variant, **kw: calls.append(variant) or len(calls)
    try:
        got = [R.oracle_head(None, None, None, key='cache test', **v)
               for v in (dict(), dict(radar_gate=R.CIRCLE), dict(radar_gate=R.WIDE3), dict(num_fusion_layers=2),
                         dict(num_fusion_layers=2, radar_gate=R.CIRCLE), dict(radar_gate=R.CIRCLE), dict())]
    finally:
        R.oracle_forward = real
        for k in [k for k in R._ORACLE if k[0] == 'cache test']:
            del R._ORACLE[k]
    assert got == [1, 2, 3, 4, 5, 2, 1] and len(calls) == 5


@pytest.fixture(scope='module')
def tiny():
    """The tiny maps, 37 queries and 60 radar points: the oracle's inputs and its head_forward with every default."""
    from oracle import transcar_oracle as O
    from transcar_amd import synth
    sd = O.to_torch_sd(synth.make_state_dict(seed=3, num_query=37))
    args = (sd, [torch.from_numpy(f) for f in synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)],
            torch.from_numpy(synth.make_lidar2img()).float()[None], R.HW,
            O.build_radar_features(synth.make_radar_frame(seed=2, n_per_radar=12)), R.PCR)
    with torch.no_grad():
        return O, sd, args, O.head_forward(*args, return_debug=True)


def test_oracle_defaults_are_8_heads_and_10_classes(tiny):
    O, sd, args, (outs, dbg) = tiny
    with torch.no_grad():
        outs8, dbg8 = O.head_forward(*args, return_debug=True, num_heads=8)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(outs[k], outs8[k]), k
    for k in ('hs', 'inter_refs', 'tmp'):
        assert torch.equal(dbg[k], dbg8[k]), k
    from transcar_amd import synth
    boxes, labels = (torch.from_numpy(a) for a in synth.make_gt(seed=7, n=24))
    with torch.no_grad():
        a, ma = O.loss(outs, boxes, labels, sd['code_weights'])
        b, mb = O.loss(outs, boxes, labels, sd['code_weights'], num_classes=10)
    assert set(a) == set(b) and len(a) == 6
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(ma, mb):
        assert torch.equal(x, y)


def test_oracle_head_count_reaches_the_decoder_self_attention(tiny):
    O, sd, args, (_, dbg) = tiny
    feats, l2i, hw = args[1], args[2], args[3]
    with torch.no_grad():
        hs4 = O.transformer(sd, feats, R.PCR, l2i, hw, num_heads=4)[0]
    assert float((hs4.permute(0, 2, 1, 3) - dbg['hs']).abs().max()) > 0.1      # (dbg: the default, 8 heads)


@pytest.mark.parametrize('gate', [None, R.CIRCLE], ids=['three-circle', 'circle'])
def test_oracle_first_fusion_layers_are_the_first_levels(tiny, gate):
    """head_forward(num_fusion_layers=N) is levels [:N] of the three-layer call bit for bit, on the three-layer state
    dict and on the one that holds the first N layers' keys only; on a frame near the predicted boxes (rows with a hit
    in every layer) and on the module's (none)."""
    from num_classes_rig import centres_of
    O, sd, args, (_, dbg0) = tiny
    from transcar_amd import synth
    near = O.build_radar_features(synth.make_radar_frame(seed=2, n_per_radar=12, centres=centres_of(dbg0)))
    trace = (dbg0['hs'].permute(0, 2, 1, 3), dbg0['init_ref'], dbg0['inter_refs'], dbg0['tmp_dec'])
    for f36, hit in ((near, True), (args[4], False)):
        kw = dict(return_debug=True, decoder_trace=trace, radar_gate=gate)
        with torch.no_grad():
            full, dbg = O.head_forward(*args[:4], f36, args[5], **kw)
            assert full['all_cls_scores'].shape[0] == 3 and (min(int((h > 0).sum()) for h in dbg['hit_counts']) > 0) == hit
            for depth in R.DEPTHS:
                own = O.to_torch_sd(synth.make_state_dict(seed=3, num_query=37, num_fusion_layers=depth))
                assert len(own) < len(sd)
                for weights in (sd, own):
                    got, gdbg = O.head_forward(weights, *args[1:4], f36, args[5], num_fusion_layers=depth, **kw)
                    for k in ('all_cls_scores', 'all_bbox_preds'):
                        assert got[k].shape[0] == depth and torch.equal(got[k], full[k][:depth]), (depth, k)
                    assert len(gdbg['hit_counts']) == len(gdbg['hit_rows']) == depth
                    for a, b in zip(gdbg['hit_counts'], dbg['hit_counts']):
                        assert torch.equal(a, b)
