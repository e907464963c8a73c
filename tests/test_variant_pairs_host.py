"""variant_pairs_rig.py on the CPU: the two tables cover every admissible pair of their axes within their caps and are what
the committed generator gives; configs.head_cfg builds every row; every stored radar frame is the one the rig makes, with the
margin it states, at least radar_input_rig.MIN_MARGIN from every gate decision, and has the content its row needs
(truncation at 64 tokens, rows on both sides of a moved face, queries with and without a hit, cameras from index 8 up);
the fp32 oracle and its fp64 evaluation take the same gate decisions on every row (the hit-count cap of the GPU test is
then the kernels' alone); the training frames' ReLU ties are within radar_heads_rig.TIE_BOUND; and the oracle tells the keys
apart that leave the state dict's shapes alone, by more than ten times the tolerance the GPU test applies.

The oracle's results are kept per row in variant_pairs_rig's caches: the module evaluates each row once.  pytest -s prints the
coverage counts, the margins and the sensitivity ratios (recorded in DESIGN.md)."""
import itertools

import numpy as np
import pytest

import head_variant_rig as R
import num_cams_rig as NR
import radar_heads_rig as RR
import radar_input_rig as RI
import variant_pairs_rig as VP
from transcar_amd import configs

TABLES = {'inference': (VP.INFERENCE_AXES, VP.cam_logits_ok, VP.INFERENCE_ROWS, VP.MAX_INFERENCE_ROWS, VP.INFERENCE_SEED, VP.INFERENCE_FRAMES),
          'training': (VP.TRAINING_AXES, VP.unconstrained, VP.TRAINING_ROWS, VP.MAX_TRAINING_ROWS, VP.TRAINING_SEED, VP.TRAINING_FRAMES)}
ALL_ROWS = VP.INFERENCE_ROWS + VP.TRAINING_ROWS
IDS = ['%s%02d-%s' % ('i' if i < len(VP.INFERENCE_ROWS) else 't', i if i < len(VP.INFERENCE_ROWS) else i - len(VP.INFERENCE_ROWS),
                      VP.row_id(r)) for i, r in enumerate(ALL_ROWS)]


# ---- 1. the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table', sorted(TABLES))
def test_rows_cover_every_admissible_pair(table):
    axes, ok, rows, cap, seed, frames = TABLES[table]
    names = list(axes)
    want = VP.admissible_pairs(axes, ok)
    every = {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va in axes[a] for vb in axes[b]}
    got = set()
    for row in rows:
        assert list(row) == names and all(row[a] in axes[a] for a in names), row
        if table == 'inference':
            assert VP.cam_logits_ok(row['num_cams'], row['num_levels'], row['num_points']), row
        got |= VP.covered(row, names)
    print('%s: %d rows (cap %d) cover %d admissible pairs of %d; not admissible: %s' % (
        table, len(rows), cap, len(want), len(every), sorted(every - want)))
    assert got == want and len(rows) <= cap and len(frames) == len(rows)
    if table == 'inference':
        assert len(rows) >= 24                              # 6 paths x 4 values
        # the constraint excludes 16 x 4 x 5 only: each of its pairs stands in an admissible row, none is lost
        assert not VP.cam_logits_ok(16, 4, 5) and every == want
    else:
        assert every == want
        used = {row['decoder'] for row in rows}
        assert used == set(VP.DECODERS) and any(VP.DECODERS[d]['num_cams'] > 8 for d in used)
        assert all(any(v != VP.DEFAULTS[k] for k, v in d.items()) for d in VP.DECODERS.values())


@pytest.mark.parametrize('table', sorted(TABLES))
def test_generator_gives_the_committed_rows(table):
    axes, ok, rows, cap, seed, _ = TABLES[table]
    assert VP.generate(axes, ok, seed=seed) == rows


@pytest.mark.parametrize('row', ALL_ROWS, ids=IDS)
def test_head_cfg_builds_every_row(row):
    cfg, full = configs.head_cfg(**R.variant_kw(**VP.variant(row))), VP.full(row)
    layers = cfg['transformer']['decoder']['transformerlayers']['attn_cfgs']
    assert cfg['num_query'] == full['num_query'] and cfg['num_classes'] == cfg['bbox_coder']['num_classes'] == full['num_classes']
    assert layers[0]['num_heads'] == full['num_heads'] and layers[1].get('num_cams', 6) == full['num_cams']
    assert (layers[1].get('num_levels', 4), layers[1]['num_points']) == (full['num_levels'], full['num_points'])
    assert cfg['with_box_refine'] == full['with_box_refine'] and cfg.get('num_fusion_layers', 3) == full['num_fusion_layers']
    assert cfg.get('radar_num_heads', 8) == full['radar_num_heads'] and cfg.get('radar_num_tokens', 1500) == full['radar_num_tokens']
    assert cfg.get('radar_in_dims', 36) == full['radar_in_dims']
    assert (cfg.get('radar_point_range') is None) == (full['radar_point_range'] == 'default')
    assert (cfg.get('radar_gate') is None) == (full['radar_gate'] == 'default')
    assert tuple(cfg['bbox_coder']['pc_range']) == VP.ring(row).pc_range
    sd = R.state_dict(**VP.variant(row))
    assert sd['query_embedding.weight'].shape[0] == full['num_query'] and sd['radar_feat_encoder.0.weight'].shape == (64, full['radar_in_dims'])
    assert sd['transformer.decoder.layers.0.attentions.1.attention_weights.weight'].shape[0] == \
        full['num_cams'] * full['num_levels'] * full['num_points']
    assert ('rf_linear1_3.weight' in sd) == (full['num_fusion_layers'] == 3) and sd['final_cls.6.weight'].shape[0] == full['num_classes']


# ---- 2. the frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ALL_ROWS, ids=IDS)
def test_frames_keep_their_gate_decisions_off_the_edge_and_have_the_rows_content(row):
    full = VP.full(row)
    frames = VP.TRAINING_FRAMES[VP.TRAINING_ROWS.index(row)] if 'decoder' in row else VP.INFERENCE_FRAMES[VP.INFERENCE_ROWS.index(row)]
    assert len(frames) == full['samples']
    for b, (seed, margin) in enumerate(frames):
        assert seed in VP.SEED_RANGE
        o = VP.oracle_row(row, b)
        hits = [int((h > 0).sum()) for h in o['dbg']['hit_counts']]
        print('%s sample %d: seed %d, closest gate decision %.3e m from its radius; %d rows, %d kept; queries with a hit %s of %d' % (
            VP.row_id(row), b, seed, o['margin'], len(o['rows']), len(o['kept']), hits, full['num_query']))
        assert abs(o['margin'] - margin) <= 1e-3 * margin and o['margin'] >= RI.MIN_MARGIN, (o['margin'], margin)      # (four digits are stored)
        assert abs(VP.gate_margin(row, b, seed) - o['margin']) == 0.0
        assert 0 < hits[0] < full['num_query']
        assert len(o['masks']) == full['num_fusion_layers'] and o['masks'][0].shape == (full['num_query'], full['radar_num_tokens'])
        if full['radar_num_tokens'] == 64:
            assert len(o['kept']) > 64                                               # truncation
        if full['radar_num_tokens'] == 2048 and full['radar_point_range'] == 'default':
            assert len(o['kept']) > 1500                                             # tokens beyond the reference's count
        if full['radar_point_range'] == 'face':
            dropped = o['rows'][~RI.in_range(o['rows'], VP.FACE_RANGE)]
            assert RI.in_range(dropped, RI.POINT_RANGE).all() and 0 < len(dropped) < len(o['rows']) and len(o['kept']) > 0
            d = np.sqrt(((dropped[:, None, :2].astype(np.float64) - VP.gate_centres(row, b)[None]) ** 2).sum(-1)).min(1)
            assert int((d < 0.5).sum()) >= 5            # dropped rows inside a gate of layer 1 (every radius >= 0.5 m): they would hit
        else:
            assert len(o['kept']) == len(o['rows'])
        if full['num_cams'] > 8:
            NR.assert_coverage(full['num_cams'], o['dbg'], NR.JITTER if b else None, VP.GEOMS[full['geometry']], VP.LEAST[full['num_cams']])


SEARCHED = [0, 10, 23, len(VP.INFERENCE_ROWS) + 0, len(VP.INFERENCE_ROWS) + 3, len(VP.INFERENCE_ROWS) + 16]


@pytest.mark.parametrize('row', [ALL_ROWS[i] for i in SEARCHED], ids=[IDS[i] for i in SEARCHED])
def test_stored_seeds_are_the_searchs_choice(row):
    """variant_pairs_rig.search_seed repeated on some rows -- one of two samples, and training row 03, the one whose seed
    spares no tie -- gives the stored (seed, margin)."""
    stored = VP.TRAINING_FRAMES[VP.TRAINING_ROWS.index(row)] if 'decoder' in row else VP.INFERENCE_FRAMES[VP.INFERENCE_ROWS.index(row)]
    for b, (seed, margin) in enumerate(stored):
        got_seed, got = VP.search_seed(row, b)
        assert got_seed == seed and abs(got - margin) <= 1e-3 * margin, (b, got_seed, got, seed, margin)


# ---- 3. the reference alone stays within the hit-count cap: at 0 rows -------------------------------------------------------------------
@pytest.mark.parametrize('row', ALL_ROWS, ids=IDS)
def test_fp32_and_fp64_oracle_take_the_same_gate_decisions(row):
    for b in range(VP.full(row)['samples']):
        o, o64 = VP.oracle_row(row, b), VP.oracle_fp64(row, b)
        differ = sum(int((h != h64).sum()) for h, h64 in zip(o['dbg']['hit_counts'], o64['hit_counts']))
        print('%s sample %d: gate decisions that differ between the fp32 and the fp64 oracle: %d; fp32 oracle vs fp64: states %.2e, outputs %.2e' % (
            VP.row_id(row), b, differ, o64['hs_dev'].max(), o64['out_dev'].max()))
        assert len(o64['hit_counts']) == VP.full(row)['num_fusion_layers'] and differ == 0


# ---- 4. the training frames' ReLU ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', VP.TRAINING_ROWS, ids=IDS[len(VP.INFERENCE_ROWS):])
def test_training_frames_relu_ties(row):
    """Without dropout (the masks are read back from the device): with at most MAX_TIED ties set apart, all the others at
    once move the gradient figures by less than TIE_BOUND; the oracle gives the expected number of gradients."""
    apart, rest = VP.influential_ties(row)
    print('%s: ties taken on either side %s; the others at once move the figures by %.2e' % (VP.row_id(row), apart, rest))
    assert len(apart) <= VP.MAX_TIED and rest < RR.TIE_BOUND
    grads = VP.oracle_training(row)[1]
    assert sum(g is not None and float(g.abs().max()) > 0 for g in grads.values()) == VP.expected_gradients(row)


# ---- 5. the oracle tells the keys apart -----------------------------------------------------------------------------------------------------
SENSITIVE = ('num_heads', 'radar_num_heads', 'radar_gate', 'radar_num_tokens', 'radar_point_range', 'geometry', 'with_box_refine')


@pytest.mark.parametrize('key', SENSITIVE)
def test_the_oracle_tells_the_key_apart(key):
    """For each key that leaves the state dict's shapes alone: on the rows that set it (radar_num_tokens: that truncate),
    the oracle with that one key put back to its default -- what a kernel that ignored the key would compute -- differs from
    the row's by more than 10 x E2E_TOL, the tolerance the GPU test applies to scores and boxes; at least one row must."""
    rows = [r for r in VP.INFERENCE_ROWS if r[key] != VP.DEFAULTS[key] and (key != 'radar_num_tokens' or r[key] == 64)]
    ratios = []
    for row in rows[:3]:
        o, other = VP.oracle_row(row), VP.oracle_with(row, **{key: VP.DEFAULTS[key]})
        ratios.append(max(float((o['want'][k] - other[k]).abs().max()) for k in ('all_cls_scores', 'all_bbox_preds')) / R.E2E_TOL)
    print('%s back to %r: the oracle\'s outputs move by %s x E2E_TOL' % (key, VP.DEFAULTS[key], ['%.0f' % r for r in ratios]))
    assert len(ratios) == 3 and max(ratios) > 10
