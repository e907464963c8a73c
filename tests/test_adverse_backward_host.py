"""The fp64 reference of the radar stack's BACKWARD on the adverse frames (adverse_rig.py), on the host.

test_gpu_adverse_backward.py holds the HIP backward to `2 x the fp32 reference formula's deviation from fp64 + 1e-4`
per gradient tensor.  That yardstick means something only while the fp32 formula itself is close to fp64, and it is
not on every query row: a ReLU input within fp32 rounding of zero lands on different sides in fp32 and fp64, and the
row's contribution to every query-side weight gradient flips (without exclusions: of the order of 1e-2 of a tensor's
maximum on these frames).  adverse_rig.tie_rows names those rows from the fp64 forward and the tests zero their cotangents.
delta is a CONDITION, not a tolerance: 3 x the largest deviation of the fp32 formula's ReLU inputs from fp64, measured
per frame, for the 15 query-side sites and for the encoder's 5 token-side sites separately (adverse_rig.tie_delta).

Measured on the CPU (re-measured and asserted by the tests; `p` = dropout on every site of the fusion layers, host-drawn
multipliers):

  frame      p    delta query / token   rows excluded, layers 1 / 2 / 3   max |g32 - g64| / max |g64|, 98 tensors
  keep       0    1.31e-05 / 3.88e-05   52 /  67 /  82                    2.5e-06
  keep       0.1  1.68e-05 / 3.88e-05   55 /  72 /  90                    2.1e-06
  mid        0    1.70e-05 / 2.89e-05   57 /  81 / 115                    2.5e-06
  mid        0.1  1.91e-05 / 2.89e-05   69 /  99 / 121                    1.7e-06
  truncated  0    2.61e-05 / 3.03e-05   70 / 109 / 154                    2.4e-06
  truncated  0.1  2.97e-05 / 3.03e-05   83 / 124 / 165                    3.9e-06
  all_hit    0    2.32e-05 / 3.44e-05   99 / 151 / 172                    2.5e-06
  all_hit    0.1  2.15e-05 / 3.44e-05  102 / 122 / 144                    2.4e-06

The largest share of a layer's rows that is excluded: 19.1 % (all_hit, p = 0, layer 3); the cap is 25 %.

Rows with >= 8 hits in fusion layer 1 (adverse_rig._cluster_far_returns; at least 100 are required): 117 (keep), 123 (mid),
119 (truncated), 130 (all_hit)."""
import numpy as np
import pytest
import torch

import adverse_rig as A

P = [0.0, 0.1]
FP32_BOUND = 1e-5       # the fp32 formula against fp64, relative to each tensor's maximum (measured: 3.9e-6)


@pytest.fixture(scope='module')
def rig():
    return A.build()


@pytest.mark.parametrize('frame', list(A.FRAMES))
def test_radar_stack_in_eval_mode_is_the_oracles_head(rig, frame):
    """radar_stack (the fusion layers composed by hand, masks given) reproduces O.head_forward's outputs bit for bit, and
    the launch's T and pad_mult are those of FRAMES."""
    case = A.radar_case(rig, frame)
    with torch.no_grad():
        cls, box = A.radar_stack(rig['sd'], torch.float32, rig, case, A.radar_masks(rig, case))
    want = case['trace'][0]
    assert torch.equal(cls, want['all_cls_scores']) and torch.equal(box, want['all_bbox_preds'])
    T, pad_mult = A.FRAMES[frame][2]
    assert case['tok_np'].shape == (1, T, 36) and case['pad_mult'] == pad_mult


@pytest.mark.parametrize('frame', list(A.FRAMES))
def test_rows_with_many_hits(rig, frame):
    """Per frame at least 100 rows with >= 8 hits in fusion layer 1 (measured: 117 / 123 / 119 / 130)."""
    n = int((A.radar_case(rig, frame)['hits'][0] >= A.MANY_HITS).sum())
    print('%s: %d rows with >= %d hits in fusion layer 1' % (frame, n, A.MANY_HITS))
    assert A.MANY_HITS == 8 and A.MANY_HIT_ROWS == 100 and n >= A.MANY_HIT_ROWS, (frame, n)


@pytest.mark.parametrize('p', P)
@pytest.mark.parametrize('frame', list(A.FRAMES))
def test_fp32_gradients_are_the_fp64_gradients_off_the_tie_rows(rig, frame, p):
    """With the tie rows' cotangents zeroed, torch autograd in fp32 is within 1e-5 of fp64 on each of the 98 trainable
    tensors; no layer loses more than a quarter of its rows; every tensor has a non-zero fp64 gradient."""
    drop = A.host_dropout(p, 900, seed=1) if p else None
    bc = A.backward_case(rig, frame, drop)
    excluded = bc['ties'].sum(1)
    assert (np.diff(excluded) >= 0).all() and excluded.max() <= A.MAX_EXCLUDED * bc['ties'].shape[1], excluded
    d_cls, d_box = A.cotangents(5)
    g32, g64 = A.reference_gradients(rig, bc['case'], drop, d_cls, d_box, ~bc['ties'], bc['masks'])
    assert len(g64) == 98 and sorted(g32) == sorted(g64)
    worst = 0.0
    for k, g in g64.items():
        scale = float(g.abs().max())
        assert scale > 0, k
        worst = max(worst, float((g32[k].double() - g).abs().max()) / scale)
        A.group_of(k)                                   # every tensor belongs to a group of the GPU test's report
    print('%s p=%.1f: delta %.2e / %.2e, rows excluded %s, max|g32 - g64| / max|g64| = %.2e'
          % (frame, p, bc['delta'][0], bc['delta'][1], excluded.tolist(), worst))
    assert worst <= FP32_BOUND, worst
