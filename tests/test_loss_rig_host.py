"""Anchors of tests/loss_rig.py on the CPU, so that test_gpu_loss_kernels.py does not rest on an unchecked reference:
the rig's loss against the reference's own numbers (fixture G7), its cost matrix against the reference's assignment,
its AdamW against torch.optim.AdamW, and for every seeded case the fp32 reference alone inside every condition the GPU
tests state (finite outputs, exact zeros where they demand them)."""
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import loss_rig as R
from transcar_amd import synth

KEYS = [('d0_loss_cls', 'd0_loss_bbox'), ('d1_loss_cls', 'd1_loss_bbox'), ('loss_cls', 'loss_bbox')]
CODE_W = [1.0] * 8 + [0.2] * 2


def _g5_g7(golden_dir, n_gt):
    g5 = np.load(os.path.join(golden_dir, 'g5_head_tiny.npz'))
    cls = torch.from_numpy(g5['all_cls_scores']).double()
    box = torch.from_numpy(g5['all_bbox_preds']).double()
    boxes, labels = synth.make_gt(seed=7, n=24)
    gt = torch.from_numpy(boxes[:n_gt]).double().clone()
    gt[:, 2] += gt[:, 5] * 0.5                                   # gravity centre, HEAD:963-965
    gtn = R.normalize(gt)[None] if n_gt else torch.ones((1, 1, 10), dtype=torch.float64)
    lab = torch.from_numpy(labels[:n_gt])[None] if n_gt else torch.zeros((1, 1), dtype=torch.long)
    return cls, box, gtn, lab


def test_loss_given_assignment_reproduces_reference_losses(golden_dir):
    g7 = np.load(os.path.join(golden_dir, 'g7_loss.npz'))
    cls, box, gtn, lab = _g5_g7(golden_dir, 24)
    assigned = (g7['gt_inds'] - 1)[:, None, :]                   # the reference stores gt index + 1, 0 = unmatched
    out = R.loss_given_assignment(cls, box, gtn, lab, assigned, [[24.0, 24.0]] * 3, CODE_W, 0.25, 2.0, 2.0, 0.25)
    for l in range(3):
        for j in range(2):
            ref = float(g7[KEYS[l][j]])
            assert abs(float(out[l, j]) - ref) <= 1e-5 * max(1, abs(ref)), (KEYS[l][j], float(out[l, j]), ref)


def test_loss_given_assignment_without_ground_truth(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g7_loss_empty.npz'))
    cls, box, gtn, lab = _g5_g7(golden_dir, 0)
    assigned = np.full((3, 1, cls.shape[2]), -1)
    out = R.loss_given_assignment(cls, box, gtn, lab, assigned, [[1.0, 1.0]] * 3, CODE_W, 0.25, 2.0, 2.0, 0.25)
    for l in range(3):
        for j in range(2):
            ref = float(g[KEYS[l][j]])
            assert abs(float(out[l, j]) - ref) <= 1e-5 * max(1, abs(ref)), (KEYS[l][j], float(out[l, j]), ref)
        assert float(out[l, 1]) == 0.0


def test_match_cost_gives_the_reference_assignment(golden_dir):
    g7 = np.load(os.path.join(golden_dir, 'g7_loss.npz'))
    cls, box, gtn, lab = _g5_g7(golden_dir, 24)
    cost = R.match_cost(cls, box, gtn, lab, [24]).numpy()
    for l in range(3):
        rows, cols = linear_sum_assignment(cost[l, 0])
        got = np.zeros(cost.shape[2], dtype=np.int64)
        got[rows] = cols + 1
        assert np.array_equal(got, g7['gt_inds'][l]), l


@pytest.mark.parametrize('max_norm', [35.0, 0.0])
def test_adamw_reference_follows_torch(max_norm):
    rng = np.random.RandomState(1)
    n = 20011
    p0 = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    grads = [(rng.standard_normal(n) * s / 0.5).astype(np.float32) for s in R.ADAM_GRAD_SCALES]
    kw = dict(lr=R.f32(2e-4), b1=R.f32(0.9), b2=R.f32(0.999), eps=R.f32(1e-8), wd=R.f32(0.01), grad_scale=0.5,
              max_norm=max_norm)
    mine = R.adamw_reference(p0, grads, dtype=np.float32, **kw)
    theirs = R.adamw_torch32(p0, grads, **kw)
    norms = [float(np.linalg.norm(g.astype(np.float64) * 0.5)) for g in grads]
    assert sum(x > 35.0 for x in norms) >= 2 and sum(x < 35.0 for x in norms) >= 2        # clipped and unclipped steps
    for (p, m, v), (pt, mt, vt) in zip(mine, theirs):
        assert p.dtype == np.float32
        # "within 2 ulp of p" is read as 2 ulp of p at the TENSOR's scale, spacing(max|p|), not of each element: an element
        # that an update of lr carries across zero has an ulp of its own far below the rounding of that update (measured:
        # up to 1.8e4 of its own ulps)
        assert np.abs(p.astype(np.float64) - pt).max() <= 2 * np.spacing(np.abs(pt).max())
        # (torch forms m by lerp_, v by addcmul_: a rounding or two apart per step)
        assert np.abs(m - mt).max() <= 8 * 2.0 ** -24 * np.abs(mt).max()
        assert np.abs(v - vt).max() <= 8 * 2.0 ** -24 * np.abs(vt).max()
    # fp64 and fp32 tell the same story
    for (p, m, v), (pt, mt, vt) in zip(R.adamw_reference(p0, grads, dtype=np.float64, **kw), theirs):
        assert np.abs(p - pt).max() <= 1e-5 * 2e-4 * 6 and np.abs(m - mt).max() <= 1e-5 * np.abs(m).max()


def test_adamw_torch32_starts_late_with_zero_moments():
    c = R.make_case('adam-late-n257-gs1-mn0')
    a, b = R.adamw_torch32(c['p0'], c['grads'], **R.adam_args(c)), R.adamw_reference(c['p0'], c['grads'], **R.adam_args(c))
    for (p, m, v), (p64, m64, v64) in zip(a, b):
        assert np.abs(p - p64).max() <= 1e-5 * 2e-4 * 6 and np.abs(m - m64).max() <= 1e-5 * np.abs(m64).max()
        assert np.abs(v - v64).max() <= 1e-5 * np.abs(v64).max()


@pytest.mark.parametrize('name', R.COST_CASES)
def test_cost_cases_fp32_reference_is_finite(name):
    c = R.make_case(name)
    t = lambda k: torch.from_numpy(c[k])
    cost = R.match_cost(t('cls'), t('box'), t('gtn'), t('labels'), c['counts'], c['w_cls'], c['w_box'], c['alpha'],
                        c['gamma'], c['eps']).numpy()
    assert cost.dtype == np.float32 and np.isfinite(cost).all()
    for b, n in enumerate(c['counts']):
        assert (cost[:, b, :, n:] == 0).all()
    assert 0 in c['labels'][0, :c['counts'][0]] and c['ncls'] - 1 in c['labels'][0, :c['counts'][0]]
    x = np.abs(c['cls'])
    assert (x >= 90).any() and (x == 0).any() and ((x >= 8) & (x < 14)).any()


@pytest.mark.parametrize('name', R.LOSS_CASES + R.NONFINITE_CASES)
def test_loss_cases_fp32_reference_is_finite_with_exact_zeros(name):
    c = R.make_case(name)
    avg = [[7.5, 3.25], [1.0, 33.0], [12.75, 1.0]]
    for dtype in (torch.float32, torch.float64):
        out, d_cls, d_box = R.loss_and_gradients(c, avg, dtype)
        assert np.isfinite(out).all() and np.isfinite(d_cls).all() and np.isfinite(d_box).all()
        assert (d_box[..., 10:] == 0).all() and (d_box[c['assigned'] < 0] == 0).all()
        for l, b, q, j in c['planted_equal']:
            assert d_box[l, b, q, j] == 0
        for l, b, q in c['nonfinite_rows']:
            assert (d_box[l, b, q] == 0).all()
    a = c['assigned']
    assert (a[:, c['counts'] == 0] == -1).all() and c['counts'][1] > 0 and (a[1, 1] == -1).all()
    assert (a[0, 0] >= 0).sum() == 24
    for l in range(R.LYR):
        for b in range(c['B']):                                  # a partial matching: no box twice, inside the count
            m = a[l, b][a[l, b] >= 0]
            assert len(np.unique(m)) == len(m) and (m < c['counts'][b]).all()
    if c['nonfinite_rows']:
        clean, _, _ = R.loss_and_gradients(c['clean'], avg, torch.float64)
        assert (out[:, 1] < clean[:, 1]).all() and np.array_equal(out[:, 0], clean[:, 0])
        assert len(c['nonfinite_rows']) == 2 * R.LYR


@pytest.mark.parametrize('name', R.NORMALIZE_CASES)
def test_normalize_cases_are_finite(name):
    c = R.make_case(name)
    out = R.normalize(torch.from_numpy(c['gt9'])).numpy()
    assert out.shape == (c['n'], 10) and np.isfinite(out).all()
    assert c['gt9'][:, 3:6].min() >= np.float32(0.05) and c['gt9'][:, 3:6].max() <= np.float32(30.0)
    assert np.abs(c['gt9'][:, 6]).max() <= 4 * np.pi
    if c['n'] >= 127:
        assert {0.0, float(np.float32(np.pi / 2)), -float(np.float32(np.pi / 2))} <= set(c['gt9'][:, 6].tolist())


@pytest.mark.parametrize('name', R.SQNORM_CASES)
def test_sqnorm_cases_fp32_sum_is_finite_and_in_range(name):
    c = R.make_case(name)
    g = np.abs(c['g'])
    assert len(g) == c['n'] and g.min() >= np.float32(1e-4) and g.max() <= np.float32(1e3)
    sq = c['g'] * c['g']                                          # every term a normal fp32 number: a relative bound holds
    assert sq.dtype == np.float32 and sq.min() >= np.finfo(np.float32).tiny
    total32, total64 = float(np.sum(sq, dtype=np.float32)), float(np.sum(c['g'].astype(np.float64) ** 2))
    assert np.isfinite(total32) and abs(total32 - total64) <= 37 * 2.0 ** -24 * total64


@pytest.mark.parametrize('name', R.ADAM_CASES)
def test_adam_cases_fp32_reference_is_finite(name):
    c = R.make_case(name)
    assert len(c['grads']) == 6 and not c['grads'][3].any() and c['p0'].shape == (c['n'],)
    for p, m, v in R.adamw_torch32(c['p0'], c['grads'], **R.adam_args(c)):
        assert p.dtype == np.float32 and np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
        assert (v >= 0).all()


def test_adam_case_alternates_clipped_and_unclipped_steps():
    c = R.make_case('adam-small-n100003-gs0.5-mn35')
    norms = [float(np.linalg.norm(g.astype(np.float64) * 0.5)) for g in c['grads']]
    assert [x > 35.0 for x in norms] == [True, False, True, False, False, True] and norms[3] == 0.0
