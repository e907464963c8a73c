"""Detr3DHead(radar_gate=...) on the MI355X: the single circle's inclusive edge at the smallest shape that has it, the
threshold self-check over the accepted radius range, the circle gate and a three-circle gate with other radii end to end
against the CPU oracle under the same gate (head_forward(radar_gate=)) on every chain path -- the circle also against the
reference's single-circle head (tests/golden/make_golden_radar_gate.py) --, the identities (default spellings, row
orders, nine-frame launch, plugin graph, shallower heads), and a training iteration against the reference's gradients and
the oracle's autograd under the same gate.  Tiny level shapes, 900 queries, G5's radar centres.  pytest -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from transcar_amd import _lib as L

pytestmark = pytest.mark.gpu

#: (tile rows, matrix path) of the chains, and the operator-by-operator path
PATHS = [(4, 'f32'), (4, 'f16x2'), (8, 'f32'), (8, 'f16x2'), (16, 'f32'), (16, 'f16x2'), (32, 'f16x2'), (0, 'unfused')]
KEYS = ('all_cls_scores', 'all_bbox_preds')
GATES = {'circle': R.CIRCLE, 'wide3': R.WIDE3}


def shared_head(T, name, depth=3):
    return R.shared_head(T, radar_gate=GATES[name], num_fusion_layers=depth)[0]


def frame_of(name):
    """the circle on the frame of the reference's single-circle fixture, the others on G5's"""
    return R.g5_frame(int(R.gold(R.G5_CIRCLE)['radar_seed'])) if name == 'circle' else R.g5_frame()


def oracle(T, name):
    return R.oracle_head(R.shared_head(T)[1], *frame_of(name), key='gate frame ' + name, radar_gate=GATES[name])


def run(head, rows, matrix, name=None, **extra):
    feats, frame = frame_of(name)
    if matrix == 'unfused':
        return R.run_head(head, feats, frame, unfused=True, **extra)
    return R.run_head(head, feats, frame, tile_rows=rows, matrix_path=matrix, **extra)


# ---- 1. the edge ---------------------------------------------------------------------------------------------------------
def _edge_inputs():
    B, Q, Tn, C = 1, 8, 64, 256
    g = torch.Generator().manual_seed(11)
    qp = torch.randn((B, Q, C), generator=g) * 0.3
    kv = torch.randn((B, Tn, 2 * C), generator=g) * 0.3
    cxy = torch.full((B, Q, 2), 50.0)
    cxy[0, :4] = 0.0                                     # four queries gate at (0, 0), four far from every token
    box = torch.zeros((B, Q, 10))
    box[..., 3] = float(np.log(1e-3))                    # length 1 mm; sin = cos = 0: front and rear ON the centre
    tok = torch.zeros((B, Tn, 2))
    tok[0, :, 0] = -40.0
    tok[0, :, 1] = 35.0
    up = float(np.nextafter(np.float32(2.0), np.float32(np.inf)))
    tok[0, 5] = torch.tensor([2.0, 0.0])                 # |y|^2 = 4 exactly: dist == 2.0 in the _euclidean_dist form
    tok[0, 17] = torch.tensor([0.0, -2.0])
    tok[0, 40] = torch.tensor([up, 0.0])                 # the next float beyond the edge
    return qp, kv, cxy, box, tok


def test_the_circles_edge_is_inside_and_the_three_circles_is_not(T):
    from transcar_amd import autograd_ops as A
    qp, kv, cxy, box, tok = _edge_inputs()
    d = torch.cdist(cxy[:, :1], tok, p=2.0)[0, 0]
    assert float(d[5]) == 2.0 and float(d[17]) == 2.0 and float(d[40]) > 2.0          # the reference's own distances
    args = [gpu(t) for t in (cxy,)]
    with torch.enable_grad():
        qg, kg = gpu(qp).requires_grad_(True), gpu(kv).requires_grad_(True)
        out, hits = A.radar_attn_core(qg, kg, args[0], 2, gpu(box), gpu(tok), 1, L.TC_RADAR_GATE_CIRCLE, 2.0)
        out.sum().backward()
    torch.cuda.synchronize()
    assert hits.cpu().tolist() == [[2, 2, 2, 2, 0, 0, 0, 0]]
    # the backward re-evaluates the gate in its literal form: gradients reach the two edge tokens and no other
    touched = (kg.grad[0].abs().sum(1) > 0).cpu().nonzero().flatten().tolist()
    assert touched == [5, 17], touched
    assert float(out[0, 4:].abs().max()) == 0.0 and float(out[0, :4].abs().max()) > 0.0
    # the softmax over exactly those two tokens
    q, k, v = qp[0, :4].double(), kv[0, [5, 17], :256].double(), kv[0, [5, 17], 256:].double()
    s = torch.einsum('qhd,thd->hqt', q.view(4, 8, 32), k.view(2, 8, 32)) / 32 ** 0.5
    want = torch.einsum('hqt,thd->qhd', s.softmax(-1), v.view(2, 8, 32)).reshape(4, 256)
    np.testing.assert_allclose(out[0, :4].detach().cpu().numpy(), want.numpy(), atol=1e-5, rtol=0)
    # just inside and just outside the radius
    for rad, n in ((float(np.nextafter(np.float32(2.0), np.float32(0.0))), 0), (float(d[40]), 3)):
        _, h2 = A.radar_attn_core(gpu(qp), gpu(kv), args[0], 2, gpu(box), gpu(tok), 1, L.TC_RADAR_GATE_CIRCLE, rad)
        assert h2.cpu().tolist() == [[n] * 4 + [0] * 4], rad
    # three circles of radius clamp(., 2, 2) = 2 compare dist < 2: none of the three tokens
    _, h3 = A.radar_attn_core(gpu(qp), gpu(kv), args[0], 2, gpu(box), gpu(tok), 1, 2.0, 2.0)
    assert h3.cpu().tolist() == [[0] * 8]


@pytest.mark.parametrize('inclusive', [0, 1], ids=['less-than', 'not-greater'])
def test_threshold_selfcheck_over_the_accepted_range(T, inclusive):
    lib = L.lib()
    bad = torch.zeros(1, dtype=torch.int64, device=R.dev())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for lo, hi, n in ((L.TC_RADAR_RADIUS_MIN, L.TC_RADAR_RADIUS_MAX, 4096), (0.125, 0.125, 2), (16.0, 16.0, 2), (0.5, 2.0, 512)):
        L.check(lib.tc_radar_gate_selfcheck_range(n, 20261020 + inclusive, lo, hi, inclusive, bad.data_ptr(), s),
                'tc_radar_gate_selfcheck_range')
        torch.cuda.synchronize()
        assert int(bad.item()) == 0, (lo, hi)


# ---- 2. end to end against the oracle under the same gate ------------------------------------------------------------------
@pytest.mark.parametrize('rows,matrix', PATHS)
@pytest.mark.parametrize('name', sorted(GATES))
def test_end_to_end_against_the_oracle(T, name, rows, matrix):
    want, dbg = oracle(T, name)
    rows_hit = [int((h > 0).sum()) for h in dbg['hit_counts']]
    assert min(rows_hit) > 32, rows_hit
    outs = run(shared_head(T, name), rows, matrix, name)
    if name == 'circle':                             # ... and the reference's backup head on the same frame
        R.check_against_fixture(outs, want, dbg, R.gold(R.G5_CIRCLE))
    want_hits = np.stack([h.numpy() for h in dbg['hit_counts']])
    differ = int((~np.all(outs['aux']['radar_hit_counts'][:, 0].cpu().numpy() == want_hits, axis=0)).sum())
    print('%s %s/%s: hit rows %s, %d rows differ in a hit count' % (name, rows, matrix, rows_hit, differ))
    R.check_against_oracle(outs, want, dbg)          # E2E_TOL, REFS_TOL; at most MAX_GATE_ROWS rows differ in a hit count


# ---- 3. identities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2'), (0, 'unfused')])
def test_default_spellings_are_one_head(T, rows, matrix):
    base = run(R.shared_head(T)[0], rows, matrix)
    for gate in (None, dict(type='three_circle'), dict(type='three_circle', radii=[(1.0, 2.0), (1.0, 2.0), (0.5, 1.0)])):
        got = run(R.make_head(T, radar_gate=gate)[0], rows, matrix)
        for k in KEYS:
            assert torch.equal(got[k], base[k]), (gate, k)
        assert torch.equal(got['aux']['radar_hit_counts'], base['aux']['radar_hit_counts'])


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2')])
def test_row_orders_agree_with_the_circle(T, rows, matrix):
    h = shared_head(T, 'circle')
    a, b = run(h, rows, matrix, radar_compact=False), run(h, rows, matrix, radar_compact=True)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a['aux']['radar_hit_counts'], b['aux']['radar_hit_counts'])


def test_circle_frame_of_nine_and_plugin_graph(T):
    R.check_frame_of_nine(shared_head(T, 'circle'))
    R.check_plugin_graph_replay(R.make_head(T, radar_gate=R.CIRCLE)[0], R.make_head(T, radar_gate=R.CIRCLE)[0])


@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (16, 'f16x2'), (32, 'f16x2'), (0, 'unfused')])
@pytest.mark.parametrize('depth', R.DEPTHS)
def test_shallower_circle_heads_are_the_first_levels(T, depth, rows, matrix):
    full, got = run(shared_head(T, 'circle'), rows, matrix), run(shared_head(T, 'circle', depth), rows, matrix)
    for k in KEYS:
        assert got[k].shape[0] == depth and torch.equal(got[k], full[k][:depth]), k
    assert torch.equal(got['aux']['radar_hit_counts'], full['aux']['radar_hit_counts'][:depth])


# ---- 4. training -----------------------------------------------------------------------------------------------------------
def test_training_iteration_against_the_reference_and_the_oracle(T):
    """One iteration's losses and gradients on the chain backward, the deterministic one (twice: bit-identical) and the
    per-operator backward, against the reference's backup head (g8_train_grads_gate_circle.npz) and against the oracle's
    autograd under the same gate, 2e-3 as test_gpu_training holds G8."""
    g8_ref = R.gold(R.G8_CIRCLE)
    frame = R.g8_frame('g5_head_tiny.npz', radar_seed=int(g8_ref['radar_seed']))
    _, oracle_losses, _, oracle_grads = R.oracle_training(frame, radar_gate=R.CIRCLE)
    total, g8 = sum(oracle_losses.values()), R.GradStats(oracle_grads)
    assert abs(total - float(g8_ref['total_loss'])) < 1e-4 * float(g8_ref['total_loss'])
    runs = {}
    for what, kw in (('chain', dict(chain_forward=True, chain_backward=True)),
                     ('deterministic', dict(chain_forward=True, chain_backward=True, deterministic=True)),
                     ('deterministic again', dict(chain_forward=True, chain_backward=True, deterministic=True)),
                     ('operators', dict(chain_forward=False, chain_backward=False))):
        losses, grads = R.trainer_iteration(frame, radar_gate=R.CIRCLE, **kw)
        loss = sum(losses.values())
        print('%s: total loss %.6f (oracle %.6f, reference %.6f)' % (what, loss, total, float(g8_ref['total_loss'])))
        assert abs(loss - total) < 2e-3 * max(1.0, abs(total)), (what, loss, total)
        for k, v in losses.items():
            ref = float(g8_ref['loss__' + k.replace('.', '_')])
            assert abs(v - ref) < 2e-3 * max(1.0, abs(ref)), (what, k, v, ref)
        assert R.check_grads_against_g8(grads, g8_ref, 2e-3, what + ' vs reference') == 98
        assert R.check_grads_against_g8(grads, g8, 2e-3, what + ' vs oracle') == 98
        runs[what] = grads
    for k, g in runs['deterministic'].items():
        if g is not None:
            assert torch.equal(g, runs['deterministic again'][k]), k
