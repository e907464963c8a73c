"""The decoder self-attention with 4 and 16 heads (head dimension 64 and 16; the configs: 8 heads of 32) on the MI355X:
both attention cores against float64, the entry points that take the head dimension, the operator, and the whole head
on its chain paths against the CPU oracle at num_heads=H and the reference's fixtures (tests/golden/make_golden_variants.py
`heads`); train mode, a training iteration, and the bit-identity checks.  The shared checks are head_variant_rig.py's,
called with num_heads=H.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import head_variant_rig as R
from head_variant_rig import SMOOTH, TINY, T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from transcar_amd import synth

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


# ---- 1. the cores against softmax(S) V in float64 ------------------------------------------------------------------------
def _score_case(case, B, Q, H, seed=7):
    """test_gpu_parity.test_sdpa_lazy_recentring_extreme_scores' operands at head dimension D = 256 / H: one channel
    per head carries a key-dependent offset, q[..., 0] = 1 and k[..., 0] = f(key) * sqrt(D / 32) -- the scores in nats,
    q k^T / sqrt(D), are then those of that test."""
    rng = np.random.RandomState(seed)
    D = 256 // H
    C = H * D
    q = rng.standard_normal((B, Q, C)).astype(np.float32)
    k = rng.standard_normal((B, Q, C)).astype(np.float32)
    v = rng.standard_normal((B, Q, C)).astype(np.float32)
    f = {'ramp_up': np.linspace(-150.0, 150.0, Q), 'ramp_down': np.linspace(150.0, -150.0, Q),
         'huge_negative_start': np.where(np.arange(Q) < 16, -400.0, rng.uniform(-3, 3, Q)),
         'spikes': np.where(rng.uniform(size=Q) < 0.01, 120.0, 0.0),
         'short_ragged': np.linspace(-40.0, 40.0, Q)}[case].astype(np.float32)
    for h in range(H):
        q[:, :, h * D] = 1.0
        k[:, :, h * D] = f[None, :] * np.float32(np.sqrt(D / 32.0))
    return q, k, v


def _sdpa_both(q, k, v, H, matrix):
    """(the library's result, softmax(q k^T / sqrt(D)) v in float64), both [B, Q, C] double on the CPU"""
    from transcar_amd import ops
    B, Q, C = q.shape
    D = C // H
    # the kernel's q is pre-scaled by log2(e) / sqrt(D) and its softmax is 2^x
    qs = torch.from_numpy(q) * (LOG2E / np.sqrt(D))
    qpad = ((Q + 15) // 16) * 16
    vt = torch.zeros((B, C, qpad), dtype=torch.float32)
    vt[:, :, :Q] = torch.from_numpy(v).permute(0, 2, 1)
    got = ops.sdpa(gpu(qs), gpu(k), gpu(vt), num_heads=H, matrix_path=matrix, head_dim=D).cpu().double()
    qd, kd, vd = (torch.from_numpy(a).double().view(B, Q, H, D).permute(0, 2, 1, 3) for a in (q, k, v))
    p = torch.softmax(qd @ kd.transpose(-1, -2) / np.sqrt(D), -1)
    return got, (p @ vd).permute(0, 2, 1, 3).reshape(B, Q, C)


def _check_sdpa(q, k, v, H, matrix, what):
    got, want = _sdpa_both(q, k, v, H, matrix)
    assert torch.isfinite(got).all()
    d = (got - want).abs()
    print('%s: max |library - float64| = %.3e, worst excess over 2e-5 + 1e-4 |want| = %.3e'
          % (what, float(d.max()), float((d - (2e-5 + 1e-4 * want.abs())).max())))
    np.testing.assert_allclose(got.numpy(), want.numpy(), atol=2e-5, rtol=1e-4)


@pytest.mark.parametrize('matrix', ['f32', 'f16x2'])
@pytest.mark.parametrize('case', ['ramp_up', 'ramp_down', 'huge_negative_start', 'spikes', 'short_ragged'])
@pytest.mark.parametrize('H', R.HEADS)
def test_sdpa_heads_extreme_scores(T, H, case, matrix):
    """Both cores at head dimension 64 and 16 on the score sequences that stress the lazy re-centring.  (B, Q) =
    (2, 300): two whole 128-query groups of the staged core plus a ragged one, nine key pairs plus a ragged one (and 18
    whole 16-key tiles plus a ragged one for the fp32 core's eight waves); short_ragged: 37 queries, several waves
    without a tile.  The tolerance is the 8-head test's."""
    Q = 37 if case == 'short_ragged' else 300
    q, k, v = _score_case(case, 2, Q, H)
    _check_sdpa(q, k, v, H, matrix, '%s H=%d %s' % (case, H, matrix))


@pytest.mark.parametrize('B', [1, 3])
def test_sdpa_staged_core_plain_block_mapping(T, B):
    """B * H = 4 and 12 take the staged core's plain (batch * head, query group) mapping; the (2, 300, 4) cases above,
    B * H = 8, the one that keeps a (batch, head) on one XCD."""
    q, k, v = _score_case('spikes', B, 300, 4, seed=11 + B)
    _check_sdpa(q, k, v, 4, 'f16x2', 'spikes B=%d H=4 f16x2' % B)


# ---- 2. the entry points with an explicit head dimension, at 32 -----------------------------------------------------------
@pytest.mark.parametrize('matrix', ['f32', 'f16x2'])
def test_sdpa_head_dim_32_is_the_8_head_entry_point(T, matrix):
    from transcar_amd import ops
    q, k, v = _score_case('spikes', 2, 300, 8)
    qs = gpu(torch.from_numpy(q) * (LOG2E / np.sqrt(32.0)))
    vt = torch.zeros((2, 256, 304), dtype=torch.float32)
    vt[:, :, :300] = torch.from_numpy(v).permute(0, 2, 1)
    old = ops.sdpa(qs, gpu(k), gpu(vt), num_heads=8, matrix_path=matrix)
    new = ops.sdpa(qs, gpu(k), gpu(vt), num_heads=8, matrix_path=matrix, head_dim=32)
    assert torch.equal(old, new) and float(old.abs().max()) > 0.1
    with pytest.raises(T.TransCARHipError, match='head_dim=64'):
        ops.sdpa(qs, gpu(k), gpu(vt), num_heads=8, matrix_path=matrix, head_dim=64)


# ---- 3. the operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', R.HEADS)
def test_self_attn_heads_vs_torch(T, H):
    """tc_self_attn_fwd with 4 / 16 heads against torch.nn.MultiheadAttention on the CPU, same weights, with the
    tolerance of test_gpu_parity.test_self_attn_vs_oracle."""
    from transcar_amd import bricks, ops
    torch.manual_seed(43 + H)
    mha = torch.nn.MultiheadAttention(256, H).eval()
    with torch.no_grad():
        mha.in_proj_bias.normal_(0.0, 0.2)
        mha.out_proj.bias.normal_(0.0, 0.2)
    rng = np.random.RandomState(41)
    x = torch.from_numpy(rng.standard_normal((2, 300, 256)).astype(np.float32))
    pos = torch.from_numpy(rng.standard_normal((2, 300, 256)).astype(np.float32))
    xq, pq = x.transpose(0, 1), pos.transpose(0, 1)
    want = x + mha(xq + pq, xq + pq, xq, need_weights=False)[0].transpose(0, 1)
    dev_mha = torch.nn.MultiheadAttention(256, H).eval()
    dev_mha.load_state_dict(mha.state_dict())
    dev_mha = dev_mha.to(R.dev())
    got = ops.self_attn(bricks.mha_view(dev_mha), gpu(x), gpu(pos), H)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=3e-5, rtol=1e-5)


# ---- 4. the whole head, free-running ----------------------------------------------------------------------------------------
PATHS = {'auto': {}, 'f16x2-16': dict(tile_rows=16, matrix_path='f16x2'), 'f32-16': dict(tile_rows=16, matrix_path='f32'),
         'f16x2-32': dict(tile_rows=32, matrix_path='f16x2')}


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('H', R.HEADS)
def test_head_heads_paths_oracle_and_golden(T, H, path):
    """The whole head with a 4- / 16-head decoder, free-running through all nine layers on the fixture's frame: against
    the oracle at H heads (every decoder state: layer 0's starts from the pack-time evaluation of its attention, which runs
    the fp32 core at H heads) and against the reference's outputs (G5-H4 / -H16)."""
    gold = R.gold('g5_head_tiny_h%d.npz' % H)
    head, sd = R.shared_head(T, num_heads=H)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=gold['radar_centres'])
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='golden', num_heads=H)          # (the paths share one oracle forward)
    outs = R.run_head(head, feats_np, frame, **PATHS[path])
    R.check_against_oracle(outs, want, dbg, R.E2E_TOL)
    R.check_against_fixture(outs, want, dbg, gold)


def test_the_head_count_reaches_the_kernels(T):
    """The 4-head and the 16-head head part by O(1) on the same frame and weights: neither runs the other's split."""
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    a = R.run_head(R.shared_head(T, num_heads=4)[0], feats_np, frame)['aux']['inter_states']
    b = R.run_head(R.shared_head(T, num_heads=16)[0], feats_np, frame)['aux']['inter_states']
    assert float((a - b).abs().max()) > 0.1


# ---- 5. one combined variant ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
def test_head_16_heads_two_levels_three_points_no_refinement(T, path):
    variant = dict(num_heads=16, num_levels=2, num_points=3, with_box_refine=False)
    head, sd = R.make_head(T, **variant)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    feats_np = synth.make_feats(TINY[:2], seed=1, smooth=SMOOTH)
    want, dbg = R.oracle_head(sd, feats_np, frame, key='combined', **variant)
    outs = R.run_head(head, feats_np, frame, **PATHS[path])
    R.check_against_oracle(outs, want, dbg, R.HS_TOL_F16X2 if path == 'f16x2-32' else R.E2E_TOL, refs_initial=True)


# ---- 6. / 7. train mode and training -------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,matrix', [(4, 'f32'), (32, 'f16x2')])
@pytest.mark.parametrize('H', R.HEADS)
def test_train_mode_decoder_heads_matches_reference_formula(T, H, rows, matrix):
    """The DROP instantiations of both cores at head dimension 64 / 16: the masks on the probabilities are read back as
    [H, Q, Q] per layer and handed to the oracle's decoder at H heads."""
    R.check_train_mode_decoder(R.g8_frame('g5_head_tiny_h%d.npz' % H), rows, matrix, num_heads=H)


def test_training_iteration_4_heads_gradients_match_reference(T):
    R.check_training_iteration(R.g8_frame('g5_head_tiny_h4.npz'), 'g8_train_grads_h4.npz', 'fused h4', num_heads=4)


# ---- 8. bit-identity with a 4-head head ---------------------------------------------------------------------------------
def test_heads_frame_of_nine_is_its_own(T):
    R.check_frame_of_nine(R.shared_head(T, num_heads=4)[0])


def test_frame_pipeline_heads_equals_forward_nhwc(T):
    R.check_frame_pipeline(R.shared_head(T, num_heads=4)[0], 2)


def test_plugin_graph_replay_heads_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, num_heads=4)[0], R.make_head(T, num_heads=4)[0])


def test_cam_pregather_heads_is_bit_identical(T):
    """The pre-gather workgroups ride in the staged core's launch whatever its head dimension."""
    head = R.shared_head(T, num_heads=4)[0]
    feats_np = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    frame = synth.make_radar_frame(seed=2, n_per_radar=51)
    a = R.run_head(head, feats_np, frame, tile_rows=32, matrix_path='f16x2')
    b = R.run_head(head, feats_np, frame, tile_rows=32, matrix_path='f16x2', cam_pregather=True)
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a['aux']['inter_states'], b['aux']['inter_states'])
