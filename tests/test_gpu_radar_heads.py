"""Detr3DHead(radar_num_heads=H) on the MI355X, H = 4 / 16 beside the reference's 8: the gated attention core alone against
float64 (forward, backward, dropout on the probabilities) on rows with tens of hits over several 64-token chunks, the
operator against torch.nn.MultiheadAttention(256, H), the whole head on every chain path against the CPU oracle with its
fusion attention at H heads and against the reference's fixtures (tests/golden/make_golden_radar_heads.py), training
iterations against the reference's gradients, and the bit-identities of a 4-head fusion stack.  pytest -m gpu"""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import radar_heads_rig as RR
from head_variant_rig import T, gpu, no_grad  # noqa: F401  (T, no_grad: fixtures)
from oracle import transcar_oracle as O
from transcar_amd import _lib as L

pytestmark = pytest.mark.gpu

KEYS = ('all_cls_scores', 'all_bbox_preds')
COUNTS = (8, 4, 16)             # 8 runs beside the new counts as the measure of every bound below
THREE = (1.0, 2.0)              # the reference's clamp pair of fusion layers 1 and 2
CIRCLE = (L.TC_RADAR_GATE_CIRCLE, 2.0)
MARGIN = 1e-3                   # metres: no token of a case lies this close to a circle's edge of any row (float64)
TOKENS_REF = R.CONFIGS['radar_num_tokens']      # the reference's padded token count: the last axis of its dropout mask on the probabilities


# ---- 1. the core alone against float64 ------------------------------------------------------------------------------------
def _circles(cen, box, gate):
    """float64 [Q, n, 2] centres and [Q, 1] radii of a row's circles, as O.circle_mask / O.single_circle_mask place them"""
    if gate[0] == L.TC_RADAR_GATE_CIRCLE:
        return cen[:, None], np.full((len(cen), 1), gate[1])
    length = np.exp(box[:, 3])
    off = np.stack((length * 0.25 * -box[:, 6], length * 0.25 * -box[:, 7]), -1)
    return np.stack((cen, cen + off, cen - off), 1), np.clip(length / 2.0, gate[0], gate[1])[:, None]


def _case(name):
    """-> dict(q [B,Q,256], kv [B,T,512], cen [B,Q,2], box [B,Q,10], tok [B,T,36], pad_mult), float32, made on the CPU.
    a: B = 2, Q = 75 (ragged for every rows-per-workgroup), T = 130 (two whole 64-token chunks and two tokens); the tokens
       lie within 0.6 m of 12 centres 2.2 m apart and every query near one of them, so a row's circles take in its own
       cluster and parts of the neighbours': 8 to 45 hits, in both whole chunks for every row and in the tail for a quarter
       of them.
    b: a with q scaled by 8 (scores span tens of nats: the running max jumps).
    c: B = 1, Q = 75, T = 64, pad_mult = 1437: the last token is the pad token, query 5 sits on it, and every third row
       is far from every token.
    A token within MARGIN of the edge of any circle of any row, under either gate, is dropped and drawn again."""
    rng = np.random.RandomState(20261020)
    Bn, Q, Tn, pad_mult = (1, 75, 64, 1437) if name == 'c' else (2, 75, 130, 1)
    grid = np.array([(2.2 * (i % 4) - 3.3, 2.2 * (i // 4) - 2.2) for i in range(12)])
    cen = np.zeros((Bn, Q, 2))
    box = rng.standard_normal((Bn, Q, 10)) * 0.5
    box[..., 3] = rng.uniform(0.0, 1.8, (Bn, Q))
    tok = rng.standard_normal((Bn, Tn, 36))
    for b in range(Bn):
        cen[b] = grid[np.arange(Q) % 12] + rng.uniform(-0.3, 0.3, (Q, 2))
        tok[b, :, :2] = grid[rng.permutation(Tn) % 12] + rng.uniform(-0.6, 0.6, (Tn, 2))
    if name == 'c':
        cen[0, 2::3] += 150.0                      # a third of the rows: no token anywhere near
        tok[0, -1, :] = 500.0                      # the pad token, pad_mult times
        cen[0, 5] = (499.5, 500.2)                 # ... and the one query that sits on it
    cen, box, tok = (a.astype(np.float32) for a in (cen, box, tok))
    for b in range(Bn):
        for _ in range(100):                       # (about one token in six is drawn again once, a few twice)
            close = np.zeros(Tn, bool)
            for gate in (THREE, CIRCLE):
                c, r = _circles(cen[b].astype(np.float64), box[b].astype(np.float64), gate)
                d = np.linalg.norm(c[:, :, None, :] - tok[b, None, None, :, :2].astype(np.float64), axis=-1)     # [Q, n, T]
                close |= (np.abs(d - r[:, :, None]) < MARGIN).any(axis=(0, 1))
            if not close.any():
                break
            assert not (name == 'c' and close[-1])
            n = int(close.sum())
            tok[b, close, :2] = (grid[rng.randint(0, 12, n)] + rng.uniform(-0.6, 0.6, (n, 2))).astype(np.float32)
        assert not close.any()
    q = rng.standard_normal((Bn, Q, 256)).astype(np.float32) * (8.0 if name == 'b' else 1.0)
    kv = rng.standard_normal((Bn, Tn, 512)).astype(np.float32)
    d_out = rng.standard_normal((Bn, Q, 256)).astype(np.float32)
    return dict(q=q, kv=kv, cen=cen, box=box, tok=tok, pad_mult=pad_mult, d_out=d_out)


def _mask64(cen, box, xy, gate):
    """True = masked, float64, [Q, T] of one sample"""
    if gate[0] == L.TC_RADAR_GATE_CIRCLE:
        return O.single_circle_mask(cen[None], xy[None], gate[1])
    return O.circle_mask(cen[None], box[None, :, 3], box[None, :, 6], box[None, :, 7], xy[None], gate[0], gate[1])


def _reference64(c, gate, H, prob_mult=None):
    """test_gpu_training._attn_reference's formula in float64 with autograd leaves q, kv; prob_mult [B, H, Q, T]: the
    multipliers of nn.MultiheadAttention's dropout on the probabilities.  -> (out, hit counts, q, kv, masks)"""
    q = torch.from_numpy(c['q']).double().requires_grad_(True)
    kv = torch.from_numpy(c['kv']).double().requires_grad_(True)
    cen, box, tok = (torch.from_numpy(c[k]).double() for k in ('cen', 'box', 'tok'))
    Bn, Q, C = q.shape
    Tn, hd = kv.shape[1], C // H
    outs, hits, masks = [], [], []
    for b in range(Bn):
        mask = _mask64(cen[b], box[b], tok[b, :, :2].contiguous(), gate)
        qh = (q[b] / hd ** 0.5).view(Q, H, hd).transpose(0, 1)
        k = kv[b, :, :C].view(Tn, H, hd).transpose(0, 1)
        v = kv[b, :, C:].view(Tn, H, hd).transpose(0, 1)
        mult = torch.ones(Tn, dtype=torch.float64)
        mult[-1] = c['pad_mult']
        s = (qh @ k.transpose(1, 2) + torch.log(mult)[None, None]).masked_fill(mask[None], float('-inf'))
        any_hit = (~mask).any(1)
        p = torch.where(any_hit[None, :, None], torch.softmax(s, -1), torch.zeros_like(s))
        if prob_mult is not None:
            p = p * prob_mult[b]
        outs.append((p @ v).transpose(0, 1).reshape(Q, C))
        hits.append(((~mask).double() * mult[None]).sum(1))
        masks.append(mask)
    return torch.stack(outs), torch.stack(hits), q, kv, torch.stack(masks)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def _run_core(c, gate, H, drop=(0.0, 0, 0)):
    from transcar_amd import autograd_ops as A
    with torch.enable_grad():
        qg, kg = gpu(c['q']).requires_grad_(True), gpu(c['kv']).requires_grad_(True)
        out, hits = A.radar_attn_core(qg, kg, gpu(c['cen']), 2, gpu(c['box']), gpu(c['tok']), c['pad_mult'], gate[0], gate[1],
                                      heads=H, drop=drop)
        out.backward(gpu(c['d_out']))
    torch.cuda.synchronize()
    return out.detach(), hits, qg.grad, kg.grad


def _check_core(c, gate, H, what, drop=(0.0, 0, 0), prob_mult=None):
    with torch.enable_grad():
        ref, hits_ref, q, kv, _ = _reference64(c, gate, H, prob_mult)
        ref.backward(torch.from_numpy(c['d_out']).double())
    out, hits, dq, dkv = _run_core(c, gate, H, drop)
    assert torch.equal(hits.cpu().double(), hits_ref), what          # every row: the case keeps its tokens off the edges
    d_out, r_q, r_kv = float((out.cpu().double() - ref.detach()).abs().max()), _rel(dq, q.grad), _rel(dkv, kv.grad)
    print('%s: max|out - fp64| %.3g, dq %.3g, dkv %.3g (relative)' % (what, d_out, r_q, r_kv))
    assert d_out < 2e-5, (what, d_out)
    assert r_q < 1e-4 and r_kv < 1e-4, (what, r_q, r_kv)
    return hits_ref


def test_the_cases_are_what_they_claim():
    """The geometry on the CPU (float64): hits per row and the chunks they come from."""
    for name in ('a', 'c'):
        c = _case(name)
        _, hits, _, _, masks = _reference64(c, THREE, 8)
        n = (~masks).sum(-1)                                     # tokens hit, [B, Q]
        if name == 'a':
            assert int(n.min()) >= 8 and 30 <= int(n.max()) <= 48 and float(n.double().mean()) >= 15, (n.min(), n.max())
            per_chunk = torch.stack([(~masks[..., 0:64]).any(-1), (~masks[..., 64:128]).any(-1), (~masks[..., 128:]).any(-1)])
            assert float(per_chunk[:2].all(0).double().mean()) == 1.0          # every row: hits in both whole chunks
            assert int(per_chunk.all(0).sum()) >= 20                           # ... and many in the two-token tail too
        else:
            assert int((n[0] == 0).sum()) == 24 and int(n[0, 5]) == 1 and float(hits[0, 5]) == 1437.0
            _, hits_c, _, _, _ = _reference64(c, CIRCLE, 8)
            assert int((hits_c[0] == 0).sum()) == 24 and float(hits_c[0, 5]) == 1437.0
            assert not torch.equal(hits_c, hits)                               # the two gates select other tokens


@pytest.mark.parametrize('H', COUNTS)
@pytest.mark.parametrize('case,gate', [('a', THREE), ('b', THREE), ('c', THREE), ('c', CIRCLE)],
                         ids=['a', 'b-q-times-8', 'c-pad-three-circle', 'c-pad-circle'])
def test_core_against_float64(T, case, gate, H):
    hits = _check_core(_case(case), gate, H, 'case %s H=%d' % (case, H))
    assert int((hits > 0).sum()) >= 50


@pytest.mark.parametrize('H', COUNTS)
def test_core_dropout_against_float64(T, H):
    """dropout_p = 0.1 on the probabilities, forward and backward, with the kernels' own mask read back: site 3, index
    (row * H + head) * 1500 + token by the row of the LAUNCH (b * Q + q)."""
    c = _case('a')
    p, seed, site = 0.1, 0x5EED0000 + H, 3
    Bn, Q, Tn = c['q'].shape[0], c['q'].shape[1], c['kv'].shape[1]
    flat = R.dropout_mask(p, seed, site, Bn * Q * H * TOKENS_REF)
    mult = flat.view(Bn, Q, H, TOKENS_REF).permute(0, 2, 1, 3)[..., :Tn].double()
    assert set(np.unique(mult.numpy()).tolist()) == {0.0, float(np.float32(1.0 / (1.0 - p)))}
    _check_core(c, THREE, H, 'case a dropout H=%d' % H, drop=(p, seed, site), prob_mult=mult)
    # and the mask matters: without it the same launch is far from this reference
    out0 = _run_core(c, THREE, H)[0]
    out1 = _run_core(c, THREE, H, drop=(p, seed, site))[0]
    assert float((out0 - out1).abs().max()) > 1e-2


# ---- 2. the operator -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H', COUNTS)
def test_operator_against_torch_multihead_attention(T, H):
    """ops.radar_gated_xattn(num_heads=H) against torch.nn.MultiheadAttention(256, H) under the oracle's circle_mask on case
    a's geometry, with the tolerance of test_gpu_parity.test_radar_xattn_teacher_forced."""
    from transcar_amd import bricks, ops
    c = _case('a')
    torch.manual_seed(50 + H)
    mha = torch.nn.MultiheadAttention(256, H).eval()
    mha.in_proj_bias.normal_(0.0, 0.2)
    mha.out_proj.bias.normal_(0.0, 0.2)
    rng = np.random.RandomState(51)
    query = torch.from_numpy(rng.standard_normal(c['q'].shape).astype(np.float32))
    feat = torch.from_numpy(rng.standard_normal(c['kv'].shape[:2] + (256,)).astype(np.float32))
    cen, box, xy = (torch.from_numpy(c[k]) for k in ('cen', 'box', 'tok'))
    xy = xy[..., :2].contiguous()
    want, want_hits = query.clone(), []
    for b in range(query.shape[0]):
        mask = O.circle_mask(cen[b:b + 1], box[b:b + 1, :, 3], box[b:b + 1, :, 6], box[b:b + 1, :, 7], xy[b:b + 1], *THREE)
        rows = torch.where((~mask).any(1))[0]
        want[b, rows] += mha(query[b, rows][:, None], feat[b][:, None], feat[b][:, None], attn_mask=mask[rows],
                             need_weights=False)[0][:, 0]
        want_hits.append((~mask).sum(1))
    dev_mha = torch.nn.MultiheadAttention(256, H).eval()
    dev_mha.load_state_dict(mha.state_dict())
    got, hits = ops.radar_gated_xattn(bricks.mha_view(dev_mha.to(R.dev())), gpu(query), gpu(cen), gpu(box), gpu(feat), gpu(xy),
                                      1, *THREE, num_heads=H)
    assert torch.equal(hits.cpu().long(), torch.stack(want_hits))
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=5e-5, rtol=1e-5)


# ---- 3. the whole head, free-running, on the fixture's frame ---------------------------------------------------------------
PATHS = {'auto': {}, 'f16x2-16': dict(tile_rows=16, matrix_path='f16x2'), 'f32-16': dict(tile_rows=16, matrix_path='f32'),
         'f16x2-32': dict(tile_rows=32, matrix_path='f16x2'), 'unfused': dict(unfused=True)}


def _whole_head(T, H, path):
    head, sd = R.shared_head(T, radar_num_heads=H)
    feats, frame = RR.g5_frame(H)
    want, dbg = R.oracle_head(sd, feats, frame, key='fixture frame', radar_num_heads=H)          # (the paths share one oracle forward)
    outs = R.run_head(head, feats, frame, **PATHS[path])
    R.check_against_oracle(outs, want, dbg)
    R.check_against_fixture(outs, want, dbg, R.gold(RR.g5_name(H)))


@pytest.mark.parametrize('path', ['auto', 'f16x2-16', 'f32-16', 'f16x2-32'])
@pytest.mark.parametrize('H', RR.HEADS)
def test_head_paths_oracle_and_reference(T, H, path):
    _whole_head(T, H, path)


def test_head_unfused_oracle_and_reference(T):
    _whole_head(T, 16, 'unfused')


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
def test_head_16_radar_heads_two_layers_circle_gate_23_classes(T, path):
    variant = dict(num_fusion_layers=2, radar_gate=R.CIRCLE, num_classes=23)
    head, sd = R.make_head(T, radar_num_heads=16, **variant)
    feats, frame = R.g5_frame()
    want, dbg = R.oracle_head(sd, feats, frame, key='combined', radar_num_heads=16, **variant)
    outs = R.run_head(head, feats, frame, **PATHS[path])
    assert outs['all_cls_scores'].shape[0] == 2 and outs['all_cls_scores'].shape[-1] == 23
    R.check_against_oracle(outs, want, dbg)


@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
def test_decoder_of_4_heads_under_a_radar_stack_of_16(T, path):
    """The two counts are not confused: against the oracle with ITS decoder at 4 and its fusion attention at 16; the oracle
    with the counts swapped is far from this head."""
    head, sd = R.make_head(T, radar_num_heads=16, num_heads=4)
    feats, frame = R.g5_frame()
    want, dbg = R.oracle_head(sd, feats, frame, key='4 under 16', radar_num_heads=16, num_heads=4)
    outs = R.run_head(head, feats, frame, **PATHS[path])
    R.check_against_oracle(outs, want, dbg)
    swapped, _ = R.oracle_head(sd, feats, frame, key='16 under 4', radar_num_heads=4, num_heads=16)
    assert float((outs['all_cls_scores'].cpu() - swapped['all_cls_scores']).abs().max()) > 0.1


# ---- 4. the count reaches the kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['auto', 'f16x2-32'])
def test_the_count_reaches_the_kernels(T, path):
    feats, frame = RR.g5_frame(4)
    outs = {8: R.run_head(R.shared_head(T)[0], feats, frame, **PATHS[path])}
    for H in RR.HEADS:
        outs[H] = R.run_head(R.shared_head(T, radar_num_heads=H)[0], feats, frame, **PATHS[path])
    for a, b in ((4, 8), (16, 8), (4, 16)):
        assert float((outs[a]['all_cls_scores'] - outs[b]['all_cls_scores']).abs().max()) > 0.1, (a, b)
        assert torch.equal(outs[a]['aux']['inter_states'], outs[b]['aux']['inter_states']), (a, b)
        assert torch.equal(outs[a]['aux']['inter_references'], outs[b]['aux']['inter_references']), (a, b)


# ---- 5. training -----------------------------------------------------------------------------------------------------------
BACKWARDS = {'chain': dict(chain_forward=True, chain_backward=True), 'operators': dict(chain_forward=False, chain_backward=False)}


@pytest.mark.parametrize('backward', sorted(BACKWARDS))
@pytest.mark.parametrize('H', RR.HEADS)
def test_training_iteration_gradients_match_reference(T, H, backward):
    """One iteration against the reference's losses and gradients at H heads, 2e-3 as head_variant_rig's
    check_training_iteration holds the 4-head decoder's.

    The frame is the gradient fixtures' own (tests/golden/make_golden_radar_heads.py): on the forward fixtures' frame one ReLU
    input of the 4-head stack lies 6.8e-6 from zero in a matched row, the kernels take it on the other side than the
    reference, and radar_position_encoder.0.bias then sits at 2.05e-3 of this bound's unit -- the oracle with that one input
    taken on the other side gives the same figures."""
    g8 = R.gold(RR.g8_name(H))
    what = 'rh%d %s' % (H, backward)
    h = R.train_head(radar_num_heads=H)
    assert len(h.trainable_parameters()) == 98
    losses, grads = R.trainer_iteration(RR.g8_frame(H), head=h, **BACKWARDS[backward])
    assert sorted('loss__' + k.replace('.', '_') for k in losses) == sorted(k for k in g8.files if k.startswith('loss__'))
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        print('%s %s: %.6f (reference %.6f)' % (what, k, v, ref))
        assert abs(v - ref) < 2e-3 * max(1.0, abs(ref)), (what, k, v, ref)
    assert R.check_grads_against_g8(grads, g8, 2e-3, what) == 98


@pytest.mark.parametrize('H', RR.HEADS)
def test_fused_training_with_dropout_matches_reference_formula(T, H):
    """The fused training forward and backward with p = 0.1 at every site of the fusion layers against the oracle at H heads
    fed the SAME masks (read back; the probabilities' as [H, Q, 1500]), with the bounds of
    test_gpu_training.test_fused_training_with_dropout_matches_reference_formula."""
    from transcar_amd.trainer import FusionTrainer
    p = 0.1
    frame = RR.g8_frame(H)
    h = R.train_head(radar_num_heads=H)
    tr = FusionTrainer(h, dropout=p, seed=5)
    h._train_forwards = 3
    with torch.enable_grad():
        losses = tr.step_fused_nhwc(*R.iteration_inputs(h, frame), update=False)
    torch.cuda.synchronize()
    seed = tr.last_dropout_seed
    hip_grads = {n: q.grad.detach().cpu().clone() for n, q in h.trainable_parameters()}
    drop = R.radar_dropout_masks(p, seed, H, h.num_query)
    assert drop[0]['probs'].shape == (H, h.num_query, TOKENS_REF)
    from transcar_amd import synth
    sd = O.to_torch_sd(synth.make_state_dict(3))
    for k, v in sd.items():
        if R.trainable(k):
            v.requires_grad_(True)
    with torch.enable_grad():
        outs = R.oracle_forward(sd, frame['feats_np'], frame['frame'], dict(radar_num_heads=H), drop=drop)
        res, _ = O.loss(outs, torch.from_numpy(frame['boxes']), torch.from_numpy(frame['labels']), sd['code_weights'])
        sum(res.values()).backward()
    for k, v in losses.items():
        ref = float(res[k])
        assert abs(float(v) - ref) < 2e-3 * max(1.0, abs(ref)), (k, float(v), ref)
    worst = 0.0
    for n, g in hip_grads.items():
        ref = sd[n].grad
        d = float((g.double() - ref.double()).norm() / max(float(ref.double().norm()), 1e-12))
        worst = max(worst, d)
        assert d < 5e-3, (n, d)
    print('rh%d dropout: worst relative gradient difference %.3g' % (H, worst))
    # and they are NOT the no-dropout gradients
    g8, k0 = R.gold(RR.g8_name(H)), 'rf_linear2.weight'
    ref = float(g8[k0.replace('.', '__') + '__stats'][2])
    assert abs(float(hip_grads[k0].double().norm()) - ref) > 1e-3 * ref


def test_deterministic_trainer_at_4_heads_is_bit_identical(T):
    frame = RR.g8_frame(4)
    runs = [R.trainer_iteration(frame, head=R.train_head(radar_num_heads=4), chain_forward=True, chain_backward=True, deterministic=True)[1]
            for _ in range(2)]
    assert sum(g is not None for g in runs[0].values()) == 98
    for k, g in runs[0].items():
        if g is not None:
            assert float(g.abs().max()) >= 0.0 and torch.equal(g, runs[1][k]), k


# ---- 6. bit-identity at H = 4 ---------------------------------------------------------------------------------------------
def test_frame_of_nine_is_its_own(T):
    R.check_frame_of_nine(R.shared_head(T, radar_num_heads=4)[0])


def test_frame_pipeline_equals_forward_nhwc(T):
    R.check_frame_pipeline(R.shared_head(T, radar_num_heads=4)[0], 2)


def test_plugin_graph_replay_is_the_eager_entry(T):
    R.check_plugin_graph_replay(R.make_head(T, radar_num_heads=4)[0], R.make_head(T, radar_num_heads=4)[0])
