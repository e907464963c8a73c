"""Radar input as configuration on the GPU: Detr3DHead(radar_num_tokens=N, radar_in_dims=F, radar_point_range=...).

1. tc_radar_pack_rows_batch against numpy, exactly: ragged samples, every feature count's edge, the filter's faces and a
   NaN, T < N and T = N, an offsets array that does not ascend (on a token buffer with a canary around it).
2. The forward against the CPU oracle at N tokens (radar_input_rig) on the rig's tile heights and matrix paths, with
   head_variant_rig's tolerances.  The frames keep 120 rows near gate centres and the rest out of every gate's reach:
   with all 1700 rows near centres no seed keeps every gate decision 1e-3 m from its radius, which the hit-count cap needs
   (by the density of close query-token pairs some thirty of them would fall inside that band).  About 68 of the 128 rows hit, up to 4 tokens each.
3. One training iteration with dropout 0.1 against the oracle's with the same masks (read back through
   head_variant_rig.radar_dropout_masks at stride N): FusionTrainer's chain and per-operator backward, the deterministic
   backward once, and the head's own train-mode forward (forward_train_nhwc) under torch autograd.
4. The routes agree bit for bit: CUDA rows through the eager forward, through FramePipeline(radar_rows_capacity=), host
   pack_tokens through forward_nhwc; the plugin graphs at N = 2048 replay the eager entry.
5. A default head equals the head with the defaults spelled out."""
import numpy as np
import pytest
import torch

import head_variant_rig as R
import radar_heads_rig as RR
import radar_input_rig as RI
from head_variant_rig import T, no_grad  # noqa: F401
from oracle import transcar_oracle as O
from transcar_amd import synth

pytestmark = pytest.mark.gpu
gpu = R.gpu
PATHS = {'f32-4': dict(tile_rows=4, matrix_path='f32'), 'f16x2-16': dict(tile_rows=16, matrix_path='f16x2'),
         'f16x2-32': dict(tile_rows=32, matrix_path='f16x2')}
FACE_RANGE = RI.FACE_RANGE


# ---- 1. the pack kernel ------------------------------------------------------------------------------------------------------
def _pack_ref(samples, T_, N, rng):
    """numpy: HEAD:514-519 (strict, float64; a NaN fails), the first T - 1 (T < N) or T kept rows, 500.0 behind them"""
    limit = T_ - 1 if T_ < N else T_
    F = samples[0].shape[1]
    tok = np.full((len(samples), T_, F), 500.0, np.float32)
    count = np.zeros(len(samples), np.int32)
    for b, rows in enumerate(samples):
        kept = rows[RI.in_range(rows, rng)] if rng is not None else rows
        count[b] = len(kept)
        tok[b, :min(len(kept), limit)] = kept[:limit]
    return tok, count


def _ragged(N, F, rng):
    """four samples of 0, N - 1, N and N + 37 rows; with a filter, one row on each face of the range and one NaN coordinate
    among those of the second sample, a third of the rest outside"""
    r = np.random.RandomState(N * 100 + F)
    lo, hi = np.asarray(FACE_RANGE[:3]), np.asarray(FACE_RANGE[3:])
    out = []
    for n in (0, N - 1, N, N + 37):
        rows = r.standard_normal((n, F)).astype(np.float32)
        rows[:, :3] = (lo - 5.0 + r.uniform(0, 1, (n, 3)) * (hi - lo + 10.0)).astype(np.float32)
        out.append(rows)
    mid = ((lo + hi) / 2).astype(np.float32)
    for j in range(6):                    # exactly on a face: dropped (the values are exact in float32)
        out[1][10 + j, :3] = mid
        out[1][10 + j, j % 3] = FACE_RANGE[j]
    out[1][20, :3] = mid
    out[1][20, 1] = np.nan
    out[1][21, :3] = mid                  # and one safely inside
    return out


@pytest.mark.parametrize('full', [False, True], ids=['T-below-N', 'T-is-N'])
@pytest.mark.parametrize('filtered', [False, True], ids=['no-filter', 'filter'])
@pytest.mark.parametrize('F', [4, 36, 64])
@pytest.mark.parametrize('N', [128, 2048])
def test_pack_rows_against_numpy(T, N, F, filtered, full):
    from transcar_amd import ops
    samples = _ragged(N, F, FACE_RANGE)
    rng = FACE_RANGE if filtered else None
    T_ = N if full else N // 2
    want, want_count = _pack_ref(samples, T_, N, rng)
    if filtered:
        keep = RI.in_range(samples[1], rng)
        assert not keep[10:16].any() and not keep[20] and keep[21] and 0.1 < keep.mean() < 0.9
    assert want_count[2] > T_ - 1 or filtered                       # an overflow the count shows
    rows = gpu(np.concatenate(samples))
    offsets = torch.tensor(np.concatenate(([0], np.cumsum([len(s) for s in samples]))), dtype=torch.int32).to(R.dev())
    tok, count, pad_mult = ops.radar_pack_rows(rows, offsets, T_, N, ops.radar_range_tensor(rng, R.dev()) if filtered else None)
    torch.cuda.synchronize()
    assert pad_mult == N - T_ + 1 and tuple(tok.shape) == (4, T_, F)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(tok.cpu().numpy().view(np.int32), want.view(np.int32))         # bits: a kept NaN included
    if not full:
        assert np.all(want[:, T_ - 1] == 500.0)                     # row T - 1 stays the pad row
    if not filtered:
        assert np.isnan(tok.cpu().numpy()[1, 20, 1])


def test_pack_rows_clamps_offsets_that_do_not_ascend(T):
    """offsets [0, 50, 30, 9999, 60] over 200 rows read as [0, 50, 50, 200, 200]; nothing is written outside the token
    matrix (a canary on both sides of it) and nothing is read outside the rows."""
    from transcar_amd import ops
    N, F, T_, guard = 128, 36, 128, 4096
    r = np.random.RandomState(7)
    rows_np = r.uniform(-1.0, 1.0, (200, F)).astype(np.float32)
    big = torch.full((guard + 4 * T_ * F + guard,), -7.0, dtype=torch.float32, device=R.dev())
    out = big[guard:guard + 4 * T_ * F].view(4, T_, F)
    offsets = torch.tensor([0, 50, 30, 9999, 60], dtype=torch.int32).to(R.dev())
    _, count, _ = ops.radar_pack_rows(gpu(rows_np), offsets, T_, N, None, out=out)
    torch.cuda.synchronize()
    want, want_count = _pack_ref([rows_np[0:50], rows_np[50:50], rows_np[50:200], rows_np[200:200]], T_, N, None)
    assert np.array_equal(count.cpu().numpy(), want_count) and want_count.tolist() == [50, 0, 150, 0]
    assert np.array_equal(out.cpu().numpy(), want)
    assert bool((big[:guard] == -7.0).all()) and bool((big[-guard:] == -7.0).all())
    # negative and descending from the start
    offsets = torch.tensor([-5, -1, 120, 100, 2 ** 31 - 1], dtype=torch.int32).to(R.dev())
    big.fill_(-7.0)
    _, count, _ = ops.radar_pack_rows(gpu(rows_np), offsets, T_, N, None, out=out)
    torch.cuda.synchronize()
    want, want_count = _pack_ref([rows_np[0:0], rows_np[0:120], rows_np[120:120], rows_np[120:200]], T_, N, None)
    assert np.array_equal(count.cpu().numpy(), want_count) and np.array_equal(out.cpu().numpy(), want)
    assert bool((big[:guard] == -7.0).all()) and bool((big[-guard:] == -7.0).all())


# ---- 2. the forward against the oracle -------------------------------------------------------------------------------------------
_HEADS = {}


def _head(T, N, F, rng=None):
    if (N, F, rng) not in _HEADS:
        _HEADS[N, F, rng] = R.make_head(T, **RI.variant(N, F, rng))[0]
    return _HEADS[N, F, rng]


def _run(head, rows, **options):
    from transcar_amd.detr3d_head import head_options
    head.forward_options = head_options(**options) if options else None
    try:
        outs = head([gpu(f) for f in RI.feats_np()], RI.metas([rows], R.dev()), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    return outs


@pytest.mark.parametrize('path', sorted(PATHS))
@pytest.mark.parametrize('case', [c for c in RI.CASES if not c.startswith('train')])
def test_forward_against_oracle(T, case, path):
    c = RI.oracle_case(case)                    # (CPU: before the GPU is touched)
    N, F, n = c['N'], c['F'], len(c['rows'])
    print('%s: the oracle\'s closest gate decision sits %.2e m from its radius; rows hit %s' % (
        case, c['margin'], [int((h > 0).sum()) for h in c['dbg']['hit_counts']]))
    assert c['margin'] >= RI.MIN_MARGIN, (case, c['margin'])
    hit_tokens = [torch.where(~m)[1] for m in c['masks']]
    assert all(len(t) >= 10 for t in hit_tokens)
    if case.startswith('N2048'):
        assert max(int(t.max()) for t in hit_tokens) >= 1500          # a hit beyond the reference's count: the new ground
    if case == 'range':
        dropped = c['rows'][~RI.in_range(c['rows'], c['point_range'])]
        assert RI.in_range(dropped, RI.POINT_RANGE).all() and 0 < len(dropped) < n
        d = np.sqrt(((dropped[:, None, :2].astype(np.float64) - RI.gate_centres()[None]) ** 2).sum(-1)).min(1)
        assert int((d < 1.0).sum()) >= 5                              # rows inside a layer-1 circle (radius >= 1 m): they would hit
    head = _head(T, N, F, c['point_range'])
    tokens, pad_mult = head.radar_tokens(RI.metas([c['rows']], R.dev()), R.dev())
    kept = min(len(c['kept']), N)
    T_ = min(N, (kept + 1 + 63) // 64 * 64) if c['point_range'] is None else tokens.shape[1]
    assert tuple(tokens.shape) == (1, T_, F) and pad_mult == N - T_ + 1
    assert {'N2048-n1700': (1728, 321), 'N2048-n2048': (2048, 1), 'N2048-n2100': (2048, 1), 'N128-n40': (64, 65)}.get(
        case, (T_, pad_mult)) == (T_, pad_mult)
    assert np.array_equal(tokens[0, :kept].cpu().numpy(), c['kept'][:kept]) and bool((tokens[0, kept:] == 500.0).all())
    outs = _run(head, c['rows'], **PATHS[path])
    R.check_against_oracle(outs, c['want'], c['dbg'], hs_tol=R.HS_TOL_F16X2 if 'f16x2' in path else R.E2E_TOL)
    got_hits = outs['aux']['radar_hit_counts'][:, 0].cpu().numpy()
    assert int((got_hits > 0).sum()) >= 60 or N == 128


# ---- 3. training ---------------------------------------------------------------------------------------------------------------
TRAIN = {'N2048': 'N2048-n1700', 'F8': 'train-F8'}
BACKWARDS = RI.BACKWARDS
P_DROP = 0.1
_ORACLE_TRAIN = {}


def _gt():
    boxes, labels = synth.make_gt(seed=7, n=24)
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    return boxes, labels, gt.to(R.dev()), torch.from_numpy(labels).to(R.dev())


def _tied_inputs(c):
    """(query, hidden unit) pairs of fusion layer 1's FFN whose ReLU input the oracle has within radar_heads_rig.TIE_TAU of
    zero on a row without a hit (such a row reaches rf_linear1 untouched by the radar and by every dropout site: the
    decoder's last state through rf_norm2; found on the CPU).  Two fp32 evaluation orders part by that much, and the side
    such an input is taken on moves that unit's row of rf_linear1's gradient by one query's whole contribution.  On
    these frames: unit 77 at query 70, 2.1e-5 from zero (and unit 198 at query 101 on the F = 8 frame, 4.7e-6)."""
    sd = O.to_torch_sd(R.state_dict(**RI.variant(F=c['F'])))
    hs = RI.decoder_trace()[0].permute(0, 2, 1, 3)[-1][0]
    pre = O.linear(sd, 'rf_linear1', O.layer_norm(sd, 'rf_norm2', hs))
    no_hit = (c['dbg']['hit_counts'][0] == 0)[:, None]
    q, u = torch.where((pre.abs() < RR.TIE_TAU) & no_hit)
    return sorted(zip(q.tolist(), u.tolist()))


def _oracle_iteration(case, seed, monkeypatch, flip=()):
    """The oracle's iteration on the case's frame with the masks of `seed` (read back at stride N), once per seed.
    flip: (query, unit) inputs of fusion layer 1's FFN ReLU taken on the OTHER side of zero (as
    radar_heads_rig.tie_sensitivity flips inputs, here exactly these)."""
    flip = tuple(flip)
    if (case, seed, flip) not in _ORACLE_TRAIN:
        c = RI.oracle_case(case)
        drop = R.radar_dropout_masks(P_DROP, seed, 8, RI.Q, tokens=c['N'])
        assert drop[0]['probs'].shape == (8, RI.Q, c['N'])
        variant = RI.variant(c['N'], c['F'], c['point_range'])
        sd = O.to_torch_sd(R.state_dict(**variant))
        for k, v in sd.items():
            if R.trainable(k):
                v.requires_grad_(True)
        boxes, labels = _gt()[:2]
        plain, seen = O.F.relu, []

        def relu(x, *a, **kw):
            if flip and x.requires_grad and tuple(x.shape) == (RI.Q, 1, 512):       # the FFN hidden layers, layer 1 first
                seen.append(1)
                if len(seen) == 1:
                    keep = x.detach() > 0
                    for q, u in flip:
                        assert abs(float(x.detach()[q, 0, u])) < RR.TIE_TAU, (q, u, float(x.detach()[q, 0, u]))
                        keep[q, 0, u] = ~keep[q, 0, u]
                    return x * keep.to(x.dtype)
            return plain(x, *a, **kw)
        with monkeypatch.context() as m, torch.enable_grad():
            m.setattr(O.F, 'relu', relu)
            outs = R.oracle_forward(sd, RI.feats_np(), c['kept'], variant, decoder_trace=RI.decoder_trace(), drop=drop)
            res, _ = O.loss(outs, torch.from_numpy(boxes), torch.from_numpy(labels), sd['code_weights'])
            sum(res.values()).backward()
        assert not flip or len(seen) == 3
        _ORACLE_TRAIN[case, seed, flip] = ({k: float(v) for k, v in res.items()},
                                           {k: v.grad for k, v in sd.items() if R.trainable(k)})
    return _ORACLE_TRAIN[case, seed, flip]


def _iteration(T, c, backward):
    """One iteration of a fresh head on the case's frame -> (losses, gradients of the trainable parameters, dropout seed).
    backward 'autograd': Detr3DHead.forward_train_nhwc + Detr3DHead.loss under torch autograd (what the head's train-mode
    forward, FusionTrainer.step and step_nhwc run); else FusionTrainer.step_fused_nhwc with BACKWARDS[backward]."""
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    h = R.train_head(**RI.variant(c['N'], c['F']))
    metas = RI.metas([c['rows']], R.dev())
    tokens, pad_mult = h.radar_tokens(metas, R.dev())
    args = ([ops.to_nhwc(gpu(f)) for f in RI.feats_np()], ops.lidar2img_tensor(metas, R.dev()), metas[0]['img_shape'][0][:2],
            tokens, pad_mult)
    _, _, gt, gt_labels = _gt()
    if backward == 'autograd':
        h.set_dropout(P_DROP, decoder=False)
        h.dropout_seed, h._train_forwards = 5, 3
        h.train()
        with torch.enable_grad():
            losses = h.loss([gt], [gt_labels], h.forward_train_nhwc(*args))
            sum(losses.values()).backward()
        seed = h.last_dropout_seed
    else:
        tr = FusionTrainer(h, dropout=P_DROP, seed=5, **BACKWARDS[backward])
        h._train_forwards = 3
        with torch.enable_grad():
            losses = tr.step_fused_nhwc(*args, [gt], [gt_labels], update=False)
        seed = tr.last_dropout_seed
    torch.cuda.synchronize()
    return ({k: float(v) for k, v in losses.items()}, {n: q.grad.detach().cpu() for n, q in h.trainable_parameters()}, seed,
            tuple(tokens.shape), pad_mult, h)


@pytest.mark.parametrize('backward,which', [('chain', 'N2048'), ('operators', 'N2048'), ('deterministic', 'N2048'),
                                            ('autograd', 'N2048'), ('chain', 'F8'), ('operators', 'F8'), ('autograd', 'F8')])
def test_training_iteration_with_dropout_against_oracle(T, monkeypatch, which, backward):
    """The losses within 2e-3 of the oracle's, the gradients within the G8 tests' 2e-3 (check_grads_against_g8 on the
    oracle's gradients), and EVERY gradient element within 2e-3 of its tensor's largest value: the masks are the kernels'
    own, the probabilities' indexed (row * heads + head) * N + token -- on FusionTrainer's chain, per-operator and
    deterministic backward and on the head's own train-mode forward under torch autograd.

    ReLU ties.  On these weights and maps the oracle has a ReLU input of fusion layer 1's FFN within TIE_TAU = 3e-5 of zero
    on a row without a hit (_tied_inputs).  The kernels may take such an input on either side, so the row of rf_linear1's
    gradient that belongs to such a hidden unit is held to the oracle OR to the oracle re-run with exactly those inputs
    taken on the other side, whichever it matches -- within the same 2e-3, all of the row against one of the two.  Nothing
    is left out: every other element is held to the plain oracle.  Measured on the MI355X, all four routes alike: losses within 1e-6; row 77
    of rf_linear1.weight is 2.6e-2 (N = 2048) / 3.6e-2 (F = 8) of the tensor's maximum from the plain oracle and 6e-8 / 2e-7
    from the oracle with query 70's input on the other side; unit 198 (F = 8) sits on the plain oracle's side (3e-6); the
    largest other element is 1.7e-3 / 1.4e-3 (rf_norm2.weight)."""
    case = TRAIN[which]
    c = RI.oracle_case(case)
    assert c['margin'] >= RI.MIN_MARGIN
    tied = _tied_inputs(c)                      # (CPU)
    assert len(tied) <= 2, tied
    losses, grads, seed, shape, pad_mult, h = _iteration(T, c, backward)
    assert (shape[1], pad_mult) == ((1728, 321) if which == 'N2048' else (320, 1181))
    want_losses, want = _oracle_iteration(case, seed, monkeypatch)
    _, flipped = _oracle_iteration(case, seed, monkeypatch, flip=tied) if tied else (None, want)
    for k, v in losses.items():
        print('%s %s %s: %.6f (oracle %.6f)' % (which, backward, k, v, want_losses[k]))
    assert len(grads) == 98
    for k, v in losses.items():
        assert abs(v - want_losses[k]) < 2e-3 * max(1.0, abs(want_losses[k])), (k, v, want_losses[k])
    # the G8 tests' own check and bound, the oracle's gradients in the fixtures' layout
    named = {k: grads.get(k) for k, p_ in h.named_parameters() if R.trainable(k)}
    assert R.check_grads_against_g8(named, R.GradStats({k: want[k] if named[k] is not None else None for k in named}), 2e-3,
                                    '%s %s' % (which, backward)) == 98
    # and element by element, relative to each tensor's largest value
    units = sorted({u for _, u in tied})
    worst = ('', 0.0)
    for n, g in grads.items():
        scale = max(float(want[n].abs().max()), 1e-12)
        dd = (g.double() - want[n].double()).abs() / scale
        if n in ('rf_linear1.weight', 'rf_linear1.bias'):
            for u in units:                     # the whole row against one side or the other
                other = (g[u].double() - flipped[n][u].double()).abs() / scale
                print('   %s unit %d: %.3g from the oracle, %.3g from the oracle with the tied input on the other side' % (
                    n, u, float(dd[u].max()), float(other.max())))
                if float(other.max()) < float(dd[u].max()):
                    dd[u] = other
        worst = max(worst, (n, float(dd.max())), key=lambda t: t[1])
    print('%s %s: largest gradient difference relative to its tensor\'s maximum %.3g (%s)' % (which, backward, worst[1], worst[0]))
    assert worst[1] < 2e-3, worst


# ---- 4. the routes agree bit for bit ------------------------------------------------------------------------------------------------
def test_routes_agree_bit_for_bit(T):
    from transcar_amd import ops, radar
    from transcar_amd.pipeline import FramePipeline
    c = RI.oracle_case('N2048-n1700')
    N, rows = c['N'], c['rows']
    assert RI.in_range(rows, RI.POINT_RANGE).all()
    head = _head(T, N, 36)
    eager = _run(head, rows)
    # host pack_tokens -> forward_nhwc
    tok_np, pad_mult = radar.pack_tokens([rows], num_tokens=N)
    assert tok_np.shape == (1, 1728, 36) and pad_mult == N - 1728 + 1
    feats = [gpu(f) for f in RI.feats_np()]
    metas = RI.metas([rows])
    nhwc, l2i, hw = ops.to_nhwc_levels(feats), ops.lidar2img_tensor(metas, R.dev()), metas[0]['img_shape'][0][:2]
    host = head.forward_nhwc(nhwc, l2i, hw, gpu(tok_np), pad_mult)
    # the same numpy rows through the module entry (the host route of forward)
    entry = head(feats, metas)
    # CUDA rows through a lane's device rows stage
    lane = dict(nhwc=nhwc, l2i=l2i, hw=hw, tokens=torch.zeros((1, 1728, 36), device=R.dev()), pad_mult=pad_mult)
    pipe = FramePipeline(head, [lane], radar_rows_capacity=2048)
    for frame in (rows, rows[:900], rows):              # a shorter frame in between: the slot's rows behind it are dropped
        pipe.write_inputs(0, radar_rows=gpu(frame), slot=0)
        i, (outs, dec) = pipe.launch()
        pipe.wait(i)
        assert not pipe.radar_overflow(0) and int(pipe.radar_stage[0].count[0]) == len(frame)
        assert torch.equal(lane['tokens'], gpu(radar.pack_tokens([frame], T=1728, num_tokens=N)[0]))
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(eager[k], host[k]), k
        assert torch.equal(eager[k], entry[k]), k
        assert torch.equal(eager[k], outs[k]), k
    # an overflow shows in the lane's count
    pipe.write_inputs(0, radar_rows=gpu(RI.make_rows(3, 2040, 36)), slot=0)
    i, _ = pipe.launch()
    pipe.wait(i)
    assert pipe.radar_overflow(0)
    with pytest.raises(T._lib.TransCARHipError, match='radar_in_dims=36'):
        pipe.write_inputs(0, radar_rows=gpu(np.zeros((5, 8), np.float32)), slot=0)


def test_plugin_graphs_replay_at_2048_tokens(T):
    hg, he = R.make_head(T, **RI.variant(2048))[0], R.make_head(T, **RI.variant(2048))[0]
    R.check_plugin_graph_replay(hg, he)
    e = next(iter(hg._plugin_graphs.entries.values()))
    assert e.pad_mult == 2048 - e.T + 1 and e.stage.num_tokens == 2048


def test_raw_sweeps_beyond_1500_points_are_attended_at_2048(T):
    """a denser radar: 1700 raw points, all kept -- the head at 2048 tokens attends them all (T = 1728), the default head
    cuts them off at 1500, and the raw-sweep device ingest equals the host builder's tokens"""
    from transcar_amd import radar
    frame = synth.make_radar_frame(seed=11, n_per_radar=340)
    f36 = radar.build_radar_features(frame)
    assert 1500 < len(f36) <= 1700
    wide, default = _head(T, 2048, 36), _head(T, 1500, 36)
    metas = synth.make_img_metas(1, synth.make_lidar2img(), radar=frame)
    tok, pad_mult = wide.radar_tokens(metas, R.dev())
    assert tok.shape[1] == 1728
    want, want_pm = radar.pack_tokens([f36], T=1728, num_tokens=2048)
    assert tuple(tok.shape) == want.shape and pad_mult == want_pm == 2048 - 1728 + 1
    got = tok.cpu().numpy()
    exact, vel = [c for c in range(36) if c not in range(9, 15)], list(range(9, 15))
    assert np.array_equal(got[..., exact], want[..., exact])
    # (the rotated-velocity columns: float64 products rounded once on either side, 1 ulp as test_radar_ingest_on_device)
    assert np.all(np.abs(got[..., vel] - want[..., vel]) <= np.spacing(np.abs(want[..., vel])))
    tok_d, pm_d = default.radar_tokens(metas, R.dev())
    assert tuple(tok_d.shape) == (1, 1500, 36) and pm_d == 1 and torch.equal(tok_d[0], tok[0, :1500])


# ---- 5. the default head -------------------------------------------------------------------------------------------------------------
def test_default_head_equals_the_defaults_spelled_out(T):
    from transcar_amd import configs
    sd = {k: torch.from_numpy(v) for k, v in R.state_dict(**RI.variant()).items()}
    plain = T.build_head(configs.head_cfg(num_query=RI.Q))
    spelled = T.build_head(dict(configs.head_cfg(num_query=RI.Q), radar_num_tokens=1500, radar_in_dims=36,
                                radar_point_range=(-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)))
    outs = []
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=RI.gate_centres())
    rows = RI.oracle_case('range')['rows']
    for h in (plain, spelled):
        h.load_state_dict(sd, strict=True)
        h = h.to(R.dev()).eval()
        h.plugin_graphs = False
        feats = [gpu(f) for f in RI.feats_np()]
        outs.append((h(feats, synth.make_img_metas(1, synth.make_lidar2img(), radar=frame), aux=True), _run(h, rows)))
    for a, b in zip(*outs):
        for k in ('all_cls_scores', 'all_bbox_preds'):
            assert torch.equal(a[k], b[k]), k
        assert torch.equal(a['aux']['radar_hit_counts'], b['aux']['radar_hit_counts'])
    assert int((outs[0][0]['aux']['radar_hit_counts'] > 0).sum()) > 50


def test_forward_nhwc_names_tokens_of_the_wrong_shape(T):
    from transcar_amd import ops
    head = _head(T, 1500, 4)
    feats = [gpu(f) for f in RI.feats_np()]
    metas = RI.metas([np.zeros((0, 4), np.float32)])
    nhwc, l2i, hw = ops.to_nhwc_levels(feats), ops.lidar2img_tensor(metas, R.dev()), metas[0]['img_shape'][0][:2]
    for bad in (torch.zeros((64, 4), device=R.dev()), torch.zeros((1, 64, 36), device=R.dev())):
        with pytest.raises(T._lib.TransCARHipError, match='radar_in_dims=4'):
            head.forward_nhwc(nhwc, l2i, hw, bad, 1)
