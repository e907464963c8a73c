"""FusionTrainer.checkpoint / load_checkpoint on the MI355X (pytest -m gpu): a run that is interrupted, written out, read
back into a fresh head and a fresh trainer continues bit for bit (deterministic=True); the checkpoint aliases nothing;
the moments find their parameters in another bucket layout and in a state torch.optim.AdamW wrote; a FramePipeline
captured before the load keeps replaying and sees the loaded weights.

The rig is the one of test_deterministic_backward_is_bit_identical_on_any_schedule: 900 queries, the tiny G8 frame and a
second synthetic frame alternating, FusionTrainer(h, dropout=0.1, seed=2, lr=1e-3, deterministic=True)."""
import io
import os

import numpy as np
import pytest
import torch

from test_gpu_training import dev, frame_inputs, train_head
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

CTOR = dict(dropout=0.1, lr=1e-3, deterministic=True)


@pytest.fixture(scope='module')
def rig(golden_dir):
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    from transcar_amd import ops
    feats, metas, gt, labels = frame_inputs(golden_dir)
    frames = []
    for i in range(2):
        f = feats if i == 0 else [torch.from_numpy(x).to(dev()) for x in synth.make_feats('tiny', seed=9, smooth=(4, 6))]
        frames.append(dict(feats_nhwc=[ops.to_nhwc(x) for x in f], lidar2img=ops.lidar2img_tensor(metas, dev()),
                           img_hw=metas[0]['img_shape'][0][:2]))
    return dict(frames=frames, metas=metas, gt=gt, labels=labels, feats=feats, golden_dir=golden_dir)


def other_head(seed):
    """train_head (tests/test_gpu_training.py) with weights of ANOTHER seed: nothing of it may survive a load."""
    import transcar_amd as T
    cfg = configs.head_cfg()
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(seed).items()})
    return h.to(dev()).freeze_decoder().set_dropout(0.0)


def new_trainer(rig, head=None, seed=2, **kw):
    from transcar_amd.trainer import FusionTrainer
    h = train_head(rig['golden_dir']) if head is None else head
    tr = FusionTrainer(h, seed=seed, **dict(CTOR, **kw))
    tokens, pad_mult = h.radar_tokens(rig['metas'], dev())
    # (frame dicts of its own: the look-ahead recognises a frame by its tensors, the token tensor among them)
    tr.test_frames = [dict(fr, tokens=tokens, pad_mult=pad_mult) for fr in rig['frames']]
    return h, tr


def iterate(rig, tr, first, count, lookahead=False):
    """Iterations first .. first + count - 1 (frame i % 2); -> [(losses, the iteration's dropout seed)]."""
    hist = []
    for it in range(first, first + count):
        cur, nxt = tr.test_frames[it % 2], tr.test_frames[(it + 1) % 2]
        losses = tr.step_fused_nhwc(cur['feats_nhwc'], cur['lidar2img'], cur['img_hw'], cur['tokens'], cur['pad_mult'],
                                    [rig['gt']], [rig['labels']], prefetch=nxt if lookahead else None)
        hist.append(({k: float(v) for k, v in losses.items()}, tr.last_dropout_seed))
    torch.cuda.synchronize()
    return hist


def through_a_file(ckpt):
    f = io.BytesIO()
    torch.save(ckpt, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


def by_name(tr, flat=None):
    flat = tr.bucket.params if flat is None else flat
    return {n: flat[off:off + p.numel()].clone() for n, p, off in zip(tr.bucket.names, tr.bucket.items, tr.bucket.offsets)}


def tensors_of(obj, path=''):
    if torch.is_tensor(obj):
        yield path, obj
    elif isinstance(obj, dict):
        for k, v in obj.items():
            yield from tensors_of(v, '%s/%s' % (path, k))
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            yield from tensors_of(v, '%s/%d' % (path, i))


@pytest.fixture(scope='module')
def straight(rig):
    """Run A: four iterations without an interruption (no look-ahead: the deterministic mode does not depend on it)."""
    h, tr = new_trainer(rig)
    hist = iterate(rig, tr, 0, 4)
    return dict(hist=hist, params=tr.bucket.params.clone(), m=tr.m.clone(), v=tr.v.clone(), iter=tr.iter,
                forwards=h._train_forwards, named=by_name(tr))


@pytest.mark.parametrize('lookahead', [False, True])
def test_resumed_run_is_bit_identical_to_the_uninterrupted_one(rig, straight, lookahead):
    h, tr = new_trainer(rig)
    hist = iterate(rig, tr, 0, 2, lookahead)
    assert tr.lookahead_pending() == (1 if lookahead else 0)      # a pending look-ahead at checkpoint time changes nothing
    ckpt = through_a_file(tr.checkpoint(meta=dict(epoch=0, iter=2)))
    del h, tr
    assert ckpt['meta'] == dict(epoch=0, iter=2) and ckpt['format'] == 'transcar_amd.trainer/1'
    assert all(not t.is_cuda for _, t in tensors_of(ckpt))
    h2, tr2 = new_trainer(rig, head=other_head(11), seed=0)
    assert not torch.equal(tr2.bucket.params, straight['params'])
    report = tr2.load_checkpoint(ckpt)
    assert report['form'] == 'named' and not report['differed'] and not report['not_restored']
    assert report['clip_sum_order'] == 'bucket' and tr2._clip_index is None        # the same layout: the step path as it was
    assert not report['missing_keys'] and not report['unexpected_keys']
    assert tr2.iter == 2 and tr2.seed == 2 and h2.dropout_seed == 2 and h2._train_forwards == 2
    hist += iterate(rig, tr2, 2, 2, lookahead)
    assert torch.equal(tr2.bucket.params, straight['params'])
    assert torch.equal(tr2.m, straight['m']) and torch.equal(tr2.v, straight['v'])
    assert tr2.iter == straight['iter'] == 4 and h2._train_forwards == straight['forwards'] == 4
    for i, ((la, sa), (lb, sb)) in enumerate(zip(straight['hist'], hist)):
        assert sa == sb, i
        for k in la:                # (the loss VALUES still meet in float atomics of the loss kernel: equal to rounding)
            print('iteration', i, k, la[k], lb[k])
            assert abs(la[k] - lb[k]) <= 2e-6 * max(1.0, abs(la[k])), (i, k, la[k], lb[k])
    # the parameters are still views of the bucket
    for (n, p), off in zip(h2.trainable_parameters(), tr2.bucket.offsets):
        assert p.data_ptr() == tr2.bucket.params.data_ptr() + 4 * off, n


def test_checkpoint_aliases_nothing_and_state_dict_keeps_its_keys(rig):
    h, tr = new_trainer(rig)
    iterate(rig, tr, 0, 1)
    ckpt = tr.checkpoint(to_cpu=False)
    assert any(t.is_cuda for _, t in tensors_of(ckpt))
    copies = {k: t.clone() for k, t in tensors_of(ckpt)}
    assert len(copies) == len(h.state_dict()) + 3 * len(tr.bucket.names)
    before = tr.bucket.params.clone()
    iterate(rig, tr, 1, 1)
    assert not torch.equal(before, tr.bucket.params)
    for k, t in tensors_of(ckpt):
        assert torch.equal(t, copies[k]), k
    legacy = tr.state_dict()
    assert set(legacy) == {'head', 'm', 'v', 'iter'}
    # the legacy dict loads into a bucket of the same layout (all that can be checked is the length)
    want = (tr.bucket.params.clone(), tr.m.clone(), tr.v.clone())
    saved = dict(legacy, head={k: v.clone() for k, v in legacy['head'].items()})     # (its head part aliases the bucket)
    iterate(rig, tr, 2, 1)
    assert not torch.equal(tr.bucket.params, want[0])
    report = tr.load_checkpoint(saved)
    assert report['form'] == 'legacy' and 'seed' in report['not_restored'] and tr.iter == 2
    assert torch.equal(tr.bucket.params, want[0]) and torch.equal(tr.m, want[1]) and torch.equal(tr.v, want[2])
    from transcar_amd import TransCARHipError
    with pytest.raises(TransCARHipError, match='legacy'):
        tr.load_checkpoint(dict(saved, m=saved['m'][:-1], v=saved['v'][:-1]))


@pytest.mark.parametrize('max_norm', [35.0, 1e9])
def test_moments_find_their_parameters_in_another_bucket_layout(rig, monkeypatch, max_norm):
    """A checkpoint of the exchange-chunk layout loaded into a bucket in named_parameters order; one more deterministic
    iteration in each: parameters torch.equal per name.
    max_norm=1e9 (the clip never engages): everything is element-wise and the two layouts agree bit for bit.
    max_norm=35, the constructor's default: the gradient norm of this rig is 138.9, the clip engages, and its coefficient
    comes from tc_sq_norm's sum of squares, which adds the bucket up IN BUCKET ORDER (256 workgroup partials) -- another
    layout is another order of a float sum.  Summed in its own order the second trainer got 19305.974496 against
    19305.974915 (relative 2.2e-8): a coefficient that differs in its last bit, 19 of 98 parameters torch.equal, the
    largest difference 2.98e-8, with moments, loaded parameters and gradients equal per name.  So the trainer that loads
    a checkpoint of another layout keeps the order of the run it continues (FusionTrainer._adopt_clip_order)."""
    from transcar_amd import trainer as trainer_mod
    h, tr = new_trainer(rig, max_norm=max_norm)
    iterate(rig, tr, 0, 2)
    ckpt = through_a_file(tr.checkpoint())
    iterate(rig, tr, 2, 1)
    want, want_g, want_sq = by_name(tr), by_name(tr, tr.bucket.grads), float(tr.sq.double().sum())
    monkeypatch.setattr(trainer_mod, 'exchange_chunk_of', lambda name, num_fusion_layers=3: 0)
    h2, tr2 = new_trainer(rig, head=other_head(11), seed=0, max_norm=max_norm)
    assert tr2.bucket.names == tr.bucket.names and tr2.bucket.offsets != tr.bucket.offsets
    assert len(tr2.bucket.chunk_ranges) == 1 and len(tr.bucket.chunk_ranges) == 4
    assert tr2.load_checkpoint(ckpt)['clip_sum_order'] == 'checkpoint'
    assert tr2.checkpoint()['trainer']['bucket_order'] == ckpt['trainer']['bucket_order'] != tr2._bucket_order()
    for key, flat in (('exp_avg', tr2.m), ('exp_avg_sq', tr2.v)):
        m_want, m_got = by_name(tr, ckpt_flat(tr, ckpt, key)), by_name(tr2, flat)
        assert all(torch.equal(m_want[n], m_got[n]) for n in m_want), key
    iterate(rig, tr2, 2, 1)
    got, got_g, got_sq = by_name(tr2), by_name(tr2, tr2.bucket.grads), float(tr2.sq.double().sum())
    print('max_norm', max_norm, 'gradient norm', float(tr2.bucket.grads.double().norm()),
          'gradients equal per name:', sum(torch.equal(want_g[n], got_g[n]) for n in want), 'of', len(want),
          '; sum of squares (tc_sq_norm)', repr(want_sq), repr(got_sq), 'relative', abs(want_sq - got_sq) / want_sq,
          '; parameters equal per name:', sum(torch.equal(want[n], got[n]) for n in want),
          '; largest parameter difference', max(float((want[n] - got[n]).abs().max()) for n in want))
    assert all(torch.equal(want_g[n], got_g[n]) for n in want)
    for n in want:
        assert torch.equal(want[n], got[n]), n


def ckpt_flat(tr, ckpt, key):
    """The checkpoint's moments laid out like tr's bucket."""
    flat = torch.empty_like(tr.m)
    for i, (p, off) in enumerate(zip(tr.bucket.items, tr.bucket.offsets)):
        flat[off:off + p.numel()].copy_(ckpt['optimizer']['state'][i][key].reshape(-1))
    return flat


def test_state_written_by_torch_adamw_continues_as_torch_does(rig):
    """Two steps of a real torch.optim.AdamW on CPU clones, its state_dict() loaded positionally (a reference-style file:
    {'meta', 'state_dict', 'optimizer'}, keys under pts_bbox_head.), then ONE _optimizer_step with the third gradient in
    the bucket: torch's third step within 2e-6, the bound test_adamw_step_matches_torch has for the same kernel."""
    h, tr = new_trainer(rig, head=other_head(11), max_norm=1e9, lr=5e-5)
    names = tr.bucket.names
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for _, p in train_head(rig['golden_dir']).trainable_parameters()]
    opt = torch.optim.AdamW(ref, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    rng = np.random.RandomState(0)
    grads = [[torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32) * s) for p in ref]
             for s in (1.0, 0.01, 1.0)]
    for g in grads[:2]:
        for p, gi in zip(ref, g):
            p.grad = gi.clone()
        opt.step()
    sd = {'pts_bbox_head.' + k: v.detach().cpu().clone() for k, v in train_head(rig['golden_dir']).state_dict().items()}
    for n, p in zip(names, ref):
        sd['pts_bbox_head.' + n] = p.detach().clone()
    sd['img_backbone.conv1.weight'] = torch.zeros(4, 3, 7, 7)
    report = tr.load_checkpoint(through_a_file(dict(meta=dict(epoch=1, iter=2), state_dict=sd, optimizer=opt.state_dict())))
    assert report['form'] == 'positional' and tr.iter == 2 and tr.lr == 2e-4 and tr.max_norm == 1e9
    assert 'seed' in report['not_restored']
    for p, gi in zip(ref, grads[2]):
        p.grad = gi.clone()
    opt.step()
    tr.bucket.zero_grad()
    for p, gi in zip(tr.bucket.items, grads[2]):
        p.grad.copy_(gi)
    tr._optimizer_step()
    torch.cuda.synchronize()
    got = by_name(tr)
    worst = max(float((got[n].cpu() - p.detach().reshape(-1)).abs().max()) for n, p in zip(names, ref))
    print('largest difference to torch after the third step', worst)
    assert worst < 2e-6 and tr.iter == 3
    # a positional state of another length is refused, and nothing is loaded
    from transcar_amd import TransCARHipError
    short = torch.optim.AdamW(ref[:-1]).state_dict()
    before = tr.bucket.params.clone()
    with pytest.raises(TransCARHipError, match='positional'):
        tr.load_checkpoint(dict(state_dict=sd, optimizer=short))
    assert torch.equal(before, tr.bucket.params) and tr.iter == 3


def test_a_captured_pipeline_replays_the_loaded_weights_without_recapture(rig):
    from transcar_amd import ops
    from transcar_amd.pipeline import FramePipeline
    h, tr = new_trainer(rig)
    iterate(rig, tr, 0, 2)
    ckpt = through_a_file(tr.checkpoint())
    h2, tr2 = new_trainer(rig, head=other_head(11), seed=0)
    nhwc = [ops.to_nhwc(f) for f in rig['feats']]
    l2i = ops.lidar2img_tensor(rig['metas'], dev())
    img_hw = rig['metas'][0]['img_shape'][0][:2]
    tokens, pad_mult = h2.radar_tokens(rig['metas'], dev())
    lane = dict(nhwc=nhwc, l2i=l2i, hw=img_hw, tokens=tokens, pad_mult=pad_mult)
    with torch.no_grad():
        pipe = FramePipeline(h2.eval(), [lane], decode=False)
        pipe.launch()
        pipe.synchronize()
        before = pipe.outputs[0][0]['all_cls_scores'].clone()
        eager_before = h2.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult)['all_cls_scores'].clone()
    # the packed cls / reg branches of the decoder levels (camera-only outputs): a buffer of their own a graph may point at
    levels, g = h2.transformer.decoder.num_layers, torch.Generator().manual_seed(0)
    aux = dict(inter_states=(torch.randn(levels, 1, h2.num_query, h2.embed_dims, generator=g) * 0.5).to(dev()),
               init_reference=(torch.rand(1, h2.num_query, 3, generator=g) * 0.9 + 0.05).to(dev()),
               inter_references=(torch.rand(levels, 1, h2.num_query, 3, generator=g) * 0.9 + 0.05).to(dev()))
    with torch.no_grad():
        levels_before = [t.clone() for t in h2.decoder_outputs(aux)]
    packed_levels = h2._dec_heads[0].data_ptr()
    generation = h2.buffers_generation
    tr2.load_checkpoint(ckpt)
    assert h2.buffers_generation == generation
    assert h2._dec_heads[0].data_ptr() == packed_levels
    with torch.no_grad():
        got, want = h2.decoder_outputs(aux), h.eval().decoder_outputs(aux)
        torch.cuda.synchronize()
    assert h2._dec_heads[0].data_ptr() == packed_levels               # written again where it lay, not allocated anew
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert float((got[0] - levels_before[0]).abs().max()) > 1e-3
    with torch.no_grad():
        h2.eval()
        pipe.launch()                                   # no recapture()
        pipe.synchronize()
        after = pipe.outputs[0][0]['all_cls_scores'].clone()
        fresh = h2.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult)['all_cls_scores']
        torch.cuda.synchronize()
    assert torch.equal(fresh, after)
    assert float((fresh - eager_before).abs().max()) > 1e-3 and float((after - before).abs().max()) > 1e-3
    # ... and it is the head that was checkpointed
    with torch.no_grad():
        theirs = h.eval().forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult)['all_cls_scores']
    assert torch.equal(theirs, fresh)


def test_checkpoint_file_round_trip_leaves_no_temporary_file(rig, tmp_path):
    h, tr = new_trainer(rig)
    iterate(rig, tr, 0, 1)
    path = str(tmp_path / 'latest.pth')
    tr.save_checkpoint(path, meta=dict(epoch=5))
    assert sorted(os.listdir(str(tmp_path))) == ['latest.pth']
    tr.save_checkpoint(path, meta=dict(epoch=5))         # over an existing file
    assert sorted(os.listdir(str(tmp_path))) == ['latest.pth']
    assert torch.load(path, weights_only=True)['meta'] == dict(epoch=5)
    h2, tr2 = new_trainer(rig, head=other_head(11), seed=0)
    report = tr2.load_checkpoint_file(path)
    assert not report['differed'] and not report['not_restored']
    assert torch.equal(tr2.bucket.params, tr.bucket.params) and torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v)
    assert (tr2.iter, tr2.seed, tr2.dropout, tr2.decoder_dropout, tr2.max_norm, tr2.lr, tr2.betas, tr2.eps,
            tr2.weight_decay) == (tr.iter, tr.seed, tr.dropout, tr.decoder_dropout, tr.max_norm, tr.lr, tr.betas, tr.eps,
                                  tr.weight_decay)
    assert (h2.dropout_seed, h2._train_forwards) == (h.dropout_seed, h._train_forwards)
    own, theirs = h.state_dict(), h2.state_dict()
    assert all(torch.equal(own[k], theirs[k]) for k in own)
    # a constructor choice that differs is reported, not an error
    h3, tr3 = new_trainer(rig, head=other_head(11), seed=0, prefetch_depth=2)
    assert tr3.load_checkpoint_file(path)['differed'] == {'prefetch_depth': (1, 2)}
