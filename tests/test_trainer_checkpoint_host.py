"""The trainer's checkpoint format (transcar_amd/checkpoint.py) on the CPU: Adam moments travel BY NAME between bucket
layouts, torch.optim.AdamW reads and writes the same dict, and what cannot be mapped is refused by name."""
import copy
import io

import pytest
import torch

from transcar_amd import build_head, configs
from transcar_amd import checkpoint as K
from transcar_amd._lib import TransCARHipError
from transcar_amd.trainer import FlatBucket, exchange_chunk_of

HYPER = dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.02)
STEP = 7


def layout(bucket):
    return bucket.names, [tuple(p.shape) for p in bucket.items], bucket.offsets


@pytest.fixture(scope='module')
def rig():
    """One CPU head, its trainable parameters in two bucket layouts, distinct moments per element in the first, packed."""
    head = build_head(configs.head_cfg())
    chunked = layout(FlatBucket(head.trainable_parameters(), chunk_of=exchange_chunk_of))
    plain = layout(FlatBucket(head.trainable_parameters(), chunk_of=None))
    n = sum(p.numel() for _, p in head.trainable_parameters())
    m = torch.arange(n, dtype=torch.float32) * 0.5 + 1.0
    v = torch.arange(n, dtype=torch.float32) * 0.25 + 3.0
    packed = K.pack_optimizer_state(*chunked, m, v, STEP, HYPER)
    return dict(head=head, chunked=chunked, plain=plain, n=n, m=m, v=v, packed=packed)


def slices(lay, flat):
    names, shapes, offsets = lay
    return {nm: flat[off:off + torch.Size(sh).numel()] for nm, sh, off in zip(names, shapes, offsets)}


def test_moments_travel_by_name_between_bucket_layouts(rig):
    names, shapes, off_a = rig['chunked']
    names_b, _, off_b = rig['plain']
    assert names == names_b and off_a != off_b           # the two layouts really differ
    assert sorted(off_b) == off_b and sorted(off_a) != off_a
    m2, v2 = torch.full((rig['n'],), -1.0), torch.full((rig['n'],), -1.0)
    assert K.unpack_optimizer_state(rig['packed'], *rig['plain'], m2, v2) == STEP
    for flat_a, flat_b in ((rig['m'], m2), (rig['v'], v2)):
        a, b = slices(rig['chunked'], flat_a), slices(rig['plain'], flat_b)
        for nm in names:
            assert torch.equal(a[nm], b[nm]), nm
    # the packed state aliases nothing
    assert rig['packed']['state'][0]['exp_avg'].data_ptr() != rig['m'].data_ptr() + 4 * off_a[0]
    assert rig['packed']['param_names'] == names


def test_torch_adamw_reads_and_writes_the_packed_state(rig):
    names, shapes, _ = rig['chunked']
    params = [torch.nn.Parameter(p.detach().clone()) for _, p in rig['head'].trainable_parameters()]
    opt = torch.optim.AdamW(params)
    opt.load_state_dict(rig['packed'])
    g = opt.param_groups[0]
    assert g['lr'] == HYPER['lr'] and tuple(g['betas']) == HYPER['betas'] and g['eps'] == HYPER['eps']
    assert g['weight_decay'] == HYPER['weight_decay']
    written = opt.state_dict()                            # torch's own: positional, no param_names
    assert 'param_names' not in written
    m2, v2 = torch.zeros(rig['n']), torch.zeros(rig['n'])
    assert K.unpack_optimizer_state(written, *rig['chunked'], m2, v2) == STEP
    assert torch.equal(m2, rig['m']) and torch.equal(v2, rig['v'])
    assert K.optimizer_hyper(written) == HYPER
    # an optimizer that has not stepped: empty state -> step 0, zero moments
    fresh = torch.optim.AdamW(params).state_dict()
    assert K.unpack_optimizer_state(fresh, *rig['chunked'], m2, v2) == 0
    assert float(m2.abs().max()) == 0 and float(v2.abs().max()) == 0


def unpack(rig, state):
    m2, v2 = torch.full((rig['n'],), -1.0), torch.full((rig['n'],), -1.0)
    try:
        return K.unpack_optimizer_state(state, *rig['plain'], m2, v2)
    except TransCARHipError:                              # a refusal writes nothing
        assert float(m2.max()) == -1.0 and float(v2.max()) == -1.0
        raise


def test_refusals_name_the_offender(rig):
    names, shapes, offsets = rig['plain']
    victim = names[5]
    dropped = copy.deepcopy(rig['packed'])
    dropped['param_names'] = [n for n in names if n != victim]
    with pytest.raises(TransCARHipError, match='missing.*' + victim.replace('.', r'\.')):
        unpack(rig, dropped)
    extra = copy.deepcopy(rig['packed'])
    extra['param_names'] = names + ['rf_norm9.weight']
    extra['state'][len(names)] = copy.deepcopy(extra['state'][0])
    with pytest.raises(TransCARHipError, match=r'unexpected.*rf_norm9\.weight'):
        unpack(rig, extra)
    shape = copy.deepcopy(rig['packed'])
    shape['state'][5]['exp_avg'] = shape['state'][5]['exp_avg'].reshape(-1)[:-1].clone()
    with pytest.raises(TransCARHipError, match='shape.*' + victim.replace('.', r'\.')):
        unpack(rig, shape)
    steps = copy.deepcopy(rig['packed'])
    steps['state'][5]['step'] = torch.tensor(float(STEP + 1))
    with pytest.raises(TransCARHipError, match='step differs.*' + victim.replace('.', r'\.')):
        unpack(rig, steps)
    for flag in ('amsgrad', 'maximize'):
        on = copy.deepcopy(rig['packed'])
        on['param_groups'][0][flag] = True
        with pytest.raises(TransCARHipError, match=flag):
            unpack(rig, on)
    positional = copy.deepcopy(rig['packed'])
    del positional['param_names']
    del positional['state'][len(names) - 1]
    positional['param_groups'][0]['params'] = list(range(len(names) - 1))
    with pytest.raises(TransCARHipError, match='positional.*%d parameters.*%d' % (len(names) - 1, len(names))):
        unpack(rig, positional)
    # more than five offenders: five are named, the rest counted
    many = copy.deepcopy(rig['packed'])
    many['param_names'] = names[8:]
    with pytest.raises(TransCARHipError) as e:
        unpack(rig, many)
    assert all(n in str(e.value) for n in names[:5]) and names[5] not in str(e.value) and '+3 more' in str(e.value)


def test_a_two_layer_checkpoint_is_refused_by_a_three_layer_trainer(rig):
    two = build_head(configs.head_cfg(num_fusion_layers=2))
    lay = layout(FlatBucket(two.trainable_parameters(), chunk_of=lambda n: exchange_chunk_of(n, 2)))
    n = sum(p.numel() for _, p in two.trainable_parameters())
    opt = K.pack_optimizer_state(*lay, torch.zeros(n), torch.ones(n), STEP, HYPER)
    ckpt = K.make_checkpoint(two.state_dict(), opt, dict(iter=STEP, num_fusion_layers=2))
    names3 = rig['plain'][0]
    with pytest.raises(TransCARHipError, match='num_fusion_layers=2.*num_fusion_layers=3'):
        K.check_structure(ckpt, names3, 3)
    del ckpt['trainer']['num_fusion_layers']              # (a file that does not say: the parameter set does)
    with pytest.raises(TransCARHipError, match=r'lacks trainable.*final_cls3\.'):
        K.check_structure(ckpt, names3, 3)
    with pytest.raises(TransCARHipError, match='missing.*3'):
        unpack(rig, opt)
    # ... and the other way round
    with pytest.raises(TransCARHipError, match='unexpected'):
        K.unpack_optimizer_state(rig['packed'], *lay, torch.zeros(n), torch.zeros(n))
    assert K.check_structure(K.make_checkpoint(two.state_dict(), opt, dict(num_fusion_layers=2)), lay[0], 2).keys() \
        == two.state_dict().keys()


def test_checkpoint_survives_a_weights_only_load(rig):
    head = rig['head']
    trainer = dict(iter=STEP, seed=2, dropout=0.1, decoder_dropout=0.0, max_norm=35.0, train_forwards=9,
                   dropout_seed=2, num_fusion_layers=3, deterministic=True, prefetch_depth=1, world_size=1)
    ckpt = K.make_checkpoint(head.state_dict(), rig['packed'], trainer, meta=dict(epoch=3, iter=1234, note='x'))
    assert ckpt['format'] == 'transcar_amd.trainer/1'
    # nothing aliases the head
    own = head.state_dict()
    assert all(ckpt['state_dict'][k].data_ptr() != own[k].data_ptr() for k in own)
    f = io.BytesIO()
    torch.save(ckpt, f)
    f.seek(0)
    back = torch.load(f, weights_only=True)
    assert back['trainer'] == trainer and back['meta'] == dict(epoch=3, iter=1234, note='x') and back['format'] == ckpt['format']
    assert back['state_dict'].keys() == own.keys() and all(torch.equal(back['state_dict'][k], own[k]) for k in own)
    m2, v2 = torch.zeros(rig['n']), torch.zeros(rig['n'])
    assert K.unpack_optimizer_state(back['optimizer'], *rig['chunked'], m2, v2) == STEP
    assert torch.equal(m2, rig['m']) and torch.equal(v2, rig['v'])
    torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for _, p in head.trainable_parameters()]) \
        .load_state_dict(back['optimizer'])


def test_reference_detector_keys_lose_their_prefix():
    sd = {'pts_bbox_head.rf_norm2.weight': torch.ones(2), 'img_backbone.conv1.weight': torch.zeros(1),
          'pts_bbox_head.code_weights': torch.ones(3)}
    assert sorted(K.head_state_dict(sd)) == ['code_weights', 'rf_norm2.weight']
    own = {'rf_norm2.weight': torch.ones(2)}
    assert K.head_state_dict(own).keys() == own.keys()
    assert K.is_legacy(dict(head=own, m=torch.zeros(2), v=torch.zeros(2), iter=0))
    assert not K.is_legacy(dict(state_dict=own, optimizer={}, meta={}))
