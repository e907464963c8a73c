"""Checkpoint format of a training run of the fusion head (FusionTrainer.checkpoint / load_checkpoint).

The reference resumes with ``--resume-from``: mmcv writes ``{'meta', 'state_dict', 'optimizer'}``, the optimizer entry being
``torch.optim.AdamW.state_dict()`` -- per-parameter state addressed by POSITION in the optimizer's parameter list.  The
trainer here keeps its Adam moments in two flat buffers laid out like the gradient bucket (trainer.FlatBucket), which is a
permutation of ``named_parameters()`` that depends on ``num_fusion_layers``: a position says nothing about it.  So the
optimizer entry written here is torch's own form -- ``torch.optim.AdamW.load_state_dict`` accepts it -- plus a
``param_names`` list beside ``state`` and ``param_groups`` (torch ignores it): the moments are found by NAME, whatever the
layout of the bucket that wrote them and of the one that reads them.

Pure torch, no library call: everything here works on CPU tensors.
"""
import torch

from ._lib import TransCARHipError

FORMAT = 'transcar_amd.trainer/1'
#: the head's key prefix inside the reference detector's state_dict (DET: ``self.pts_bbox_head``)
HEAD_PREFIX = 'pts_bbox_head.'
#: keys of the ``trainer`` entry that are restored / only compared with the constructor's choice
RESTORED = ('iter', 'seed', 'dropout', 'decoder_dropout', 'max_norm', 'train_forwards', 'dropout_seed')
COMPARED = ('deterministic', 'prefetch_depth', 'world_size')


def _some(items):
    """Up to five offenders of an error message."""
    items = [str(i) for i in items]
    return ', '.join(items[:5]) + (' (+%d more)' % (len(items) - 5) if len(items) > 5 else '')


def _adamw_group_defaults():
    """The keys a param group of the INSTALLED torch.optim.AdamW carries (they differ between torch versions)."""
    opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)])
    return {k: v for k, v in opt.param_groups[0].items() if k != 'params'}


def pack_optimizer_state(names, shapes, offsets, m, v, step, hyper):
    """The Adam moments of flat buffers ``m`` / ``v`` (parameter i at ``offsets[i]``, ``shapes[i]``) as a dict
    ``torch.optim.AdamW.load_state_dict`` accepts, parameters indexed in the order of ``names`` (the order of
    ``head.trainable_parameters()``).  hyper: dict(lr, betas, eps, weight_decay)."""
    names = [str(n) for n in names]
    if not (len(names) == len(shapes) == len(offsets)):
        raise TransCARHipError('pack_optimizer_state: %d names, %d shapes, %d offsets'
                               % (len(names), len(shapes), len(offsets)))
    state = {}
    for i, (shape, off) in enumerate(zip(shapes, offsets)):
        shape = tuple(int(s) for s in shape)
        k = 1
        for s in shape:
            k *= s
        state[i] = {'step': torch.tensor(float(step), dtype=torch.float32),
                    'exp_avg': m[off:off + k].detach().reshape(shape).clone(),
                    'exp_avg_sq': v[off:off + k].detach().reshape(shape).clone()}
    group = _adamw_group_defaults()
    group.update(lr=float(hyper['lr']), betas=[float(b) for b in hyper['betas']], eps=float(hyper['eps']),
                 weight_decay=float(hyper['weight_decay']))
    group['params'] = list(range(len(names)))
    return {'state': state, 'param_groups': [group], 'param_names': names}


def optimizer_hyper(opt_state):
    """dict(lr, betas, eps, weight_decay) of the first param group of an optimizer state, or None without one."""
    groups = opt_state.get('param_groups') or []
    if not groups:
        return None
    g = groups[0]
    return dict(lr=float(g['lr']), betas=tuple(float(b) for b in g['betas']), eps=float(g['eps']),
                weight_decay=float(g['weight_decay']))


def unpack_optimizer_state(opt_state, names, shapes, offsets, m_out, v_out):
    """Scatter the moments of ``opt_state`` BY NAME into the flat buffers ``m_out`` / ``v_out`` of any layout (parameter
    ``names[i]`` at ``offsets[i]``); -> the optimizer's step count.  A dict without ``param_names`` (torch wrote it itself)
    is taken positionally, in the order of ``names``.  Everything is checked before anything is written."""
    names = [str(n) for n in names]
    for g in opt_state.get('param_groups', []):
        on = [k for k in ('amsgrad', 'maximize') if g.get(k)]
        if on:
            raise TransCARHipError('optimizer state: %s is set; tc_adamw_step implements neither' % _some(on))
    state = opt_state.get('state', {})
    saved = opt_state.get('param_names')
    if saved is None:
        ids = [i for g in opt_state.get('param_groups', []) for i in g['params']]
        if len(ids) != len(names):
            raise TransCARHipError('optimizer state without param_names (positional) holds %d parameters, the trainer %d: '
                                   'the positions cannot be matched to names' % (len(ids), len(names)))
        where = dict(zip(names, ids))
    else:
        saved = [str(n) for n in saved]
        missing = [n for n in names if n not in set(saved)]
        if missing:
            raise TransCARHipError('optimizer state: missing parameter(s) %s' % _some(missing))
        extra = [n for n in saved if n not in set(names)]
        if extra:
            raise TransCARHipError('optimizer state: unexpected parameter(s) %s' % _some(extra))
        ids = [i for g in opt_state.get('param_groups', []) for i in g['params']]
        if len(ids) != len(saved):
            ids = list(range(len(saved)))
        where = dict(zip(saved, ids))
    if len(state) == 0:                      # an optimizer that has not stepped yet
        m_out.zero_()
        v_out.zero_()
        return 0
    absent = [n for n in names if where[n] not in state]
    if absent:
        raise TransCARHipError('optimizer state: no state for parameter(s) %s' % _some(absent))
    bad, steps = [], {}
    for n, shape in zip(names, shapes):
        st = state[where[n]]
        want = tuple(int(s) for s in shape)
        for key in ('exp_avg', 'exp_avg_sq'):
            if tuple(st[key].shape) != want:
                bad.append('%s.%s %s (the trainer: %s)' % (n, key, tuple(st[key].shape), want))
        steps.setdefault(int(float(st['step'])), []).append(n)
    if bad:
        raise TransCARHipError('optimizer state: shape differs for %s' % _some(bad))
    if len(steps) != 1:
        common = max(steps, key=lambda s: len(steps[s]))
        odd = ['%s (step %d)' % (n, s) for s, ns in sorted(steps.items()) if s != common for n in ns]
        raise TransCARHipError('optimizer state: step differs between parameters -- %s, the others step %d; tc_adamw_step has '
                               'one bias-correction step for the whole bucket' % (_some(odd), common))
    for n, shape, off in zip(names, shapes, offsets):
        st = state[where[n]]
        k = st['exp_avg'].numel()
        m_out[off:off + k].copy_(st['exp_avg'].detach().reshape(-1))
        v_out[off:off + k].copy_(st['exp_avg_sq'].detach().reshape(-1))
    return next(iter(steps))


def head_state_dict(state_dict, prefix=HEAD_PREFIX):
    """The head's part of a state_dict: keys under the reference detector's ``pts_bbox_head.`` lose that prefix and every
    other key (``img_backbone.`` ...) is dropped; a dict without the prefix is the head's own and is taken as it is."""
    if any(k.startswith(prefix) for k in state_dict):
        return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    return dict(state_dict)


def clone_tensors(obj, to_cpu=False):
    """A copy of a tree of dicts / lists whose tensors alias nothing (on the CPU with ``to_cpu``)."""
    if torch.is_tensor(obj):
        return obj.detach().to('cpu', copy=True) if to_cpu else obj.detach().clone()
    if isinstance(obj, dict):
        return {k: clone_tensors(v, to_cpu) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [clone_tensors(v, to_cpu) for v in obj]
    return obj


def make_checkpoint(head_state, optimizer, trainer, meta=None, to_cpu=True):
    """The checkpoint dict: only tensors, numbers, strings, lists and dicts (``torch.load(weights_only=True)`` reads it).
    head_state: ``head.state_dict()`` -- cloned here; optimizer: from ``pack_optimizer_state`` (clones already)."""
    return {'format': FORMAT,
            'state_dict': clone_tensors(dict(head_state), to_cpu),
            'optimizer': optimizer,
            'trainer': dict(trainer),
            'meta': clone_tensors(meta, to_cpu) if meta is not None else {}}


def is_legacy(ckpt):
    """The dict ``FusionTrainer.state_dict()`` returns: flat moments in the layout of the bucket that wrote them."""
    return 'format' not in ckpt and 'state_dict' not in ckpt and {'head', 'm', 'v', 'iter'} <= set(ckpt)


def check_structure(ckpt, names, num_fusion_layers):
    """Refuse a checkpoint of another architecture: a ``num_fusion_layers`` or a set of trainable parameters that differs
    from the trainer's (``names``).  -> the head's part of the checkpoint's state_dict."""
    fmt = ckpt.get('format')
    if fmt is not None and fmt != FORMAT:
        raise TransCARHipError('checkpoint format %r; this version reads %r' % (fmt, FORMAT))
    if 'state_dict' not in ckpt:
        raise TransCARHipError('checkpoint without a state_dict entry (keys: %s)' % _some(sorted(map(str, ckpt))))
    theirs = (ckpt.get('trainer') or {}).get('num_fusion_layers')
    if theirs is not None and int(theirs) != int(num_fusion_layers):
        raise TransCARHipError('checkpoint of a head with num_fusion_layers=%d, the trainer\'s head has num_fusion_layers=%d'
                               % (int(theirs), int(num_fusion_layers)))
    sd = head_state_dict(ckpt['state_dict'])
    missing = [n for n in names if n not in sd]
    if missing:
        raise TransCARHipError('checkpoint lacks trainable parameter(s) %s' % _some(missing))
    saved = (ckpt.get('optimizer') or {}).get('param_names')
    if saved is not None:
        extra = [n for n in saved if n not in set(names)]
        if extra:
            raise TransCARHipError('checkpoint trains parameter(s) the trainer does not: %s' % _some(extra))
    return sd
