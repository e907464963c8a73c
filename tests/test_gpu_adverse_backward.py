"""The training BACKWARD of the radar stack on the adverse frames, against fp64 autograd (-m gpu).

Every earlier check of the backward beyond T = 256 compares one of this project's paths with another (chain against
operators, deterministic against atomic); both sides share radar_attn_bwd_row (rowdev.hpp), the gate it re-evaluates,
its pad_mult weighting and its dropout index.  Here the reference is torch autograd in fp64 through
adverse_rig.radar_stack -- the three fusion layers composed from the oracle's functions with the fp32 oracle's gate
masks and the dropout multipliers the kernels drew -- on the four frames of adverse_rig.FRAMES (T = 448 / 704 / 1500,
pad_mult = 1053 / 797 / 1, rows with up to 55 hits, q projections x 8).

* a. autograd_ops.radar_attn_core alone on the oracle's layer-1 operands of keep / mid / truncated, against
  test_gpu_training._attn_reference in fp64; on keep one query sits on the folded pad token (pad_mult = 1053).
* b. FusionTrainer.step_fused_nhwc, teacher-forced: the decoder's forward is replaced by the oracle's last state, the
  loss by  sum(all_cls * d_cls) + sum(all_box * d_box)  with unit-normal cotangents, so that the backward receives
  exactly those.  The forward is compared with the fp32 / fp64 stacks first (the first independent check of the training
  forward with dropout at T != 256), then each of the 98 gradient tensors:
      max|g_hip - g64| <= 2 max|g_o32 - g64| + 1e-4 max|g64|
  (1e-4: the per-operator backward tolerance of test_gpu_training.py; g_o32: the same stack by autograd in fp32).
  Rows with a ReLU input within delta of zero are excluded on both sides (adverse_rig.tie_rows; the measured deltas and
  counts are in test_adverse_backward_host.py).  Four frames x p in {0, 0.1} x three paths.
* c. [truncated, all_hit] as one iteration of two samples at T = 1500: the sum of the two single-frame references.
* d. deterministic mode on all_hit with p = 0.1: two runs bit-identical, within 2e-6 of the atomic run, and (b).

Every test prints its figures (pytest -s).
Report of one run on an MI355X.  Every pair is HIP / fp32 torch (the fp32 stack or fp32 autograd), both against fp64.  HIP is
far below the 1e-4 floor, which is the project's own and was not tuned from these numbers: the gradients are within 4.9e-6
of each tensor's maximum (fp32 autograd: 2.1e-6), the deterministic and the atomic backward differ by 2.8e-7 of their scale.
core: max |d| of the attention core's output, dq and dK | dV, the rows / tokens on the folded pad token apart (max = the
reference's own maximum there).  Then per frame, p and path: fwd = max |d| of the training forward's scores and boxes over
the three layers, excl = rows excluded in layers 1 / 2 / 3 (of them by the forward check: rows beyond LAYER_TOL); below it
max|g - g64| / max|g64| of the worst tensor per group.  The excluded rows depend on the host's fp32 arithmetic through delta.
  core, keep (T 448, pad_mult 1053): max|d| out hip 2.14e-06 / 2.08e-06 (max 1.03e+01); out on the pad hip 1.53e-05 / 1.53e-05 (max 1.98e+02); dq hip 1.13e-05 / 3.72e-06 (max 2.31e+00); dq on the pad hip 2.13e-03 / 4.26e-03 (max 1.93e-12); dkv hip 1.59e-05 / 1.65e-05 (max 1.07e+01); dkv on the pad hip 1.12e-04 / 2.23e-04 (max 2.64e+00); 1 rows disagree on the hit count
  core, mid (T 704, pad_mult 797): max|d| out hip 2.67e-06 / 3.66e-06 (max 1.05e+01); dq hip 5.76e-06 / 5.92e-06 (max 2.25e+00); dkv hip 1.15e-05 / 1.48e-05 (max 1.17e+01); dkv on the pad hip 0.00e+00 / 0.00e+00 (max 0.00e+00); 0 rows disagree on the hit count
  core, truncated (T 1500, pad_mult 1): max|d| out hip 2.73e-06 / 3.70e-06 (max 1.02e+01); dq hip 7.71e-06 / 6.17e-06 (max 2.49e+00); dkv hip 2.19e-05 / 1.50e-05 (max 1.74e+01); 0 rows disagree on the hit count
  keep      p=0.0 chain:         fwd 7.3e-06 / 7.6e-06  excl [41,55,73] (1)
      attn 1.0e-06 / 9.3e-07  ffn 7.8e-07 / 8.0e-07  norms 1.9e-06 / 8.3e-07  branches 8.3e-07 / 6.8e-07  encoders 1.7e-06 / 1.4e-06
  keep      p=0.0 deterministic: fwd 7.3e-06 / 7.6e-06  excl [41,55,73] (1)
      attn 1.0e-06 / 9.3e-07  ffn 7.8e-07 / 8.0e-07  norms 6.8e-07 / 8.3e-07  branches 8.3e-07 / 6.8e-07  encoders 1.7e-06 / 1.4e-06
  keep      p=0.0 operators:     fwd 7.3e-06 / 7.6e-06  excl [41,55,73] (1)
      attn 3.0e-06 / 9.3e-07  ffn 8.3e-07 / 8.0e-07  norms 8.2e-07 / 8.3e-07  branches 5.6e-07 / 6.8e-07  encoders 1.7e-06 / 1.4e-06
  keep      p=0.1 chain:         fwd 7.3e-06 / 7.5e-06  excl [48,78,96] (1)
      attn 1.4e-06 / 1.3e-06  ffn 1.0e-06 / 7.1e-07  norms 8.7e-07 / 7.2e-07  branches 8.7e-07 / 1.0e-06  encoders 1.5e-06 / 1.7e-06
  keep      p=0.1 deterministic: fwd 7.3e-06 / 7.5e-06  excl [48,78,96] (1)
      attn 1.4e-06 / 1.3e-06  ffn 1.0e-06 / 7.1e-07  norms 8.1e-07 / 7.2e-07  branches 7.6e-07 / 1.0e-06  encoders 1.7e-06 / 1.7e-06
  keep      p=0.1 operators:     fwd 6.8e-06 / 7.5e-06  excl [48,78,96] (1)
      attn 2.6e-06 / 1.3e-06  ffn 1.5e-06 / 7.1e-07  norms 1.7e-06 / 7.2e-07  branches 9.2e-07 / 1.0e-06  encoders 1.9e-06 / 1.7e-06
  mid       p=0.0 chain:         fwd 8.2e-06 / 7.7e-06  excl [47,67,95] (0)
      attn 1.9e-06 / 1.1e-06  ffn 1.0e-06 / 8.4e-07  norms 8.1e-07 / 6.9e-07  branches 8.6e-07 / 9.4e-07  encoders 2.3e-06 / 2.1e-06
  mid       p=0.0 deterministic: fwd 8.2e-06 / 7.7e-06  excl [47,67,95] (0)
      attn 1.9e-06 / 1.1e-06  ffn 1.0e-06 / 8.4e-07  norms 8.1e-07 / 6.9e-07  branches 8.8e-07 / 9.4e-07  encoders 2.2e-06 / 2.1e-06
  mid       p=0.0 operators:     fwd 7.3e-06 / 7.7e-06  excl [47,67,95] (0)
      attn 1.1e-06 / 1.1e-06  ffn 1.2e-06 / 8.4e-07  norms 7.8e-07 / 6.9e-07  branches 5.9e-07 / 9.4e-07  encoders 1.6e-06 / 2.1e-06
  mid       p=0.1 chain:         fwd 8.3e-06 / 7.2e-06  excl [61,82,107] (0)
      attn 1.9e-06 / 1.1e-06  ffn 1.4e-06 / 9.9e-07  norms 9.6e-07 / 6.7e-07  branches 7.4e-07 / 7.9e-07  encoders 2.2e-06 / 1.6e-06
  mid       p=0.1 deterministic: fwd 8.3e-06 / 7.2e-06  excl [61,82,107] (0)
      attn 1.9e-06 / 1.1e-06  ffn 1.4e-06 / 9.9e-07  norms 9.0e-07 / 6.7e-07  branches 7.4e-07 / 7.9e-07  encoders 2.4e-06 / 1.6e-06
  mid       p=0.1 operators:     fwd 6.7e-06 / 7.2e-06  excl [61,82,107] (0)
      attn 1.8e-06 / 1.1e-06  ffn 1.3e-06 / 9.9e-07  norms 1.0e-06 / 6.7e-07  branches 7.3e-07 / 7.9e-07  encoders 1.9e-06 / 1.6e-06
  truncated p=0.0 chain:         fwd 9.2e-06 / 7.5e-06  excl [73,91,112] (0)
      attn 1.7e-06 / 1.1e-06  ffn 1.3e-06 / 7.6e-07  norms 2.7e-06 / 1.5e-06  branches 8.1e-07 / 6.9e-07  encoders 2.2e-06 / 1.5e-06
  truncated p=0.0 deterministic: fwd 9.2e-06 / 7.5e-06  excl [73,91,112] (0)
      attn 1.7e-06 / 1.1e-06  ffn 1.3e-06 / 7.6e-07  norms 2.5e-06 / 1.5e-06  branches 7.5e-07 / 6.9e-07  encoders 2.2e-06 / 1.5e-06
  truncated p=0.0 operators:     fwd 7.2e-06 / 7.5e-06  excl [73,91,112] (0)
      attn 1.6e-06 / 1.1e-06  ffn 1.1e-06 / 7.6e-07  norms 9.1e-07 / 1.5e-06  branches 6.3e-07 / 6.9e-07  encoders 1.9e-06 / 1.5e-06
  truncated p=0.1 chain:         fwd 8.1e-06 / 7.6e-06  excl [78,99,123] (0)
      attn 1.8e-06 / 1.4e-06  ffn 2.6e-06 / 9.0e-07  norms 2.4e-06 / 1.2e-06  branches 8.9e-07 / 1.3e-06  encoders 3.7e-06 / 1.9e-06
  truncated p=0.1 deterministic: fwd 8.1e-06 / 7.6e-06  excl [78,99,123] (0)
      attn 1.8e-06 / 1.4e-06  ffn 2.6e-06 / 9.0e-07  norms 2.4e-06 / 1.2e-06  branches 8.2e-07 / 1.3e-06  encoders 3.5e-06 / 1.9e-06
  truncated p=0.1 operators:     fwd 8.1e-06 / 7.6e-06  excl [78,99,123] (0)
      attn 1.5e-06 / 1.4e-06  ffn 1.3e-06 / 9.0e-07  norms 2.6e-06 / 1.2e-06  branches 6.1e-07 / 1.3e-06  encoders 2.5e-06 / 1.9e-06
  all_hit   p=0.0 chain:         fwd 7.4e-06 / 8.2e-06  excl [50,68,94] (0)
      attn 1.7e-06 / 9.7e-07  ffn 1.5e-06 / 8.8e-07  norms 1.4e-06 / 1.2e-06  branches 6.5e-07 / 6.3e-07  encoders 2.4e-06 / 1.3e-06
  all_hit   p=0.0 deterministic: fwd 7.4e-06 / 8.2e-06  excl [50,68,94] (0)
      attn 1.7e-06 / 9.7e-07  ffn 1.5e-06 / 8.8e-07  norms 1.3e-06 / 1.2e-06  branches 6.3e-07 / 6.3e-07  encoders 2.3e-06 / 1.3e-06
  all_hit   p=0.0 operators:     fwd 7.3e-06 / 8.2e-06  excl [50,68,95] (1)
      attn 1.4e-06 / 9.7e-07  ffn 1.1e-06 / 9.3e-07  norms 9.4e-07 / 1.2e-06  branches 7.3e-07 / 6.4e-07  encoders 2.0e-06 / 1.3e-06
  all_hit   p=0.1 chain:         fwd 8.1e-06 / 8.1e-06  excl [72,110,135] (1)
      attn 1.8e-06 / 1.5e-06  ffn 1.2e-06 / 1.2e-06  norms 1.6e-06 / 1.6e-06  branches 1.0e-06 / 9.1e-07  encoders 2.6e-06 / 2.1e-06
  all_hit   p=0.1 deterministic: fwd 8.1e-06 / 8.1e-06  excl [72,110,135] (1)
      attn 1.8e-06 / 1.5e-06  ffn 1.2e-06 / 1.2e-06  norms 1.6e-06 / 1.6e-06  branches 9.0e-07 / 9.1e-07  encoders 2.5e-06 / 2.1e-06
  all_hit   p=0.1 operators:     fwd 7.3e-06 / 8.1e-06  excl [72,109,134] (0)
      attn 2.4e-06 / 1.5e-06  ffn 1.8e-06 / 1.2e-06  norms 2.3e-06 / 1.5e-06  branches 7.3e-07 / 9.3e-07  encoders 2.2e-06 / 2.1e-06
  B=2 truncated:   fwd 9.2e-06 / 7.5e-06  excl [73,91,112] (0)
  B=2 all_hit:     fwd 7.4e-06 / 8.2e-06  excl [50,68,94] (0)
  [truncated, all_hit] in one iteration, chain:
      attn 1.5e-06 / 6.8e-07  ffn 1.6e-06 / 7.5e-07  norms 4.9e-06 / 7.8e-07  branches 1.0e-06 / 8.6e-07  encoders 2.4e-06 / 1.6e-06
  deterministic vs atomic backward, all_hit p=0.1: max|d| 1.37e-04 of a scale of 4.96e+02
  all_hit p=0.1 deterministic:
      attn 1.8e-06 / 1.5e-06  ffn 1.2e-06 / 1.2e-06  norms 1.6e-06 / 1.6e-06  branches 9.0e-07 / 9.1e-07  encoders 2.5e-06 / 2.1e-06
"""
import numpy as np
import pytest
import torch

import adverse_rig as A
from head_variant_rig import dropout_mask
from teacher_forced_checks import LAYER_TOL, PCR, dev, gpu
from test_gpu_training import _attn_reference
from transcar_amd import configs

pytestmark = pytest.mark.gpu

GRAD_FLOOR = 1e-4       # of a tensor's maximum: the project's per-operator backward tolerance (test_gpu_training.py)
PATHS = {'chain': dict(chain_forward=True, chain_backward=True),
         'deterministic': dict(chain_forward=True, chain_backward=True, deterministic=True),
         'operators': dict(chain_forward=False, chain_backward=False)}
FORWARDS = 3            # the forward counter every step starts from: one dropout seed for every path and frame


@pytest.fixture(scope='module')
def rig():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    rig = A.build()
    rig['T'] = transcar_amd
    return rig


# --------------------------------------------------------------------------
# a. the attention core's backward alone
# --------------------------------------------------------------------------
def _layer1_operands(rig, case):
    """(qproj [1,Q,C] unscaled, kv [1,T,2C], gate centres [1,Q,2], box [1,Q,10], tokens [1,T,36]) of fusion layer 1 on
    the oracle's state: projected on the host in fp64 and rounded once, so that no HIP arithmetic precedes the core."""
    sd64 = rig['sd64']
    _, dbg = case['trace']
    T = case['tok_np'].shape[1]
    W, b = sd64['rf_multihead_attn.in_proj_weight'], sd64['rf_multihead_attn.in_proj_bias']
    hs = dbg['hs'][-1].double()                                                  # [1,Q,C]
    rf = dbg['radar_feat'].permute(1, 0, 2)[:, :T].double()                     # [1,T,C]
    qp = torch.nn.functional.linear(hs, W[:256], b[:256]).float()
    kv = torch.nn.functional.linear(rf, W[256:], b[256:]).float()
    ref = dbg['inter_refs'][-1]
    cxy = torch.stack([ref[..., 0] * (PCR[3] - PCR[0]) + PCR[0], ref[..., 1] * (PCR[4] - PCR[1]) + PCR[1]], -1)
    return qp, kv, cxy.contiguous(), dbg['tmp'].contiguous(), torch.from_numpy(case['tok_np']).float()


@pytest.mark.parametrize('frame', ['keep', 'mid', 'truncated'])
def test_attention_core_backward_on_adverse_operands(rig, frame):
    """tc_radar_attn_core_fwd / _bwd (radar_attn_bwd_row) on layer 1's operands: output, dq and dK | dV against
    _attn_reference in fp64, over the rows whose hit count agrees (at most 2 may not).  Bound per tensor: 2 x the
    deviation of the same function in fp32, measured here, + 1e-4 of the tensor's maximum."""
    from transcar_amd import autograd_ops
    case = A.radar_case(rig, frame)
    T, pad_mult = A.FRAMES[frame][2]
    qp, kv, cxy, box, tok = _layer1_operands(rig, case)
    assert kv.shape[1] == T and case['pad_mult'] == pad_mult
    if frame == 'keep':                         # one query that does hit the folded pad token: mult enters pass 0 and pass 1
        assert pad_mult > 1000 and float(tok[0, -1, 0]) == 500.0
        cxy[0, 5] = torch.tensor([499.5, 500.2])
    d_out = torch.randn(qp.shape, generator=torch.Generator().manual_seed(T))
    xy = tok[..., :2].contiguous()

    qg, kg = (t.clone().to(dev()).requires_grad_(True) for t in (qp, kv))
    out, hits = autograd_ops.radar_attn_core(qg, kg, gpu(cxy), 2, gpu(box), gpu(tok), pad_mult, 1.0, 2.0)
    res = {}
    for dtype in (torch.float64, torch.float32):
        q_, kv_ = (t.clone().to(dtype).requires_grad_(True) for t in (qp, kv))
        ref, hits_ref = _attn_reference(q_, kv_, cxy, box, xy, 1.0, 2.0, pad_mult)
        if dtype == torch.float64:
            agree = hits.cpu().float() == hits_ref
            assert int((~agree).sum()) <= 2, int((~agree).sum())
            w = agree.float()[..., None]
            out.backward((d_out * w).to(dev()))
        ref.backward((d_out * w).to(dtype))
        res[dtype] = ((ref.detach() * w).double(), q_.grad.double(), kv_.grad.double())
    real = hits_ref.clone()
    if frame == 'keep':
        assert float(hits_ref[0, 5]) >= pad_mult and bool(agree[0, 5])
        real[0, 5] = 0
    # rows with many hits, in several 64-token chunks: the rig's recorded figures, as test_gpu_adverse_frame.py asks
    assert float(real[agree].max()) >= 0.75 * A.FRAMES[frame][4]
    assert int((hits_ref > 0).sum()) >= 0.9 * A.FRAMES[frame][3][0]
    got = ((out.detach().cpu() * w).double(), qg.grad.cpu().double(), kg.grad.cpu().double())
    # the bound holds for the rows / tokens on the folded pad token (|K|, |V| ~ 1e3: the fp32 formula itself is coarse
    # there) and for all the others separately, so that the pad's scale does not loosen the bound of the rest
    on_pad_q = hits_ref[0] >= pad_mult if pad_mult > 1 else torch.zeros(qp.shape[1], dtype=torch.bool)
    on_pad_t = torch.arange(T) >= min(case['f36'].shape[0], T)
    line = []
    for name, g, r64, r32, on_pad in zip(('out', 'dq', 'dkv'), got, res[torch.float64], res[torch.float32],
                                         (on_pad_q, on_pad_q, on_pad_t)):
        assert torch.isfinite(g).all(), name
        for part, sel in (('', ~on_pad), (' on the pad', on_pad)):
            if not bool(sel.any()):
                continue
            e_hip, e_o32 = float((g - r64)[0, sel].abs().max()), float((r32 - r64)[0, sel].abs().max())
            scale = float(r64[0, sel].abs().max())
            line.append('%s%s hip %.2e / fp32 torch %.2e (max %.2e)' % (name, part, e_hip, e_o32, scale))
            assert (scale > 0 or part) and e_hip <= 2.0 * e_o32 + GRAD_FLOOR * scale, (frame, line[-1])
    print('attention core backward vs fp64, %s (T %d, pad_mult %d): max|d| %s; %d rows disagree on the hit count'
          % (frame, T, pad_mult, '; '.join(line), int((~agree).sum())))


# --------------------------------------------------------------------------
# b. the stack's backward, teacher-forced
# --------------------------------------------------------------------------
def _trainer(rig, path):
    """A training head with the adverse weights and its FusionTrainer on `path`, built once per module."""
    cache = rig.setdefault('_trainers', {})
    if path not in cache:
        from transcar_amd.trainer import FusionTrainer
        cfg = configs.head_cfg()
        cfg['train_cfg'] = configs.train_cfg_pts
        head = rig['T'].build_head(cfg)
        head.load_state_dict({k: torch.from_numpy(v) for k, v in rig['sd_np'].items()}, strict=True)
        head = head.to(dev()).freeze_decoder().set_dropout(0.0)
        tr = FusionTrainer(head, dropout=0.0, seed=5, decoder_dropout=0.0, **PATHS[path])
        tr.device_loss = False
        cache[path] = (head, tr)
    return cache[path]


def _kernel_dropout(rig, p, seed, Q):
    """The multipliers the kernels draw for `seed`, as O.radar_layer takes them: sites 4 r + {0 probabilities, 1
    rf_dropout2, 2 rf_dropout, 3 rf_dropout3}; the probabilities are indexed ((row * 8 + head) * 1500 + token) -- the
    reference's token count, whatever T the launch has."""
    if p == 0.0:
        return None
    cache = rig.setdefault('_drop', {})
    if (p, seed) not in cache:
        def m(site, *shape):
            return dropout_mask(p, seed, site, int(np.prod(shape))).view(*shape)
        cache[p, seed] = [dict(probs=m(4 * r, Q, 8, 1500).permute(1, 0, 2).contiguous(), d2=m(4 * r + 1, Q, 256),
                               ffn=m(4 * r + 2, Q, 512), d3=m(4 * r + 3, Q, 256)) for r in range(3)]
    return cache[p, seed]


def _reference(rig, frame, p, drop, cot, keep):
    """(backward_case, g32, g64) of one frame: evaluated once per (frame, p, cotangent seed, rows kept)."""
    cache = rig.setdefault('_reference', {})
    if (frame, p) not in cache:
        cache[frame, p] = A.backward_case(rig, frame, drop)
    bc = cache[frame, p]
    if keep is None:
        return bc
    key = (frame, p, cot, keep.tobytes())
    if key not in cache:
        d_cls, d_box = A.cotangents(cot)
        cache[key] = A.reference_gradients(rig, bc['case'], drop, d_cls, d_box, keep, bc['masks'])
    return (bc,) + cache[key]


def _check_forward(got_cls, got_box, bc, what):
    """The HIP training forward of one sample against the fp32 and fp64 stacks (same masks, same multipliers).  A row
    beyond LAYER_TOL of the fp32 stack is a gate disagreement: at most 2 new ones per layer, excluded from that layer on.
    Every other row: within 2 x the fp32 stack's own deviation from fp64 + 0.2 LAYER_TOL, the inference test's rule.
    -> (bool [3,Q] rows excluded, report lines)."""
    o32, o64 = bc['x32']['outputs'], bc['x64']['outputs']
    bad = np.zeros(tuple(got_cls.shape[:2]), dtype=bool)         # [3,Q]
    lines = []
    for r in range(3):
        far = np.zeros(bad.shape[1], dtype=bool)
        for got, want in ((got_cls, o32[0]), (got_box, o32[1])):
            far |= ((got[r] - want[r, 0]).abs().amax(-1) > LAYER_TOL).numpy()
        new = far & ~(bad[r - 1] if r else np.zeros_like(far))
        assert int(new.sum()) <= 2, '%s, fusion layer %d: %d new rows beyond LAYER_TOL' % (what, r + 1, int(new.sum()))
        bad[r] = far | (bad[r - 1] if r else False)
        ok = torch.from_numpy(~bad[r])
        for name, got, k in (('cls', got_cls, 0), ('box', got_box, 1)):
            e_hip = float((got[r].double() - o64[k][r, 0]).abs()[ok].max())
            e_o32 = float((o32[k][r].double() - o64[k][r]).abs().max())
            lines.append('layer %d %s %.2e / %.2e' % (r + 1, name, e_hip, e_o32))
            assert e_hip <= 2.0 * e_o32 + 0.2 * LAYER_TOL, (what, lines[-1])
    return bad, lines


def _step(rig, path, frames, p, monkeypatch, cots):
    """One teacher-forced iteration (update=False) of `frames` as one batch on `path`.  -> dict(grads {name: tensor on the
    host}, flat = the bucket's gradients, keep = [bool [3,Q] per sample], drop, lines)."""
    head, tr = _trainer(rig, path)
    B, Q = len(frames), head.num_query
    cases = [A.radar_case(rig, f) for f in frames]
    T, pad_mult = A.FRAMES[frames[0]][2]
    assert all(A.FRAMES[f][2] == (T, pad_mult) for f in frames)
    tr.dropout = float(p)
    head._train_forwards = FORWARDS
    seed = head.peek_dropout_seed(1)
    assert p == 0.0 or B == 1                    # (a batch draws sample b's probabilities from rows b Q ..: not needed here)
    drop = _kernel_dropout(rig, p, seed, Q)
    _, dbg = cases[0]['trace']                                   # the decoder reads no radar: one state for every frame
    aux = dict(inter_states=gpu(dbg['hs'][-1])[None].repeat(1, B, 1, 1),
               inter_references=gpu(dbg['inter_refs'][-1])[None].repeat(1, B, 1, 1),
               last_box=gpu(dbg['tmp']).repeat(B, 1, 1))
    seen = {}

    def decoder_forward(*a, **kw):
        return {'aux': aux}

    def loss(gt_bboxes_list, gt_labels_list, outs):
        all_cls, all_box = outs['all_cls_scores'], outs['all_bbox_preds']
        assert all_cls.shape == (3, B, Q, 10) and all_box.shape == (3, B, Q, 10)
        c, b = all_cls.detach().cpu(), all_box.detach().cpu()
        assert torch.isfinite(c).all() and torch.isfinite(b).all()
        seen['keep'], seen['lines'], w_cls, w_box = [], [], [], []
        for i, f in enumerate(frames):
            bc = _reference(rig, f, p, drop, None, None)
            bad, lines = _check_forward(c[:, i], b[:, i], bc, '%s / %s' % (f, path))
            keep = ~(bc['ties'] | bad)
            assert (~keep).sum(1).max() <= A.MAX_EXCLUDED * Q, (~keep).sum(1)
            d_cls, d_box = A.cotangents(cots[i])
            k = torch.from_numpy(keep).float()[:, None, :, None]
            w_cls.append(d_cls * k)
            w_box.append(d_box * k)
            seen['keep'].append(keep)
            seen['lines'].append('forward vs fp64, hip / fp32 stack: %s; rows excluded %s (%d by the forward check)'
                                 % ('  '.join(lines), (~keep).sum(1).tolist(), int(bad[-1].sum())))
        return {'loss_inject': (all_cls * torch.cat(w_cls, 1).to(dev())).sum() + (all_box * torch.cat(w_box, 1).to(dev())).sum()}

    monkeypatch.setattr(tr, '_decoder_forward', decoder_forward)
    monkeypatch.setattr(head, 'loss', loss)
    tokens = gpu(np.concatenate([c['tok_np'] for c in cases]))
    assert tokens.shape == (B, T, 36)
    l2i = gpu(torch.cat([rig['l2i']] * B))
    with torch.enable_grad():
        tr.step_fused_nhwc([], l2i, A.HW, tokens, pad_mult, [None] * B, [None] * B, update=False)
    torch.cuda.synchronize()
    assert tr.last_dropout_seed == seed
    grads = {n: q.grad.detach().cpu().clone() for n, q in head.trainable_parameters()}
    return dict(grads=grads, flat=tr.bucket.grads.clone(), keep=seen['keep'], drop=drop, lines=seen['lines'])


def _check_gradients(got, g32, g64, what):
    """Each of the 98 tensors: max|g_hip - g64| <= 2 max|g_o32 - g64| + 1e-4 max|g64|.  -> report lines per group
    (the worst tensor's figures relative to its own maximum)."""
    assert len(got) == 98 and sorted(got) == sorted(g64)
    groups, failed = {}, []
    for n, g in got.items():
        assert torch.isfinite(g).all(), n
        r64 = g64[n]
        scale = float(r64.abs().max())
        e_hip, e_o32 = float((g.double() - r64).abs().max()), float((g32[n].double() - r64).abs().max())
        worst = groups.setdefault(A.group_of(n), [0.0, 0.0])
        worst[0], worst[1] = max(worst[0], e_hip / scale), max(worst[1], e_o32 / scale)
        if not e_hip <= 2.0 * e_o32 + GRAD_FLOOR * scale:
            failed.append('%s: hip %.3e, fp32 autograd %.3e, max|g64| %.3e' % (n, e_hip, e_o32, scale))
    lines = ['%-21s %.2e / %.2e' % (title, groups[title][0], groups[title][1]) for title, _ in A.GROUPS]
    print('\n'.join(['%s: max|g - g64| / max|g64| per group, hip / fp32 autograd' % what] + ['    ' + ln for ln in lines]))
    assert not failed, (what, failed)
    return lines


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('p', [0.0, 0.1])
@pytest.mark.parametrize('frame', list(A.FRAMES))
def test_stack_backward_teacher_forced_on_adverse_frames(rig, monkeypatch, frame, p, path):
    """One iteration of the trainable stack from the oracle's decoder state with seeded cotangents: the forward against
    the fp32 / fp64 stacks with the kernels' own dropout multipliers, then the 98 gradient tensors against fp64 autograd."""
    run = _step(rig, path, [frame], p, monkeypatch, [5])
    _, g32, g64 = _reference(rig, frame, p, run['drop'], 5, run['keep'][0])
    what = 'stack backward, %s (T %d, pad_mult %d) p=%.1f %s' % ((frame,) + A.FRAMES[frame][2] + (p, path))
    print('%s: %s' % (what, run['lines'][0]))
    _check_gradients(run['grads'], g32, g64, what)


# --------------------------------------------------------------------------
# c. two samples in one iteration
# --------------------------------------------------------------------------
def test_two_samples_in_one_iteration_sum_the_single_frame_references(rig, monkeypatch):
    """[truncated, all_hit] as B = 2 at T = 1500 on the chain path, p = 0: the per-sample offsets of dK | dV and of the
    tape at the largest T.  The gradients are the sum of the two single-frame fp64 references, under the same bound."""
    frames = ['truncated', 'all_hit']
    run = _step(rig, 'chain', frames, 0.0, monkeypatch, [5, 6])
    refs = [_reference(rig, f, 0.0, None, cot, keep) for f, cot, keep in zip(frames, (5, 6), run['keep'])]
    g32 = {n: refs[0][1][n] + refs[1][1][n] for n in refs[0][1]}
    g64 = {n: refs[0][2][n] + refs[1][2][n] for n in refs[0][2]}
    for f, line in zip(frames, run['lines']):
        print('two samples, %s: %s' % (f, line))
    _check_gradients(run['grads'], g32, g64, 'stack backward, [truncated, all_hit] in one iteration, chain')


# --------------------------------------------------------------------------
# d. deterministic mode
# --------------------------------------------------------------------------
def test_deterministic_backward_on_the_all_hit_frame(rig, monkeypatch):
    """all_hit with p = 0.1: two deterministic runs are bit-identical, within 2e-6 of their scale of the atomic run
    (the criterion of test_deterministic_backward_is_bit_identical_on_any_schedule), and hold (b)'s bound."""
    runs = [_step(rig, path, ['all_hit'], 0.1, monkeypatch, [5]) for path in ('deterministic', 'deterministic', 'chain')]
    _, tr = _trainer(rig, 'deterministic')
    assert int(tr._shadow[:-8].abs().max()) == 0
    assert float(runs[0]['flat'].abs().max()) > 0 and torch.equal(runs[0]['flat'], runs[1]['flat'])
    assert all(np.array_equal(runs[0]['keep'][0], r['keep'][0]) for r in runs[1:])
    scale = float(runs[0]['flat'].abs().max())
    d = float((runs[0]['flat'] - runs[2]['flat']).abs().max())
    print('deterministic vs atomic backward, all_hit p=0.1: max|d| %.2e of a scale of %.2e' % (d, scale))
    assert d <= 2e-6 * scale, (d, scale)
    _, g32, g64 = _reference(rig, 'all_hit', 0.1, runs[0]['drop'], 5, runs[0]['keep'][0])
    _check_gradients(runs[0]['grads'], g32, g64, 'stack backward, all_hit p=0.1 deterministic')
