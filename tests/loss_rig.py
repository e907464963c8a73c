"""Reference side of the loss / match-cost / optimizer kernel tests (test_loss_rig_host.py on the CPU,
test_gpu_loss_kernels.py on the MI355X).  No fixtures, no GPU.

Every reference is the project's own host formulation (transcar_amd.losses, transcar_amd.bbox_util: the reference's
PyTorch ops) or plain numpy, written once and evaluated in the dtype of its inputs: fp64 is the yardstick, fp32 the
measure of what fp32 arithmetic costs on the same inputs.  The check of a kernel output is `bound`:

    max|hip - ref64| <= 2 max|ref32 - ref64| + floor

Scalar parameters (alpha, gamma, eps, the weights, the optimizer's lr / betas / eps / weight decay) are rounded to fp32
first (`f32`), so that the kernels -- which take them as C floats -- and both references see the same numbers.
"""
import math

import numpy as np
import torch

from transcar_amd import losses
from transcar_amd.bbox_util import normalize_bbox

LYR = 3
GMAX = 24
SHAPES = {'b3q37': (3, 37, (24, 8, 0)), 'b2q130': (2, 130, (24, 1))}
#: (alpha, gamma, eps of the cost, cls weight, box weight): the configs' cost / loss parameters and one other set
PARAM_SETS = {'s0': (0.25, 2.0, 1e-12, 2.0, 0.25), 's1': (0.4, 1.5, 1e-12, 1.0, 0.5)}
#: the configs' code weights and a vector with a zero entry
CODE_WEIGHTS = {'s0': [1.0] * 8 + [0.2] * 2, 's1': [1.0, 1.0, 0.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.2, 0.2]}
PLANTED_LOGITS = (90.0, -90.0, 104.0, -104.0, 0.0, -0.0, 17.0, -17.0)
LOGIT_BINS = ((0.0, 8.0), (8.0, 14.0), (14.0, float('inf')))

COST_CASES = ['cost-%s-c%d-k%d-%s' % (s, c, k, ps) for s in SHAPES for c in (1, 10, 23, 32) for k in (10, 12)
              for ps in PARAM_SETS]
LOSS_CASES = ['loss-%s-c%d-k%d-%s' % (s, c, k, ps) for s in SHAPES for c in (1, 15, 16, 17, 32) for k in (10, 12)
              for ps in PARAM_SETS]
NONFINITE_CASES = ['loss-b3q37-c17-k12-s0-nf', 'loss-b2q130-c10-k10-s1-nf']
NORMALIZE_CASES = ['norm-n%d' % n for n in (1, 127, 128, 129)]
SQNORM_CASES = ['sq-n%d-%s' % (n, a) for n in (1, 3, 4, 5, 1023, 262147, 1048579) for a in ('aligned', 'offset')]
ADAM_SIZES = (1, 255, 256, 257, 100003, 524288 + 5)
ADAM_CASES = (['adam-small-n%d-gs%s-mn%d' % (n, gs, mn) for n in ADAM_SIZES for gs in ('1', '0.5') for mn in (35, 0)] +
              ['adam-small-n100003-gs0.5-mn35-nosq', 'adam-late-n100003-gs0.5-mn35', 'adam-late-n257-gs1-mn0',
               'adam-decay-n100003-gs1-mn35', 'adam-decay-n100003-gs0.5-mn0', 'adam-decay-n257-gs1-mn35'])
ADAM_GRAD_SCALES = (1.0, 0.01, 1.0, 0.0, 1e-6, 30.0)


def f32(x):
    """A Python float that fp32 holds exactly: what a kernel receives through a C float argument."""
    return float(np.float32(x))


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31)


# --------------------------------------------------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------------------------------------------------
def normalize(gt9):
    """UTIL:4-24 on [..., 9] boxes, in the dtype of `gt9`."""
    return normalize_bbox(gt9)


def match_cost(cls, box, gtn, labels, counts, w_cls=2.0, w_reg=0.25, alpha=0.25, gamma=2.0, eps=1e-12):
    """-> [Lyr, B, Q, Gmax]: FocalLossCost + BBox3DL1Cost of every (query, ground-truth box) pair as the assigner forms
    them (ASSIGN:106-116), 0 beyond a sample's count as tc_match_cost writes it.  cls [Lyr,B,Q,ncls],
    box [Lyr,B,Q,code], gtn [B,Gmax,10] (normalised boxes), labels [B,Gmax] (long), counts: B ints."""
    Lyr, B, Q, _ = cls.shape
    out = torch.zeros((Lyr, B, Q, gtn.shape[1]), dtype=cls.dtype)
    cls_cost, reg_cost = losses.FocalLossCost(w_cls, alpha, gamma, eps), losses.BBox3DL1Cost(w_reg)
    for l in range(Lyr):
        for b in range(B):
            n = int(counts[b])
            if n:
                out[l, b, :, :n] = cls_cost(cls[l, b], labels[b, :n].long()) + reg_cost(box[l, b, :, :10], gtn[b, :n, :10])
    return out


def loss_given_assignment(cls, box, gtn, labels, assigned, avg, code_w, alpha, gamma, w_cls, w_box):
    """-> [Lyr, 2] (loss_cls, loss_bbox per level): Detr3DHead.loss_single (HEAD:849-917) with the assignment GIVEN.
    assigned [Lyr,B,Q]: index of the matched ground-truth box or -1; avg [Lyr,2]: the (cls, box) normalisers as they
    divide.  Labels, targets and weights as the head builds them: the background label num_classes for -1, the batch
    flattened, box weights 1 on matched rows times the code weights, rows whose target is not finite dropped
    (`isfinite(...).all(-1)`).  Differentiable in cls / box."""
    Lyr, B, Q, ncls = cls.shape
    code = box.shape[-1]
    assigned = torch.as_tensor(assigned).long()
    labels = torch.as_tensor(labels).long()
    cw = torch.as_tensor(code_w, dtype=cls.dtype)
    out = []
    for l in range(Lyr):
        a = assigned[l]                                               # [B, Q]
        pos = a >= 0
        lab = torch.full((B, Q), ncls, dtype=torch.long)
        tgt = torch.zeros((B, Q, 10), dtype=cls.dtype)
        for b in range(B):
            lab[b, pos[b]] = labels[b, a[b, pos[b]]]
            tgt[b, pos[b]] = gtn[b, a[b, pos[b]], :10]
        w = torch.zeros((B, Q, 10), dtype=cls.dtype)
        w[pos] = 1.0
        lab, tgt, w = lab.reshape(-1), tgt.reshape(-1, 10), w.reshape(-1, 10) * cw
        loss_cls = losses.sigmoid_focal_loss(cls[l].reshape(-1, ncls), lab, torch.ones(B * Q, dtype=cls.dtype),
                                             gamma=gamma, alpha=alpha, avg_factor=avg[l][0], loss_weight=w_cls)
        ok = torch.isfinite(tgt).all(dim=-1)
        pred = box[l].reshape(-1, code)
        loss_box = losses.l1_loss(pred[ok, :10], tgt[ok], w[ok], avg_factor=avg[l][1], loss_weight=w_box)
        out.append(torch.stack((loss_cls, loss_box)))
    return torch.stack(out)


def loss_and_gradients(case, avg, dtype):
    """loss_given_assignment on a `make_case('loss-...')` dict in `dtype` + autograd of the summed loss.
    -> (losses [Lyr,2], d_cls, d_box) as numpy arrays of `dtype`."""
    cls = torch.from_numpy(case['cls']).to(dtype).requires_grad_(True)
    box = torch.from_numpy(case['box']).to(dtype).requires_grad_(True)
    gtn = torch.from_numpy(case['gtn']).to(dtype)
    avg_t = torch.as_tensor(np.asarray(avg), dtype=dtype)
    out = loss_given_assignment(cls, box, gtn, case['labels'], case['assigned'], avg_t, case['code_w'], case['alpha'],
                                case['gamma'], case['w_cls'], case['w_box'])
    out.sum().backward()
    d_box = box.grad if box.grad is not None else torch.zeros_like(box)
    return out.detach().numpy(), cls.grad.numpy(), d_box.numpy()


def adamw_reference(p, g_list, lr, b1, b2, eps, wd, step0=1, grad_scale=1.0, max_norm=0.0, clip=True,
                    dtype=np.float64):
    """torch.optim.AdamW (decoupled weight decay, bias corrections from Python floats) behind mmcv's gradient clip
    (coef = max_norm / (norm + 1e-6), applied when below 1), `grad_scale` applied to the gradient first; plain numpy in
    `dtype`.  g_list: one gradient per step, the first at step number `step0`.  -> [(p, m, v) after every step]."""
    dt = np.dtype(dtype).type
    p = np.asarray(p, dtype=dtype).copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for k, g in enumerate(g_list):
        step = step0 + k
        g = np.asarray(g, dtype=dtype) * dt(grad_scale)
        if clip and max_norm > 0:
            norm = dt(math.sqrt(float(np.sum(g.astype(np.float64) ** 2))))
            coef = dt(max_norm) / (norm + dt(1e-6))
            if coef < 1:
                g = g * coef
        bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
        p = p * dt(1.0 - lr * wd)
        m = dt(b1) * m + dt(1.0 - b1) * g
        v = dt(b2) * v + dt(1.0 - b2) * g * g
        denom = np.sqrt(v) / dt(math.sqrt(bc2)) + dt(eps)
        p = p - dt(lr / bc1) * (m / denom)
        out.append((p.copy(), m.copy(), v.copy()))
    return out


def adamw_torch32(p, g_list, lr, b1, b2, eps, wd, step0=1, grad_scale=1.0, max_norm=0.0, clip=True):
    """The same steps by torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ in fp32 -> [(p, m, v) after every step]."""
    par = torch.nn.Parameter(torch.from_numpy(np.asarray(p, dtype=np.float32).copy()))
    opt = torch.optim.AdamW([par], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    if step0 > 1:                         # a run that is `step0 - 1` steps old with zero moments
        par.grad = torch.zeros_like(par)
        saved = par.detach().clone()
        opt.step()
        with torch.no_grad():
            par.copy_(saved)
        st = opt.state[par]
        st['exp_avg'].zero_()
        st['exp_avg_sq'].zero_()
        st['step'] = torch.as_tensor(float(step0 - 1)) if torch.is_tensor(st['step']) else step0 - 1
    out = []
    for g in g_list:
        par.grad = torch.from_numpy(np.asarray(g, dtype=np.float32).copy()) * np.float32(grad_scale)
        if clip and max_norm > 0:
            torch.nn.utils.clip_grad_norm_([par], max_norm)
        opt.step()
        st = opt.state[par]
        out.append((par.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()))
    return out


def bound(hip, ref32, ref64, floor):
    """The check  max|hip - ref64| <= 2 max|ref32 - ref64| + floor.  -> (ok, (max|hip - ref64|, max|ref32 - ref64|,
    the right-hand side)); no element: (True, zeros).  A NaN on either side fails."""
    hip, ref32, ref64 = (np.asarray(x, dtype=np.float64).reshape(-1) for x in (hip, ref32, ref64))
    if ref64.size == 0:
        return True, (0.0, 0.0, float(floor))
    with np.errstate(invalid='ignore'):
        e_hip = float(np.max(np.abs(hip - ref64)))
        e_32 = float(np.max(np.abs(ref32 - ref64)))
    limit = 2.0 * e_32 + float(floor)
    return bool(e_hip <= limit), (e_hip, e_32, limit)


def bound_per_bin(hip, ref32, ref64, logit, rel_floor):
    """`bound` on the elements of each |logit| bin of LOGIT_BINS with floor = rel_floor * max|ref64| of the bin.
    -> (ok, [(bin, elements, max|hip - ref64|, max|ref32 - ref64|, right-hand side)])."""
    mag = np.abs(np.asarray(logit, dtype=np.float64))
    ok, rows = True, []
    for lo, hi in LOGIT_BINS:
        sel = (mag >= lo) & (mag < hi)
        n = int(sel.sum())
        floor = rel_floor * float(np.max(np.abs(ref64[sel]))) if n else 0.0
        good, fig = bound(hip[sel], ref32[sel], ref64[sel], floor)
        ok = ok and good
        rows.append(((lo, hi), n) + fig)
    return ok, rows


def fmt_bins(rows):
    return '  '.join('|x| in [%g,%g) n=%d: %.2e / %.2e (<= %.2e)' % (lo, hi, n, a, b, c) for (lo, hi), n, a, b, c in rows)


# --------------------------------------------------------------------------------------------------------------------
# seeded inputs
# --------------------------------------------------------------------------------------------------------------------
def _logits(rng, shape):
    """N(0, 3^2), uniform on [-40, 40] and the planted saturated / zero values, mixed element by element."""
    x = rng.standard_normal(shape) * 3.0
    kind = rng.uniform(size=shape)
    u = rng.uniform(-40.0, 40.0, shape)
    x = np.where(kind < 0.35, u, x)
    planted = np.asarray(PLANTED_LOGITS)[rng.randint(0, len(PLANTED_LOGITS), shape)]
    x = np.where(kind > 0.94, planted, x)
    return x.astype(np.float32)


def _ground_truth(rng, B, counts, ncls):
    """[B, GMAX, 9] boxes (ones beyond a sample's count, as device_loss.py pads), [B, GMAX] labels with class 0 and
    class ncls - 1 among them."""
    gt9 = np.ones((B, GMAX, 9), dtype=np.float32)
    labels = np.zeros((B, GMAX), dtype=np.int32)
    for b in range(B):
        n = counts[b]
        gt9[b, :n, 0:2] = rng.uniform(-50, 50, (n, 2))
        gt9[b, :n, 2] = rng.uniform(-2.5, 0.5, n)
        gt9[b, :n, 3:6] = np.exp(rng.normal(0.5, 0.3, (n, 3)))
        gt9[b, :n, 6] = rng.uniform(-np.pi, np.pi, n)
        gt9[b, :n, 7:9] = rng.normal(0, 2, (n, 2))
        labels[b, :n] = rng.randint(0, ncls, n)
        if n >= 2:
            labels[b, 0], labels[b, 1] = 0, ncls - 1
        elif n == 1:
            labels[b, 0] = ncls - 1
    return gt9, labels


BOX_SCALE = np.asarray([30, 30, 0.5, 0.5, 2, 0.5, 0.7, 0.7, 2, 2, 1, 1], dtype=np.float64)


def _head_case(name, shape, ncls, code, pset, nonfinite):
    rng = np.random.RandomState(_seed(name))
    B, Q, counts = SHAPES[shape]
    alpha, gamma, eps, w_cls, w_box = (f32(x) for x in PARAM_SETS[pset])
    cls = _logits(rng, (LYR, B, Q, ncls))
    box = (rng.standard_normal((LYR, B, Q, code)) * BOX_SCALE[:code]).astype(np.float32)
    gt9, labels = _ground_truth(rng, B, counts, ncls)
    gtn = normalize(torch.from_numpy(gt9)).numpy()
    # a random partial matching per (level, sample); one sample with boxes is left entirely unmatched on one level
    assigned = np.full((LYR, B, Q), -1, dtype=np.int32)
    for l in range(LYR):
        for b in range(B):
            n = min(counts[b], Q)
            if n == 0 or (b == 1 and l == 1):
                continue
            k = n if (l == 0 and b == 0) else rng.randint(1, n + 1)
            assigned[l, b, rng.permutation(Q)[:k]] = rng.permutation(counts[b])[:k]
    if nonfinite:                        # boxes 2 and 5 of sample 0 are matched on every level (see below)
        for l in range(LYR):
            for g in (2, 5):
                if not (assigned[l, 0] == g).any():
                    free = np.flatnonzero(assigned[l, 0] < 0)
                    assigned[l, 0, free[rng.randint(len(free))]] = g
    # the matched class on saturated logits of both signs, and pred == target elements (gradient exactly 0)
    planted_equal = []
    for l in range(LYR):
        for b in range(B):
            rows = np.flatnonzero(assigned[l, b] >= 0)
            for i, q in enumerate(rows[:8]):
                cls[l, b, q, labels[b, assigned[l, b, q]]] = PLANTED_LOGITS[(i + l) % len(PLANTED_LOGITS)]
            for i, q in enumerate(rows[:5]):
                j = (3 * i + l + b) % 10
                box[l, b, q, j] = gtn[b, assigned[l, b, q], j]
                planted_equal.append((l, b, int(q), j))
    case = dict(name=name, B=B, Q=Q, counts=np.asarray(counts, dtype=np.int32), ncls=ncls, code=code, cls=cls, box=box,
                gt9=gt9, gtn=gtn, labels=labels, assigned=assigned, alpha=alpha, gamma=gamma, eps=eps, w_cls=w_cls,
                w_box=w_box, code_w=np.asarray(CODE_WEIGHTS[pset], dtype=np.float32), planted_equal=planted_equal,
                nonfinite_rows=[])
    if nonfinite:
        clean = dict(case)
        gtn = gtn.copy()
        gtn[0, 2, 3] = np.nan
        gtn[0, 5, 7] = np.inf
        case['gtn'] = gtn
        case['clean'] = clean
        case['nonfinite_rows'] = [(l, 0, int(q)) for l in range(LYR) for q in np.flatnonzero(
            (assigned[l, 0] == 2) | (assigned[l, 0] == 5))]
    return case


def _normalize_case(name, n):
    rng = np.random.RandomState(_seed(name))
    gt9 = np.zeros((n, 9), dtype=np.float32)
    gt9[:, 0:2] = rng.uniform(-60, 60, (n, 2))
    gt9[:, 2] = rng.uniform(-5, 3, n)
    gt9[:, 3:6] = np.exp(rng.uniform(np.log(0.05), np.log(30.0), (n, 3)))      # sizes in [0.05, 30]
    gt9[:, 6] = rng.uniform(-4 * np.pi, 4 * np.pi, n)
    special = [0.0, np.float32(np.pi / 2), -np.float32(np.pi / 2)]
    for i in range(min(n, 3)):
        gt9[(i * 41) % n, 6] = special[i] if n > 1 else 0.0
    if n >= 2:
        gt9[0, 3], gt9[1 % n, 4] = 0.05, 30.0
    gt9[:, 7:9] = rng.normal(0, 3, (n, 2))
    return dict(name=name, n=n, gt9=gt9)


def _sqnorm_case(name, n, offset):
    rng = np.random.RandomState(_seed(name))
    mag = np.exp(rng.uniform(np.log(1e-4), np.log(1e3), n))                    # 1e-4 .. 1e3
    g = (mag * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)).astype(np.float32)
    return dict(name=name, n=n, offset=offset, g=g)


def _adam_case(name, cfg, n, grad_scale, max_norm, nosq):
    rng = np.random.RandomState(_seed(name))
    if cfg == 'decay':
        lr, wd, p0, step0 = 0.1, 0.5, rng.standard_normal(n), 1
    else:
        lr, wd, p0, step0 = 2e-4, 0.01, 1e-3 * rng.standard_normal(n), (100000 if cfg == 'late' else 1)
    # the gradient as the kernel receives it (a SUM over 1 / grad_scale ranks when grad_scale < 1)
    grads = [(rng.standard_normal(n) * s / grad_scale).astype(np.float32) for s in ADAM_GRAD_SCALES]
    return dict(name=name, n=n, p0=p0.astype(np.float32), grads=grads, lr=f32(lr), b1=f32(0.9), b2=f32(0.999),
                eps=f32(1e-8), wd=f32(wd), step0=step0, grad_scale=f32(grad_scale), max_norm=f32(max_norm),
                clip=not nosq)


def make_case(name):
    """The seeded inputs of one named case (COST_CASES, LOSS_CASES, NONFINITE_CASES, NORMALIZE_CASES, SQNORM_CASES,
    ADAM_CASES) as a dict of numpy arrays and Python scalars."""
    part = name.split('-')
    if part[0] in ('cost', 'loss'):
        return _head_case(name, part[1], int(part[2][1:]), int(part[3][1:]), part[4], nonfinite=name.endswith('-nf'))
    if part[0] == 'norm':
        return _normalize_case(name, int(part[1][1:]))
    if part[0] == 'sq':
        return _sqnorm_case(name, int(part[1][1:]), 1 if part[2] == 'offset' else 0)
    if part[0] == 'adam':
        return _adam_case(name, part[1], int(part[2][1:]), float(part[3][2:]), float(part[4][2:]), name.endswith('-nosq'))
    raise KeyError(name)


def adam_args(case):
    return dict(lr=case['lr'], b1=case['b1'], b2=case['b2'], eps=case['eps'], wd=case['wd'], step0=case['step0'],
                grad_scale=case['grad_scale'], max_norm=case['max_norm'], clip=case['clip'])
