"""The two ends of the training iteration alone, at their edges, against fp64 (-m gpu).

The radar stack's forward and backward are compared with fp64 on the adverse frames (test_gpu_adverse_frame.py,
test_gpu_adverse_backward.py); the backward test is teacher-forced, so the kernels that PRODUCE its cotangents --
normalize_gt_kernel, match_cost_kernel, detr_loss_kernel (csrc/loss.hip) -- and the kernels that CONSUME the gradients --
sqnorm_kernel, adamw_kernel (csrc/train.hip) -- were seen only end to end on one benign fixture.  Here each is called
through its C entry point on seeded inputs (tests/loss_rig.py; anchored on the CPU by test_loss_rig_host.py) and compared
with the reference's own PyTorch formulation in fp64, fp32 torch on the same inputs being the measure of what fp32 costs:

    max|hip - ref64| <= 2 max|ref32 - ref64| + floor                                        (loss_rig.bound)

Both sides receive the same fp32 inputs and no element is excluded.  The floors of a to d were fixed before the first run and
have not changed; those of e were corrected once after it, see below.

* a. tc_normalize_bbox, n = 1 / 127 / 128 / 129, sizes 0.05 .. 30, yaw in [-4 pi, 4 pi] with 0 and fp32 +-pi/2:
  |hip - ref64| <= 2^-22 max(1, |v|) per element (4 ulp: device logf / sinf / cosf may be an ulp or two looser).
* b. tc_match_cost, 1 / 10 / 23 / 32 classes, code size 10 / 12, two parameter sets, logits N(0, 9) + uniform on
  [-40, 40] + planted +-90, +-104, +-0, +-17: `bound` per bin of the ground-truth class's |logit| ([0, 8), [8, 14),
  [14, inf): `1 - p + eps` at p == 1 leaves fp64 by several units in fp32 whoever evaluates it) with floor 2e-5 x the
  bin's maximum; all finite; exactly 0 beyond a sample's count; scipy's assignment on the device's lowest-bin costs,
  priced in fp64, within G x that bin's bound of the fp64 optimum.
* c. tc_detr_loss_fwd_bwd / tc_detr_loss_fwd_bwd_counts with a GIVEN random partial matching (one sample unmatched, one
  without boxes), 1 / 15 / 16 / 17 / 32 classes, code size 10 / 12, gamma 2 / 1.5, a code weight of 0, fractional and
  unequal normalisers, raw counts 0 / 0.5 / 33, `losses +=`, matched classes on saturated logits, pred == target elements
  (gradient exactly 0), sentinel-filled outputs (every element written; columns >= 10 and unmatched rows of d_box
  exactly 0), NaN / inf targets (rows dropped, normaliser and classification side unchanged).  Losses: floor
  2e-5 max(1, |ref|); d_cls: per |logit| bin, 2e-5 x bin maximum; d_box: 2e-5 x maximum.
* d. tc_sq_norm, n = 1 / 3 / 4 / 5 / 1023 / 262 147 / 1 048 579, 16-byte aligned and offset by one float (the scalar
  branch), |g| from 1e-4 to 1e3: every slot within K 2^-24 (relative; non-negative terms) of the fp64 sum over the
  elements its workgroup owns, K = the fp32 roundings on the longest path (`sq_roundings`: <= 37, 2.2e-6;
  test_adamw_step_matches_torch asks 1e-3 of the sum); a second call adds to the slots bit for bit.
* e. tc_adamw_step, six steps, p / m / v after every step: |p0| ~ 1e-3 with lr 2e-4 (and |p0| ~ 1, lr 0.1, weight decay
  0.5), gradient scales 1, 0.01, 1, 0, 1e-6, 30 (clipped and unclipped steps alternate), grad_scale 1 / 0.5, max_norm
  35 / 0 / 35 without sq_norm, n = 1 / 255 / 256 / 257 / 100 003 / 524 293, a start at step 100 000.  ref32 is
  torch.optim.AdamW + clip_grad_norm_; floors k 2^-24 max|x| with the per-step counts of `adam_roundings` (p 11, m 4, v 5)
  and max|x| taken over the steps so far: p, m and v are state, a rounding is relative to the operand it rounds
  (b1 m_prev, not a sum that cancellation made smaller), and with one element the tensor's maximum is that sum.  The first
  run used the current step's maximum alone (and counted the clip coefficient's roundings, since dropped: a tighter floor),
  and one n = 1 case missed m by 0.3 % at step 5 after |m| had fallen 20-fold; the running maximum is the one widening made
  to a floor after a run.

Every test prints its figures, and the module its worst figures per test when it is done (pytest -s).
Report of one run on an MI355X: the lines the module prints last.  Per test and figure, the case with the largest |d| of
HIP against its bound; hip / fp32 torch are max|d| against fp64 (normalize: in units of its floor; sq_norm: relative, and
there is no fp32 side).  The loss sums meet in float atomics (torch: a threaded fp32 sum), so their last digits differ from
run to run; everything else repeats.  At saturation ([14, inf)) both fp32 cost formulas leave fp64 by the same 16 units
(`1 - p + eps` at p == 1); the assignment on the device's lowest-bin costs was the fp64 optimum in every case.
The one finding: launch_adamw formed the bias corrections in float; 1 - powf(b2, step) was off by 5e-6 of itself at step 2,
2.5e-6 of the update, and showed on a single parameter (adam-small-n1-gs1-mn35, step 2: p 4.59e-10 / 6.57e-12 against a
bound of 1.83e-10).  They are formed in double now, as torch forms them; the figures below are from after that.
  worst figures per test: max|d| hip / torch fp32 (<= bound) in the case named
  adamw      m                  6.65e-09 / 5.32e-09 (<= 2.24e-08) adam-late-n100003-gs0.5-mn35 step 100001
  adamw      p                  1.75e-09 / 1.49e-09 (<= 6.14e-09) adam-small-n100003-gs1-mn0 step 6
  adamw      v                  8.63e-09 / 3.78e-09 (<= 1.94e-08) adam-small-n256-gs1-mn35 step 6
  cost       |x| in [0,8)       3.40e-04 / 3.40e-04 (<= 1.78e-03) cost-b2q130-c10-k10-s0
  cost       |x| in [14,inf)    1.64e+01 / 1.64e+01 (<= 3.29e+01) cost-b3q37-c32-k10-s0
  cost       |x| in [8,14)      9.65e-02 / 9.65e-02 (<= 1.94e-01) cost-b3q37-c23-k12-s0
  loss       d_box              2.87e-09 / 2.87e-09 (<= 5.01e-06) loss-b3q37-c1-k10-s0 avg given
  loss       d_cls [0,8)        1.71e-06 / 1.47e-06 (<= 3.68e-05) loss-b2q130-c32-k10-s0 counts, +=
  loss       d_cls [14,inf)     2.69e-06 / 2.70e-06 (<= 3.54e-05) loss-b3q37-c17-k12-s0-nf NaN / inf targets, counts
  loss       d_cls [8,14)       2.27e-06 / 2.13e-06 (<= 3.44e-05) loss-b3q37-c32-k10-s0 avg given
  loss       loss_bbox          2.64e-06 / 1.18e-06 (<= 3.52e-04) loss-b3q37-c15-k10-s0 counts, +=
  loss       loss_cls           1.12e-04 / 2.07e-05 (<= 8.69e-03) loss-b2q130-c16-k12-s1 counts, +=
  normalize  log                6.99e-01 / 2.99e-01 (<= 1.00e+00) norm-n129
  normalize  sin/cos            2.09e-01 / 1.42e-01 (<= 1.00e+00) norm-n128
  sq_norm    slot (relative)    1.64e-07 / 0.00e+00 (<= 1.85e-06) sq-n262147-offset
  sq_norm    sum (relative)     6.88e-08 / 0.00e+00 (<= 1.73e-06) sq-n3-offset
"""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import loss_rig as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                     # fp32 unit roundoff
SENTINEL = -7777.0


@pytest.fixture(scope='module')
def lib():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    return transcar_amd.lib()


def dev():
    return torch.device('cuda:0')


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def call(rc, what):
    from transcar_amd import _lib as L
    L.check(rc, what)


def stream():
    from transcar_amd import _lib as L
    return L.stream_ptr()


case_of = functools.lru_cache(maxsize=None)(R.make_case)

WORST = {}                         # (test, figure) -> (hip, torch fp32, bound or None, case): the largest hip / bound seen


def note(test, figure, hip, ref32, limit, case):
    """Keeps, per figure of a test, the case with the largest |d| of HIP (relative to its bound where there is one)."""
    key = (test, figure)
    rank = hip / limit if limit else hip
    if key not in WORST or rank > WORST[key][0]:
        WORST[key] = (rank, hip, ref32, limit, case)


@pytest.fixture(scope='module', autouse=True)
def worst_figures():
    """When the module is done: per test and figure the worst case, HIP / fp32 torch against fp64 -- the lines of the
    report in the module docstring."""
    yield
    print('\n  worst figures per test: max|d| hip / torch fp32 (<= bound) in the case named')
    for (test, figure), (_, hip, ref32, limit, case) in sorted(WORST.items()):
        print('  %-10s %-18s %.2e / %.2e %s %s' % (test, figure, hip, ref32, '(<= %.2e)' % limit if limit else ' ' * 13, case))


def t64(a):
    return torch.from_numpy(np.asarray(a)).double()


# --------------------------------------------------------------------------------------------------------------------
# a. tc_normalize_bbox
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.NORMALIZE_CASES)
def test_normalize_bbox_against_fp64(lib, name):
    c = case_of(name)
    n = c['n']
    out = torch.full((n + 1, 10), SENTINEL, device=dev())
    gt9 = up(c['gt9'])
    call(lib.tc_normalize_bbox(gt9.data_ptr(), n, out.data_ptr(), stream()), 'tc_normalize_bbox')
    got = out.cpu().numpy().astype(np.float64)
    assert (got[n] == SENTINEL).all()                                        # nothing behind the last box
    ref64 = R.normalize(t64(c['gt9'])).numpy()
    ref32 = R.normalize(torch.from_numpy(c['gt9'])).numpy().astype(np.float64)
    floor = 2.0 ** -22 * np.maximum(1.0, np.abs(ref64))
    e_hip, e_32 = np.abs(got[:n] - ref64) / floor, np.abs(ref32 - ref64) / floor
    groups = (('copy', [0, 1, 4, 8, 9]), ('log', [2, 3, 5]), ('sin/cos', [6, 7]))
    print('\n  %s: |d| / (2^-22 max(1,|v|)), hip / torch fp32: ' % name +
          '  '.join('%s %.3f / %.3f' % (k, e_hip[:, j].max(), e_32[:, j].max()) for k, j in groups))
    for k, j in groups[1:]:                                                  # (in units of the floor)
        note('normalize', k, e_hip[:, j].max(), e_32[:, j].max(), 1.0, name)
    assert np.array_equal(got[:n][:, [0, 1, 4, 8, 9]], c['gt9'][:, [0, 1, 2, 7, 8]].astype(np.float64))
    assert (e_hip <= 1.0).all(), float(e_hip.max())


# --------------------------------------------------------------------------------------------------------------------
# b. tc_match_cost
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.COST_CASES)
def test_match_cost_against_fp64(lib, name):
    c = case_of(name)
    B, Q, ncls, code = c['B'], c['Q'], c['ncls'], c['code']
    cost = torch.full((R.LYR, B, Q, R.GMAX), SENTINEL, device=dev())
    d = {k: up(c[k]) for k in ('cls', 'box', 'gtn', 'labels', 'counts')}        # (alive until the results are read)
    call(lib.tc_match_cost(d['cls'].data_ptr(), d['box'].data_ptr(), R.LYR, B, Q, ncls, code,
                           d['gtn'].data_ptr(), d['labels'].data_ptr(), d['counts'].data_ptr(), R.GMAX,
                           c['w_cls'], c['w_box'], c['alpha'], c['gamma'], c['eps'], cost.data_ptr(), stream()),
         'tc_match_cost')
    got = cost.cpu().numpy().astype(np.float64)
    args = (c['counts'], c['w_cls'], c['w_box'], c['alpha'], c['gamma'], c['eps'])
    lab = torch.from_numpy(c['labels'])
    ref64 = R.match_cost(t64(c['cls']), t64(c['box']), t64(c['gtn']), lab, *args).numpy()
    ref32 = R.match_cost(*(torch.from_numpy(c[k]) for k in ('cls', 'box', 'gtn')), lab, *args).numpy().astype(np.float64)
    assert np.isfinite(got).all()
    valid = np.zeros(got.shape, dtype=bool)
    for b in range(B):
        valid[:, b, :, :c['counts'][b]] = True
    assert (got[~valid] == 0).all()                                          # exactly 0 beyond a sample's count
    # the logit each entry was made from: x[l, b, q, labels[b, g]]
    x = np.take_along_axis(c['cls'], np.broadcast_to(c['labels'][None, :, None, :].astype(np.int64),
                                                     (R.LYR, B, Q, R.GMAX)), axis=3)
    ok, rows = R.bound_per_bin(got[valid], ref32[valid], ref64[valid], x[valid], 2e-5)
    print('\n  %s: max|d| hip / torch fp32: %s' % (name, R.fmt_bins(rows)))
    for (lo, hi), cnt, a, b32, lim in rows:
        note('cost', '|x| in [%g,%g)' % (lo, hi), a, b32, lim, name)
    assert ok, rows
    # the assignment on the device's lowest-bin costs (the other entries: fp64 on both sides), priced in fp64
    low = valid & (np.abs(x) < R.LOGIT_BINS[0][1])
    mixed = np.where(low, got, ref64)
    limit_low = rows[0][4]
    worst = 0.0
    for l in range(R.LYR):
        for b in range(B):
            G = int(c['counts'][b])
            if G:
                r_d, c_d = linear_sum_assignment(mixed[l, b, :, :G])
                r_o, c_o = linear_sum_assignment(ref64[l, b, :, :G])
                excess = ref64[l, b, r_d, c_d].sum() - ref64[l, b, r_o, c_o].sum()
                worst = max(worst, excess / (G * limit_low) if limit_low > 0 else 0.0)
                assert excess <= G * limit_low, (l, b, excess, G * limit_low)
    print('      assignment on the device costs: at most %.3g of G x bound above the fp64 optimum' % worst)


# --------------------------------------------------------------------------------------------------------------------
# c. tc_detr_loss_fwd_bwd / tc_detr_loss_fwd_bwd_counts
# --------------------------------------------------------------------------------------------------------------------
AVG_GIVEN = [[7.5, 3.25], [1.0, 33.0], [12.75, 1.0]]          # fractional (rank-averaged), cls and box columns differ
AVG_COUNTS = [[0.0, 33.0], [0.5, 0.0], [33.0, 0.5]]           # raw counts: the kernel clamps at 1
LOSS_START = [[0.5, -0.25], [1.0, 2.0], [0.125, 0.0]]


def device_loss(lib, c, avg, counts_entry, start=None):
    B, Q, ncls, code = c['B'], c['Q'], c['ncls'], c['code']
    d_cls = torch.full((R.LYR, B, Q, ncls), SENTINEL, device=dev())
    d_box = torch.full((R.LYR, B, Q, code), SENTINEL, device=dev())
    losses = up(np.asarray(start if start is not None else np.zeros((R.LYR, 2)), dtype=np.float32))
    fn = lib.tc_detr_loss_fwd_bwd_counts if counts_entry else lib.tc_detr_loss_fwd_bwd
    d = {k: up(c[k]) for k in ('cls', 'box', 'gtn', 'labels', 'assigned', 'code_w')}     # (alive until the results are read)
    d['avg'] = up(np.asarray(avg, dtype=np.float32))
    call(fn(d['cls'].data_ptr(), d['box'].data_ptr(), R.LYR, B, Q, ncls, code, d['gtn'].data_ptr(),
            d['labels'].data_ptr(), R.GMAX, d['assigned'].data_ptr(), d['avg'].data_ptr(),
            d['code_w'].data_ptr(), c['alpha'], c['gamma'], c['w_cls'], c['w_box'], losses.data_ptr(),
            d_cls.data_ptr(), d_box.data_ptr(), stream()), 'tc_detr_loss')
    return losses.cpu().numpy(), d_cls.cpu().numpy(), d_box.cpu().numpy()


def check_loss_outputs(c, got, avg, tag, start=None):
    """The three outputs of one launch against loss_rig.loss_and_gradients in fp64 / fp32; prints the figures."""
    losses, d_cls, d_box = got
    l32, c32, b32 = R.loss_and_gradients(c, avg, torch.float32)
    l64, c64, b64 = R.loss_and_gradients(c, avg, torch.float64)
    assert (d_cls != SENTINEL).all() and (d_box != SENTINEL).all()           # every element written
    assert (d_box[..., 10:] == 0).all() and (d_box[c['assigned'] < 0] == 0).all()
    for l, b, q, j in c['planted_equal']:
        assert d_box[l, b, q, j] == 0, (l, b, q, j)
    for l, b, q in c['nonfinite_rows']:
        assert (d_box[l, b, q] == 0).all(), (l, b, q)
    s = np.asarray(start if start is not None else np.zeros((R.LYR, 2)), dtype=np.float64)
    worst = (0.0, 0.0)
    for l in range(R.LYR):
        for j in range(2):
            ok, fig = R.bound(losses[l, j], s[l, j] + np.float64(l32[l, j]), s[l, j] + l64[l, j],
                              2e-5 * max(1.0, abs(l64[l, j])))
            worst = max(worst, (fig[0] / max(1.0, abs(l64[l, j])), fig[1] / max(1.0, abs(l64[l, j]))))
            note('loss', 'loss_cls' if j == 0 else 'loss_bbox', fig[0], fig[1], fig[2], c['name'] + ' ' + tag)
            assert ok, ('loss', l, j, float(losses[l, j]), float(s[l, j] + l64[l, j]), fig)
    ok_c, rows = R.bound_per_bin(d_cls.astype(np.float64), c32.astype(np.float64), c64, c['cls'], 2e-5)
    ok_b, fig_b = R.bound(d_box, b32, b64, 2e-5 * float(np.abs(b64).max()))
    print('\n  %s %s: losses (rel) %.2e / %.2e;  d_box %.2e / %.2e (max %.2e);  d_cls %s' % (
        c['name'], tag, worst[0], worst[1], fig_b[0], fig_b[1], float(np.abs(b64).max()), R.fmt_bins(rows)))
    for (lo, hi), cnt, a, b32, lim in rows:
        note('loss', 'd_cls [%g,%g)' % (lo, hi), a, b32, lim, c['name'] + ' ' + tag)
    note('loss', 'd_box', fig_b[0], fig_b[1], fig_b[2], c['name'] + ' ' + tag)
    assert ok_c, rows
    assert ok_b, fig_b


@pytest.mark.parametrize('name', R.LOSS_CASES)
def test_detr_loss_given_assignment_against_fp64(lib, name):
    c = case_of(name)
    check_loss_outputs(c, device_loss(lib, c, AVG_GIVEN, False), AVG_GIVEN, 'avg given')
    # raw counts 0 / 0.5 / 33 clamp to 1 / 1 / 33; `losses` is added to
    clamped = np.maximum(np.asarray(AVG_COUNTS), 1.0).tolist()
    check_loss_outputs(c, device_loss(lib, c, AVG_COUNTS, True, LOSS_START), clamped, 'counts, +=', LOSS_START)


@pytest.mark.parametrize('name', R.NONFINITE_CASES)
def test_detr_loss_drops_rows_with_non_finite_targets(lib, name):
    c = case_of(name)
    assert len(c['nonfinite_rows']) == 2 * R.LYR and not np.isfinite(c['gtn']).all()
    got = device_loss(lib, c, AVG_GIVEN, False)
    check_loss_outputs(c, got, AVG_GIVEN, 'NaN / inf targets')             # the reference's filter, same normaliser
    clean = device_loss(lib, c['clean'], AVG_GIVEN, False)
    assert np.array_equal(got[1], clean[1])                                  # the classification side: bit for bit
    assert np.abs(got[0][:, 0] - clean[0][:, 0]).max() <= 32 * U * np.abs(clean[0][:, 0]).max()     # (float atomics)
    assert (got[0][:, 1] < clean[0][:, 1]).all() and np.isfinite(got[0]).all()
    keep = np.ones(c['assigned'].shape, dtype=bool)
    for l, b, q in c['nonfinite_rows']:
        keep[l, b, q] = False
    assert np.array_equal(got[2][keep], clean[2][keep])                      # every other row of d_box: bit for bit
    got_c = device_loss(lib, c, AVG_COUNTS, True)
    check_loss_outputs(c, got_c, np.maximum(np.asarray(AVG_COUNTS), 1.0).tolist(), 'NaN / inf targets, counts')


# --------------------------------------------------------------------------------------------------------------------
# d. tc_sq_norm
# --------------------------------------------------------------------------------------------------------------------
SQ_THREADS, SQ_BLOCKS = 1024, 256                    # sqnorm_kernel: 256 workgroups of 1024 threads, grid stride


def sq_roundings(n, vec):
    """fp32 roundings on the longest path from an element to its slot in sqnorm_kernel:
    a 16-byte trip: square, pair add, quad add, add to the thread's sum = 4;  a scalar trip: square, add = 2;
    then the wave tree (6 DPP adds), the 16 wave partials added in turn (16), `out[b] += t` (1), and 4 of margin.  The
    slots are added up in fp64 here."""
    stride = SQ_THREADS * SQ_BLOCKS
    n4 = n // 4 if vec else 0
    trips = 4 * -(-n4 // stride) + 2 * -(-(n - 4 * n4) // stride)
    return trips + 6 + 16 + 1 + 4


def sq_owner_sums(g, vec):
    """fp64 sum of squares over the elements each workgroup owns."""
    n = len(g)
    n4 = n // 4 if vec else 0
    i = np.arange(n)
    block = np.where(i < 4 * n4, (i // 4) // SQ_THREADS, (i - 4 * n4) // SQ_THREADS) % SQ_BLOCKS
    return np.bincount(block, weights=g.astype(np.float64) ** 2, minlength=SQ_BLOCKS)


@pytest.mark.parametrize('name', R.SQNORM_CASES)
def test_sq_norm_against_fp64(lib, name):
    c = case_of(name)
    n, off = c['n'], c['offset']
    buf = torch.zeros(n + 8, device=dev())
    g = buf[off:off + n]
    g.copy_(torch.from_numpy(c['g']))
    vec = g.data_ptr() % 16 == 0
    assert vec == (off == 0)
    out = torch.zeros(SQ_BLOCKS + 1, device=dev())
    out[SQ_BLOCKS] = SENTINEL
    call(lib.tc_sq_norm(g.data_ptr(), n, out.data_ptr(), stream()), 'tc_sq_norm')
    first = out.cpu().numpy()
    assert first[SQ_BLOCKS] == np.float32(SENTINEL)
    want = sq_owner_sums(c['g'], vec)
    K = sq_roundings(n, vec)
    err = np.abs(first[:SQ_BLOCKS].astype(np.float64) - want)
    assert (first[:SQ_BLOCKS][want == 0] == 0).all()                         # a workgroup without elements adds nothing
    rel = float((err[want > 0] / want[want > 0]).max())
    total = abs(first[:SQ_BLOCKS].astype(np.float64).sum() - want.sum()) / want.sum()
    print('\n  %s: %d slots in use, worst slot %.2e, sum %.2e relative (<= %d x 2^-24 = %.2e)' % (
        name, int((want > 0).sum()), rel, total, K, K * U))
    note('sq_norm', 'slot (relative)', rel, 0.0, K * U, name)
    note('sq_norm', 'sum (relative)', total, 0.0, K * U, name)
    assert rel <= K * U and total <= K * U
    # a second call adds to what the slots hold, slot by slot
    start = np.random.RandomState(n + off).uniform(0.5, 2.0, SQ_BLOCKS).astype(np.float32)
    out[:SQ_BLOCKS] = torch.from_numpy(start)
    call(lib.tc_sq_norm(g.data_ptr(), n, out.data_ptr(), stream()), 'tc_sq_norm')
    second = out.cpu().numpy()
    assert np.array_equal(second[:SQ_BLOCKS], start + first[:SQ_BLOCKS]) and second[SQ_BLOCKS] == np.float32(SENTINEL)


# --------------------------------------------------------------------------------------------------------------------
# e. tc_adamw_step
# --------------------------------------------------------------------------------------------------------------------
def adam_roundings():
    """fp32 roundings per step in adamw_kernel's expressions (k of the floors k 2^-24 max|x|):
      g     a.g * coef: 1 (coef is grad_scale, or grad_scale times the clip coefficient)
      m     (1 - b1) * g, b1 * m, the add: 3, and g's: 4   (1 - b1 and 1 - b2 are exact for a beta in [0.5, 1])
      v     (1 - b2) * g, * g, b2 * v, the add: 4, and g's: 5
      p     lr * wd, 1 - that, pv *=, sqrtf(v), sqrtf(bc2), their quotient, + eps, m / denom, lr / bc1, the product,
            the subtraction: 11
    The clip coefficient's own roundings (the slots of tc_sq_norm, their add-up, the square root and the division) are
    not counted: fp32 torch forms its norm with roundings of its own, which the 2 max|ref32 - ref64| term carries.
    max|x| is the largest over the steps so far (for p: p0 included): p, m and v are state, and a rounding is relative
    to the operand it rounds -- b1 m_prev -- not to a sum that cancellation made smaller."""
    return dict(p=11, m=4, v=5)


@pytest.mark.parametrize('name', R.ADAM_CASES)
def test_adamw_steps_against_fp64(lib, name):
    c = case_of(name)
    n, kw = c['n'], R.adam_args(c)
    ref64 = R.adamw_reference(c['p0'], c['grads'], dtype=np.float64, **kw)
    ref32 = R.adamw_torch32(c['p0'], c['grads'], **kw)
    p = up(c['p0'].copy())
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    K = adam_roundings()
    scale = dict(p=float(np.abs(c['p0']).max()), m=0.0, v=0.0)
    lines, failed = [], []
    for k, g in enumerate(c['grads']):
        gd = up(g)
        sq = torch.zeros(SQ_BLOCKS, device=dev())
        call(lib.tc_sq_norm(gd.data_ptr(), n, sq.data_ptr(), stream()), 'tc_sq_norm')
        call(lib.tc_adamw_step(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, c['lr'], c['b1'], c['b2'],
                               c['eps'], c['wd'], c['step0'] + k, c['grad_scale'], c['max_norm'],
                               sq.data_ptr() if c['clip'] else None, stream()), 'tc_adamw_step')
        norm = float(np.linalg.norm(g.astype(np.float64) * c['grad_scale']))
        clip = c['clip'] and c['max_norm'] > 0 and c['max_norm'] / (norm + 1e-6) < 1
        got = dict(p=p.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())
        figs = []
        for j, key in enumerate('pmv'):
            scale[key] = max(scale[key], float(np.abs(ref64[k][j]).max()))
            ok, fig = R.bound(got[key], ref32[k][j], ref64[k][j], K[key] * U * scale[key])
            figs.append((key, fig))
            note('adamw', key, fig[0], fig[1], fig[2], '%s step %d' % (name, c['step0'] + k))
            if not ok:
                failed.append((name, c['step0'] + k, key, fig, scale[key]))
        lines.append('    step %d%s: ' % (c['step0'] + k, ' (clip)' if clip else '') +
                     '  '.join('%s %.2e / %.2e (<= %.2e)' % ((key,) + f) for key, f in figs))
    print('\n  %s: max|d| hip / torch fp32\n%s' % (name, '\n'.join(lines)))
    assert not failed, failed
