"""The device Hungarian assignment beyond 1 024 queries / 128 boxes (tc_lsa_assign_ws, pytest -m gpu): equal to scipy
query for query up to 4 096 x 512, equal to the kernel for the small shapes wherever both apply (ties included), a
valid optimum where the costs tie, refusals before any launch, capturable, and the route `detr_loss_device` and
`FusionTrainer` now take for a 1 300-query head or a sample with 129 boxes."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from transcar_amd import _lib as L
from transcar_amd import configs, synth

pytestmark = pytest.mark.gpu

LYR = 3


def dev():
    return torch.device('cuda:0')


def make_costs(Q, G, B):
    """Random costs with a few cheap queries per box (as a trained head produces), ragged counts (one sample a third
    full, one empty) and zeros beyond a sample's count (as tc_match_cost writes them)."""
    rng = np.random.RandomState(Q * 131 + G)
    cost = rng.rand(LYR, B, Q, G).astype(np.float32) * 4.0
    for g in range(G):
        cost[:, :, (7 * g) % Q, g] *= 0.05
        cost[1, :, (7 * g + 3) % Q, g] *= 0.02
    counts = np.full(B, G, dtype=np.int32)
    if B > 1:
        counts[1] = max(0, G // 3)
    if B > 2:
        counts[2] = 0
    for b in range(B):
        cost[:, b, :, counts[b]:] = 0.0
    return cost, counts


def scipy_assign(cost, counts):
    _, B, Q, _ = cost.shape
    want = np.full((LYR, B, Q), -1, dtype=np.int32)
    for l in range(LYR):
        for b in range(B):
            if counts[b]:
                rows, cols = linear_sum_assignment(cost[l, b, :, :counts[b]])
                want[l, b, rows] = cols
    return want


class Problem:
    """The device buffers of one tc_lsa_assign_ws call; `run` fills them again and calls."""

    def __init__(self, cost, counts, ws_bytes=None):
        _, self.B, self.Q, self.G = cost.shape
        self.cost = torch.from_numpy(cost).to(dev())
        self.counts = torch.from_numpy(counts).to(dev())
        self.asg = torch.empty((LYR, self.B, self.Q), dtype=torch.int32, device=dev())
        self.z = torch.empty(4 * LYR + 1, dtype=torch.float32, device=dev())
        self.num_pos, self.poison = self.z[:2 * LYR].view(LYR, 2), self.z[2 * LYR:4 * LYR].view(LYR, 2)
        self.status = self.z[4 * LYR:].view(torch.int32)
        self.ws_bytes = L.lsa_large_workspace_bytes(LYR, self.B, self.Q, self.G) if ws_bytes is None else ws_bytes
        self.ws = torch.empty(max(self.ws_bytes, 1), dtype=torch.uint8, device=dev())

    def run(self, path=L.TC_LSA_AUTO, ws_bytes=None):
        self.z.zero_()
        self.asg.fill_(-7)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().tc_lsa_assign_ws(
            self.cost.data_ptr(), self.counts.data_ptr(), LYR, self.B, self.Q, self.G, self.asg.data_ptr(),
            self.num_pos.data_ptr(), self.status.data_ptr(), self.poison.data_ptr(), self.ws.data_ptr(),
            self.ws_bytes if ws_bytes is None else ws_bytes, path, st), 'tc_lsa_assign_ws')
        return self.asg.cpu().numpy()


@pytest.fixture(scope='module', autouse=True)
def library():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()


@pytest.mark.parametrize('Q,G,B', [(1025, 1, 1), (900, 129, 1), (1300, 150, 3), (512, 512, 1), (4096, 512, 1)])
def test_large_assignment_equals_scipy(Q, G, B):
    """Continuous random costs: the optimum is unique, so the assignment is scipy's, query for query.  The workspace is
    exactly tc_lsa_workspace_bytes."""
    cost, counts = make_costs(Q, G, B)
    need = L.lib().tc_lsa_workspace_bytes(LYR, B, Q, G)
    assert need == L.lsa_large_workspace_bytes(LYR, B, Q, G)
    p = Problem(cost, counts, ws_bytes=need)
    got = p.run()
    want = scipy_assign(cost, counts)
    assert int(p.status.item()) == 0
    for l in range(LYR):
        for b in range(B):
            assert np.array_equal(got[l, b], want[l, b]), (l, b, int((got[l, b] != want[l, b]).sum()))
    assert np.array_equal(p.num_pos.cpu().numpy(), np.full((LYR, 2), float(counts.sum()), dtype=np.float32))
    assert float(p.poison.abs().max()) == 0.0
    # a non-finite cost: that problem unassigned, status raised, its output's loss pair poisoned, the others untouched
    cost[0, 0, 5, 0] = np.nan
    p.cost.copy_(torch.from_numpy(cost))
    got2 = p.run()
    assert int(p.status.item()) == 1 and (got2[0, 0] == -1).all()
    assert np.array_equal(got2[1:], got[1:]) and np.array_equal(got2[0, 1:], got[0, 1:])
    poison = p.poison.cpu().numpy()
    assert np.isnan(poison[0]).all() and (poison[1:] == 0.0).all()


@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('Q,G,B', [(900, 24, 2), (1024, 128, 1), (37, 37, 3), (64, 5, 2)])
def test_the_two_kernels_agree_where_both_apply(Q, G, B, ties):
    """The tie order belongs to the column, not to the thread that holds it: 4 and 16 columns per thread give the same
    assignment, also on costs rounded to multiples of 0.5 (many exact ties)."""
    cost, counts = make_costs(Q, G, B)
    if ties:
        cost = np.round(cost * 2.0) / 2.0
        assert np.unique(cost).size <= 9                # multiples of 0.5 in [0, 4]
    assert L.lib().tc_lsa_workspace_bytes(LYR, B, Q, G) == 0
    p = Problem(cost, counts)
    small = p.run(L.TC_LSA_SMALL)
    n_small = p.num_pos.cpu().numpy()
    large = p.run(L.TC_LSA_LARGE)
    assert int(p.status.item()) == 0
    assert np.array_equal(small, large), int((small != large).sum())
    assert np.array_equal(p.num_pos.cpu().numpy(), n_small)
    p.ws_bytes = 0                                     # AUTO takes the small kernel here: no workspace
    assert np.array_equal(p.run(L.TC_LSA_AUTO), small)


def test_tied_costs_beyond_the_old_limits_give_a_valid_optimum():
    """Small integer costs: many optima of exactly the same total (sums of integers are exact in float64).  The result
    is a one-to-one matching of all boxes whose total is scipy's."""
    Q, G = 1300, 150
    rng = np.random.RandomState(5)
    cost = rng.randint(0, 8, (LYR, 1, Q, G)).astype(np.float32)
    assert ((cost == 0).sum(axis=2) > 1).all()         # every box has several zero-cost queries: tied optima exist
    counts = np.full(1, G, dtype=np.int32)
    p = Problem(cost, counts)
    got = p.run()
    assert int(p.status.item()) == 0
    for l in range(LYR):
        q = np.nonzero(got[l, 0] >= 0)[0]
        assert (got[l, 0] >= -1).all() and np.array_equal(np.sort(got[l, 0, q]), np.arange(G))
        rows, cols = linear_sum_assignment(cost[l, 0])
        assert cost[l, 0].astype(np.float64)[q, got[l, 0, q]].sum() == cost[l, 0].astype(np.float64)[rows, cols].sum()


@pytest.mark.parametrize('Q,G,path,short,named', [
    (4097, 24, L.TC_LSA_AUTO, 0, 'Q=4097'),
    (900, 513, L.TC_LSA_AUTO, 0, 'Gmax=513'),
    (100, 101, L.TC_LSA_AUTO, 0, 'Gmax=101'),
    (1300, 150, L.TC_LSA_SMALL, 0, 'Q=1300'),
    (1300, 150, L.TC_LSA_LARGE, 1, 'workspace_bytes='),
    (1300, 150, 7, 0, 'path=7'),
])
def test_refusals_name_the_value_and_launch_nothing(Q, G, path, short, named):
    cost = np.zeros((LYR, 1, Q, G), dtype=np.float32)
    p = Problem(cost, np.full(1, min(G, Q), dtype=np.int32))
    if short:
        named += str(p.ws_bytes - 1)
    with pytest.raises(L.TransCARHipError, match=named):
        p.run(path, ws_bytes=p.ws_bytes - short)
    torch.cuda.synchronize()
    assert (p.asg == -7).all()


def test_large_route_is_capturable():
    """Pre-pass, flag fill and solver are stream-ordered and allocate nothing: captured once, replayed once."""
    cost, counts = make_costs(1300, 150, 1)
    p = Problem(cost, counts)
    eager = p.run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        p.z.zero_()
        p.asg.fill_(-7)
        L.check(L.lib().tc_lsa_assign_ws(
            p.cost.data_ptr(), p.counts.data_ptr(), LYR, 1, 1300, 150, p.asg.data_ptr(), p.num_pos.data_ptr(),
            p.status.data_ptr(), p.poison.data_ptr(), p.ws.data_ptr(), p.ws_bytes, L.TC_LSA_AUTO,
            C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tc_lsa_assign_ws')
    torch.cuda.current_stream().wait_stream(side)
    p.asg.fill_(-9)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(p.asg.cpu().numpy(), eager)
    assert int(p.status.item()) == 0 and float(p.num_pos[0, 0]) == 150.0


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def train_head(num_query=900):
    import transcar_amd as T
    cfg = configs.head_cfg(num_query=num_query)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(3, num_query=num_query).items()})
    return h.to(dev()).freeze_decoder().set_dropout(0.0)


def ground_truth(n):
    boxes, labels = synth.make_gt(seed=7, n=n)
    gt = torch.from_numpy(boxes).clone()
    gt[:, 2] += gt[:, 5] * 0.5
    return gt.to(dev()), torch.from_numpy(labels).to(dev())


@pytest.fixture(scope='module')
def head900():
    return train_head()


@pytest.mark.parametrize('Q,n_gt', [(1300, 150), (900, 129)])
def test_detr_loss_device_takes_the_device_route_beyond_the_old_limits(head900, Q, n_gt):
    """A fresh status word equal to 0 proves the device route ran; the assignment is scipy's and the losses and
    gradients are those of the host route."""
    from transcar_amd.device_loss import detr_loss_device
    h = head900
    rng = np.random.RandomState(Q + n_gt)
    cls = torch.from_numpy(rng.standard_normal((LYR, 1, Q, 10)).astype(np.float32) - 2.0).to(dev())
    box = torch.from_numpy(rng.standard_normal((LYR, 1, Q, 10)).astype(np.float32) * 0.5).to(dev())
    gt, lab = ground_truth(n_gt)
    h.last_assign_status = None
    losses, d_cls, d_box, assigned = detr_loss_device(h, cls, box, [gt], [lab], device_assign=True)
    assert h.last_assign_status is not None and int(h.last_assign_status.item()) == 0
    ws = h._lsa_workspace
    assert ws.numel() >= L.lib().tc_lsa_workspace_bytes(LYR, 1, Q, n_gt) > 0
    detr_loss_device(h, cls, box, [gt], [lab], device_assign=True)
    assert h._lsa_workspace is ws                      # steady state: the cached workspace, no allocation
    h.last_assign_status = None
    ref_losses, r_cls, r_box, r_assigned = detr_loss_device(h, cls, box, [gt], [lab], device_assign=False)
    assert h.last_assign_status is None
    assert np.array_equal(assigned.cpu().numpy(), r_assigned)
    assert int((r_assigned >= 0).sum()) == LYR * n_gt
    assert sorted(losses) == sorted(ref_losses) and len(losses) == 2 * LYR
    for k, v in losses.items():
        ref = float(ref_losses[k])
        assert abs(float(v) - ref) <= 2e-5 * max(1.0, abs(ref)), (k, float(v), ref)
    assert rel(d_cls, r_cls) < 2e-5 and rel(d_box, r_box) < 2e-5


def test_trainer_with_1300_queries_and_150_boxes_stays_on_the_device(golden_dir):
    """FusionTrainer.step_fused_nhwc on a 1 300-query head with 150 boxes: the device loss (now with the device
    assignment) against the PyTorch loss, within the bounds of the 900 x 24 test."""
    from transcar_amd import ops
    from transcar_amd.trainer import FusionTrainer
    h = train_head(num_query=1300)
    feats = synth.make_feats('tiny', seed=1, smooth=(4, 6))
    l2i = synth.make_lidar2img()
    centres = np.load(os.path.join(golden_dir, 'g5_head_tiny.npz'))['radar_centres']
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=centres)
    metas = synth.make_img_metas(1, l2i)
    metas[0]['radar'] = frame
    gt, labels = ground_truth(150)
    nhwc = [ops.to_nhwc(torch.from_numpy(f).to(dev())) for f in feats]
    l2i_t = ops.lidar2img_tensor(metas, dev())
    img_hw = metas[0]['img_shape'][0][:2]
    tokens, pad_mult = h.radar_tokens(metas, dev())
    tr = FusionTrainer(h, dropout=0.0)
    h.last_assign_status = None
    tr.device_loss = True
    l_dev = tr.step_fused_nhwc(nhwc, l2i_t, img_hw, tokens, pad_mult, [gt], [labels], update=False)
    g_dev = tr.bucket.grads.clone()
    assert h.last_assign_status is not None and int(h.last_assign_status.item()) == 0
    tr.device_loss = False
    l_torch = tr.step_fused_nhwc(nhwc, l2i_t, img_hw, tokens, pad_mult, [gt], [labels], update=False)
    g_torch = tr.bucket.grads
    for k in l_torch:
        assert abs(float(l_torch[k]) - float(l_dev[k])) < 1e-5 * max(1.0, abs(float(l_torch[k]))), k
    assert float((g_dev - g_torch).abs().max() / g_torch.abs().max()) < 1e-4
