"""The rig the tests of the head's variants share (every key of configs.head_cfg, the decoder levels' own outputs and
decoder layer 0's fold): heads and frames, the CPU oracle's forward and training iteration, and the checks every variant
repeats -- against the oracle, against the reference's fixtures, the train-mode decoder with read-back dropout masks, a
training iteration against the reference's gradients, the plugin graphs, FramePipeline and a frame inside a nine-frame
launch.  The side rigs (num_cams_rig, radar_heads_rig, radar_input_rig, ffn_dims_rig, variant_pairs_rig) keep the frames,
seeds and case tables of their axes and build every head and make every oracle call through this module.

A variant is keyword arguments named as CONFIGS' keys; what a key reaches differs (variant_kw, state_dict_kw, decoder_kw,
oracle_kw, oracle_forward): the state dict depends on neither head count, the gate, the token count nor a range (they
add no parameter), the oracle reads num_levels, num_points, num_classes, num_query, radar_in_dims and
feedforward_channels off the state dict, the maps and the radar rows, and its decoder reads nothing of the radar side.
The oracle is told every key by argument; nothing here or in a side rig assigns to an attribute of the oracle or of the
library.  One more key, `geometry`, is a Geometry: the point-cloud range of the coder, the attentions and the assigner,
the coder's post_center_range, the image size, the cameras' intrinsics and -- a num_cams_rig.Ring -- their count.  It reaches
the head's config, the oracle's pc_range / img_hw / num_cams arguments, lidar2img and img_metas; of the state dict only
the camera count's share depends on it.  Left out, it is DEFAULT, the TransCAR configs' -- whose x and y intervals are
equal and centred on 0, so that an x / y swap, `2 * pc[3]` for `pc[3] - pc[0]`, `-pc[3]` for `pc[0]` or a folded 51.2
compute what correct code computes.
GEOM has six distinct magnitudes, extents 100 / 96 / 10, and is off-centre.

A plain helper module (as adverse_rig.py): the test modules import the fixtures `T` and `no_grad` by name.  The
checkers take torch tensors on any device; tests/test_head_variant_rig.py pins their caps on the CPU."""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import transcar_oracle as O
from transcar_amd import configs, synth


class Geometry(collections.namedtuple('Geometry', 'pc_range post_center_range img_shape focal pp')):
    """pc_range, post_center_range: six floats each; img_shape (H, W, 3) of every camera image; focal, pp: the pinhole
    cameras' focal length and principal point (x, y) in pixels (synth.make_lidar2img)."""
    __slots__ = ()

    @property
    def hw(self):
        return tuple(self.img_shape[:2])

    def lidar2img(self):
        return synth.make_lidar2img(focal=self.focal, pp=self.pp)

    def metas(self, batch=1, radar=None, l2i=None):
        return synth.make_img_metas(batch, self.lidar2img() if l2i is None else l2i, radar=radar, img_shape=self.img_shape)

    def head_kw(self):
        """configs.head_cfg's arguments that leave the configs' values"""
        return {k: getattr(self, k) for k in ('pc_range', 'post_center_range') if getattr(self, k) != getattr(DEFAULT, k)}


DEFAULT = Geometry(tuple(configs.point_cloud_range), tuple(configs.pts_bbox_head['bbox_coder']['post_center_range']),
                   tuple(configs.IMG_SHAPE), 1266.0, (800.0, 464.0))
GEOM_PCR = (-30.0, -60.0, -4.0, 70.0, 36.0, 6.0)
GEOM_POST = (-40.0, -70.0, -6.0, 80.0, 45.0, 8.0)
GEOM_IMG_SHAPE = (640, 1152, 3)
GEOM = Geometry(GEOM_PCR, GEOM_POST, GEOM_IMG_SHAPE, 1266.0 * 1152 / 1600, (576.0, 320.0))
# the configs' range and image size, for the test modules that name them; no function of this module reads them
PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
SMOOTH = (4, 6)
TINY = configs.LEVEL_SHAPES['tiny']
E2E_TOL = 1e-3          # test_gpu_parity.test_head_end_to_end
# the decoder states on the f16x2 matrix path: at P = 5 the sampling weights are sums of five sigmoids, so the sampled
# values (and the two-plane path's absolute error, which scales with them) are up to five times those of P = 1.  Measured
# on the 32-row tiles: 3 of 1 382 400 states beyond 1e-3, the largest 1.20e-3.  The f32 paths keep E2E_TOL, and box
# codes, logits and reference points keep test_head_end_to_end's tolerances on every path.
HS_TOL_F16X2 = 2e-3
REFS_TOL = 5e-5         # inter_references against the oracle and the reference
MAX_GATE_ROWS = 6       # rows whose radar gate decisions (hit counts) may differ: the gate is discontinuous
BOX_TOL = 5e-5          # metres: fp32 spacing at 50 m is 3.8e-6, the reference and the oracle order add / sigmoid / scale differently
# the TransCAR configs' variant
CONFIGS = dict(num_levels=4, num_points=1, with_box_refine=True, num_heads=8, num_classes=10, num_query=900,
               num_fusion_layers=3, radar_gate=None, radar_num_heads=8, radar_num_tokens=1500, radar_in_dims=36,
               radar_point_range=None, feedforward_channels=512)
POINT_RANGE = (-51.2, -51.2, -5.0, 51.2, 51.2, 3.0)          # the radar filter's range under radar_point_range=None: HEAD:304
HEADS = (4, 16)         # num_heads beside the configs' 8: head dimension 64 and 16
DEPTHS = (1, 2)         # num_fusion_layers beside the configs' 3
CIRCLE = dict(type='circle', radii=[2.0, 2.0, 1.0])                 # the single circle of the paper: 2 / 2 / 1 m
WIDE3 = dict(type='three_circle', radii=[(0.75, 3.0), (0.5, 1.5), (0.25, 0.75)])
# the reference's single-circle fixtures (tests/golden/make_golden_radar_gate.py), on g5_frame(<the seed they store>)
G5_CIRCLE, G8_CIRCLE = 'g5_head_tiny_gate_circle.npz', 'g8_train_grads_gate_circle.npz'


@pytest.fixture(autouse=True)
def no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope='module')
def T():
    import transcar_amd
    assert torch.cuda.is_available(), 'gpu tests need a GPU'
    transcar_amd.lib()
    return transcar_amd


def dev():
    return torch.device('cuda:0')


def gpu(x):
    return torch.as_tensor(x).float().contiguous().to(dev())


def gold(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', name))


# ---- heads and frames ---------------------------------------------------------------------------------------------------
def geometry_of(variant):
    geom = variant.get('geometry', DEFAULT)
    assert isinstance(geom, Geometry), geom
    return geom


def variant_kw(**variant):
    """The arguments of configs.head_cfg that leave the configs' values."""
    geom = geometry_of(variant)
    variant.pop('geometry', None)
    assert set(variant) <= set(CONFIGS), variant
    return dict({k: v for k, v in variant.items() if v != CONFIGS[k]}, **geom.head_kw())


def state_dict_kw(**variant):
    """variant_kw for synth.make_state_dict, which spells radar_in_dims `radar_in`: the state dict does not depend on the
    head counts, the gate, the token count or a range (of the geometry it keeps a ring's camera count)."""
    kw = {k: v for k, v in variant_kw(**variant).items()
          if k not in ('num_heads', 'radar_num_heads', 'radar_gate', 'radar_num_tokens', 'radar_point_range', 'pc_range',
                       'post_center_range')}
    if 'radar_in_dims' in kw:
        kw['radar_in'] = kw.pop('radar_in_dims')
    return kw


def state_dict(seed=3, **variant):
    """the variant's seeded weights {key: float32 ndarray}"""
    return synth.make_state_dict(seed=seed, **state_dict_kw(**variant))


def decoder_kw(**variant):
    """What the oracle's decoder (O.transformer) cannot read off the state dict and the maps (their defaults spelled
    out); the camera count is the geometry's."""
    variant_kw(**variant)
    return dict({k: variant.get(k, CONFIGS[k]) for k in ('with_box_refine', 'num_heads')},
                num_cams=getattr(geometry_of(variant), 'num_cams', 6))


def oracle_kw(**variant):
    """decoder_kw and what the fusion stack of O.head_forward cannot read off the state dict and the radar rows."""
    return dict(decoder_kw(**variant), radar_num_heads=variant.get('radar_num_heads', CONFIGS['radar_num_heads']),
                num_radar_tokens=variant.get('radar_num_tokens', CONFIGS['radar_num_tokens']))


def variant_key(**variant):
    """Hashable, for the caches; a gate enters normalised (the two spellings of one gate are one entry; None is left out)."""
    from transcar_amd._lib import check_radar_gate
    geom = geometry_of(variant)
    kw = variant_kw(**variant)
    if 'radar_gate' in kw:
        gate = check_radar_gate(kw['radar_gate'], kw.get('num_fusion_layers', CONFIGS['num_fusion_layers']))
        kw['radar_gate'] = (gate['type'], gate['radii'])
    if 'radar_point_range' in kw:
        kw['radar_point_range'] = tuple(kw['radar_point_range'])
    return tuple(sorted(kw.items())) + (() if geom == DEFAULT else (('geometry', geom),))


def _build(T, sd_np, train=False, **variant):
    """A fresh head of the variant on the CPU with the weights sd_np, checked; train: with the configs' train_cfg."""
    cfg = configs.head_cfg(**variant_kw(**variant))
    if train:
        cfg.setdefault('train_cfg', configs.train_cfg_pts)        # (head_cfg(pc_range=...) brings its own)
    h = T.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    check_head(h, **variant)
    return h


def make_head(T, *, seed=3, shared_branches=False, **variant):
    """A fresh eval-mode head of the variant with seeded weights, and those weights as the oracle takes them.
    shared_branches: the weights of with_box_refine=False (one cls / reg branch under every index) whatever the head."""
    sd_np = state_dict(seed, **(dict(variant, with_box_refine=False) if shared_branches else variant))
    return _build(T, sd_np, **variant).to(dev()).eval(), O.to_torch_sd(sd_np)


def check_head(h, **variant):
    """The head carries every key of the variant where the kernels and the unfused path read it."""
    from transcar_amd import _lib as L
    from transcar_amd.detr3d_head import fusion_modules
    want = dict(CONFIGS, **variant)
    geom = geometry_of(variant)
    w = h.weights_struct()
    assert tuple(h.pc_range) == geom.pc_range, h.pc_range
    assert tuple(w.pc_range) == tuple(float(np.float32(v)) for v in geom.pc_range)
    assert tuple(h.bbox_coder.post_center_range) == geom.post_center_range
    assert (w.num_cams, w.num_levels, max(w.num_points, 1)) == (getattr(geom, 'num_cams', 6), want['num_levels'], want['num_points'])
    H = want['radar_num_heads']
    assert w.num_heads == L.pack_num_heads(want['num_heads'], H)
    assert (w.num_heads & 0xffff) == want['num_heads'] and (w.num_heads >> 16) == (0 if H == 8 else H)
    assert h.radar_num_heads == H and h.with_box_refine == want['with_box_refine']
    for r in range(h.num_fusion_layers):
        assert fusion_modules(h, r).attn.num_heads == H and fusion_modules(h, r).attn.head_dim == 256 // H
    for ly in h.transformer.decoder.layers:
        assert ly.attentions[0].num_heads == want['num_heads']
    assert w.num_classes == h.bbox_coder.num_classes == want['num_classes'] and w.num_query == want['num_query']
    assert h.num_fusion_layers == w.num_radar_layers == want['num_fusion_layers']
    assert h.radar_gate == L.check_radar_gate(want['radar_gate'], want['num_fusion_layers'])
    assert (w.num_radar_tokens_ref, w.radar_in_dims) == (h.radar_num_tokens, h.radar_in_dims) \
        == (want['radar_num_tokens'], want['radar_in_dims'])
    assert w.ffn_dims == want['feedforward_channels']


_HEADS = {}


def shared_head(T, **variant):
    """make_head(T, **variant), one per variant for the tests that leave it as they found it."""
    key = variant_key(**variant)
    if key not in _HEADS:
        _HEADS[key] = make_head(T, **variant)
    return _HEADS[key]


def train_head(**variant):
    """A fresh head of the variant as the trainer takes it: the seed-3 weights, frozen decoder, no dropout yet."""
    import transcar_amd as T_
    return _build(T_, state_dict(**variant), train=True, **variant).to(dev()).freeze_decoder().set_dropout(0.0)


def g5_frame(radar_seed=2):
    """G5's tiny rig: (feats_np, radar frame of `radar_seed` near the centres tests/golden/g5_head_tiny.npz stores)."""
    feats = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
    return feats, synth.make_radar_frame(seed=radar_seed, n_per_radar=51, centres=gold('g5_head_tiny.npz')['radar_centres'])


def empty_frame():
    """A radar frame without a single return: every token is padding, no query has a hit in any layer."""
    return synth.make_radar_frame(seed=5, n_per_radar=[0, 0, 0, 0, 0])


def g8_frame(g5_name, shapes='tiny', radar_seed=2, num_classes=10, centres=None, geometry=DEFAULT):
    """The frame of a gradient fixture: G5's maps, the radar of `radar_seed` near `centres` (None: those fixture
    `g5_name` stores), G7's ground truth drawn from `num_classes` classes, cameras and image size of `geometry`.  -> the host side (feats_np, l2i_np, frame,
    boxes, labels) and, where there is a GPU, the device side (feats, metas, gt, gt_labels)."""
    feats_np = synth.make_feats(shapes, seed=1, smooth=SMOOTH)
    l2i = geometry.lidar2img()
    frame = synth.make_radar_frame(seed=radar_seed, n_per_radar=51,
                                   centres=gold(g5_name)['radar_centres'] if centres is None else centres)
    boxes, labels = synth.make_gt(seed=7, n=24, num_classes=num_classes)
    assert labels.max() > 15 or num_classes <= 16
    key = (g5_name, shapes if isinstance(shapes, str) else tuple(shapes), radar_seed, num_classes,
           None if centres is None else np.asarray(centres).tobytes(), geometry)
    f = dict(feats_np=feats_np, l2i_np=l2i, frame=frame, boxes=boxes, labels=labels, key=key)
    if torch.cuda.is_available():
        metas = geometry.metas(1, l2i=l2i)
        metas[0]['radar'] = frame
        gt = torch.from_numpy(boxes).clone()
        gt[:, 2] += gt[:, 5] * 0.5
        f.update(feats=[gpu(x) for x in feats_np], metas=metas, gt=gt.to(dev()), gt_labels=torch.from_numpy(labels).to(dev()))
    return f


_ORACLE = {}


def oracle_forward(sd, feats_np, frame, variant, **kw):
    """O.head_forward of the variant (its geometry, depth, gate and oracle_kw) on one frame; kw: head_forward's other
    arguments.  frame: a raw radar frame, filtered by the variant's range, or [n, F] feature rows already filtered
    (radar_input_rig.in_range)."""
    geom = geometry_of(variant)
    want = dict(CONFIGS, **variant)
    l2i = torch.from_numpy(geom.lidar2img()).float()[None]
    rows = O.build_radar_features(frame, want['radar_point_range'] or POINT_RANGE) if isinstance(frame, dict) else frame
    return O.head_forward(sd, [torch.as_tensor(f) for f in feats_np], l2i, geom.hw, rows,
                          list(geom.pc_range), num_fusion_layers=want['num_fusion_layers'], radar_gate=want['radar_gate'],
                          **oracle_kw(**variant), **kw)


def oracle_head(sd, feats_np, frame, key=None, **variant):
    """The oracle's head_forward of the variant with its debug dict.  key: keep the result under it and the variant (one
    forward for the parametrised cases that share weights, maps and radar frame)."""
    key = None if key is None else (key, variant_key(**variant))
    if key is None or key not in _ORACLE:
        res = oracle_forward(sd, feats_np, frame, variant, return_debug=True)
        if key is None:
            return res
        _ORACLE[key] = res
    return _ORACLE[key]


def margin_probe(margins, masks=None):
    """A gate_probe for O.head_forward that appends, per fusion layer, the distance (m) between the layer's closest gate
    decision and its radius: the minimum over the queries, the gate's circles and the radar tokens of |distance - radius|.
    The padding tokens are left out (they sit far outside every circle).  masks: a list that receives the layer's gate
    mask [Q, tokens] (True = masked)."""
    from transcar_amd._lib import TC_RADAR_GATE_CIRCLE

    def probe(centre_xy, length_log, rot_sin, rot_cos, radar_xy, rmin, rmax):
        if masks is not None:
            masks.append(O.single_circle_mask(centre_xy, radar_xy, rmax) if rmin == TC_RADAR_GATE_CIRCLE
                         else O.circle_mask(centre_xy, length_log, rot_sin, rot_cos, radar_xy, rmin, rmax))
        centres, radii = [centre_xy], rmax
        if rmin != TC_RADAR_GATE_CIRCLE:             # O.circle_mask's front and rear circles and its clamped radius
            length = length_log.exp()
            off = torch.stack((length * 0.25 * -rot_sin, length * 0.25 * -rot_cos), -1)
            centres += [centre_xy + off, centre_xy - off]
            radii = torch.clamp((length / 2.0).reshape(-1, 1), min=rmin, max=rmax)
        live = radar_xy[0, :, 0] != O.PAD_VALUE
        margins.append(min(float((torch.cdist(c, radar_xy, p=2.0)[0][:, live] - radii).abs().min()) for c in centres))
    return probe


def gate_margin(sd, feats_np, frame, **variant):
    """The distance (m) between the frame's closest gate decision and its radius: the minimum over the variant's fusion
    layers of what margin_probe measures on the oracle through head_forward's gate_probe."""
    margins = []
    with torch.no_grad():
        oracle_forward(sd, feats_np, frame, variant, gate_probe=margin_probe(margins))
    assert len(margins) == dict(CONFIGS, **variant)['num_fusion_layers']
    return min(margins)


_TRACE, _OUT = {}, {}


def oracle_trace(**variant):
    """The oracle's decoder on the g5_head_tiny rig (feature maps seed 1, state dict seed 3), once per variant:
    -> (sd, hs [L,B,Q,C], init_ref [B,Q,3], inter_refs [L,B,Q,3])."""
    key = variant_key(**variant)
    if key not in _TRACE:
        sd = O.to_torch_sd(state_dict(**variant))
        feats = synth.make_feats('tiny', seed=1, smooth=SMOOTH)
        geom = geometry_of(variant)
        l2i = torch.from_numpy(geom.lidar2img()).float()[None]
        with torch.no_grad():
            hs, init_ref, inter_refs, _ = O.transformer(sd, [torch.from_numpy(f) for f in feats], list(geom.pc_range), l2i,
                                                        geom.hw, **decoder_kw(**variant))
        _TRACE[key] = (sd, hs.permute(0, 2, 1, 3).contiguous(), init_ref, inter_refs)
    return _TRACE[key]


def oracle_outputs(**variant):
    """O.decoder_outputs on oracle_trace(**variant), computed once and shared: (cls, box) as numpy arrays"""
    key = variant_key(**variant)
    if key not in _OUT:
        with torch.no_grad():
            cls, box = O.decoder_outputs(*oracle_trace(**variant), list(geometry_of(variant).pc_range))
        _OUT[key] = (cls.numpy(), box.numpy())
    return _OUT[key]


def run_head(head, feats_np, frame, geometry=DEFAULT, **options):
    """One frame (cameras and image size of `geometry`) through the module entry with aux outputs, under
    head_options(**options) (none: the automatic ones)."""
    from transcar_amd.detr3d_head import head_options
    head.forward_options = head_options(**options) if options else None
    try:
        outs = head([gpu(f) for f in feats_np], geometry.metas(1, radar=frame), aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    return outs


# ---- the checkers (torch tensors on any device) ----------------------------------------------------------------------------
def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def refs_are_initial(aux):
    """without box refinement: inter_references[l] is init_reference bit for bit, every l"""
    init, refs = aux['init_reference'], aux['inter_references']
    for l in range(refs.shape[0]):
        assert torch.equal(refs[l], init), l


def assert_all_but_two_queries(got, want, tol, what):
    """[layers, Q, D]: every query within tol but at most two, and those within 1e-2.  At res101 shapes and P = 5, two
    of the 900 queries (220, 324) carry a reference point the free-running decoder puts next to a sampling
    discontinuity: there ANY two fp32 evaluation orders part by up to 3e-3 -- measured, the oracle on two different
    CPUs against the same reference fixture: 5e-4 on one, 2.4e-3 on query 324 on the other; the library: query 220
    3.0e-3 on both matrix paths, every other query within 1e-3."""
    d = np.abs(got - want).max(axis=(0, 2))
    bad = np.where(d > tol)[0]
    assert len(bad) <= 2 and (len(bad) == 0 or d.max() < 1e-2), (what, bad.tolist(), d[bad].tolist())


def oracle_fp64_deviation(sd, feats_np, frame, want, dbg, **variant):
    """How far the fp32 oracle's free-running decoder is from the fp64 evaluation of the same decoder, per query: where a
    rig puts a query's reference point next to a sampling discontinuity, ANY two fp32 evaluation orders part there, and
    the adverse-frame rule bounds a comparison with the oracle by twice this deviation plus the existing floor.
    -> (hs_dev [Q]: max over layers and channels of |hs - hs64|; out_dev [Q]: max over both outputs, the fusion levels
    and the columns of |outputs - outputs of the fusion stack on the fp64 decoder's states|)."""
    geom = geometry_of(variant)
    l2i = torch.from_numpy(geom.lidar2img()).float()[None]
    feats = [torch.from_numpy(f) for f in feats_np]
    trace64 = O.transformer({k: v.double() for k, v in sd.items()}, [f.double() for f in feats], list(geom.pc_range),
                            l2i.double(), geom.hw, **decoder_kw(**variant))
    hs_dev = (dbg['hs'].double() - trace64[0].permute(0, 2, 1, 3)).abs().amax(dim=(0, 1, 3))
    trace = tuple(t.float() if torch.is_tensor(t) else t for t in trace64)
    outs64 = oracle_forward(sd, feats, frame, variant, decoder_trace=trace)
    out_dev = torch.stack([(want[k] - outs64[k]).abs().amax(dim=(0, 1, 3)) for k in ('all_cls_scores', 'all_bbox_preds')]).amax(0)
    return hs_dev.numpy(), out_dev.numpy()


def _assert_within(got, want, tol, what):
    """np.testing.assert_allclose(atol=tol, rtol=0) that also takes an array of bounds (broadcast against the values)"""
    if not np.ndim(tol):
        np.testing.assert_allclose(got, want, atol=tol, rtol=0)
        return
    over = np.abs(got - want) > tol
    assert not over.any(), '%s: %d values beyond their bounds, the largest difference among them %.3g' % (
        what, int(over.sum()), float(np.abs(got - want)[over].max()))


def check_against_oracle(outs, want, dbg, hs_tol=E2E_TOL, refs_initial=False, out_tol=E2E_TOL):
    """A free-running head's outputs against oracle_head's: reference points, decoder states, and scores and boxes on
    the rows whose radar gate decisions agree.  hs_tol, out_tol: a number, or one bound per query [Q] (the adverse-frame
    rule on a rig whose oracle is itself ill-conditioned at a few queries: oracle_fp64_deviation)."""
    if np.ndim(hs_tol):
        hs_tol = np.asarray(hs_tol, np.float64)[:, None]
    aux = outs['aux']
    if refs_initial:
        refs_are_initial(aux)
    np.testing.assert_allclose(_np(aux['inter_references']), _np(dbg['inter_refs']), atol=REFS_TOL, rtol=0)
    _assert_within(_np(aux['inter_states']), _np(dbg['hs']), hs_tol, 'inter_states')
    want_hits = np.stack([_np(h) for h in dbg['hit_counts']])
    agree = np.all(_np(aux['radar_hit_counts'][:, 0]) == want_hits, axis=0)
    assert int((~agree).sum()) <= MAX_GATE_ROWS
    if np.ndim(out_tol):
        out_tol = np.asarray(out_tol, np.float64)[agree][:, None]
    for k in ('all_cls_scores', 'all_bbox_preds'):
        _assert_within(_np(outs[k][:, 0])[:, agree], _np(want[k][:, 0])[:, agree], out_tol, k)


def check_against_fixture(outs, want, dbg, fixture, tie_rule=False, refs_initial=False):
    """A free-running head's outputs against the reference's (a G5 fixture) on the rows whose radar gate decisions
    agree with the oracle's AND the reference's, and against the oracle on the same rows.  The head may have fewer fusion
    layers than the oracle's run and the fixture: its N levels are held to their levels [:N] (the layers are causally
    ordered).

    tie_rule: a radar gate decision of the rig can sit within 1e-4 m of its radius (G5-L2: query 880, 2.1e-4 m in fusion
    layer 3): where the oracle on this machine and the reference took it differently, the stored hit counts cannot say
    which row flipped (the fixture keeps the selected rows only, and their count then differs).  Such a query departs
    from the reference in the ORACLE too (by more than 1e-2; at most two may); it is left out of the comparison with the
    reference only -- the library is held to the oracle on every agreeing row."""
    aux = outs['aux']
    if refs_initial:
        refs_are_initial(aux)
    np.testing.assert_allclose(_np(aux['inter_references']), fixture['inter_refs'], atol=REFS_TOL, rtol=0)
    levels = outs['all_cls_scores'].shape[0]
    # the fixture stores the hit counts of the selected rows; rebuilt to [levels, Q] as test_head_end_to_end does
    want_hits = np.stack([_np(h) for h in dbg['hit_counts']])[:levels]
    gold_hits = np.zeros_like(want_hits)
    for i in range(levels):
        rows = np.where(want_hits[i] > 0)[0]
        gold_hits[i] = want_hits[i]
        if len(rows) == int(fixture['Lq'][i]):
            gold_hits[i] = 0
            gold_hits[i, rows] = fixture['hit_counts%d' % i]
    hits = _np(aux['radar_hit_counts'][:, 0])
    assert hits.shape == want_hits.shape, (hits.shape, want_hits.shape)
    agree = np.all(hits == want_hits, axis=0) & np.all(hits == gold_hits, axis=0)
    assert int((~agree).sum()) <= MAX_GATE_ROWS
    cut = {k: (_np(want[k][:levels, 0]), fixture[k][:levels, 0]) for k in ('all_cls_scores', 'all_bbox_preds')}
    tie = np.zeros(agree.shape, bool)
    if tie_rule:
        for oracle, reference in cut.values():
            tie |= np.abs(oracle - reference).max(axis=(0, 2)) > 1e-2
        assert int(tie.sum()) <= 2, np.where(tie)[0].tolist()
    for k, (oracle, reference) in cut.items():
        got = _np(outs[k][:, 0])
        assert got.shape == oracle.shape == reference.shape, (k, got.shape, oracle.shape, reference.shape)
        assert_all_but_two_queries(got[:, agree & ~tie], reference[:, agree & ~tie], E2E_TOL, k + ' vs reference')
        # and the oracle, which tests/test_*_golden.py hold to the same fixture
        assert_all_but_two_queries(got[:, agree], oracle[:, agree], E2E_TOL, k + ' vs oracle')


# ---- dropout masks as the kernels draw them ------------------------------------------------------------------------------
def dropout_mask(p, seed, site, n):
    """The n multipliers (0 | 1/(1-p)) the kernels draw at a dropout site, read back through tc_dropout_mask (CPU)."""
    from transcar_amd import _lib as L
    out = torch.empty(n, dtype=torch.float32, device=dev())
    L.check(L.lib().tc_dropout_mask(p, seed, site, n, out.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'tc_dropout_mask')
    return out.cpu()


def decoder_dropout_masks(p, seed, Q, Cd=256, Fd=512, H=8, layers=6):
    """The oracle's ``dec_drop`` for one frame: site = 16 + 8 * layer + {0 probs [B*heads,Q,Q], 1 self-attn out,
    2 cross-attn out, 3 FFN hidden, 4 FFN out}."""
    def m(site, *shape):
        return dropout_mask(p, seed, site, int(np.prod(shape))).view(*shape)
    return [dict(probs=m(s0, H, Q, Q), sa=m(s0 + 1, Q, 1, Cd), ca=m(s0 + 2, Q, 1, Cd), ffn_h=m(s0 + 3, Q, 1, Fd),
                 ffn_o=m(s0 + 4, Q, 1, Cd)) for s0 in range(16, 16 + 8 * layers, 8)]


def prob_masks(p, seed, H, Q, layers=3, tokens=1500):
    """The multipliers on the attention probabilities of the fusion layers, one [H, Q, tokens] tensor per layer as the
    reference's nn.MultiheadAttention(dropout=p) would draw one: site 4 r + 0, index (q * H + h) * tokens + tok."""
    return [dropout_mask(p, seed, 4 * r + 0, Q * H * tokens).view(Q, H, tokens).permute(1, 0, 2).contiguous()
            for r in range(layers)]


def radar_dropout_masks(p, seed, H, Q, Cd=256, Fd=512, layers=3, tokens=1500):
    """The oracle's ``drop`` for one frame (test_gpu_training's layout) at H radar heads and the head's padded token count:
    per layer probs [H, Q, tokens] (site 4 r), d2 [Q, Cd] (4 r + 1), ffn [Q, Fd] (4 r + 2), d3 [Q, Cd] (4 r + 3)."""
    probs = prob_masks(p, seed, H, Q, layers, tokens)
    return [dict(probs=probs[r], d2=dropout_mask(p, seed, 4 * r + 1, Q * Cd).view(Q, Cd),
                 ffn=dropout_mask(p, seed, 4 * r + 2, Q * Fd).view(Q, Fd),
                 d3=dropout_mask(p, seed, 4 * r + 3, Q * Cd).view(Q, Cd)) for r in range(layers)]


# ---- the checks every variant repeats ------------------------------------------------------------------------------------
def check_train_mode_decoder(frame, rows, matrix, refs_atol=2e-4, **variant):
    """The frozen decoder's train-mode forward (dropout on, layer 0 not folded: the DROP instantiations of the chain
    kernels) against the oracle's decoder with the SAME masks, as
    test_gpu_training.test_decoder_train_mode_dropout_matches_reference_formula does for the configs' head.
    frame: g8_frame(...); without box refinement the references are also the initial one, bit for bit."""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    p, seed = 0.1, 0x5EED1234ABCD
    h = train_head(**variant)
    h.set_decoder_dropout(p)
    feats, metas = frame['feats'], frame['metas']
    nhwc = ops.to_nhwc_levels(feats)
    l2i = ops.lidar2img_tensor(metas, dev())
    img_hw = metas[0]['img_shape'][0][:2]
    tokens, pad_mult = h.radar_tokens(metas, dev())
    h.train()
    opts = dict(decoder_dropout_p=p, dropout_seed=seed, tile_rows=rows, matrix_path=matrix)
    a = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=head_options(**opts))
    b = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=head_options(**opts))
    hs = a['aux']['inter_states']
    assert torch.equal(hs, b['aux']['inter_states'])                 # same seed, same masks
    if (rows, matrix) == (16, 'f32'):          # no f32 16-row dropout kernel: the launch runs the 8-row one, bit for bit
        c = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True,
                           options=head_options(**dict(opts, tile_rows=8)))
        for k in ('inter_states', 'inter_references'):
            assert torch.equal(a['aux'][k], c['aux'][k]), k
    okw = decoder_kw(**variant)
    geom = geometry_of(variant)
    assert tuple(img_hw) == geom.hw             # the frame is g8_frame(..., geometry=<the variant's>)
    if not okw['with_box_refine']:
        refs_are_initial(a['aux'])
    Fd = dict(CONFIGS, **variant)['feedforward_channels']
    masks = decoder_dropout_masks(p, seed, h.num_query, Fd=Fd, H=okw['num_heads'])     # the hidden site's index: row * Fd + column
    assert all(m['ffn_h'].numel() == h.num_query * Fd for m in masks)
    keep = float(torch.stack([m['ffn_h'] for m in masks]).ne(0).float().mean())
    assert abs(keep - (1.0 - p)) < 5e-3, keep
    want_hs, init_ref, want_refs, _ = O.transformer(
        O.to_torch_sd(state_dict(**variant)), [torch.from_numpy(f) for f in frame['feats_np']],
        list(geom.pc_range), torch.from_numpy(frame['l2i_np']).float()[None], geom.hw, dec_drop=masks, **okw)
    np.testing.assert_allclose(a['aux']['init_reference'].cpu().numpy(), init_ref.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), want_refs.numpy(), atol=refs_atol, rtol=0)
    print('%r %d rows %s train mode: max|hs - oracle with the same masks| = %.3g' % (
        variant, rows, matrix, np.abs(hs.cpu().numpy()[:, 0] - want_hs[:, :, 0].numpy()).max()))
    np.testing.assert_allclose(hs.cpu().numpy()[:, 0], want_hs[:, :, 0].numpy(), atol=2e-3, rtol=0)


# ---- a training iteration: the reference's gradient fixtures (G8), the oracle's autograd, the trainer -------------------------
FROZEN = ('transformer.', 'cls_branches.', 'reg_branches.', 'query_embedding.', 'code_weights')


def trainable(name):
    """tools/train.py:245-252 freezes the DETR3D part of the head."""
    return not name.startswith(FROZEN)


def g8_name(tag='tiny'):
    return 'g8_train_grads.npz' if tag == 'tiny' else 'g8_train_grads_%s.npz' % tag


def g8_inputs(golden_dir, tag='tiny'):
    """tag: 'tiny' FPN shapes, or 'res101' = the ResNet-101 shapes of BASELINE.json configs[2]"""
    g5 = np.load(os.path.join(golden_dir, 'g5_head_%s.npz' % tag))
    feats = synth.make_feats(tag, seed=1, smooth=(4, 6))
    l2i = synth.make_lidar2img()
    frame = synth.make_radar_frame(seed=2, n_per_radar=51, centres=g5['radar_centres'])
    boxes, labels = synth.make_gt(seed=7, n=24)
    return feats, l2i, frame, boxes, labels


class GradStats(dict):
    """Gradients {name: tensor or None} in the layout of a G8 fixture (make_golden.write_g8): the reference side of
    check_grads_against_g8 where no fixture exists."""
    def __init__(self, grads):
        super().__init__()
        for k, g in grads.items():
            key = k.replace('.', '__')
            if g is None:
                self[key + '__none'] = np.zeros(1)
                continue
            g = g.detach().double().flatten().cpu()
            self[key + '__stats'] = np.array([g.sum(), g.abs().sum(), g.norm()], np.float64)
            self[key + '__head'] = g[:16].float().numpy()

    @property
    def files(self):
        return list(self)


def check_grads_against_g8(grads, g8, rtol, what, expected=98):
    """grads {state_dict key: tensor or None} against a G8 fixture (or GradStats): every parameter of `grads` has an entry
    in the fixture -- its gradient's [sum, sum|.|, l2] and first 16 values, or `__none` (the reference's forward never
    uses it: no gradient, or a zero one) -- the fixture has no entry beyond them, and `expected` of them carry a
    gradient (the three-layer head: 98; N fusion layers: the encoders' 14 + 28 N)."""
    stats = {k[:-len('__stats')] for k in g8.files if k.endswith('__stats')}
    nones = {k[:-len('__none')] for k in g8.files if k.endswith('__none')}
    assert len(stats) == expected, (what, len(stats), expected)
    keys = {k.replace('.', '__') for k in grads}
    assert keys == stats | nones, (what, sorted(keys ^ (stats | nones)))
    checked = 0
    for k, g in grads.items():
        key = k.replace('.', '__')
        if key in nones:
            assert g is None or float(g.abs().max()) == 0.0, k
            continue
        assert g is not None, (what, k)
        ref = g8[key + '__stats']
        gd = g.detach().double().flatten().cpu()
        got = np.array([gd.sum(), gd.abs().sum(), gd.norm()])
        scale = ref[1]                      # sum |g|: the natural magnitude for all three
        assert abs(got[1] - ref[1]) <= rtol * scale, (what, k, got, ref)
        assert abs(got[2] - ref[2]) <= rtol * max(ref[2], 1e-12), (what, k, got, ref)
        assert abs(got[0] - ref[0]) <= rtol * scale, (what, k, got, ref)
        head = g8[key + '__head']
        tol = rtol * max(np.abs(head).max(), ref[2] / np.sqrt(gd.numel()))
        assert np.abs(gd[:16].float().numpy() - head).max() <= 4 * tol, (what, k)
        checked += 1
    assert checked == expected, (what, checked, expected)
    return checked


_FORWARD, _TRAINING = {}, {}


def _training_forward(host, variant):
    sd = O.to_torch_sd(state_dict(**variant))
    for k, v in sd.items():
        if trainable(k):
            v.requires_grad_(True)
    with torch.enable_grad():
        return sd, oracle_forward(sd, host['feats_np'], host['frame'], variant)


def _training_backward(sd, outs, host, levels, variant):
    for v in sd.values():
        v.grad = None
    with torch.enable_grad():
        cut = {k: outs[k][:levels] for k in ('all_cls_scores', 'all_bbox_preds')}
        res, matches = O.loss(cut, torch.from_numpy(host['boxes']), torch.from_numpy(host['labels']), sd['code_weights'],
                              num_classes=dict(CONFIGS, **variant)['num_classes'])
        sum(res.values()).backward(retain_graph=True)
    return ({k: v.detach() for k, v in cut.items()}, {k: float(v.detach()) for k, v in res.items()}, matches,
            {k: v.grad for k, v in sd.items() if trainable(k)})


def oracle_training(host, levels=None, keep=True, **variant):
    """One training iteration of the oracle on the host side of a g8_frame: the variant's seed-3 weights with the
    trainable ones as autograd leaves, head_forward, O.loss at the variant's class count, backward.  levels=N: the loss
    and the backward on levels [:N] of that forward (the fusion layers are causally ordered: one forward serves every N).
    -> (outs, losses {name: float}, matched gt per level, {name: gradient or None} of the trainable parameters), kept per
    variant, frame and levels.  keep=False: computed now and not kept (the tie analysis runs it under its ReLU hook)."""
    if not keep:
        return _training_backward(*_training_forward(host, variant), host, levels, variant)
    key = (host['key'], variant_key(**variant))
    if key not in _FORWARD:
        _FORWARD[key] = _training_forward(host, variant)
    if (key, levels) not in _TRAINING:
        _TRAINING[key, levels] = _training_backward(*_FORWARD[key], host, levels, variant)
    return _TRAINING[key, levels]


def iteration_inputs(h, frame):
    """FusionTrainer.step_fused_nhwc's arguments for head `h` on a g8_frame"""
    from transcar_amd import ops
    metas = frame['metas']
    tokens, pad_mult = h.radar_tokens(metas, dev())
    return ([ops.to_nhwc(f) for f in frame['feats']], ops.lidar2img_tensor(metas, dev()), metas[0]['img_shape'][0][:2], tokens,
            pad_mult, [frame['gt']], [frame['gt_labels']])


def trainer_iteration(frame, head=None, **kw):
    """One FusionTrainer.step_fused_nhwc(update=False) (frozen decoder -> radar stack -> loss -> backward) of a fresh
    head (or of `head`, a train_head of the variant).  frame: g8_frame(...); kw: the variant, and what is no variant key
    goes to FusionTrainer.
    -> (losses {name: float}, {name: gradient or None} of the trainable parameters)"""
    from transcar_amd.trainer import FusionTrainer
    variant = {k: kw.pop(k) for k in list(kw) if k in CONFIGS or k == 'geometry'}
    h = head or train_head(**variant)
    tr = FusionTrainer(h, dropout=0.0, **kw)
    with torch.enable_grad():
        losses = tr.step_fused_nhwc(*iteration_inputs(h, frame), update=False)
    torch.cuda.synchronize()
    used = {n for n, _ in h.trainable_parameters()}
    grads = {k: (p.grad.clone() if (p.grad is not None and k in used) else None)
             for k, p in h.named_parameters() if trainable(k)}
    return {k: float(v) for k, v in losses.items()}, grads


def check_training_iteration(frame, g8_name, what, expected=98, **variant):
    """trainer_iteration against the reference's losses and gradients (a G8 fixture), 2e-3 as test_training's
    oracle-vs-reference check.  expected: the parameters an iteration gives a gradient, as the caller states it; it is
    the head's count and the fixture's."""
    g8 = gold(g8_name)
    h = train_head(**variant)
    assert len(h.trainable_parameters()) == expected
    losses, grads = trainer_iteration(frame, head=h)
    assert sorted('loss__' + k.replace('.', '_') for k in losses) == sorted(k for k in g8.files if k.startswith('loss__'))
    for k, v in losses.items():
        ref = float(g8['loss__' + k.replace('.', '_')])
        print('%s %s: %.6f (reference %.6f)' % (what, k, v, ref))
        assert abs(v - ref) < 2e-3 * max(1.0, abs(ref)), (what, k, v, ref)
    assert check_grads_against_g8(grads, g8, 2e-3, what, expected) == expected


def check_plugin_graph_replay(hg, he, shapes='tiny', geometry=DEFAULT, num_cams=6):
    """The plugin entry's captured graphs (plugin_graph.py) of head `hg` replay, bit for bit, what the eager entry of
    its twin `he` computes.  Two fresh heads: `he` loses its graphs.  geometry: the frames' cameras and image size, or
    one Geometry per call (the warm-up call and the three compared ones): a graph keyed without the image size would
    replay a stale one.  num_cams: the cameras of the maps (a ring geometry's count).  The radar inputs are raw sweeps:
    the graphs serve no other (a head of another radar_in_dims takes [n, F] rows on the eager path)."""
    geoms = list(geometry) if isinstance(geometry, list) else [geometry] * 4
    assert len(geoms) == 4
    if isinstance(shapes, str):
        shapes = configs.LEVEL_SHAPES[shapes]
    he.plugin_graphs = False
    g = torch.Generator(device=dev())
    g.manual_seed(5)
    radar = [synth.make_radar_frame(seed=39 + it, n_per_radar=30) for it in range(4)]
    feats = [torch.randn((1, num_cams, 256, h_, w_), device=dev(), generator=g) for (h_, w_) in shapes]
    hg(feats, geoms[0].metas(1, radar=radar[0]))
    base = dict(hg._plugin_graphs.stats)
    for it in range(3):
        for f in feats:
            f.mul_(0.9).add_(0.01 * (it + 1))
        metas = geoms[it + 1].metas(1, radar=radar[it + 1])
        og, oe = hg(feats, metas), he(feats, metas)
        torch.cuda.synchronize()
        for k in ('all_cls_scores', 'all_bbox_preds'):
            assert torch.equal(og[k], oe[k]), (it, k)
    st = {k: v - base[k] for k, v in hg._plugin_graphs.stats.items()}
    assert st['replays'] >= 1, st


def check_frame_pipeline(head, nlanes=2, shapes='tiny', pregather_off=False, geometry=DEFAULT):
    """A FramePipeline of `nlanes` lanes (bench.make_inputs' lane layout) gives bit for bit what forward_nhwc gives.
    pregather_off: the pipeline must have left the camera pre-gather off.  geometry: the lanes' cameras and image size,
    or one Geometry per lane (a lane that kept another lane's image size would not equal its own forward_nhwc)."""
    geoms = list(geometry) if isinstance(geometry, list) else [geometry] * nlanes
    assert len(geoms) == nlanes
    import bench
    bench._imports()
    from transcar_amd.pipeline import FramePipeline
    lanes = [bench.make_inputs(head, dev(), shapes, 1, seed=11 + i) for i in range(nlanes)]
    for inp, geom in zip(lanes, geoms):
        if geom != DEFAULT:
            inp.update(l2i_np=geom.lidar2img(), l2i=gpu(geom.lidar2img()[None]), hw=geom.hw)
    want = []
    for inp in lanes:
        outs, dec = bench.one_step(head, inp)
        want.append([outs['all_cls_scores'].clone(), outs['all_bbox_preds'].clone()] + [d.clone() for d in dec])
    torch.cuda.synchronize()
    pipe = FramePipeline(head, lanes)
    if pregather_off:
        assert pipe.options.cam_pregather == 0
    for _ in range(2):
        for _ in range(nlanes):
            pipe.launch()
    pipe.synchronize()
    for i in range(nlanes):
        outs, dec = pipe.outputs[i]
        for a_, b_ in zip([outs['all_cls_scores'], outs['all_bbox_preds']] + list(dec), want[i]):
            assert torch.equal(a_, b_)


def check_frame_of_nine(head, shapes='tiny', refs_initial=False, geometry=DEFAULT, num_cams=6, radar=None):
    """One frame of a nine-frame launch (32-row tiles) is bit-identical to that frame launched alone with the same
    tile height and matrix path.  refs_initial (no box refinement): so are its reference points, the initial ones.
    num_cams: the cameras of the maps (a ring geometry's count).  radar: the nine frames' radar inputs as img_metas carry
    them (raw frames, or [n, F] rows for a head of another radar_in_dims); None: raw frames of seeds 60 .. 68."""
    from transcar_amd.detr3d_head import head_options
    feats = [synth.make_feats(shapes, seed=40 + i, num_cams=num_cams, smooth=SMOOTH) for i in range(9)]
    frames = [synth.make_radar_frame(seed=60 + i, n_per_radar=45) for i in range(9)] if radar is None else list(radar)
    assert len(frames) == 9
    kw = dict(aux=True) if refs_initial else {}
    head.forward_options = head_options(tile_rows=32, matrix_path='f16x2')
    try:
        many = head([gpu(np.concatenate([f[l] for f in feats], 0)) for l in range(len(feats[0]))],
                    geometry.metas(9, radar=frames), **kw)
        one = head([gpu(f) for f in feats[4]], geometry.metas(1, radar=frames[4]), **kw)
    finally:
        head.forward_options = None
    for k in ('all_cls_scores', 'all_bbox_preds'):
        assert torch.equal(many[k][:, 4], one[k][:, 0]), k
    if refs_initial:
        assert torch.equal(many['aux']['inter_references'][:, 4], one['aux']['inter_references'][:, 0])
        refs_are_initial(many['aux'])
