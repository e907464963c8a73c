"""What the tests of the head's camera count (Detr3DCrossAtten.num_cams 1 .. 16; the configs: 6) add to
head_variant_rig.py: a Geometry whose cameras are a ring of N (synth.ring_yaws) and whose head_kw carries num_cams, so
that the rig's heads, oracle forwards (which pass the ring's count to the oracle), gate-margin search, frames and
checkers serve a camera count as they serve a point-cloud range; the radar seeds chosen per count; and the coverage a rig must have before a GPU case on it proves anything (cameras with index >= 8 are the new ground).

Tiny level shapes, 6 decoder layers, state dict seed 3, smooth maps (4, 6) seed 1, 72 queries: two 32-row tiles and a
ragged one.  A plain helper module; what is computed on the CPU is computed once per count and kept."""
import numpy as np
import torch

import head_variant_rig as R
from num_classes_rig import centres_of
from oracle import transcar_oracle as O
from transcar_amd import synth

NQ = 72
JITTER = 4                             # jitter_seed of the batch's second lidar2img set (mounts moved by up to 0.1 m): of 1, 2, .. the first whose
                                       # sample keeps the coverage below at 9, 12 and 16 cameras (its maps are the batch's second sample's)
COUNTS = (1, 5, 8, 9, 12, 16)          # 1, 5, 8: the fixed-level kernels; 9, 12, 16: the generic ones (more than 32 logits)
# (tile rows, matrix path) of the decoder chains: the automatic choice and every variant a launch can name
PATHS = {'auto': {}, 'f32-4': dict(tile_rows=4, matrix_path='f32'), 'f32-8': dict(tile_rows=8, matrix_path='f32'),
         'f32-16': dict(tile_rows=16, matrix_path='f32'), 'f16x2-16': dict(tile_rows=16, matrix_path='f16x2'),
         'f16x2-32': dict(tile_rows=32, matrix_path='f16x2')}
G5_CAMS12, G8_CAMS12 = 'g5_head_tiny_cams12.npz', 'g8_train_grads_cams12.npz'


class Ring(R.Geometry):
    """A geometry (`base`; None: the configs') with a ring of `num_cams` cameras (jitter_seed: the mounts moved, a second
    lidar2img set).  Equal to no Geometry but a Ring of the same base, count and seed."""

    def __new__(cls, num_cams, jitter_seed=None, base=None):
        self = super().__new__(cls, *(R.DEFAULT if base is None else tuple(base)))
        self.num_cams, self.jitter_seed = int(num_cams), jitter_seed
        return self

    def _id(self):
        return tuple(self) + (self.num_cams, self.jitter_seed)

    def __eq__(self, other):
        return isinstance(other, Ring) and self._id() == other._id()

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self._id())

    def lidar2img(self):
        return synth.make_lidar2img(focal=self.focal, pp=self.pp, yaws_deg=synth.ring_yaws(self.num_cams),
                                    jitter_seed=self.jitter_seed)

    def head_kw(self):
        kw = super().head_kw()
        if self.num_cams != 6:
            kw['num_cams'] = self.num_cams
        return kw


def variant(N, **kw):
    """head_variant_rig's variant of N cameras (kw: its other keys)"""
    return dict(dict(num_query=NQ, geometry=Ring(N)), **kw)


def feats(N, batch=1, num_levels=4, **_):
    """the rig's maps [batch, N, C, H, W], the first num_levels tiny levels (the other variant keys do not reach them)"""
    return synth.make_feats(R.TINY[:num_levels], seed=1, batch=batch, num_cams=N, smooth=R.SMOOTH)


def state_dict(N, **kw):
    return R.state_dict(**variant(N, **kw))


# ---- radar frames: the gate-margin search of the other variants, on the oracle's own centres ---------------------------------
# Of seeds 2 .. 39 the one whose closest gate decision (oracle, this count's rig) is farthest from its radius, and that
# distance in metres.  tests/test_num_cams_host.py repeats the search for the counts the fixtures use and holds every
# stored pair to the oracle.  Keys: (count, other variant keys ...), as _vkey spells them.
RADAR_SEEDS = {(1,): (6, 1.865e-3), (5,): (24, 1.344e-3), (8,): (39, 1.454e-3), (9,): (20, 1.649e-3), (12,): (26, 1.475e-3),
               (16,): (22, 2.317e-3),
               # the other generic corners with many cameras
               (16, ('num_levels', 2)): (37, 8.336e-4), (16, ('num_points', 4)): (32, 1.405e-3),
               (12, ('with_box_refine', False)): (4, 9.159e-4)}
SEED_RANGE = range(2, 40)
# the frame of both fixtures (G5-cams12's second pass and G8-cams12): the same search on the centres G5-cams12's first
# pass stores (tests/golden/make_golden_num_cams.py stores seed and distance in both)
G8_CAMS12_RADAR_SEED = 26         # 1.475e-3 m

_CENTRES, _SEARCH = {}, {}


def _vkey(N, kw):
    return (N,) + tuple(sorted(kw.items()))


def centres(N, **kw):
    """xy of the decoder's last reference points on the count's rig (a first pass of the oracle)"""
    key = _vkey(N, kw)
    if key not in _CENTRES:
        with torch.no_grad():
            _, dbg = R.oracle_forward(O.to_torch_sd(state_dict(N, **kw)), feats(N, **kw), synth.make_radar_frame(seed=2, n_per_radar=51),
                                      variant(N, **kw), return_debug=True)
        _CENTRES[key] = centres_of(dbg)
    return _CENTRES[key]


def frame(N, seed=None, **kw):
    """the radar frame of the count's rig: 255 returns, most of them near the oracle's centres"""
    if seed is None:
        seed = RADAR_SEEDS[_vkey(N, kw)][0]
    return synth.make_radar_frame(seed=seed, n_per_radar=51, centres=centres(N, **kw))


def search_seed(N, **kw):
    """-> (seed, margin): the gate-margin search"""
    key = _vkey(N, kw)
    if key not in _SEARCH:
        sd, f = O.to_torch_sd(state_dict(N, **kw)), feats(N, **kw)
        margins = {s: R.gate_margin(sd, f, frame(N, s, **kw), **variant(N, **kw)) for s in SEED_RANGE}
        best = max(margins, key=margins.get)
        _SEARCH[key] = (best, margins[best])
    return _SEARCH[key]


_ORACLE = {}


def oracle(N, jitter_seed=None, **kw):
    """-> (sd, feats_np [1, N, ...], frame, want, dbg): the oracle's head on the count's rig, B = 1; jitter_seed: on the
    second lidar2img set with the maps of the batch's second sample"""
    key = _vkey(N, kw) + (jitter_seed,)
    if key not in _ORACLE:
        sd = O.to_torch_sd(state_dict(N, **kw))
        f = feats(N, **kw) if jitter_seed is None else [x[1:] for x in feats(N, batch=2, **kw)]
        fr = frame(N, **kw)
        v = dict(variant(N, **kw), geometry=Ring(N, jitter_seed))
        with torch.no_grad():
            want, dbg = R.oracle_forward(sd, f, fr, v, return_debug=True)
        _ORACLE[key] = (sd, f, fr, want, dbg)
    return _ORACLE[key]


# ---- coverage: what a count's rig must exercise -------------------------------------------------------------------------------
def visibility(N, dbg, jitter_seed=None, base=None):
    """[layers, Q, N] bool: camera n sees the reference point layer l samples at (the oracle's projection); base: the
    ring's base geometry (None: the configs')"""
    refs = [dbg['init_ref']] + list(dbg['inter_refs'][:-1])
    ring = Ring(N, jitter_seed, base)
    l2i = torch.from_numpy(ring.lidar2img()).float()[None]
    return np.stack([O.project_points(r, list(ring.pc_range), l2i, ring.hw)[1][0].numpy().T for r in refs])


def coverage(N, dbg=None, jitter_seed=None, base=None):
    """Per decoder layer: queries per visible-camera count, queries seeing only cameras >= 8, queries seeing a camera below
    8 and one from 8 up, queries seeing the last camera.  -> list of dicts"""
    vis = visibility(N, oracle(N)[4] if dbg is None else dbg, jitter_seed, base)
    out = []
    for v in vis:
        lo, hi = v[:, :8].any(1), v[:, 8:].any(1)
        out.append(dict(per_count=np.bincount(v.sum(1), minlength=4).tolist(), high_only=int((hi & ~lo).sum()),
                        low_and_high=int((lo & hi).sum()), last=int(v[:, -1].sum()), pairs=int(v.sum())))
    return out


LEAST = dict(high_only=2, low_and_high=9, three=3, last=10)       # what a 72-query rig of the configs' geometry must show


def assert_coverage(N, dbg=None, jitter_seed=None, base=None, least=LEAST):
    """The conditions of a rig with more than 8 cameras, in every decoder layer.  least: the queries that must see only
    cameras >= 8, a camera below 8 and one from 8 up, three cameras or more (N > 9), the last camera; `either` (optional):
    those of the first two kinds together"""
    for l, c in enumerate(coverage(N, dbg, jitter_seed, base)):
        assert c['high_only'] >= least['high_only'], (N, l, c)
        assert c['low_and_high'] >= least['low_and_high'], (N, l, c)
        assert c['high_only'] + c['low_and_high'] >= least.get('either', 0), (N, l, c)
        assert N == 9 or sum(c['per_count'][3:]) >= least['three'], (N, l, c)
        assert c['last'] >= least['last'], (N, l, c)


# ---- the device side ----------------------------------------------------------------------------------------------------------
def run_head(head, N, feats_np, frames, geoms, **options):
    """`len(geoms)` samples (maps [B, N, ...], one radar frame and one Ring each) through the module entry with aux outputs"""
    from transcar_amd.detr3d_head import head_options
    metas = [g.metas(1, radar=fr)[0] for g, fr in zip(geoms, frames)]
    head.forward_options = head_options(**options) if options else None
    try:
        outs = head([R.gpu(f) for f in feats_np], metas, aux=True)
        torch.cuda.synchronize()
    finally:
        head.forward_options = None
    return outs


def sample(outs, b):
    """sample b of a batched forward, as a one-sample forward's outputs (the checkers read [:, 0])"""
    cut = {k: outs[k][:, b:b + 1] for k in ('all_cls_scores', 'all_bbox_preds')}
    cut['aux'] = {k: (v[b:b + 1] if k in ('init_reference', 'last_box') else v[:, b:b + 1])
                  for k, v in outs['aux'].items() if k != 'sample_pairs'}
    return cut
