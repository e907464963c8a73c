"""What the tests of the radar input's configuration (Detr3DHead(radar_num_tokens=N, radar_in_dims=F,
radar_point_range=...)) add to head_variant_rig.py, whose variants carry the three keys: the cases at 128 queries on the
tiny maps, frames of [n,F] feature rows scattered around the oracle's gate centres, the rows' filter, and one decoder trace
for all cases.

The reference writes 1500 and 36 into its program text, so there is no reference fixture off those values: the yardstick
is the oracle, which the G5 / G8 fixtures pin to the reference at 1500 / 36.  It reads F off the rows and the state dict and
is given N by argument (head_variant_rig.oracle_kw)."""
import numpy as np
import torch

import head_variant_rig as R
from oracle import transcar_oracle as O
from transcar_amd import synth

Q = 128
POINT_RANGE = R.POINT_RANGE                                    # HEAD:304
MIN_MARGIN = 1e-3       # metres between every gate decision of the oracle and its radius on the frames below
# case -> (N, F, n rows, seed of the frame, radar_point_range or None).  The seeds are chosen (on the CPU oracle, gate_probe)
# so that no gate decision sits within MIN_MARGIN of its radius; `oracle_case` measures it again wherever the tests run.
CASES = {
    'N2048-n1700': (2048, 36, 1700, 8, None),          # T = 1728: above 256, 512 and 1500
    'N2048-n2048': (2048, 36, 2048, 8, None),          # no pad row
    'N2048-n2100': (2048, 36, 2100, 2, None),          # truncation to the first 2048
    'N128-n40': (128, 4, 40, 1, None),                 # T = 64, pad_mult = 65
    'N1500-F4': (1500, 4, 300, 26, None),
    'N1500-F64': (1500, 64, 300, 4, None),
    'range': (1500, 36, 300, 37, (-51.2, -51.2, -5.0, 20.0, 51.2, 3.0)),
    'train-F8': (1500, 8, 300, 38, None),            # the second training frame
}
FACE_RANGE = (-40.0, -30.0, -2.0, 25.0, 35.0, 1.5)      # a filter range with every face moved (the pack kernel's and the pair rows')
# FusionTrainer's arguments per backward of the training tests
BACKWARDS = {'chain': dict(chain_forward=True, chain_backward=True), 'operators': dict(chain_forward=False, chain_backward=False),
             'deterministic': dict(chain_forward=True, chain_backward=True, deterministic=True)}
NEAR = 120              # rows of a frame that lie near a gate centre; the others are kept out of every gate's reach


def variant(N=1500, F=36, point_range=None):
    """head_variant_rig's variant of a case.  synth draws radar_feat_encoder behind the decoder and the fusion layers, so
    every F shares the decoder's weights (and one decoder trace serves them all)."""
    return dict(num_query=Q, radar_num_tokens=N, radar_in_dims=F, radar_point_range=point_range)


_SHARED = {}


def feats_np():
    if 'feats' not in _SHARED:
        _SHARED['feats'] = synth.make_feats('tiny', seed=1, smooth=R.SMOOTH)
    return _SHARED['feats']


def decoder_trace():
    """The oracle's decoder at 128 queries on the tiny maps, once: (hs, init_ref, inter_refs, tmp) as head_forward takes it."""
    if 'trace' not in _SHARED:
        sd = O.to_torch_sd(R.state_dict(**variant()))
        with torch.no_grad():
            _SHARED['trace'] = O.transformer(sd, [torch.from_numpy(f) for f in feats_np()], list(R.PCR),
                                             torch.from_numpy(synth.make_lidar2img()).float()[None], R.HW)
    return _SHARED['trace']


def gate_centres():
    """[Q,2] metres: the decoder's last reference points, where fusion layer 1 gates (a radar-free first pass)."""
    return O.denormalised_refs(decoder_trace()[2][-1], list(R.PCR))[0, :, :2].numpy().astype(np.float64)


def make_rows(seed, n, F, near=NEAR, centres=None, near_sigma=0.6):
    """[n,F] float32 rows: `near` of them `near_sigma` m around gate centres (at random row indices, so that hits lie
    beyond any token count below n), the others at least 8 m from every centre; columns 3.. are noise.  centres: [m,2]
    metres (None: this rig's gate_centres())."""
    rng = np.random.RandomState(1000 + seed)
    cen = gate_centres() if centres is None else np.asarray(centres, np.float64)
    near = min(near, n)
    xyz = np.empty((n, 3))
    pick = cen[rng.randint(0, len(cen), near)]
    xyz[:near, :2] = pick + near_sigma * rng.standard_normal((near, 2))
    k = near
    while k < n:
        cand = rng.uniform(-50.0, 50.0, (4 * (n - k) + 16, 2))
        far = np.sqrt(((cand[:, None] - cen[None]) ** 2).sum(-1)).min(1) > 8.0
        take = cand[far][:n - k]
        xyz[k:k + len(take), :2] = take
        k += len(take)
    xyz[:, :2] = np.clip(xyz[:, :2], -50.0, 50.0)
    xyz[:, 2] = rng.uniform(-3.0, 2.0, n)
    rows = np.concatenate((xyz, 0.5 * rng.standard_normal((n, F - 3))), 1)
    return np.ascontiguousarray(rows[rng.permutation(n)], dtype=np.float32)


def in_range(rows, point_range):
    """HEAD:514-519 on float64 coordinates, strict"""
    x = rows[:, :3].astype(np.float64)
    lo, hi = np.asarray(point_range[:3]), np.asarray(point_range[3:])
    return np.all(x > lo, 1) & np.all(x < hi, 1)


_ORACLE = {}


def oracle_case(name):
    """-> dict(N, F, rows [n,F] float32 as the head gets them, kept: the rows its filter keeps, want, dbg, masks: the
    oracle's gate masks [Q,N] per layer (True = masked), margin: metres between its closest gate decision and the radius)."""
    if name not in _ORACLE:
        N, F, n, seed, rng = CASES[name]
        rows = make_rows(seed, n, F)
        kept = rows[in_range(rows, rng or POINT_RANGE)]
        v = variant(N, F, rng)
        masks, margins = [], []
        with torch.no_grad():
            want, dbg = R.oracle_forward(O.to_torch_sd(R.state_dict(**v)), feats_np(), kept, v, return_debug=True,
                                         decoder_trace=decoder_trace(), gate_probe=R.margin_probe(margins, masks))
        assert dbg['fill_in'] == min(N, len(kept)) and len(masks) == 3 and masks[0].shape == (Q, N)
        _ORACLE[name] = dict(N=N, F=F, rows=rows, kept=kept, point_range=rng, want=want, dbg=dbg, masks=masks, margin=min(margins))
    return _ORACLE[name]


def metas(rows_list, device=None):
    """img_metas of one frame per entry; device: the rows as CUDA tensors (the device route), None: numpy (the host route)"""
    m = synth.make_img_metas(len(rows_list), synth.make_lidar2img())
    for i, r in enumerate(rows_list):
        m[i]['radar'] = torch.from_numpy(r).to(device) if device is not None else r
    return m
