"""An ADVERSE frame for the parity tests (test_gpu_adverse_frame.py): inputs on which the
data-dependent branches of the kernels run that the bench's rig never reaches.

The bench's rig (test_gpu_teacher_forced.py) has 0.97-1.02 visible cameras per query, attention
scores that span ~9 octaves per row and 255 radar points (T = 256).  On it the loop over several
visible cameras, the lazy re-centring of the attention core (self_attn.hip SA_TAU: a score 2^8
above the running reference) inside a real layer, and two of the radar gate's three token-count
regimes (chain.hip K_RADAR_GATE / K_RADAR_ATTN: T <= 256 cached, T <= 512 masks kept, T > 512 gate
re-evaluated) are never compared with an independent reference.  This rig:

* weights: ``synth.make_state_dict(seed=3, reg_out_scale=1.0)`` with the q rows of every
  attention's in_proj (six decoder self-attentions, three radar attentions) scaled by 8: the
  scores of a row then span ~70 octaves and a third of the (head, row) pairs meet a 32-key chunk
  whose maximum lies more than 8 log2-units above every earlier chunk;
* cameras: ``synth.make_lidar2img(focal=500.0)``: wide, overlapping fields of view -- 1.85-1.91
  visible cameras per query in every decoder layer, some queries with three, some with none;
* maps: ``synth.make_feats('res101', seed=1, smooth=None)`` (iid noise, as the bench);
* four radar frames (FRAMES) around the oracle's last reference points, one per regime.

Everything here runs on the CPU; the oracle (fp32) and its evaluation on the .double() copy of
the same state dict are the references."""
import numpy as np
import torch

from oracle import transcar_oracle as O
from transcar_amd import configs, radar as R, synth

PCR = configs.point_cloud_range
HW = configs.IMG_SHAPE[:2]
FOCAL = 500.0
Q_SCALE = 8.0
LOG2E = 1.4426950408889634
ATTENTIONS = ['transformer.decoder.layers.%d.attentions.0.attn' % l for l in range(6)] + \
             ['rf_multihead_attn' + s for s in ('', '2', '3')]

# name -> (make_radar_frame arguments, points kept, (T, pad_mult) of the HIP launch,
#          rows hit in fusion layers 1 / 2 / 3 and the largest hit count of a row: CPU measurements)
FRAMES = {
    'keep': (dict(n_per_radar=80, near_frac=0.9), 396, (448, 1053), (481, 401, 115), 17),
    'mid': (dict(n_per_radar=140, near_frac=0.9), 692, (704, 797), (609, 540, 150), 27),
    'truncated': (dict(n_per_radar=330), 1633, (1500, 1), (790, 714, 257), 48),
    'all_hit': (dict(n_per_radar=300), 1497, (1500, 1), (900, 875, 241), 52),
}


def make_state_dict():
    """numpy state dict: the un-conditioned bench weights with every attention's q projection x 8."""
    sd = synth.make_state_dict(seed=3, reg_out_scale=1.0)
    for name in ATTENTIONS:
        w = sd[name + '.in_proj_weight'].copy()
        b = sd[name + '.in_proj_bias'].copy()
        w[:256] *= Q_SCALE
        b[:256] *= Q_SCALE
        sd[name + '.in_proj_weight'], sd[name + '.in_proj_bias'] = w, b
    return sd


def build():
    """Weights, cameras, maps and the fp32 oracle's trace of the decoder (no GPU)."""
    sd_np = make_state_dict()
    sd = O.to_torch_sd(sd_np)
    feats_np = synth.make_feats('res101', seed=1, smooth=None)
    feats = [torch.from_numpy(f) for f in feats_np]
    l2i = torch.from_numpy(synth.make_lidar2img(focal=FOCAL)).float()[None]
    xfmr = O.transformer(sd, feats, PCR, l2i, HW)               # hs [L,Q,1,C], init_ref, inter_refs, last reg
    hs, init_ref, inter_refs, _ = xfmr
    refs = inter_refs[-1][0].double().numpy()
    centres = np.round(np.stack([refs[:, 0] * (PCR[3] - PCR[0]) + PCR[0],
                                 refs[:, 1] * (PCR[4] - PCR[1]) + PCR[1]], 1), 2)     # bench.make_inputs
    return dict(sd_np=sd_np, sd=sd, sd64={k: v.double() for k, v in sd.items()}, feats_np=feats_np, feats=feats,
                l2i=l2i, xfmr=xfmr, hs=hs, init_ref=init_ref, inter_refs=inter_refs, centres=centres)


def layer_inputs(rig, lid):
    """The oracle's state in front of decoder layer `lid`: (x [1,Q,C], reference points [1,Q,3])."""
    qe = rig['sd']['query_embedding.weight']
    x = qe[:, 256:][None] if lid == 0 else rig['hs'][lid - 1].permute(1, 0, 2)
    ref = rig['init_ref'] if lid == 0 else rig['inter_refs'][lid - 1]
    return x, ref


def visibility(rig, lid):
    """fp32 and fp64 visibility masks [N,Q] of the reference points decoder layer `lid` samples at."""
    _, ref = layer_inputs(rig, lid)
    _, m32 = O.project_points(ref, PCR, rig['l2i'], HW)
    _, m64 = O.project_points(ref.double(), PCR, rig['l2i'].double(), HW)
    return m32[0], m64[0]


def self_attn_scores_log2(rig, lid):
    """fp64 scores [heads,Q,Q] of decoder layer `lid`'s self-attention in log2 units (the 2^x softmax
    of the attention core)."""
    x, _ = layer_inputs(rig, lid)
    pos = rig['sd']['query_embedding.weight'][:, :256]
    name = ATTENTIONS[lid]
    W, b = rig['sd64'][name + '.in_proj_weight'], rig['sd64'][name + '.in_proj_bias']
    qk = (x[0] + pos).double()
    Q = qk.shape[0]
    q = (qk @ W[:256].T + b[:256]).view(Q, 8, 32) / np.sqrt(32.0)
    k = (qk @ W[256:512].T + b[256:512]).view(Q, 8, 32)
    return torch.einsum('qhd,khd->hqk', q, k) * LOG2E


def recentring_share(scores, chunk=32, tau=8.0):
    """The share of (head, row) pairs in which some `chunk`-key chunk's maximum lies more than
    `tau` log2-units above every earlier chunk: a proxy of the attention core's re-centring branch
    (it re-centres when a score exceeds the running reference by 2^SA_TAU)."""
    H, Q, K = scores.shape
    n = K // chunk
    cmax = scores[..., :n * chunk].reshape(H, Q, n, chunk).amax(-1)
    run = torch.cummax(cmax, -1).values
    return float(((cmax[..., 1:] - run[..., :-1]) > tau).any(-1).float().mean())


def radar_frame(rig, name):
    """The raw radar frame `name` of FRAMES (nuScenes-devkit layout, synth.make_radar_frame)."""
    frame = synth.make_radar_frame(seed=2, centres=rig['centres'], **FRAMES[name][0])
    if name == 'all_hit':           # one return exactly on every query's centre: no row tile without a hit
        k = 0
        for chan in synth.RADAR_CHANNELS:
            p = frame['points'][chan]
            p[0, :180] = rig['centres'][k:k + 180, 0]
            p[1, :180] = rig['centres'][k:k + 180, 1]
            k += 180
        assert k == rig['centres'].shape[0] == 900
    return frame


def radar_case(rig, name):
    """Frame `name` as both sides take it and the fp32 oracle's trace of the radar part on it:
    dict(f36 = the oracle's feature rows (un-truncated), tok_np / pad_mult = the HIP launch's tokens
    (radar.pack_tokens; `truncated`: the first 1500 rows at T = 1500, as HEAD:523-530 keeps them),
    trace = (outputs, debug) of O.head_forward, hits [3,Q])."""
    cache = rig.setdefault('_radar', {})
    if name not in cache:
        frame = radar_frame(rig, name)
        f36 = O.build_radar_features(frame)
        rows = R.build_radar_features(frame)
        if name == 'truncated':
            tok_np, pad_mult = R.pack_tokens([rows[:R.NUM_RADAR_TOKENS]], T=R.NUM_RADAR_TOKENS)
        else:
            tok_np, pad_mult = R.pack_tokens([rows])
        trace = O.head_forward(rig['sd'], rig['feats'], rig['l2i'], HW, f36, PCR, return_debug=True,
                               decoder_trace=rig['xfmr'])       # the decoder's trace is the rig's: evaluate it once
        assert trace[1]['inter_refs'] is rig['inter_refs'] and torch.equal(trace[1]['hs'], rig['hs'].permute(0, 2, 1, 3))
        hits = np.stack([h.numpy() for h in trace[1]['hit_counts']])
        cache[name] = dict(frame=frame, f36=f36, rows=rows, tok_np=tok_np, pad_mult=pad_mult, trace=trace, hits=hits)
    return cache[name]


def radar_layer1_truth(rig, case):
    """fp64 evaluation of fusion layer 1 (HEAD:531-611) on the fp32 oracle's decoder state and with the
    fp32 oracle's gate decisions: class scores [Q,ncls] and boxes [Q,code] in float64, the fp32 / fp64
    gate disagreements (pairs), and the max deviation of the fp32 oracle's encoded radar features."""
    sd64 = rig['sd64']
    want, dbg = case['trace']
    tokens, _ = O.radar_tokens_from_features(case['f36'])
    ref = dbg['inter_refs'][-1]
    cxy = torch.stack([ref[..., 0] * (PCR[3] - PCR[0]) + PCR[0], ref[..., 1] * (PCR[4] - PCR[1]) + PCR[1]], -1)
    box = dbg['tmp']
    m32 = O.circle_mask(cxy, box[..., 3], box[..., 6], box[..., 7], tokens[:, :, :2], 1.0, 2.0)
    m64 = O.circle_mask(cxy.double(), box[..., 3].double(), box[..., 6].double(), box[..., 7].double(),
                        tokens[:, :, :2].double(), 1.0, 2.0)
    assert np.array_equal((~m32).sum(1).numpy(), case['hits'][0])
    rf64 = O.radar_encode(sd64, tokens.double()).permute(1, 0, 2)
    qf = dbg['hs'][-1].permute(1, 0, 2).double()
    x64, _ = O.radar_layer(sd64, '', '', qf, rf64, m32)
    xb = x64.permute(1, 0, 2)
    c64 = O.cls_branch(sd64, 'final_cls', xb)
    t64 = O.reg_branch(sd64, 'final_reg', xb)
    t64[..., 0:2] = t64[..., 0:2] + cxy.double()                # HEAD:596-600 (z stays normalised)
    t64[..., 4:5] = t64[..., 4:5] + ref.double()[..., 2:3]
    return dict(cls=c64[0], box=t64[0], gate_flips=int((m32 != m64).sum()),
                enc_dev=float((dbg['radar_feat'].double() - rf64).abs().max()))
