"""What the tests of the radar fusion attention's head count (Detr3DHead(radar_num_heads=H), H = 4 / 16 beside the
reference's 8) add to head_variant_rig.py, whose variants carry the key (heads, oracle calls, training iterations and
dropout masks at H heads are its own): the fixtures' names and frames, and the ReLU-tie analysis of a training frame."""
import numpy as np

import head_variant_rig as R
from oracle import transcar_oracle as O

HEADS = (4, 16)         # radar_num_heads beside the reference's 8: head dimension 64 and 16


def g5_name(H):
    return 'g5_head_tiny_rh%d.npz' % H


def g8_name(H):
    return 'g8_train_grads_rh%d.npz' % H


def g5_frame(H):
    """The frame of the H-head fixtures: G5's maps, the radar of the seed the fixture stores."""
    return R.g5_frame(int(R.gold(g5_name(H))['radar_seed']))


def g8_frame(H):
    return R.g8_frame('g5_head_tiny.npz', radar_seed=int(R.gold(g8_name(H))['radar_seed']))


# ---- ReLU ties: how far a frame's gradients move when the inputs nearest to zero are taken on the other side ------------------
TIE_TAU = 3e-5          # twice 256 * 2^-24: what two fp32 evaluation orders of a LayerNorm / a 256-term product part by
TIE_BOUND = 1e-3        # half of the 2e-3 the gradient checks allow: the other half is the arithmetic's


def g8_figures(grads, g8):
    """The largest of check_grads_against_g8's four figures over the parameters, each in the unit its rtol multiplies."""
    worst = 0.0
    for k, g in grads.items():
        key = k.replace('.', '__')
        if g is None or key + '__stats' not in g8.files:
            continue
        ref, head = g8[key + '__stats'], g8[key + '__head']
        gd = g.detach().double().flatten().cpu()
        got = np.array([gd.sum(), gd.abs().sum(), gd.norm()])
        unit = max(np.abs(head).max(), ref[2] / np.sqrt(gd.numel()))
        worst = max(worst, abs(got[1] - ref[1]) / ref[1], abs(got[2] - ref[2]) / max(ref[2], 1e-12), abs(got[0] - ref[0]) / ref[1],
                    float(np.abs(gd[:16].float().numpy() - head).max()) / (4 * unit))
    return worst


def tie_sensitivity(host, H, tau=TIE_TAU, **variant):
    """g8_figures between the oracle's gradients on the host side of a g8_frame and its gradients with every ReLU input of
    the trainable stack within `tau` of zero taken on the other side, all at once (O.F.relu is replaced for the call)."""
    plain, flip = O.F.relu, [False]

    def relu(x, *args, **kw):
        if flip[0] and x.requires_grad:
            return x * ((x.detach() > 0) ^ (x.detach().abs() < tau)).to(x.dtype)
        return plain(x, *args, **kw)
    O.F.relu = relu
    try:
        grads = R.oracle_training(host, keep=False, radar_num_heads=H, **variant)[3]
        flip[0] = True
        flipped = R.oracle_training(host, keep=False, radar_num_heads=H, **variant)[3]
    finally:
        O.F.relu = plain
    return g8_figures(flipped, R.GradStats(grads))


def bit_equal(a, b):
    return np.array_equal(R._np(a), R._np(b))
