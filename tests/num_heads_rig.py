"""What the tests of the decoder self-attention's head count (num_heads 4 / 16; the configs: 8) add to
head_variant_rig.py: the oracle steered to H heads, heads built with configs.head_cfg(num_heads=H), and the rig's
checkers run under both.

oracle/transcar_oracle.py::decoder_layer calls the module-level multihead_attention with its default of 8 heads;
`steered(H)` swaps that name for a wrapper which passes num_heads=H to the decoder's self-attention
(`...attentions.0.attn`) and leaves the radar fusion attention (`rf_multihead_attn*`: 8 heads in the reference whatever
the decoder uses, HEAD:129-171) as it is.  The state dict does not depend on the head count.

A plain helper module (as head_variant_rig.py); the checkers it runs are that module's own, by import."""
import contextlib
import functools

import torch

import head_variant_rig as R
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

HEADS = (4, 16)          # beside the configs' 8: head dimension 64 and 16


@contextlib.contextmanager
def steered(H):
    """The oracle with an H-head decoder self-attention, and the rig's train-mode helpers (train_head, the read-back
    dropout masks of the probabilities: [H, Q, Q] per layer) at H; everything is put back on the way out."""
    orig = O.multihead_attention

    def mha(sd, name, *a, **k):
        if 'attentions.0.attn' in name:
            k['num_heads'] = H
        else:
            assert name.startswith('rf_multihead_attn'), name
        return orig(sd, name, *a, **k)

    keep = R.train_head, R.decoder_dropout_masks
    O.multihead_attention = mha
    R.train_head = functools.partial(train_head, H)
    R.decoder_dropout_masks = functools.partial(keep[1], H=H)
    try:
        yield
    finally:
        O.multihead_attention = orig
        R.train_head, R.decoder_dropout_masks = keep


def head_cfg(H, **variant):
    return configs.head_cfg(num_heads=H, **R.variant_kw(**variant))


def make_head(T, H, *, seed=3, **variant):
    """head_variant_rig.make_head with an H-head decoder self-attention (that rig's own refuses unknown variant keys)."""
    sd_np = synth.make_state_dict(seed=seed, **R.variant_kw(**variant))
    h = T.build_head(head_cfg(H, **variant))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    assert h.weights_struct().num_heads == H
    return h.to(R.dev()).eval(), O.to_torch_sd(sd_np)


_HEADS = {}


def shared_head(T, H):
    """make_head(T, H), one per head count for the tests that leave it as they found it."""
    if H not in _HEADS:
        _HEADS[H] = make_head(T, H)
    return _HEADS[H]


def train_head(H, **variant):
    import transcar_amd as T_
    cfg = head_cfg(H, **variant)
    cfg['train_cfg'] = configs.train_cfg_pts
    h = T_.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(3, **R.variant_kw(**variant)).items()})
    return h.to(R.dev()).freeze_decoder().set_dropout(0.0)


def oracle_head(H, sd, feats_np, frame, with_box_refine=True, key=None):
    """head_variant_rig.oracle_head under steered(H); key: kept per (H, key)."""
    with steered(H):
        return R.oracle_head(sd, feats_np, frame, with_box_refine=with_box_refine,
                             key=None if key is None else ('num_heads', H, key))
