"""The rig of the tests of the decoder layers' feedforward_channels (tc_head_weights.ffn_dims, 256 .. 2048 in steps of
256; the configs: 512).  head_variant_rig.py asserts its variant keys against CONFIGS and cannot carry the width, so the
heads are built here -- configs.head_cfg(feedforward_channels=F) with synth.make_state_dict(feedforward_channels=F) --
and everything else is that rig's, unchanged: the frames, oracle_forward (the oracle's decoder_layer reads the widths
off the state dict), run_head, check_against_oracle and the tolerances.

A width is another decoder output, and the radar gate is discontinuous: SEEDS holds, per head, the radar seed of
g5_frame whose closest gate decision of the ORACLE sits at least MIN_MARGIN from its radius (picked on the CPU with
head_variant_rig.gate_margin over seeds 2, 3, ..: the first that qualifies; test_ffn_dims_rig.py re-measures them), so
that MAX_GATE_ROWS only has to cover the kernels."""
import numpy as np
import torch

import head_variant_rig as R
from oracle import transcar_oracle as O
from transcar_amd import configs, synth

WIDTHS = (256, 768, 1024, 2048)      # one narrow chunk alone, a full chunk + a narrow one, two full chunks, the maximum
MIN_MARGIN = 1e-3                    # metres, as variant_pairs_rig's rows
# (feedforward_channels, with_box_refine) -> radar seed of R.g5_frame
# (picked with half as much again to spare, so that another CPU's summation order cannot bring one below MIN_MARGIN:
# measured 2.1e-3, 2.0e-3, 1.6e-3, 1.7e-3; without box refinement 1.8e-3)
SEEDS = {(256, True): 37, (768, True): 39, (1024, True): 39, (2048, True): 9, (1024, False): 5}


def variant_of(refine=True):
    return {} if refine else dict(with_box_refine=False)


def state_dict(F, refine=True):
    return synth.make_state_dict(seed=3, feedforward_channels=F, **({} if refine else dict(with_box_refine=False)))


def head_cfg(F, refine=True, **kw):
    return configs.head_cfg(feedforward_channels=F, **dict({} if refine else dict(with_box_refine=False), **kw))


def make_head(T, F, refine=True):
    """A fresh eval-mode head of width F with the seed-3 weights, and those weights as the oracle takes them."""
    sd_np = state_dict(F, refine)
    h = T.build_head(head_cfg(F, refine))
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    assert h.weights_struct().ffn_dims == F
    return h.to(R.dev()).eval(), O.to_torch_sd(sd_np)


_HEADS = {}


def shared_head(T, F, refine=True):
    """make_head, one per width for the tests that leave it as they found it"""
    if (F, refine) not in _HEADS:
        _HEADS[F, refine] = make_head(T, F, refine)
    return _HEADS[F, refine]


def train_head(F):
    """R.train_head at width F: frozen decoder, dropout off"""
    import transcar_amd as T_
    cfg = head_cfg(F)
    cfg.setdefault('train_cfg', configs.train_cfg_pts)
    h = T_.build_head(cfg)
    h.load_state_dict({k: torch.from_numpy(v) for k, v in state_dict(F).items()}, strict=True)
    return h.to(R.dev()).freeze_decoder().set_dropout(0.0)


def frame(F, refine=True):
    """(feats_np, radar frame): G5's tiny maps and the radar of the head's seed"""
    return R.g5_frame(SEEDS[F, refine])


def margin(F, refine=True, seed=None):
    """metres between the oracle's closest gate decision on the head's frame (or that of `seed`) and its radius"""
    feats_np, fr = R.g5_frame(SEEDS[F, refine] if seed is None else seed)
    return R.gate_margin(O.to_torch_sd(state_dict(F, refine)), feats_np, fr, **variant_of(refine))


def oracle_head(sd, F, refine=True):
    """The oracle's forward with its debug dict on frame(F, refine), once per head"""
    feats_np, fr = frame(F, refine)
    return R.oracle_head(sd, feats_np, fr, key=('ffn_dims', F), **variant_of(refine))


_TRAINING = {}


def oracle_training(host, F):
    """R.oracle_training at width F (the trainable weights as autograd leaves, head_forward, O.loss, backward), once per
    width -> (losses {name: float}, {name: gradient or None} of the trainable parameters)"""
    if F not in _TRAINING:
        sd = O.to_torch_sd(state_dict(F))
        for k, v in sd.items():
            if R.trainable(k):
                v.requires_grad_(True)
        with torch.enable_grad():
            outs = R.oracle_forward(sd, host['feats_np'], host['frame'], {})
            res, _ = O.loss({k: outs[k] for k in ('all_cls_scores', 'all_bbox_preds')}, torch.from_numpy(host['boxes']),
                            torch.from_numpy(host['labels']), sd['code_weights'], num_classes=10)
            sum(res.values()).backward()
        _TRAINING[F] = ({k: float(v.detach()) for k, v in res.items()}, {k: v.grad for k, v in sd.items() if R.trainable(k)})
    return _TRAINING[F]


def check_train_mode_decoder(F, rows, matrix, refs_atol=2e-4):
    """R.check_train_mode_decoder at width F: the frozen decoder's train-mode forward (the DROP instantiations of the
    chain kernels, layer 0 not folded) against the oracle's decoder with the SAME masks, read back through
    tc_dropout_mask -- the hidden site's as [Q, 1, F]: its element index is row * F + column."""
    from transcar_amd import ops
    from transcar_amd.detr3d_head import head_options
    p, seed = 0.1, 0x5EED1234ABCD
    fr = R.g8_frame('g5_head_tiny.npz', radar_seed=SEEDS[F, True])
    h = train_head(F)
    h.set_decoder_dropout(p)
    feats, metas = fr['feats'], fr['metas']
    nhwc = ops.to_nhwc_levels(feats)
    l2i = ops.lidar2img_tensor(metas, R.dev())
    img_hw = metas[0]['img_shape'][0][:2]
    tokens, pad_mult = h.radar_tokens(metas, R.dev())
    h.train()
    opts = head_options(decoder_dropout_p=p, dropout_seed=seed, tile_rows=rows, matrix_path=matrix)
    a = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=opts)
    b = h.forward_nhwc(nhwc, l2i, img_hw, tokens, pad_mult, aux=True, _allow_train=True, options=opts)
    hs = a['aux']['inter_states']
    assert torch.equal(hs, b['aux']['inter_states'])                 # same seed, same masks
    masks = R.decoder_dropout_masks(p, seed, h.num_query, Fd=F)
    assert all(m['ffn_h'].numel() == h.num_query * F for m in masks)
    keep = float(torch.stack([m['ffn_h'] for m in masks]).ne(0).float().mean())
    assert abs(keep - (1.0 - p)) < 5e-3, keep
    want_hs, init_ref, want_refs, _ = O.transformer(
        O.to_torch_sd(state_dict(F)), [torch.from_numpy(f) for f in fr['feats_np']], list(R.DEFAULT.pc_range),
        torch.from_numpy(fr['l2i_np']).float()[None], R.DEFAULT.hw, dec_drop=masks)
    np.testing.assert_allclose(a['aux']['init_reference'].cpu().numpy(), init_ref.numpy(), atol=1e-6, rtol=0)
    np.testing.assert_allclose(a['aux']['inter_references'].cpu().numpy(), want_refs.numpy(), atol=refs_atol, rtol=0)
    d = np.abs(hs.cpu().numpy()[:, 0] - want_hs[:, :, 0].numpy())
    print('F=%d %d rows %s train mode: max|hs - oracle with the same masks| = %.3g' % (F, rows, matrix, d.max()))
    np.testing.assert_allclose(hs.cpu().numpy()[:, 0], want_hs[:, :, 0].numpy(), atol=2e-3, rtol=0)
