"""What the tests of the decoder layers' feedforward_channels (tc_head_weights.ffn_dims, 256 .. 2048 in steps of 256; the
configs: 512) add to head_variant_rig.py, whose variants carry the width (the oracle's decoder_layer reads it off the
state dict): the widths, and the radar frame of each head.

A width is another decoder output, and the radar gate is discontinuous: SEEDS holds, per head, the radar seed of
g5_frame whose closest gate decision of the ORACLE sits at least MIN_MARGIN from its radius (picked on the CPU with
head_variant_rig.gate_margin over seeds 2, 3, ..: the first that qualifies; test_ffn_dims_rig.py re-measures them), so
that MAX_GATE_ROWS only has to cover the kernels."""
import head_variant_rig as R
from oracle import transcar_oracle as O

WIDTHS = (256, 768, 1024, 2048)      # one narrow chunk alone, a full chunk + a narrow one, two full chunks, the maximum
MIN_MARGIN = 1e-3                    # metres, as variant_pairs_rig's rows
# (feedforward_channels, with_box_refine) -> radar seed of R.g5_frame
# (picked with half as much again to spare, so that another CPU's summation order cannot bring one below MIN_MARGIN:
# measured 2.1e-3, 2.0e-3, 1.6e-3, 1.7e-3; without box refinement 1.8e-3)
SEEDS = {(256, True): 37, (768, True): 39, (1024, True): 39, (2048, True): 9, (1024, False): 5}


def variant(F, refine=True):
    """head_variant_rig's variant of a head of width F"""
    return dict(feedforward_channels=F, **({} if refine else dict(with_box_refine=False)))


def frame(F, refine=True):
    """(feats_np, radar frame): G5's tiny maps and the radar of the head's seed"""
    return R.g5_frame(SEEDS[F, refine])


def margin(F, refine=True, seed=None):
    """metres between the oracle's closest gate decision on the head's frame (or that of `seed`) and its radius"""
    feats_np, fr = R.g5_frame(SEEDS[F, refine] if seed is None else seed)
    return R.gate_margin(O.to_torch_sd(R.state_dict(**variant(F, refine))), feats_np, fr, **variant(F, refine))
