"""A Detr3DTransformer without box refinement for the CPU oracle.

oracle.transcar_oracle.transformer refines the reference points after every
decoder layer (the TransCAR configs' with_box_refine=True).  A head built with
with_box_refine=False hands the decoder reg_branches=None (HEAD:271), so every
layer samples at the initial reference points and inter_references[l] is
init_reference for every l (XFMR:183-203).  The head's last-level box still
comes from reg_branches[-1] (HEAD:287-293), which oracle.head_forward evaluates
itself.  The tests monkeypatch this function over the oracle's, as
num_points_oracle.py does for the cross-attention."""
import torch

from oracle import transcar_oracle as O


def transformer(sd, mlvl_feats, pc_range, lidar2img, img_hw, num_layers=6,
                embed=256, dec_drop=None):
    """Detr3DTransformer.forward + Detr3DTransformerDecoder.forward with
    reg_branches=None.  Returns what the oracle's transformer returns:
    inter_states [L,Q,B,C], init_reference [B,Q,3], inter_references [L,B,Q,3]
    (each the initial reference), last_reg [B,Q,10] (reg_branches[L-1] of the
    last layer's output: HEAD:287 evaluates exactly this)."""
    Bsz = mlvl_feats[0].shape[0]
    qe = sd['query_embedding.weight']
    query_pos, query = torch.split(qe, embed, dim=1)          # XFMR:119
    query_pos = query_pos.unsqueeze(0).expand(Bsz, -1, -1)
    query = query.unsqueeze(0).expand(Bsz, -1, -1)
    ref = O.linear(sd, 'transformer.reference_points', query_pos).sigmoid()
    x = query.permute(1, 0, 2)
    query_pos = query_pos.permute(1, 0, 2)
    inter, inter_ref = [], []
    for lid in range(num_layers):
        p = 'transformer.decoder.layers.%d.' % lid
        x = O.decoder_layer(sd, p, x, query_pos, mlvl_feats, ref, pc_range,
                            lidar2img, img_hw, drop=None if dec_drop is None else dec_drop[lid])
        inter.append(x)
        inter_ref.append(ref)
    tmp = O.reg_branch(sd, 'reg_branches.%d' % (num_layers - 1), x.permute(1, 0, 2))
    return torch.stack(inter), ref, torch.stack(inter_ref), tmp
