"""A num_points-aware Detr3DCrossAtten for the CPU oracle (XFMR:362-373).

oracle.transcar_oracle.cross_atten views the attention logits as
[B,1,Q,N,1,L] (the TransCAR configs' num_points = 1).  This one views them as
[B,1,Q,N,P,L], P read from the shape of ``attention_weights``, exactly as the
reference does; the tests monkeypatch it over the oracle's so that
decoder_layer / head_forward use it."""
import torch

from oracle import transcar_oracle as O


def cross_atten(sd, name, query, query_pos, mlvl_feats, reference_points,
                pc_range, lidar2img, img_hw, num_cams=6, num_levels=4, out_mult=None):
    inp_residual = query
    q = (query + query_pos).permute(1, 0, 2)
    Bsz, Q, _ = q.shape
    num_points = sd[name + '.attention_weights.weight'].shape[0] // (num_cams * num_levels)
    aw = O.linear(sd, name + '.attention_weights', q).view(
        Bsz, 1, Q, num_cams, num_points, num_levels)
    sampled, mask = O.feature_sampling(mlvl_feats, reference_points, pc_range,
                                       lidar2img, img_hw)
    sampled = torch.nan_to_num(sampled, nan=0.0, posinf=float('inf'),
                               neginf=float('-inf'))
    aw = aw.sigmoid() * mask
    out = (sampled * aw).sum(-1).sum(-1).sum(-1)       # [B,C,Q]: L, then P, then N
    out = out.permute(2, 0, 1)
    out = O.linear(sd, name + '.output_proj', out)
    if out_mult is not None:
        out = out * out_mult
    pos_feat = O.pos_encoder(sd, name + '.position_encoder',
                             O.inverse_sigmoid(reference_points)).permute(1, 0, 2)
    return out + inp_residual + pos_feat


def sampling(mlvl_feats, reference_points, pc_range, lidar2img, img_hw, logits,
             num_cams=6, num_levels=4):
    """The weighted (cam, point, level) sum of one layer's sampling:
    logits [B,Q,N*P*L] -> [B,Q,C]."""
    B, Q, _ = logits.shape
    P = logits.shape[-1] // (num_cams * num_levels)
    sampled, mask = O.feature_sampling(mlvl_feats, reference_points, pc_range,
                                       lidar2img, img_hw)
    sampled = torch.nan_to_num(sampled, nan=0.0)
    aw = logits.view(B, 1, Q, num_cams, P, num_levels).sigmoid() * mask
    return (sampled * aw).sum(-1).sum(-1).sum(-1).permute(0, 2, 1)
