"""A Detr3DCrossAtten for the CPU oracle that takes any number of FPN levels (XFMR:362-373, 381-422).

oracle.transcar_oracle.cross_atten and num_points_oracle.py view the attention
logits with L = 4 (the TransCAR configs).  This one reads L from
``len(mlvl_feats)`` and P from the shape of ``attention_weights``
([N*P*L, C]), and views the logits as [B,1,Q,N,P,L] exactly as the reference
does; the tests monkeypatch it over the oracle's so that decoder_layer /
head_forward use it."""
import torch

from oracle import transcar_oracle as O


def cross_atten(sd, name, query, query_pos, mlvl_feats, reference_points,
                pc_range, lidar2img, img_hw, num_cams=6, num_levels=None, out_mult=None):
    num_levels = len(mlvl_feats)
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
             num_cams=6):
    """The weighted (cam, point, level) sum of one layer's sampling over
    L = len(mlvl_feats) levels: logits [B,Q,N*P*L] -> [B,Q,C]."""
    B, Q, _ = logits.shape
    L = len(mlvl_feats)
    P = logits.shape[-1] // (num_cams * L)
    sampled, mask = O.feature_sampling(mlvl_feats, reference_points, pc_range,
                                       lidar2img, img_hw)
    sampled = torch.nan_to_num(sampled, nan=0.0)
    aw = logits.view(B, 1, Q, num_cams, P, L).sigmoid() * mask
    return (sampled * aw).sum(-1).sum(-1).sum(-1).permute(0, 2, 1)
